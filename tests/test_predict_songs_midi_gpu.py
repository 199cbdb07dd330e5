"""decoder.predict_songs(note_events=True): mvae_note_events behind mvae_recon_songs on the same device rolls, against
events.note_events(..., device=False) - the NumPy mirror - on the rolls predict_songs returned itself, and the file written from them.

Everything is an integer: EQUAL.  The 320 windows take three engine batches of 128 and two songs straddle a batch edge (the model and
the songs of tests/test_predict_songs_gpu.py): the rolls the events are taken from were filled by three engine batches."""
import io

import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import midifile as mf
from tests.test_predict_songs_gpu import LENGTHS, small_model, split  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = ["counts", "instr", "notes", "starts", "velocity"]


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_events_are_the_mirror_on_the_returned_rolls(small_model, method, kw):
    s, m, xs, x_all, orig = small_model
    dec, V, ticks = m.decoder, 2, 8
    got = dec.predict_songs(xs, 8, sample_method=method, note_events=True, **kw)
    closed = dec.predict_songs(xs, 8, sample_method=method, note_events=True, close_at_end=True, **kw)
    assert m._shared.infer.maxB == 128 and sum(LENGTHS) == 320          # three engine batches, songs 2 and 4 straddle an edge
    assert len(got) == len(LENGTHS) and all(sorted(d) == sorted(KEYS + ["events", "programs"]) for d in got)
    spanning = across_batches = notes = 0
    first = np.cumsum(LENGTHS) - LENGTHS
    for i, (d, c) in enumerate(zip(got, closed)):
        n = LENGTHS[i]
        assert d["events"].dtype == ev.RECORD and np.array_equal(d["notes"], c["notes"])
        for have, close in ((d, False), (c, True)):
            want = ev.note_events(have["notes"], have["velocity"], have["starts"], [n], s, device=False, close_at_end=close)[0]
            assert np.array_equal(have["events"], want), "song %d (%s), close_at_end=%s" % (i, method, close)
        assert d["programs"] == ev.vote_for_programs(d["instr"], [n], s)[0] and len(d["programs"]) == V
        e = c["events"]
        spanning += int(np.sum(e["start"] // ticks != (e["end"] - 1) // ticks))
        for edge in (128, 256):          # the song's window that opens an engine batch
            w = edge - first[i]
            if 0 < w < n:
                across_batches += int(np.sum((e["start"] < w * ticks) & (e["end"] > w * ticks)))
        notes += len(d["events"])
        # the file of the song: what was extracted is what is read back
        tracks = [d["events"][d["events"]["voice"] == v] for v in range(V)]
        back = mf.read_midi(io.BytesIO(mf.to_bytes(tracks, d["programs"], 100, s["SMALLEST_NOTE"])))
        assert [t["program"] for t in back["tracks"][1:]] == d["programs"]
        assert sum(len(t["notes"]) for t in back["tracks"]) == len(d["events"])
    print("%d notes, %d span a window boundary, %d an engine batch's edge" % (notes, spanning, across_batches))
    assert notes > 0, "the model decodes no note"
    # (the entry point runs once over all windows, so an engine batch's edge is a window boundary like any other to it; whether this
    # untrained model holds a note across one is printed, not asked for)
    assert spanning > 0, "no note spans a window boundary: the test shows nothing"


def test_without_note_events_the_dicts_are_what_they_were(small_model):
    s, m, xs, x_all, orig = small_model
    dec = m.decoder
    plain = dec.predict_songs(xs, 8)
    assert all(sorted(d) == KEYS for d in plain)
    assert all(sorted(d) == sorted(KEYS + ["metrics"]) for d in dec.predict_songs(xs, 8, originals=split(orig)))
    assert all(sorted(d) == KEYS for d in dec.predict_songs(xs, 8, note_events=False, close_at_end=True))
    with_events = dec.predict_songs(xs, 8, note_events=True)
    for a, b in zip(plain, with_events):
        assert all(np.array_equal(a[k], b[k]) for k in KEYS)
    assert dec.predict_songs([], note_events=True) == []
    try:
        dec.sample_settings = dict(s, SMALLEST_NOTE=0)
        with pytest.raises(ValueError):
            dec.predict_songs(xs, 8, note_events=True)
        assert all(sorted(d) == KEYS for d in dec.predict_songs(xs[:2], 8))          # (not read without note_events)
    finally:
        dec.sample_settings = s
