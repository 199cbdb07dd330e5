"""decoder.predict_songs: whole songs decoded as one pass and finished on the device (mvae_recon_songs behind the decode) against the
host route - predict_indices on the same decoder inputs, packers.process_decoder_indices song by song, and the reference's count
arithmetic (vae_evaluation.py:2211-2236, :2380-2397; as tests/golden/make_recon_fixtures.py restates it) in NumPy on one-hot rolls.

The device reads the very bytes predict_indices brings to the host; velocities after the rules are those floats or zeros, note starts
bytes, counts integers, every metric one integer or one division of two: everything is EQUAL, no tolerance.  The 320 windows take
three engine batches of 128 and two songs straddle a batch edge: an implementation that restarts the rule per window or per engine
batch fails here."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import packers
from midi_vae_amd import reconstruction as rec
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE

pytestmark = pytest.mark.gpu
LENGTHS = [1, 5, 130, 60, 124]


@pytest.fixture(scope="module")
def small_model():
    """the small model of test_latent_sweep_gpu.py; its forward-only engine holds 128 windows"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MVAE_INFER_BATCH", "128")
        s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=32, input_length=8, output_length=8, max_voices=2, batch_size=8)
        m = VAE().create(compute_dtype="f32", seed=4, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z) == (16, 2, 32) and m._shared.infer_cap == 128
    assert s["meta_velocity"] and s["meta_instrument"] and not s["meta_held_notes"] and s["include_silent_note"]
    rng = np.random.default_rng(17)
    xs = [packers.prepare_decoder_input(s, rng.standard_normal((n, 32)) * 2.0, 0, np.zeros((n, s["signature_vector_length"])), None)
          for n in LENGTHS]
    x_all = [np.concatenate([x[k] for x in xs], 0) for k in range(len(xs[0]))]
    # originals: what the model decodes with about a third of the rows replaced by a random column (the silent one included)
    notes = m.decoder.predict_note_indices(x_all, 8)
    width = s["high_crop"] - s["low_crop"] + 1
    orig = np.where(rng.random(notes.shape) < 1 / 3, rng.integers(0, width, notes.shape), notes).astype(np.uint8)
    return s, m, xs, x_all, orig


def split(a):
    first = np.cumsum(LENGTHS) - LENGTHS
    return [a[lo:lo + n] for lo, n in zip(first, LENGTHS)]


def host_metrics(s, Y_pred, D_pred, orig, T):
    """the reference's arithmetic on the one-hot rolls of one song"""
    n_pitch, windows = Y_pred.shape[1], len(orig)
    Y = np.eye(n_pitch + 1)[orig.reshape(-1)]
    song = Y[:, :n_pitch]
    unique, counts = np.unique(song * 2 + Y_pred, return_counts=True)
    difference = dict(zip(unique.tolist(), counts.tolist()))
    original, predicted = int(np.count_nonzero(song)), int(np.count_nonzero(Y_pred))
    start = D_pred == 0
    to_predicted = int(np.sum(start & (Y_pred.sum(1) == 0)))
    to_original = int(np.sum(start & (Y[:, -1] == 1)))
    return dict(total_original_notes=original, total_predicted_notes=predicted,
                pitch_reconstruction_accuracy=difference.get(3, 0) / original if original else float("nan"),
                not_predicted_notes=difference.get(2, 0), new_predicted_notes=difference.get(1, 0),
                predicted_note_start_to_original_errors=to_original / (windows * T),
                predicted_note_start_to_predicted_errors=to_predicted / (windows * T))


def assert_song(got, s, indices, orig, T, what):
    """one song of predict_songs against process_decoder_indices on the host's indices"""
    Y, I, V, D, _ = packers.process_decoder_indices(s, indices)
    n = len(orig)
    assert np.array_equal(got["notes"], indices["notes"]) and np.array_equal(got["instr"], indices["instr"]), what
    assert got["velocity"].dtype == np.float32 and np.array_equal(got["velocity"].astype(np.float64).reshape(-1), V), what
    assert np.array_equal(got["starts"].reshape(-1), D), what
    assert np.array_equal(np.eye(I.shape[2])[got["instr"]], I), what
    want = host_metrics(s, Y, D, orig, T)
    assert tuple(got["metrics"]) == rec.METRICS == tuple(want)
    for k in want:
        assert got["metrics"][k] == want[k] or (np.isnan(got["metrics"][k]) and np.isnan(want[k])), (what, k, got["metrics"][k], want[k])
    assert got["counts"].shape == (n, 8) and np.array_equal(got["counts"].sum(0)[[0, 1, 3, 4]],
                                                            [want[k] for k in ("total_original_notes", "total_predicted_notes",
                                                                               "not_predicted_notes", "new_predicted_notes")])
    return V


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_predict_songs(small_model, method, kw):
    s, m, xs, x_all, orig = small_model
    dec, T = m.decoder, 16
    got = dec.predict_songs(xs, 8, sample_method=method, originals=split(orig), **kw)
    assert m._shared.infer.maxB == 128 and sum(LENGTHS) == 320          # three engine batches, songs 2 and 4 straddle an edge
    assert len(got) == len(LENGTHS) and all(sorted(d) == ["counts", "instr", "metrics", "notes", "starts", "velocity"] for d in got)

    host = dec.predict_indices(x_all, 8, sample_method=method, **kw)
    carried = 0
    for i, (d, o) in enumerate(zip(got, split(orig))):
        indices = {k: split(v)[i] for k, v in host.items()}
        V = assert_song(d, s, indices, o, T, "song %d (%s)" % (i, method))
        per_window = np.concatenate([packers.process_decoder_indices(s, {k: v[w:w + 1] for k, v in indices.items()})[2]
                                     for w in range(len(o))])
        carried += bool(np.any(per_window != V))
    print("songs whose velocities differ from the per-window rule: %d of %d" % (carried, len(LENGTHS)))
    assert carried >= 1, "no song needs the state carried across its windows: the test shows nothing"
    assert sum(d["counts"][:, 1].sum() for d in got) > 0, "the model decodes no note"

    if method == "argmax":          # a song decoded alone: the same song
        for i, (d, x, o) in enumerate(zip(got, xs, split(orig))):
            assert_song(d, s, dec.predict_indices(x, 8), o, T, "song %d alone" % i)
    # without originals: no metrics, the counts that need none unchanged; the mean row of the report
    plain = dec.predict_songs(xs, 8, sample_method=method, **kw)
    for a, b in zip(plain, got):
        assert "metrics" not in a and np.array_equal(a["velocity"], b["velocity"]) and np.array_equal(a["starts"], b["starts"])
        assert np.array_equal(a["counts"][:, [1, 5, 6]], b["counts"][:, [1, 5, 6]]) and np.all(a["counts"][:, [0, 2, 3, 7]] == 0)
    mean = rec.mean_metrics([d["metrics"] for d in got])
    assert mean["total_predicted_notes"] == sum(d["metrics"]["total_predicted_notes"] for d in got) / len(got)


def test_predict_songs_refuses_what_it_cannot_do(small_model):
    s, m, xs, x_all, orig = small_model
    dec = m.decoder
    assert dec.predict_songs([]) == []
    with pytest.raises(ValueError):
        dec.predict_songs(xs, originals=split(orig)[:4])
    with pytest.raises(ValueError):
        dec.predict_songs(xs, originals=[o[:, :8] for o in split(orig)])
    with pytest.raises(ValueError):
        dec.predict_songs(xs + [[a[:0] for a in xs[0]]])
    with pytest.raises(ValueError):
        dec.predict_songs(xs, seed=3)
    try:
        dec.sample_settings = dict(s, max_voices=4)
        with pytest.raises(ValueError):
            dec.predict_songs(xs)
        dec.sample_settings = dict(s, meta_instrument=False)
        with pytest.raises(NotImplementedError) as refused:
            dec.predict_songs(xs)
        with pytest.raises(NotImplementedError) as host:
            packers.process_decoder_indices(dict(s, meta_instrument=False), dict(notes=orig))
        assert str(refused.value) == str(host.value)
    finally:
        dec.sample_settings = s
