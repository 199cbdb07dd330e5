#!/usr/bin/env python3
"""Generate tests/golden/midi_events.npz: the notes the reference's own rolls_to_midi (midi_functions.py:57-137) makes of whole songs.

Runs ONLY where the reference is present (make_fixtures.REF).  midi_functions is imported with the stub modules of make_fixtures.py; the
``pretty_midi`` stub is given RECORDING PrettyMIDI, TimeSignature, Instrument and Note classes (``write`` does nothing, the save folder
is a temporary directory), and rolls_to_midi is called once per song in three passes: with V and D (the held roll), with V and
``held_notes_roll=None`` (the tick rule), and with neither (velocity 80).  What the stub recorded is the fixture: per note the start and
end tick - recovered from the times as round(time * tempo / 60), residue below 1e-9 - the pitch, the voice (the instrument's place)
and the velocity.  Only data is written: those notes, the programs, the tempo the stub was given, and the
inputs that tests/golden/recon.npz does not hold already.

  python tests/golden/make_midi_fixtures.py

Group ``a`` (T = 64 rows = 16 ticks x 4 voices): the songs of tests/golden/recon.npz - idx, vel, and its note starts as D - then
hand-made songs: a note held across three windows beside a note still sounding on the song's last row (dropped), a held flag set
on a row whose pitch changed, a silent row between two rows of one pitch; and one window of chosen velocities: exactly the threshold,
1.0, 1.5 (clamped to 127), multiples of 1/8 and values under the threshold (velocity 0).  Group ``b`` (T = 24 rows = 6 ticks x 4
voices): songs whose window boundaries are no multiples of SMALLEST_NOTE, so that under the tick rule ``i % 16`` falls inside windows
and notes span them.  Assertions keep the fixture from going soft: every pass has notes spanning a window boundary, at least one open
note is dropped, one velocity is clamped, one note has velocity 0, the held pass and the tick pass differ.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402
from make_descriptor_fixtures import random_walk_windows  # noqa: E402

PASSES = ("held", "tick", "plain")
BPM = 120


def recording_pretty_midi():
    """the stub's classes: what rolls_to_midi builds is kept, nothing is written"""
    pm = types.ModuleType("pretty_midi")

    class PrettyMIDI(object):
        last = None

        def __init__(self, initial_tempo=120.0, resolution=220):
            self.initial_tempo, self.resolution = initial_tempo, resolution
            self.time_signature_changes, self.instruments = [], []
            PrettyMIDI.last = self

        def write(self, path):
            self.path = path

    class TimeSignature(object):
        def __init__(self, numerator, denominator, time):
            self.numerator, self.denominator, self.time = numerator, denominator, time

    class Instrument(object):
        def __init__(self, program, is_drum=False, name=""):
            self.program, self.notes = program, []

    class Note(object):
        def __init__(self, velocity, pitch, start, end):
            self.velocity, self.pitch, self.start, self.end = velocity, pitch, start, end

    pm.PrettyMIDI, pm.TimeSignature, pm.Instrument, pm.Note = PrettyMIDI, TimeSignature, Instrument, Note
    return pm


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    mfx._stub_modules()
    pm = sys.modules["pretty_midi"] = recording_pretty_midi()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings
    import midi_functions as ref
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions"):
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)

    V, SN = int(settings.max_voices), int(settings.SMALLEST_NOTE)
    low, high = int(settings.low_crop), int(settings.high_crop)
    thr = float(settings.velocity_threshold_such_that_it_is_a_played_note)
    n_pitch = high - low
    assert (V, SN, n_pitch, thr, float(settings.MAX_VELOCITY), bool(settings.include_silent_note)) == (4, 16, 60, 0.5, 127.0, True)
    programs = [0, 40, 56, 32]
    tempo = BPM * (SN / 4)
    save_folder = tempfile.mkdtemp(prefix="mvae_midi_") + os.sep
    rng = np.random.default_rng(20261022)

    def reference_notes(idx, vel, held):
        """rolls_to_midi on ONE song's windows: [(start, end, pitch, voice, velocity)] in the order (voice, appended)"""
        rows = idx.reshape(-1)
        Y = np.zeros((rows.size, n_pitch))
        sounds = rows < n_pitch
        Y[np.nonzero(sounds)[0], rows[sounds]] = 1
        ref.rolls_to_midi(Y, programs, save_folder, "song", BPM, None if vel is None else vel.astype(np.float64).reshape(-1),
                          None if held is None else held.astype(np.float64).reshape(-1))
        midi = pm.PrettyMIDI.last
        assert midi.initial_tempo == tempo and midi.resolution == 1000 and [i.program for i in midi.instruments] == programs
        ts = midi.time_signature_changes
        assert len(ts) == 1 and (ts[0].numerator, ts[0].denominator, ts[0].time) == (4, 4, 0)
        out = []
        for voice, instrument in enumerate(midi.instruments):
            for note in instrument.notes:
                ticks = []
                for t in (note.start, note.end):
                    x = t * tempo / 60
                    assert abs(x - round(x)) < 1e-9, (t, x)
                    ticks.append(int(round(x)))
                assert isinstance(note.velocity, int) and ticks[0] < ticks[1]
                out.append((ticks[0], ticks[1], int(note.pitch), voice, note.velocity))
            starts = [n[0] for n in out if n[3] == voice]
            assert starts == sorted(starts)
        return out

    def velocities(n, T):
        v = rng.random((n, T))
        return np.where(rng.random((n, T)) < 1 / 3, np.round(v * 8) / 8, v).astype(np.float32)

    # ---- group a: T = 64 --------------------------------------------------------------------------------------------------------
    T = 64
    z = np.load(os.path.join(HERE, "recon.npz"))
    songs_a, lo = [], 0
    for m in z["lengths"].tolist():
        songs_a.append([z["idx"][lo:lo + m].copy(), z["vel"][lo:lo + m].copy(), z["starts"][lo:lo + m].copy()])
        lo += m
    silent = n_pitch
    # four windows.  Voice 0: column 10 through windows 0..2, held - one note across three windows; voice 1: column 20 from tick 8 of
    # window 3 to the song's last row - dropped; voice 2: columns 5 and 7 in turn, every row held - the flag on a changed pitch starts
    # a note; voice 3: column 30, a silent row, column 30, held - the silent row released it
    idx, vel, held = np.full((4, T), silent, np.uint8), velocities(4, T), np.ones((4, T), np.uint8)
    idx[0:3, 0::V] = 10
    idx[3, 8 * V + 1::V] = 20
    idx[:, 2::V] = np.where(np.arange(4 * 16) % 4 < 2, 5, 7).reshape(4, 16)
    voice3 = np.full(4 * 16, 30)
    voice3[1::3] = silent
    idx[:, 3::V] = voice3.reshape(4, 16)
    held[0, 0] = 0
    songs_a.append([idx, vel, held])
    # one window of chosen velocities on changing pitches, nothing held: exactly the threshold, 1.0, 1.5, eighths, quiet ones
    idx = (np.arange(T) * 7 % n_pitch).astype(np.uint8).reshape(1, T)
    vel = np.tile(np.array([0.5, 1.0, 1.5, 0.625, 0.875, 0.25, 0.125, 0.0, 0.75, 0.5625, 1.25, 0.4375, 0.9375, 0.375, 2.0, 0.6875], np.float32), 4).reshape(1, T)
    songs_a.append([idx, vel, np.zeros((1, T), np.uint8)])

    # ---- group b: T = 24, six ticks a window ------------------------------------------------------------------------------------
    Tb = 24
    songs_b = []
    for m in (1, 5, 8, 3):
        idx = random_walk_windows(rng, m, Tb, V, n_pitch, 0.2, 0.6)
        songs_b.append([idx, velocities(m, Tb), (rng.random((m, Tb)) < 0.7).astype(np.uint8)])
    idx = np.full((7, Tb), silent, np.uint8)          # voice 0 on one pitch through 42 ticks: struck again on ticks 16 and 32 only
    idx[:, 0::V] = 12
    songs_b.append([idx, velocities(7, Tb), np.ones((7, Tb), np.uint8)])

    out = dict(programs=np.array(programs, np.int32), bpm=np.float64(BPM), tempo=np.float64(tempo), resolution=np.int32(1000),
               s_max_voices=np.asarray(V), s_low_crop=np.asarray(low), s_high_crop=np.asarray(high),
               s_include_silent_note=np.asarray(bool(settings.include_silent_note)),
               s_velocity_threshold_such_that_it_is_a_played_note=np.asarray(thr), s_SMALLEST_NOTE=np.asarray(SN))
    dropped, spans = 0, dict.fromkeys(PASSES, 0)
    for group, songs, Tg in (("a", songs_a, T), ("b", songs_b, Tb)):
        ticks = Tg // V
        tables = {}
        for name in PASSES:
            notes, offsets, spanning = [], [0], 0
            for idx, vel, held in songs:
                got = reference_notes(idx, None if name == "plain" else vel, held if name == "held" else None)
                for voice in range(V):
                    offsets.append(offsets[-1] + sum(1 for n in got if n[3] == voice))
                spanning += sum(1 for n in got if n[0] // ticks != (n[1] - 1) // ticks)
                notes += got
            spans[name] += spanning          # (16 ticks a window in group a: under the tick rule nothing spans there)
            tables[name] = np.array(notes, np.int32).reshape(-1, 5)
            out["%s_%s_notes" % (group, name)] = np.ascontiguousarray(tables[name].T)          # (5, notes): the columns compress better
            out["%s_%s_offsets" % (group, name)] = np.array(offsets, np.int32)
            print("group %s pass %-5s %5d notes, %4d span a window boundary" % (group, name, len(notes), spanning))
        assert not np.array_equal(tables["held"][:, :2], tables["tick"][:, :2]) or len(tables["held"]) != len(tables["tick"])
        assert np.any(tables["held"][:, 4] == 127) and np.any(tables["held"][:, 4] == 0) and np.all(tables["plain"][:, 4] == 80)
        for idx, _, _ in songs:
            dropped += int(np.sum(idx[-1, -V:] < n_pitch))
        # (the songs of recon.npz are not stored twice: group a's inputs are its idx, vel and starts followed by these)
        own = songs[len(z["lengths"]):] if group == "a" else songs
        out[group + "_idx"] = np.concatenate([s[0] for s in own], 0)
        out[group + "_vel"] = np.concatenate([s[1] for s in own], 0)
        out[group + "_held"] = np.concatenate([s[2] for s in own], 0)
        out[group + "_lengths"] = np.array([s[0].shape[0] for s in own], np.int64)
    assert all(spans[name] > 0 for name in PASSES), "a pass without a note that spans a window boundary: %r" % (spans,)
    assert dropped > 0, "no note is still sounding on a song's last row"
    a = out["a_held_notes"].T
    first_hand = int(out["a_held_offsets"][len(z["lengths"]) * V])
    assert (a[first_hand, 0], a[first_hand, 1], a[first_hand, 2], a[first_hand, 3]) == (0, 48, 10 + low, 0), "the three-window note"
    chosen = a[out["a_held_offsets"][(len(songs_a) - 1) * V]:]
    assert 127 in chosen[:, 4] and 0 in chosen[:, 4] and np.sum(chosen[:, 4] == 127) >= 3, "the chosen velocities lost their point"

    path = os.path.join(HERE, "midi_events.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "bytes:", os.path.getsize(path), "(recon.npz: %d)" % os.path.getsize(os.path.join(HERE, "recon.npz")))


if __name__ == "__main__":
    main()
