#!/usr/bin/env python3
"""Generate tests/golden/import_rolls.npz: what the reference's own load_rolls (import_midi.py:13-350) makes of synthetic songs.

Runs ONLY where the reference is present (make_fixtures.REF).  import_midi is imported with the stub modules of make_fixtures.py; the
``pretty_midi`` stub is a FEEDING one: ``PrettyMIDI(path)`` looks the path up in a table of synthetic songs and offers what load_rolls
reads - ``instruments`` (``program``, ``notes`` with start / end in seconds as float64, pitch, velocity; ``get_piano_roll(fs)``),
``time_signature_changes``, ``get_tempo_changes()`` and ``get_end_time()``.  ``get_piano_roll`` is this file's ASSUMPTION of
pretty_midi's (128 x int(fs * latest end) frames, every note adding its velocity to int(start * fs):int(end * fs) of its pitch); it
only decides the ORDER of the tracks, and no two tracks of a song have equal cell counts.  Only data is written: the songs and the six
values load_rolls returned for each.

  python tests/golden/make_import_fixtures.py

Three groups, by setting the globals of the imported reference module: ``a`` MAXIMAL_NUMBER_OF_VOICES_PER_TRACK 1, windows of 64 rows;
``b`` 2 / 24; ``c`` 1 / 8 (two ticks a window).  Every group holds the hand-made songs below and seeded random ones.  The assertions at
the end keep the fixture from going soft (see ``POINTS``).
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_fixtures as mfx  # noqa: E402

GROUPS = (("a", 1, 64), ("b", 2, 24), ("c", 1, 8))
TICK = 0.125          # seconds at 120 bpm and SMALLEST_NOTE 16: exact in binary, so k + 0.5 ticks are exact too
POINTS = ("override", "silent_voice", "cropped_held", "zero_length_strikes", "two_velocities", "velocity_zero", "half_even", "half_odd",
          "off_grid_dropped", "off_grid_kept", "middle_tempo", "fewer_tracks", "more_tracks", "none", "no_padding")

SONGS = {}


def feeding_pretty_midi():
    pm = types.ModuleType("pretty_midi")

    class Note(object):
        def __init__(self, velocity, pitch, start, end):
            self.velocity, self.pitch, self.start, self.end = velocity, pitch, start, end

    class Instrument(object):
        def __init__(self, program, notes):
            self.program = program
            self.notes = [Note(int(v), int(p), float(a), float(b)) for a, b, p, v in notes]

        def get_piano_roll(self, fs=100):
            if not self.notes:
                return np.zeros((128, 0))
            roll = np.zeros((128, int(fs * max(n.end for n in self.notes))))
            for n in self.notes:
                roll[n.pitch, int(n.start * fs):int(n.end * fs)] += n.velocity
            return roll

    class PrettyMIDI(object):
        def __init__(self, path):
            song = SONGS[path]
            if song is None:
                raise ValueError("unreadable")
            self.instruments = [Instrument(prog, notes) for prog, notes in song["instruments"]]
            self.time_signature_changes = []
            self._song = song

        def get_tempo_changes(self):
            return np.array(self._song["tempo_times"], np.float64), np.array(self._song["tempo_bpm"], np.float64)

        def get_end_time(self):
            return self._song["end_time"]

    pm.PrettyMIDI, pm.Instrument, pm.Note = PrettyMIDI, Instrument, Note
    return pm


def song(instruments, tempo_times=(0.0,), tempo_bpm=(120.0,), end_time=None):
    """instruments: [(program, [(start s, end s, pitch, velocity)])]"""
    instruments = [(int(p), [tuple(n) for n in notes]) for p, notes in instruments]
    if end_time is None:
        end_time = max([n[1] for _, notes in instruments for n in notes] + [0.0])
    return dict(instruments=instruments, tempo_times=list(tempo_times), tempo_bpm=list(tempo_bpm), end_time=float(end_time))


def hand_made():
    """name -> song; N() takes times in ticks of 0.125 s"""
    N = lambda a, b, pitch, vel: (a * TICK, b * TICK, pitch, vel)
    out = {}
    # two tracks, four voices: the first (a three-note chord, most cells) gets the two free voices by the override; the second has a
    # pitch above the crop held over three ticks, a zero-length note striking a held row, two records of one key, a note of velocity 0
    out["override"] = song([
        (0, [N(0, 8, 60, 100), N(0, 8, 64, 90), N(0, 8, 67, 80), N(8, 20, 62, 70), N(10, 16, 65, 60), N(12, 14, 69, 50), N(20, 30, 50, 64)]),
        (40, [N(0, 3, 100, 77), N(4, 12, 55, 88), N(8, 8, 55, 33), N(14, 18, 48, 50), N(14, 16, 48, 90), N(20, 24, 52, 0), N(25, 29, 20, 99)]),
    ])
    # one track whose two notes of ONE pitch overlap: concurrent 2, one distinct pitch - its second voice is chosen and never sounds
    out["silent_voice"] = song([(5, [N(0, 6, 60, 80), N(3, 9, 60, 70), N(10, 12, 62, 60), N(16, 31, 64, 50)])])
    # starts on k + 0.5 ticks of both parities, notes off the grid: shorter than a tick (dropped), longer (kept); ends at 4.0 s = 32
    # ticks = exactly two windows of 64 rows: no padding
    out["grid"] = song([
        (10, [N(2.5, 5, 60, 80), N(3.5, 6, 64, 81), N(6.5, 7.5, 58, 82), N(7.5, 8.5, 57, 83), N(10.3, 10.45, 70, 84), N(12.3, 14.2, 72, 85),
              N(14.5, 14.5, 40, 86), N(20, 32, 45, 87)]),
        (20, [N(0, 4, 30, 60), N(15.3, 15.9, 33, 61), N(16.004, 16.4, 35, 62), N(28, 32, 36, 63)]),
    ])
    # three tempi, the longest part in the middle (2 s .. 10 s at 120 bpm): notes before, across and after it are cut
    out["middle_tempo"] = song([
        (1, [(0.5, 1.0, 60, 80), (1.5, 2.5, 61, 80), (2.0, 3.0, 62, 81), (4.0, 5.5, 64, 82), (9.0, 10.0, 65, 83), (9.5, 10.5, 66, 84), (11.0, 11.5, 67, 85)]),
        (2, [(2.25, 2.75, 40, 70), (3.0, 9.0, 43, 71), (5.0, 6.0, 47, 72)]),
    ], tempo_times=(0.0, 2.0, 10.0), tempo_bpm=(100.0, 120.0, 90.0), end_time=12.0)
    # six tracks of different sizes, chords in two of them
    out["more_tracks"] = song([
        (8 * k, [N(4 * i + k, 4 * i + k + 2 + (k % 3), 40 + 5 * k + (i % 4), 30 + 10 * k + i) for i in range(10 - k)] +
         ([N(2 * i, 2 * i + 3, 70 + k, 100) for i in range(4)] if k in (1, 4) else []))
        for k in range(6)])
    # monophonic tracks inside the crop, on the grid, every track with clearly fewer cells than the one before: what a file round trip
    # can reproduce (one voice per track).  Repeated pitches back to back, gaps, a note of velocity 0, a song's end inside a window
    out["mono4"] = song([
        (0, [N(2 * i, 2 * i + 2, 60 + (i // 2) % 5, 40 + 4 * i) for i in range(20)]),
        (24, [N(3 * i, 3 * i + 2, 50 + i % 3, 0 if i == 4 else 100 - 3 * i) for i in range(11)]),
        (40, [N(5 * i + 1, 5 * i + 3, 45 - i, 64) for i in range(7)]),
        (73, [N(7, 9, 30, 127), N(9, 10, 30, 1), N(30, 33, 83, 90)]),
    ])
    out["mono2"] = song([(19, [N(i, i + 1, 24 + i, 10 + i) for i in range(0, 32, 1)]), (56, [N(4 * i, 4 * i + 3, 70, 90) for i in range(6)])])
    # nothing usable: every note lies outside the longest steady part
    out["none_cut"] = song([(0, [(0.0, 0.5, 60, 80)]), (1, [(9.0, 9.5, 62, 80)])], tempo_times=(0.0, 1.0, 8.0), tempo_bpm=(120.0, 100.0, 120.0),
                           end_time=9.5)
    out["none_unreadable"] = None
    out["none_empty"] = song([])
    return out


def random_song(rng):
    tracks = int(rng.integers(1, 7))
    ticks = int(rng.integers(12, 120))
    instruments = []
    for k in range(tracks):
        depth = int(rng.integers(1, 6))
        notes = []
        for _ in range(int(rng.integers(3, 30))):
            a = float(rng.integers(0, ticks)) + float(rng.choice([0.0, 0.0, 0.0, 0.5, 0.3, 0.004]))
            d = float(rng.choice([0.0, 0.4, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0]))
            pitch = int(rng.integers(18, 100)) if rng.random() < 0.3 else int(rng.integers(40, 80))
            vel = 0 if rng.random() < 0.05 else int(rng.integers(1, 128))
            for j in range(int(rng.integers(1, depth + 1))):          # a chord, sometimes on one pitch twice
                notes.append((a * TICK, min(a + d + j * float(rng.choice([0.0, 1.0])), ticks) * TICK, min(pitch + int(rng.choice([0, 3, 4, 7])) * j, 127), vel))
        notes = [n for n in notes if n[1] >= n[0]]
        instruments.append((int(rng.integers(0, 128)), notes))
    return song(instruments)


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    mfx._stub_modules()
    sys.modules["pretty_midi"] = feeding_pretty_midi()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings
    import import_midi as ref
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions", "import_midi"):
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)
    from midi_vae_amd import midi_import as mi          # (for the assertions only: what is written is the reference's)

    V = int(settings.max_voices)
    low, high = int(settings.low_crop), int(settings.high_crop)
    thr = float(settings.velocity_threshold_such_that_it_is_a_played_note)
    assert (V, int(settings.SMALLEST_NOTE), low, high, thr, float(settings.MAX_VELOCITY)) == (4, 16, 24, 84, 0.5, 127.0)
    assert not settings.include_only_monophonic_instruments and not settings.attach_instruments and not settings.song_completion
    assert settings.include_silent_note and not settings.save_preprocessed_midi
    base = dict(max_voices=V, low_crop=low, high_crop=high, include_silent_note=True, SMALLEST_NOTE=int(settings.SMALLEST_NOTE),
                velocity_threshold_such_that_it_is_a_played_note=thr, instrument_attach_method=str(settings.instrument_attach_method),
                attach_instruments=False, song_completion=False, include_only_monophonic_instruments=False)
    out = {"s_" + k: np.asarray(v) for k, v in base.items()}
    out["groups"] = np.array([g for g, _, _ in GROUPS])
    rng = np.random.default_rng(20261020)
    hand = hand_made()
    seen = dict.fromkeys(POINTS, 0)

    for group, M, length in GROUPS:
        ref.MAXIMAL_NUMBER_OF_VOICES_PER_TRACK, ref.input_length, ref.output_length = M, length, length
        s = dict(base, MAXIMAL_NUMBER_OF_VOICES_PER_TRACK=M, input_length=length, output_length=length)
        out["%s_max_per_track" % group], out["%s_length" % group] = np.asarray(M), np.asarray(length)
        songs = list(hand.items())
        while len(songs) < len(hand) + 6:
            cand = random_song(rng)
            cells = [mi.piano_roll_cells(np.array(n, np.float64).reshape(-1, 4)) for _, n in cand["instruments"]]
            if len(set(cells)) == len(cells):          # ties in argsort are not pinned
                songs.append(("random%d" % len(songs), cand))
        out["%s_names" % group] = np.array([name for name, _ in songs])
        for i, (name, sg) in enumerate(songs):
            key = "%s/%s" % (group, name)
            SONGS[key] = sg
            X, Y, I, tempo, Vr, D = ref.load_rolls("%s/" % group, name)
            pre = "%s_%d_" % (group, i)
            out[pre + "unreadable"] = np.asarray(sg is None)
            out[pre + "none"] = np.asarray(X is None)
            if sg is not None:
                rows = [(k, a, b, p, v) for k, (_, notes) in enumerate(sg["instruments"]) for a, b, p, v in notes]
                out[pre + "notes"] = np.array(rows, np.float64).reshape(-1, 5)
                out[pre + "programs"] = np.array([p for p, _ in sg["instruments"]], np.int32)
                out[pre + "tempo_times"], out[pre + "tempo_bpm"] = np.array(sg["tempo_times"], np.float64), np.array(sg["tempo_bpm"], np.float64)
                out[pre + "end_time"] = np.float64(sg["end_time"])
            if X is None:
                seen["none"] += 1
                assert Y is None and I is None and tempo is None and Vr is None and D is None
                continue
            assert X.dtype == Y.dtype == Vr.dtype == D.dtype == np.float64 and X.shape == Y.shape == (len(Vr), length, high - low + 1)
            # X and Y are 0 / 1 and X is Y (no song_completion): kept as bytes, Y only; the tests widen them again
            assert np.array_equal(X, Y) and np.all((Y == 0) | (Y == 1))
            out[pre + "Y"], out[pre + "I"], out[pre + "tempo"], out[pre + "V"], out[pre + "D"] = Y.astype(np.uint8), I, np.float64(tempo), Vr, D.astype(np.uint8)
            print("group %s %-16s %3d windows" % (group, name, len(Y)))

            # ---- what this song shows ----
            cells = [mi.piano_roll_cells(np.array(n, np.float64).reshape(-1, 4)) for _, n in sg["instruments"]]
            table = mi.quantise(dict(instruments=[dict(program=p, notes=np.array(n, np.float64).reshape(-1, 4)) for p, n in sg["instruments"]],
                                     tempo_changes=(np.array(sg["tempo_times"]), np.array(sg["tempo_bpm"])), end_time=sg["end_time"]), s)
            r = mi.rolls_from_notes([table], s, device=False, T=V)
            conc, slots, sv = r["concurrent"][0], r["slots"][0], r["slot_voice"][0]
            notes = table["notes"]
            idx, held, raw = r["idx"].reshape(-1), r["held"].reshape(-1), r["vel_raw"].reshape(-1)
            tracks = len(cells)
            seen["fewer_tracks"] += tracks < V
            seen["more_tracks"] += tracks > V
            seen["override"] += int(np.sum(slots == 0) > M)
            for j in range(V):
                if slots[j] >= 0:
                    n_t = notes[notes["track"] == slots[j]]
                    most = max((len(set(n_t["pitch"][(n_t["start"] <= k) & (n_t["end"] > k)].tolist())) for k in range(table["ticks"])), default=0)
                    seen["silent_voice"] += sv[j] >= most
            seen["cropped_held"] += int(np.any((idx == high - low) & (held == 1))) and int(np.any((idx == high - low) & (raw > 0)))
            zero = notes[notes["start"] == notes["end"]]
            for z in zero:
                longer = notes[(notes["track"] == z["track"]) & (notes["pitch"] == z["pitch"]) & (notes["start"] < z["start"]) & (notes["end"] > z["start"])]
                seen["zero_length_strikes"] += len(longer) > 0
            keys = np.stack([notes["track"].astype(np.int64), notes["start"], notes["pitch"]], 1)
            same = np.all(keys[1:] == keys[:-1], 1) if len(keys) > 1 else np.zeros(0, bool)
            seen["two_velocities"] += int(np.any(same & (notes["velocity"][1:] != notes["velocity"][:-1])))
            seen["velocity_zero"] += int(np.any(notes["velocity"] == 0))
            fs = 8.0
            for _, ns in sg["instruments"]:
                for a, b, _, _ in ns:
                    x, y = (a - 0.0) * fs, b * fs
                    if len(sg["tempo_times"]) > 1:
                        continue
                    if x - np.floor(x) == 0.5:
                        seen["half_even" if int(np.floor(x)) % 2 == 0 else "half_odd"] += 1
                    if x - round(x) >= 10e-3:
                        seen["off_grid_dropped" if round(y) - round(x) < 1 else "off_grid_kept"] += 1
            if len(sg["tempo_times"]) > 2:
                parts = np.diff(list(sg["tempo_times"]) + [sg["end_time"]])
                seen["middle_tempo"] += 0 < int(np.argmax(parts)) < len(parts) - 1
            seen["no_padding"] += int((table["ticks"] * V) % length == 0)
            if (table["ticks"] * V) % length == 0:
                assert np.all(Y[..., -1] == 1), "the X[-0:] quirk is gone"
    missing = [k for k in POINTS if not seen[k]]
    assert not missing, "the fixture lost its point: %r" % (missing,)
    print({k: int(v) for k, v in seen.items()})

    path = os.path.join(HERE, "import_rolls.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
