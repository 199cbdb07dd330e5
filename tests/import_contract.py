"""The contract of include/midivae_import.h as a table (no test lives here): one well-formed call of mvae_rolls_from_notes and every way
the header says a call is refused.  tests/test_midi_import_cpu.py runs all rows on addresses nothing maps - with no device a well-formed
call fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch; tests/test_midi_import_gpu.py runs
the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernels would stay inside the baseline's buffers (a value the kernels only
compare, a smaller extent).  Rows that would index past a buffer, divide by zero or follow a NULL pointer are CPU-only.

Also what the test files of the import share: the fixture (tests/golden/import_rolls.npz), seeded random songs and the settings."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import hiplib as hl
from midi_vae_amd import midi_import as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def settings(V=4, T=64, M=1, low=24, high=84, threshold=0.5, smallest_note=16, **more):
    return dict(dict(max_voices=V, low_crop=low, high_crop=high, include_silent_note=True, SMALLEST_NOTE=smallest_note,
                     velocity_threshold_such_that_it_is_a_played_note=threshold, instrument_attach_method="1hot-category",
                     attach_instruments=False, song_completion=False, include_only_monophonic_instruments=False,
                     MAXIMAL_NUMBER_OF_VOICES_PER_TRACK=M, input_length=T, output_length=T), **more)


def load_fixture():
    """dict group -> dict ``s`` (the settings of the group) and ``songs``: per song a dict ``name``, ``song`` (what read_song would
    return; None for the unreadable one) and ``want``: (X, Y, I, tempo, V, D) as the reference returned them, or six None"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "import_rolls.npz"))
    base = {k[2:]: z[k].item() for k in z.files if k.startswith("s_")}
    fx = {}
    for g in z["groups"].tolist():
        s = dict(base, MAXIMAL_NUMBER_OF_VOICES_PER_TRACK=int(z[g + "_max_per_track"]), input_length=int(z[g + "_length"]),
                 output_length=int(z[g + "_length"]))
        songs = []
        for i, name in enumerate(z[g + "_names"].tolist()):
            pre = "%s_%d_" % (g, i)
            song = None
            if not bool(z[pre + "unreadable"]):
                rows = z[pre + "notes"]
                song = dict(instruments=[dict(program=int(p), notes=np.ascontiguousarray(rows[rows[:, 0] == k, 1:]))
                                         for k, p in enumerate(z[pre + "programs"].tolist())],
                            tempo_changes=(z[pre + "tempo_times"], z[pre + "tempo_bpm"]), end_time=float(z[pre + "end_time"]))
            want = (None,) * 6
            if not bool(z[pre + "none"]):
                Y = z[pre + "Y"].astype(np.float64)          # (stored as bytes; X is Y: no song_completion)
                want = (Y, Y, z[pre + "I"], float(z[pre + "tempo"]), z[pre + "V"], z[pre + "D"].astype(np.float64))
            songs.append(dict(name=name, song=song, want=want))
        fx[g] = dict(s=s, songs=songs)
    return fx


def fixture_tables(group):
    """the quantised tables of a group's readable songs"""
    return [mi.quantise(x["song"], group["s"]) for x in group["songs"] if x["song"] is not None]


def random_tables(rng, n_songs, V, T, max_windows=5, ticks=None, max_tracks=6, depth=5):
    """seeded note tables as quantise returns them: 1..max_tracks tracks, chords up to ``depth`` deep - some on one pitch twice -
    zero-length notes, repeated keys, velocity 0, pitches on both sides of the crop, notes that run past the song's end"""
    tables = []
    for _ in range(n_songs):
        n = int(rng.integers(1, max_windows * T // V + 1)) if ticks is None else ticks
        tracks = int(rng.integers(1, max_tracks + 1))
        rec = []
        for k in range(tracks):
            for _ in range(int(rng.integers(0 if k else 1, 4 + n // 3))):
                a = int(rng.integers(0, n))
                pitch = int(rng.integers(0, 128)) if rng.random() < 0.2 else int(rng.integers(40, 70))
                for j in range(int(rng.integers(1, depth + 1))):
                    b = a + int(rng.choice([0, 1, 1, 2, 3, 5, 9, n]))
                    rec.append((a, b, min(pitch + j * int(rng.choice([0, 3, 4])), 127), 0 if rng.random() < 0.05 else int(rng.integers(1, 128)), k))
        notes = np.array(rec, mi.NOTE) if rec else np.zeros(0, mi.NOTE)
        notes = notes[np.lexsort((notes["pitch"], notes["start"], notes["track"]))]
        tables.append(dict(ticks=n, programs=[int(x) for x in rng.integers(0, 128, tracks)], tempo=120.0, notes=notes))
    return tables


E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
# the baseline: two songs (2 and 3 tracks, 20 and 9 ticks), windows of 16 rows
S, T, V, TRACKS, TICKS = 2, 16, 4, (2, 3), (20, 9)
WINDOWS = tuple(-(-t * V // T) for t in TICKS)
N_WINDOWS, N_TRACKS, CELLS, N_NOTES = sum(WINDOWS), sum(TRACKS), sum(a * b for a, b in zip(TRACKS, TICKS)), 12


def baseline_tables():
    """the baseline's songs: N_NOTES / 2 records each"""
    rng = np.random.default_rng(7)
    while True:
        tables = [random_tables(rng, 1, V, T, ticks=n, max_tracks=k)[0] for n, k in zip(TICKS, TRACKS)]
        if [len(t["programs"]) for t in tables] == list(TRACKS) and all(len(t["notes"]) >= N_NOTES // 2 for t in tables):
            break
    for t in tables:
        t["notes"] = t["notes"][:N_NOTES // 2]
    return tables


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'f32', 'i32'"""
    return hl.ImportArgs(notes=alloc("notes", (N_NOTES, 3), "i32"), note_off=alloc("note_off", (S + 1,), "i32"),
                         track_off=alloc("track_off", (S + 1,), "i32"), ticks=alloc("ticks", (S,), "i32"),
                         win_off=alloc("win_off", (S + 1,), "i32"), n_songs=S, n_notes=N_NOTES, n_tracks=N_TRACKS, n_windows=N_WINDOWS,
                         T=T, voices=V, max_per_track=1, pitch_base=24, n_pitch=60, silent=60, cells=CELLS, stride_t=1, stride_w=T,
                         threshold=0.5, workspace=alloc("workspace", (9 * CELLS + S + 1,), "i32", out=True),
                         idx=alloc("idx", (N_WINDOWS, T), "u8", out=True), held=alloc("held", (N_WINDOWS, T), "u8", out=True),
                         vel_raw=alloc("vel_raw", (N_WINDOWS, T), "u8", out=True), vel=alloc("vel", (N_WINDOWS, T), "f32", out=True),
                         concurrent=alloc("concurrent", (N_TRACKS,), "i32", out=True), slots=alloc("slots", (S * V,), "i32", out=True),
                         slot_voice=alloc("slot_voice", (S * V,), "i32", out=True))


def fake_alloc(name, shape, kind, out=False):
    """addresses nothing maps, one per buffer name (never dereferenced on the host)"""
    return 0x10000000 + 0x100000 * (sum(map(ord, name)) % 251)


def F(**fields):
    def mutate(a):
        for k, v in fields.items():
            setattr(a, k, v)
        return a
    return mutate


# (what is wrong, mutate(args) -> args or None for a NULL struct, the promised code, safe on a device)
ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("notes NULL with n_notes > 0", F(notes=None), E_ARG, False),
    ("note_off NULL", F(note_off=None), E_ARG, False),
    ("track_off NULL", F(track_off=None), E_ARG, False),
    ("ticks NULL", F(ticks=None), E_ARG, False),
    ("win_off NULL", F(win_off=None), E_ARG, False),
    ("workspace NULL", F(workspace=None), E_ARG, False),
    ("idx NULL", F(idx=None), E_ARG, False),
    ("held NULL", F(held=None), E_ARG, False),
    ("concurrent NULL with n_tracks > 0", F(concurrent=None), E_ARG, False),
    ("slots NULL", F(slots=None), E_ARG, False),
    ("slot_voice NULL", F(slot_voice=None), E_ARG, False),
    ("n_songs = 0", F(n_songs=0), E_ARG, True),
    ("n_songs = -1", F(n_songs=-1), E_ARG, False),
    ("n_windows = 0", F(n_windows=0), E_ARG, True),
    ("n_windows = -3", F(n_windows=-3), E_ARG, False),
    ("n_notes = -1", F(n_notes=-1), E_ARG, True),
    ("n_tracks = -1", F(n_tracks=-1), E_ARG, True),
    ("cells = -1", F(cells=-1), E_ARG, False),
    ("T = 0", F(T=0), E_ARG, False),
    ("T = -16", F(T=-16), E_ARG, False),
    ("stride_t = 0", F(stride_t=0), E_ARG, False),
    ("stride_w = -1", F(stride_w=-1), E_ARG, False),
    ("voices = 0", F(voices=0), E_ARG, False),
    ("voices = 9 (T = 18)", F(voices=9, T=18), E_ARG, False),
    ("T % voices != 0 (T = 14)", F(T=14), E_ARG, True),
    ("max_per_track = 0", F(max_per_track=0), E_ARG, True),
    ("pitch_base = -1", F(pitch_base=-1), E_ARG, True),
    ("n_pitch = 0", F(n_pitch=0), E_ARG, True),
    ("pitch_base + n_pitch = 129", F(pitch_base=69), E_ARG, True),
    ("silent = 256", F(silent=256), E_ARG, True),
    ("silent = -1", F(silent=-1), E_ARG, True),
    ("threshold = nan", F(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", F(threshold=float("inf")), E_ARG, True),
    ("threshold = 1.0", F(threshold=1.0), E_ARG, True),
    ("threshold = -0.25", F(threshold=-0.25), E_ARG, True),
    ("n_tracks = 65536", F(n_tracks=65536), E_UNSUPPORTED, False),
    ("n_windows * T = 2^31 (n_windows = 2^27)", F(n_windows=2 ** 27), E_UNSUPPORTED, False),
    ("cells = 2^31", F(cells=2 ** 31), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
ACCEPTED = [
    ("no float velocities", F(vel=None)),
    ("no raw velocities", F(vel_raw=None)),
    ("neither", F(vel=None, vel_raw=None)),
    ("no notes", F(n_notes=0, notes=None)),
    ("no tracks", F(n_notes=0, notes=None, n_tracks=0, cells=0, concurrent=None)),
    ("time-major", F(stride_t=16, stride_w=1)),
    ("one voice", F(voices=1)),
    ("8 voices, the full MIDI range, threshold 0", F(voices=8, n_pitch=128, pitch_base=0, silent=128, threshold=0.0)),
    ("65535 tracks", F(n_tracks=65535)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_rolls_from_notes(None if args is None else C.byref(args), stream)
