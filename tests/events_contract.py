"""The contract of include/midivae_events.h as a table (no test lives here): one well-formed call of mvae_note_events and every way the
header says a call is refused.  tests/test_events_cpu.py runs all rows on addresses nothing maps - with no device a well-formed call
fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch; tests/test_events_gpu.py runs the rows
flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernels would stay inside the baseline's buffers (a value the kernels
only compare, a smaller extent, a smaller capacity).  Rows that would index past a buffer, divide by zero or follow a NULL pointer are
CPU-only.

Also what the test files of the note events share: the fixture (tests/golden/midi_events.npz on top of tests/golden/recon.npz)."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import events as ev
from midi_vae_amd import hiplib as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("held", "tick", "plain")


def load_fixture():
    """dict: ``s`` the settings, ``programs``, ``bpm``, ``tempo``, and per group ``a`` (T = 64) / ``b`` (T = 24) a dict of the inputs
    ``idx``, ``vel``, ``held``, ``lengths`` and per pass of PASSES ``notes_<pass>``: (records, offsets) as the reference recorded them"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "midi_events.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "recon.npz"))
    fx = dict(s={k[2:]: z[k].item() for k in z.files if k.startswith("s_")}, programs=z["programs"].tolist(), bpm=float(z["bpm"]),
              tempo=float(z["tempo"]))
    for g in "ab":
        d = {k: z["%s_%s" % (g, k)] for k in ("idx", "vel", "held", "lengths")}
        if g == "a":          # the songs of recon.npz come first: its note starts are the held roll
            for k, src in (("idx", "idx"), ("vel", "vel"), ("held", "starts"), ("lengths", "lengths")):
                d[k] = np.concatenate([r[src], d[k]], 0)
        for name in PASSES:
            cols = z["%s_%s_notes" % (g, name)]
            rec = np.zeros(cols.shape[1], ev.RECORD)
            for field, col in zip(("start", "end", "pitch", "voice", "velocity"), cols):
                rec[field] = col
            d["notes_" + name] = (rec, z["%s_%s_offsets" % (g, name)])
        fx[g] = d
    return fx


def pass_inputs(group, name):
    """(vel, held) of a pass"""
    return (None if name == "plain" else group["vel"]), (group["held"] if name == "held" else None)


E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
N, T, V, N_PITCH, N_SONGS = 17, 64, 4, 60, 2
CAPACITY = N * T


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'f32', 'i32'"""
    return hl.EventsArgs(idx=alloc("idx", (N, T), "u8"), stride_t=1, stride_w=T, vel=alloc("vel", (N, T), "f32"),
                         held=alloc("held", (N, T), "u8"), song=alloc("song", (N,), "i32"), n=N, T=T, voices=V, silent=N_PITCH,
                         n_pitch=N_PITCH, n_songs=N_SONGS, smallest_note=16, pitch_base=24, close_at_end=0, capacity=CAPACITY,
                         threshold=0.5, workspace=alloc("workspace", (2 * N * V + 2 * N_SONGS * (V + 1),), "i32", out=True),
                         records=alloc("records", (CAPACITY, 3), "i32", out=True),
                         offsets=alloc("offsets", (N_SONGS * V + 1,), "i32", out=True), total=alloc("total", (1,), "i32", out=True))


def fake_alloc(name, shape, kind, out=False):
    """addresses nothing maps, one per buffer name (never dereferenced on the host)"""
    return 0x10000000 + 0x100000 * (sum(map(ord, name)) % 251)


def S(**fields):
    def mutate(a):
        for k, v in fields.items():
            setattr(a, k, v)
        return a
    return mutate


# (what is wrong, mutate(args) -> args or None for a NULL struct, the promised code, safe on a device)
ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("idx NULL", S(idx=None), E_ARG, False),
    ("song NULL", S(song=None), E_ARG, False),
    ("workspace NULL", S(workspace=None), E_ARG, False),
    ("offsets NULL", S(offsets=None), E_ARG, False),
    ("total NULL", S(total=None), E_ARG, False),
    ("records NULL with capacity > 0", S(records=None), E_ARG, False),
    ("n = 0", S(n=0), E_ARG, False),
    ("n = -1", S(n=-1), E_ARG, False),
    ("T = 0", S(T=0), E_ARG, False),
    ("T = -4", S(T=-4), E_ARG, False),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, True),
    ("n_songs = 0", S(n_songs=0), E_ARG, True),
    ("n_songs = -1", S(n_songs=-1), E_ARG, False),
    ("n_songs > n (18)", S(n_songs=18), E_ARG, False),
    ("stride_t = 0", S(stride_t=0), E_ARG, False),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("voices = 0", S(voices=0), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, True),
    ("voices = 9 (T = 63)", S(voices=9, T=63), E_ARG, False),
    ("T % voices != 0 (T = 62)", S(T=62), E_ARG, True),
    ("silent = 256", S(silent=256), E_ARG, True),
    ("silent = -2", S(silent=-2), E_ARG, True),
    ("smallest_note = 0", S(smallest_note=0), E_ARG, False),
    ("smallest_note = -16", S(smallest_note=-16), E_ARG, True),
    ("threshold = nan", S(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", S(threshold=float("inf")), E_ARG, True),
    ("pitch_base = -1", S(pitch_base=-1), E_ARG, True),
    ("pitch_base + n_pitch = 257", S(pitch_base=197), E_ARG, True),
    ("close_at_end = 2", S(close_at_end=2), E_ARG, True),
    ("close_at_end = -1", S(close_at_end=-1), E_ARG, True),
    ("capacity = -1", S(capacity=-1), E_ARG, True),
    ("T = 65536 + 4", S(T=65536 + 4), E_UNSUPPORTED, False),
    ("n * T = 2^31 (n = 32768, T = 65536)", S(n=32768, T=65536), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
ACCEPTED = [
    ("no velocities", S(vel=None)),
    ("the tick rule", S(held=None)),
    ("neither", S(vel=None, held=None)),
    ("closed at the end", S(close_at_end=1)),
    ("counting only", S(capacity=0, records=None)),
    ("a small capacity", S(capacity=1)),
    ("one song", S(n_songs=1)),
    ("every window a song", S(n_songs=N)),
    ("no silent index, a negative threshold", S(silent=-1, threshold=-1.0)),
    ("time-major", S(stride_t=32, stride_w=1)),
    ("8 voices, the full MIDI range, T = 65536", S(voices=8, n_pitch=128, pitch_base=0, T=65536)),
    ("256 columns from pitch 0", S(n_pitch=256, pitch_base=0)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_note_events(None if args is None else C.byref(args), stream)
