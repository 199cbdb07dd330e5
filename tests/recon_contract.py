"""The contract of include/midivae_recon.h as a table (no test lives here): one well-formed call of mvae_recon_songs and every way the
header says a call is refused.  tests/test_recon_cpu.py runs all rows on addresses nothing maps - with no device a well-formed call
fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch; tests/test_recon_gpu.py runs the rows
flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernels would stay inside the baseline's buffers (a smaller extent, a
missing output or workspace the kernel then does not use, a value the kernel only compares).  Rows that would index past a buffer or
an LDS array, divide by zero or follow a NULL pointer are CPU-only.

Also what the test files of the song-level decode share: the fixture and the random songs."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import hiplib as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "recon.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("s_")}
    fx["s"] = {k[2:]: z[k].item() for k in z.files if k.startswith("s_")}
    return fx


def random_songs(rng, lengths, T, V, n_pitch=60):
    """(idx, vel) of sum(lengths) windows: random columns, 30 % rests, 10 % pitch column 0, a voice repeats its previous row with 30 %
    (through window and song boundaries); velocities float32 in [0, 1], a third of them multiples of 1/8"""
    n = int(np.sum(lengths))
    idx = rng.integers(0, n_pitch, (n, T)).astype(np.uint8)
    idx[rng.random((n, T)) < 0.3] = n_pitch          # rests
    idx[rng.random((n, T)) < 0.1] = 0                # pitch column 0: the `> 0` test
    hold = rng.random((n, T)) < 0.3                  # the voice's previous row again
    flat = idx.reshape(n * T // V, V)
    for i in range(1, flat.shape[0]):
        flat[i] = np.where(hold.reshape(flat.shape)[i], flat[i - 1], flat[i])
    v = rng.random((n, T))
    vel = np.where(rng.random((n, T)) < 1 / 3, np.round(v * 8) / 8, v).astype(np.float32)
    return idx, vel


E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
N, T, V, N_PITCH, LD = 17, 64, 4, 60, 8


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'f32', 'i32'"""
    return hl.ReconArgs(idx=alloc("idx", (N, T), "u8"), stride_t=1, stride_w=T, vel=alloc("vel", (N, T), "f32"),
                        held=alloc("held", (N, T), "u8"), orig=alloc("orig", (N, T), "u8"), orig_stride_t=1, orig_stride_w=T,
                        first_window=alloc("first_window", (N,), "i32"), n=N, T=T, voices=V, silent=N_PITCH, n_pitch=N_PITCH,
                        override_rules=1, threshold=0.5, carry=alloc("carry", (N * V, 2), "i32", out=True),
                        vel_out=alloc("vel_out", (N, T), "f32", out=True), start_out=alloc("start_out", (N, T), "u8", out=True),
                        counts_out=alloc("counts", (N, LD), "i32", out=True), ld_counts=LD)


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
    ("all outputs NULL", S(vel_out=None, start_out=None, counts_out=None), E_ARG, True),
    ("n = 0", S(n=0), E_ARG, False),
    ("n = -1", S(n=-1), E_ARG, False),
    ("T = 0", S(T=0), E_ARG, False),
    ("T = -4", S(T=-4), E_ARG, False),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, True),
    ("stride_t = 0", S(stride_t=0), E_ARG, False),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("orig_stride_t = 0", S(orig_stride_t=0), E_ARG, False),
    ("orig_stride_w = -1", S(orig_stride_w=-1), E_ARG, False),
    ("voices = 0", S(voices=0), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, True),
    ("voices = 9 (T = 63)", S(voices=9, T=63), E_ARG, False),
    ("T % voices != 0 (T = 62)", S(T=62), E_ARG, True),
    ("ld_counts = 7", S(ld_counts=7), E_ARG, True),
    ("silent = 256", S(silent=256), E_ARG, True),
    ("silent = -2", S(silent=-2), E_ARG, True),
    ("override_rules = 2", S(override_rules=2), E_ARG, True),
    ("override_rules = -1", S(override_rules=-1), E_ARG, True),
    ("threshold = nan", S(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", S(threshold=float("inf")), E_ARG, True),
    ("carry NULL with vel, rules and first_window", S(carry=None), E_ARG, False),
    ("n_pitch = 193", S(n_pitch=193), E_UNSUPPORTED, False),
    ("T = 65536 + 4", S(T=65536 + 4), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
ACCEPTED = [
    ("velocities only", S(start_out=None, counts_out=None, ld_counts=0)),
    ("note starts only", S(vel_out=None, counts_out=None)),
    ("counts only", S(vel_out=None, start_out=None)),
    ("no velocity head, no workspace", S(vel=None, carry=None)),
    ("no held head", S(held=None)),
    ("no originals, their strides unused", S(orig=None, orig_stride_t=0, orig_stride_w=0)),
    ("every window its own song, no workspace", S(first_window=None, carry=None)),
    ("rules off, no workspace", S(override_rules=0, carry=None)),
    ("no silent index, a negative threshold", S(silent=-1, threshold=-1.0)),
    ("time-major", S(stride_t=32, stride_w=1, orig_stride_t=32, orig_stride_w=1)),
    ("8 voices, 192 columns, T = 65536", S(voices=8, n_pitch=192, T=65536)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_recon_songs(None if args is None else C.byref(args), stream)
