"""The contract of include/midivae_sweep.h as a table (no test lives here): one well-formed call of mvae_sweep_windows and every way
the header says a call is refused.  tests/test_sweep_stats_cpu.py runs all rows on addresses nothing maps - with no device a
well-formed call fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch;
tests/test_sweep_stats_gpu.py runs the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernel would stay inside the baseline's buffers (a smaller extent, a
missing output, a value the kernel only compares).  Rows that would index past a buffer or an LDS array, divide by zero or follow a
NULL pointer are CPU-only.

Also what the sweep's test files share: the fixture and the comparison of two tables."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import hiplib as hl
from midi_vae_amd import sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD_COLUMNS = [6, 15, 21]
EXACT_COLUMNS = [c for c in range(22) if c not in STD_COLUMNS]


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sweep_stats.npz"))
    s = {k[2:]: z[k].item() for k in z.files if k.startswith("s_")}
    fx = {k: z[k] for k in z.files if not k.startswith("s_")}
    fx["s"], fx["K"] = s, int(z["K"])
    return fx


def assert_table(got, want, what):
    """the split the sweep's test files derive in their docstrings: every column but the stds bit-equal (NaN in the same places), the stds within 1e-12"""
    assert got.shape == want.shape and got.dtype == np.float64, what
    g, w = got[:, EXACT_COLUMNS], want[:, EXACT_COLUMNS]
    bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
    assert bad.size == 0, "%s: %d entries differ, first window %d column %s: %r vs %r" % (
        what, len(bad), bad[0][0], sw.COLUMNS[EXACT_COLUMNS[bad[0][1]]], g[tuple(bad[0])], w[tuple(bad[0])])
    g, w = got[:, STD_COLUMNS], want[:, STD_COLUMNS]
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    err = np.nanmax(np.abs(g - w), initial=0.0)
    print("%s: largest std difference %.3g" % (what, err))
    assert err <= 1e-12, what


E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
N, T, V, N_PITCH = 17, 64, 4, 60


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'f32', 'f64'"""
    return hl.SweepArgs(idx=alloc("idx", (N, T), "u8"), stride_t=1, stride_w=T, vel=alloc("vel", (N, T), "f32"), n=N, T=T, voices=V,
                        silent=N_PITCH, n_pitch=N_PITCH, count_a=35, count_b=39, override_rules=1, threshold=0.5, default_velocity=0.75,
                        ld_out=22, stats_out=alloc("stats", (N, 22), "f64", out=True), vel_out=alloc("vel_out", (N, T), "f32", out=True))


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
    ("both outputs NULL", S(stats_out=None, vel_out=None), E_ARG, True),
    ("n = 0", S(n=0), E_ARG, False),
    ("n = -1", S(n=-1), E_ARG, False),
    ("T = 0", S(T=0), E_ARG, False),
    ("T = -4", S(T=-4), E_ARG, False),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, True),
    ("stride_t = 0", S(stride_t=0), E_ARG, False),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("voices = 0", S(voices=0), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, True),
    ("voices = 9 (T = 63)", S(voices=9, T=63), E_ARG, False),
    ("T % voices != 0 (T = 62)", S(T=62), E_ARG, True),
    ("ld_out = 21", S(ld_out=21), E_ARG, True),
    ("silent = 256", S(silent=256), E_ARG, True),
    ("silent = -2", S(silent=-2), E_ARG, True),
    ("count_a = 256", S(count_a=256), E_ARG, False),
    ("count_a = -1", S(count_a=-1), E_ARG, False),
    ("count_b = 256", S(count_b=256), E_ARG, False),
    ("count_b = -1", S(count_b=-1), E_ARG, False),
    ("override_rules = 2", S(override_rules=2), E_ARG, True),
    ("override_rules = -1", S(override_rules=-1), E_ARG, True),
    ("threshold = nan", S(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", S(threshold=float("inf")), E_ARG, True),
    ("n_pitch = 193", S(n_pitch=193), E_UNSUPPORTED, False),
    ("T = 65536 + 4", S(T=65536 + 4), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
ACCEPTED = [
    ("statistics only", S(vel_out=None)),
    ("velocities only, ld_out unused", S(stats_out=None, ld_out=0)),
    ("no velocity head", S(vel=None)),
    ("no silent index, rules off", S(silent=-1, override_rules=0)),
    ("time-major", S(stride_t=32, stride_w=1)),
    ("counted columns 0 and 255, a negative threshold", S(count_a=0, count_b=255, threshold=-1.0)),
    ("8 voices, 192 columns, T = 65536", S(voices=8, n_pitch=192, T=65536)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_sweep_windows(None if args is None else C.byref(args), stream)
