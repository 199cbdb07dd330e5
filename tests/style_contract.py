"""The contract of include/midivae_style.h as a table (no test lives here): one well-formed call of mvae_style_scores and every way the
header says a call is refused.  tests/test_style_scores_cpu.py runs all rows on addresses nothing maps - with no device a well-formed
call fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch;
tests/test_style_scores_gpu.py runs the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernel would stay inside the baseline's buffers (a missing output, a
smaller extent, a value the kernel only computes with).  Rows that would index past a buffer or follow a NULL pointer are CPU-only.

Also what the style test files share: the fixture and the bound on a confidence mean."""
import ctypes as C
import math
import os

import numpy as np

from midi_vae_amd import hiplib as hl
from midi_vae_amd import style as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
N, NC, G, LD, LD_TABLE = 40, 3, 4, 5, 10
GROUP_OFF = (0, 17, 17, 18, 40)


def load_fixture():
    """{case: dict}: the two cases of tests/golden/style_scores.npz ('a': C = 2, instruments per window; 'b': C = 3, per song)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "style_scores.npz"))
    cases = {}
    for key in z.files:
        case, name = key.split("_", 1)
        cases.setdefault(case, {})[name] = z[key]
    for fx in cases.values():
        fx.setdefault("instr_row", None)
        fx["weights"] = tuple(float(w) for w in fx["weights"])
    return cases


def mirror_of(fx):
    return st.scores(fx["p_pitch"], fx["p_vel"], fx["p_instr"], fx["cls"], fx["group_off"], fx["instr_row"], fx["weights"], device=False)


def same_bits(a, b):
    """float arrays equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def device_mean_ratio(got, want, n_g):
    """|got - want| over the bound (ceil(n_g / 256) + 8) * 2^-53 * max(|want|, 2^-1022) of a confidence mean that the device summed
    in the header's order against the exactly rounded ``want``: a lane adds ceil(n_g / 256) terms one after the other, the tree adds
    8 levels, each addition rounds once at 2^-53 relative to a partial sum of non-negative terms (so to no more than the total);
    the division's rounding and the mirror's own are inside the bound's slack of first-order terms"""
    return abs(got - want) / ((math.ceil(n_g / 256) + 8) * 2.0 ** -53 * max(abs(want), 2.0 ** -1022))


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'i32', 'f32', 'f64'"""
    return hl.StyleArgs(p_pitch=alloc("p_pitch", (N, LD), "f32"), p_vel=alloc("p_vel", (N, LD), "f32"), p_instr=alloc("p_instr", (G, LD), "f32"),
                        instr_row=alloc("instr_row", (N,), "i32"), cls=alloc("cls", (N,), "u8"), group_off=alloc("group_off", (G + 1,), "i32"),
                        n=N, C=NC, n_groups=G, n_instr_rows=G, ld_pitch=LD, ld_vel=LD, ld_instr=LD, ld_ens=LD, ld_table=LD_TABLE,
                        weights=(C.c_double * 3)(0.499, 0.3, 0.2), ens_out=alloc("ens_out", (N, LD), "f32", out=True),
                        pred_out=alloc("pred_out", (N, 4), "u8", out=True), table_out=alloc("table_out", (G, LD_TABLE), "f64", out=True),
                        confusion_out=alloc("confusion_out", (4, NC, NC), "i32", out=True))


def fake_alloc(name, shape, kind, out=False):
    """addresses nothing maps, one per buffer name (never dereferenced on the host)"""
    return 0x10000000 + 0x100000 * (sum(map(ord, name)) % 251)


def S(**fields):
    def mutate(a):
        for k, v in fields.items():
            if k.startswith("w") and k[1:].isdigit():
                a.weights[int(k[1:])] = v
            else:
                setattr(a, k, v)
        return a
    return mutate


NO_OUTPUT = dict(ens_out=None, pred_out=None, table_out=None, confusion_out=None)

# (what is wrong, mutate(args) -> args or None for a NULL struct, the promised code, safe on a device)
ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("all three tables NULL", S(p_pitch=None, p_vel=None, p_instr=None, ens_out=None), E_ARG, True),
    ("all outputs NULL", S(**NO_OUTPUT), E_ARG, True),
    ("ens_out without p_pitch", S(p_pitch=None), E_ARG, True),
    ("ens_out without p_vel", S(p_vel=None), E_ARG, True),
    ("ens_out without p_instr", S(p_instr=None), E_ARG, True),
    ("n = 0", S(n=0), E_ARG, True),
    ("n = -1", S(n=-1), E_ARG, True),
    ("n_groups = 0", S(n_groups=0), E_ARG, True),
    ("n_groups = -3", S(n_groups=-3), E_ARG, True),
    ("cls NULL", S(cls=None), E_ARG, False),
    ("group_off NULL", S(group_off=None), E_ARG, False),
    ("ld_pitch = C - 1", S(ld_pitch=NC - 1), E_ARG, True),
    ("ld_vel = C - 1", S(ld_vel=NC - 1), E_ARG, True),
    ("ld_instr = 0", S(ld_instr=0), E_ARG, True),
    ("ld_ens = C - 1", S(ld_ens=NC - 1), E_ARG, True),
    ("ld_table = 8", S(ld_table=8), E_ARG, True),
    ("n_instr_rows = 0", S(n_instr_rows=0), E_ARG, True),
    ("n_instr_rows = -1", S(n_instr_rows=-1), E_ARG, True),
    ("weight 0 = nan", S(w0=float("nan")), E_ARG, True),
    ("weight 1 = inf", S(w1=float("inf")), E_ARG, True),
    ("weight 2 = -inf", S(w2=float("-inf")), E_ARG, True),
    ("weight sum = 0", S(w0=0.0, w1=0.0, w2=0.0), E_ARG, True),
    ("weight sum < 0", S(w0=-1.0), E_ARG, True),
    ("C = 1", S(C=1), E_UNSUPPORTED, True),
    ("C = 0", S(C=0), E_UNSUPPORTED, True),
    ("C = 65", S(C=65, ld_pitch=65, ld_vel=65, ld_instr=65, ld_ens=65), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation; GPU: they run inside the baseline's buffers)
ACCEPTED = [
    ("no pitch judge", S(p_pitch=None, ens_out=None)),
    ("no velocity judge", S(p_vel=None, ens_out=None)),
    ("no instrument judge, n_instr_rows and ld_instr unused", S(p_instr=None, ens_out=None, n_instr_rows=0, ld_instr=0)),
    ("the pitch judge alone", S(p_vel=None, p_instr=None, ens_out=None)),
    ("the table alone", S(ens_out=None, pred_out=None, confusion_out=None)),
    ("the ensemble alone, ld_table unused", S(pred_out=None, table_out=None, confusion_out=None, ld_table=0)),
    ("the confusion counts alone", S(ens_out=None, pred_out=None, table_out=None)),
    ("a negative weight, a zero weight", S(w0=1.0, w1=-0.25, w2=0.0)),
    ("C = 2", S(C=2)),
    ("instruments per window: rows past n_instr_rows are never read", S(instr_row=None)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_style_scores(None if args is None else C.byref(args), stream)
