"""The contract of include/midivae_generate.h as tables (no test lives here): one well-formed call of mvae_latent_paths and of
mvae_pianoroll and every way the header says a call is refused.  tests/test_generation_cpu.py runs all rows on addresses nothing
maps - with no device a well-formed call fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a
launch; tests/test_generation_gpu.py runs the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernel would stay inside the baseline's buffers (a missing output, a
smaller extent, a value the kernel only computes with).  Rows that would index past a buffer or follow a NULL pointer are CPU-only.

Also what the two test files share: the fixture, the settings of its image cases and the bit comparison."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import hiplib as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED

# ---- the fixture -----------------------------------------------------------------------------------------------------------------
PATH_LENGTHS = [1, 11, 32, 31]


def load_fixture():
    """{'paths_f32': dict, 'paths_f64': dict, 'image_a': dict, 'image_b': dict} of tests/golden/generation.npz"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "generation.npz"))
    cases = {}
    for key in z.files:
        kind, tag, name = key.split("_", 2)
        cases.setdefault(kind + "_" + tag, {})[name] = z[key]
    return cases


def image_settings(fx):
    """settings under which the image case ``fx`` was drawn: its pitches lie above an arbitrary low_crop, the silent index is n_pitch"""
    return dict(max_voices=int(fx["voices"]), low_crop=24, high_crop=24 + int(fx["n_pitch"]), include_silent_note=True,
                velocity_threshold_such_that_it_is_a_played_note=float(fx["threshold"]), MAX_VELOCITY=float(fx["max_velocity"]))


def same_bits(a, b):
    """float arrays equal bit for bit, signed zeros told apart, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))))


def fake_alloc(name, shape, kind, out=False):
    """addresses nothing maps, one per buffer name (never dereferenced on the host)"""
    return 0x10000000 + 0x100000 * (sum(map(ord, name)) % 251)


def S(**fields):
    def mutate(a):
        for k, v in fields.items():
            setattr(a, k, v)
        return a
    return mutate


# ---- mvae_latent_paths -------------------------------------------------------------------------------------------------------------
P_N, P_Z, P_ANCHORS, P_LD = 12, 8, 5, 10


def paths_baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'i32', 'f32', 'f64'"""
    return hl.PathsArgs(anchors=alloc("anchors", (P_ANCHORS, P_LD), "f32"), a0=alloc("a0", (P_N,), "i32"), a1=alloc("a1", (P_N,), "i32"),
                        c0=alloc("c0", (P_N,), "f64"), c1=alloc("c1", (P_N,), "f64"), first_window=alloc("first_window", (P_N,), "i32"),
                        n=P_N, lo=0, count=P_N, Z=P_Z, n_anchors=P_ANCHORS, ld_anchor=P_LD, anchor_f64=0, ld_z=P_LD, ld_hist=P_LD,
                        z_out=alloc("z_out", (P_N, P_LD), "f32", out=True), hist_out=alloc("hist_out", (P_N, P_LD), "f32", out=True))


# (what is wrong, mutate(args) -> args or None for a NULL struct, the promised code, safe on a device)
PATHS_ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("anchors NULL", S(anchors=None), E_ARG, False),
    ("a0 NULL", S(a0=None), E_ARG, False),
    ("a1 NULL", S(a1=None), E_ARG, False),
    ("c0 NULL", S(c0=None), E_ARG, False),
    ("c1 NULL", S(c1=None), E_ARG, False),
    ("z_out NULL", S(z_out=None), E_ARG, False),
    ("n = 0", S(n=0), E_ARG, True),
    ("n = -1", S(n=-1), E_ARG, True),
    ("count = 0", S(count=0), E_ARG, True),
    ("count = -2", S(count=-2), E_ARG, True),
    ("Z = 0", S(Z=0), E_ARG, True),
    ("Z = -1", S(Z=-1), E_ARG, True),
    ("n_anchors = 0", S(n_anchors=0), E_ARG, True),
    ("n_anchors = -1", S(n_anchors=-1), E_ARG, True),
    ("lo = -1", S(lo=-1, count=1), E_ARG, False),
    ("lo + count = n + 1", S(lo=1), E_ARG, False),
    ("lo + count overflows int32", S(lo=2 ** 31 - 1, count=2 ** 31 - 1), E_ARG, False),
    ("ld_anchor = Z - 1", S(ld_anchor=P_Z - 1), E_ARG, True),
    ("ld_z = Z - 1", S(ld_z=P_Z - 1), E_ARG, True),
    ("ld_hist = Z - 1", S(ld_hist=P_Z - 1), E_ARG, True),
    ("anchor_f64 = 2", S(anchor_f64=2), E_ARG, False),
    ("anchor_f64 = -1", S(anchor_f64=-1), E_ARG, False),
    ("Z = 4097", S(Z=4097, ld_anchor=4097, ld_z=4097, ld_hist=4097), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation; GPU: they run inside the baseline's buffers)
PATHS_ACCEPTED = [
    ("no history, ld_hist unused", S(hist_out=None, ld_hist=0)),
    ("every window its own song", S(first_window=None)),
    ("the last windows alone", S(lo=P_N - 3, count=3)),
    ("one window", S(lo=4, count=1)),
    ("tight rows", S(Z=P_LD)),
]

# ---- mvae_pianoroll ----------------------------------------------------------------------------------------------------------------
R_N, R_T, R_V, R_PITCH, R_LD = 6, 12, 3, 9, 11


def pianoroll_baseline(alloc):
    return hl.PianorollArgs(idx=alloc("idx", (R_N, R_T), "u8"), stride_t=1, stride_w=R_T, vel=alloc("vel", (R_N, R_T), "f32"),
                            first_window=alloc("first_window", (R_N,), "i32"), n=R_N, T=R_T, voices=R_V, silent=R_PITCH, n_pitch=R_PITCH,
                            ld_img=R_LD, threshold=0.5, max_velocity=127.0, img_out=alloc("img_out", (R_N * R_T // R_V, R_LD), "f64", out=True))


PIANOROLL_ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("idx NULL", S(idx=None), E_ARG, False),
    ("img_out NULL", S(img_out=None), E_ARG, False),
    ("n = 0", S(n=0), E_ARG, True),
    ("n = -1", S(n=-1), E_ARG, True),
    ("T = 0", S(T=0), E_ARG, True),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, True),
    ("stride_t = 0", S(stride_t=0), E_ARG, True),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, False),
    ("voices = 9", S(voices=9, T=18), E_ARG, False),
    ("T % voices != 0", S(T=11), E_ARG, True),
    ("silent = -2", S(silent=-2), E_ARG, True),
    ("silent = 256", S(silent=256), E_ARG, True),
    ("ld_img = n_pitch - 1", S(ld_img=R_PITCH - 1), E_ARG, True),
    ("threshold = nan", S(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", S(threshold=float("inf")), E_ARG, True),
    ("max_velocity = nan", S(max_velocity=float("nan")), E_ARG, True),
    ("max_velocity = -inf", S(max_velocity=float("-inf")), E_ARG, True),
    ("n_pitch = 193", S(n_pitch=193, ld_img=193), E_UNSUPPORTED, False),
    ("T = 65538", S(T=65538, voices=2), E_UNSUPPORTED, False),
]

PIANOROLL_ACCEPTED = [
    ("no velocities", S(vel=None)),
    ("every window its own song", S(first_window=None)),
    ("no silent index", S(silent=-1)),
    ("tight rows", S(ld_img=R_PITCH)),
    ("a negative max_velocity, a negative threshold", S(max_velocity=-1.0, threshold=-0.25)),
]


def invoke(lib, entry, args, stream=None):
    return getattr(lib, entry)(None if args is None else C.byref(args), stream)
