"""The contract of include/midivae_longsong.h as tables (no test lives here): one well-formed call of mvae_nearest_walk and of
mvae_feedback_rows and every way the header says a call is refused.  tests/test_long_songs_cpu.py runs all rows on addresses nothing
maps - with no device a well-formed call fails at its launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a
launch; tests/test_long_songs_gpu.py runs the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernels would stay inside the baseline's buffers (a missing output, a
smaller extent, a value the kernel only computes with).  Rows that would index past a buffer or follow a NULL pointer are CPU-only.

Also what the two test files share: the fixture, the settings of its feedback cases and the bit comparison."""
import ctypes as C
import os

import numpy as np

from midi_vae_amd import hiplib as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
WALK_KEYS = ("all_z", "start", "script", "e", "den", "picked", "z", "r0", "dist")


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_fixture():
    """(walks, feedback): walks name -> dict of WALK_KEYS; feedback a list of dicts, one per case: voices, T, n, silent, has_vel,
    has_held, override, threshold, n_pitch, the inputs idx (n, T), vel, held, instr (n, voices) and what the encoder receives:
    X, V, D (n, T) and I (n, voices)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "long_songs.npz"))
    walks = {}
    for key in z.files:
        if key.startswith("walk_"):
            _, name, field = key.split("_", 2)
            walks.setdefault(name, {})[field] = z[key]
    feedback = []
    for V, T, n, silent, has_vel, has_held, override, w0, r0, thr in z["fb_cases"].tolist():
        rows, wins = slice(r0, r0 + n * T), slice(w0, w0 + n * V)
        c = dict(voices=V, T=T, n=n, silent=bool(silent), has_vel=bool(has_vel), has_held=bool(has_held), override=bool(override),
                 threshold=thr / 1000.0, n_pitch=int(z["fb_n_pitch"]))
        for k in ("idx", "vel", "held", "X", "V", "D"):
            c[k] = z["fb_" + k][rows].reshape(n, T)
        for k in ("instr", "I"):
            c[k] = z["fb_" + k][wins].reshape(n, V)
        feedback.append(c)
    return walks, feedback


def feedback_settings(c):
    """settings under which the feedback case ``c`` was made: its pitches lie above an arbitrary low_crop"""
    return dict(max_voices=c["voices"], low_crop=24, high_crop=24 + c["n_pitch"], include_silent_note=c["silent"],
                velocity_threshold_such_that_it_is_a_played_note=c["threshold"],
                override_sampled_pitches_based_on_velocity_info=c["override"])


def feedback_id(c):
    return "v%d-T%d-%s%s%s%s" % (c["voices"], c["T"], "s" if c["silent"] else "-", "v" if c["has_vel"] else "-",
                                 "h" if c["has_held"] else "-", "o" if c["override"] else "-")


def same_bits(a, b):
    """float arrays equal bit for bit, signed zeros told apart, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))))


def walk_inputs(fx, it):
    """the codes every song of the walk case ``fx`` searches with in iteration ``it``: the float64 start codes, then the script"""
    return fx["start"] if it == 0 else np.ascontiguousarray(fx["script"][:, it - 1])


def fake_alloc(name, shape, kind, out=False):
    """addresses nothing maps, one per buffer name (never dereferenced on the host)"""
    return 0x10000000 + 0x100000 * (sum(map(ord, name)) % 251)


def S(**fields):
    def mutate(a):
        for k, v in fields.items():
            setattr(a, k, v)
        return a
    return mutate


# ---- mvae_nearest_walk ---------------------------------------------------------------------------------------------------------------
W_N, W_S, W_Z, W_LD_ALL, W_LD_R, W_CAP, W_PICKED, W_LD_Z, W_LD_HIST = 40, 3, 8, 10, 9, 6, 2, 10, 11
W_WORKSPACE = W_S * 1 * 16 + W_S * 8          # the header's formula at N <= 256


def walk_baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'i32', 'f32', 'f64'"""
    return hl.WalkArgs(all_z=alloc("all_z", (W_N, W_LD_ALL), "f32"), r_in=alloc("r_in", (W_S, W_LD_R), "f32"),
                       hist_in=alloc("hist_in", (W_S, W_LD_R), "f32"), picked=alloc("picked", (W_S, W_CAP), "i32", out=True),
                       workspace=alloc("workspace", (1, W_WORKSPACE // 4), "i32", out=True), N=W_N, S=W_S, Z=W_Z, ld_all=W_LD_ALL,
                       ld_r=W_LD_R, r_f64=0, ld_hist_in=W_LD_R, hist_f64=0, cap=W_CAP, n_picked=W_PICKED, ld_z=W_LD_Z, ld_rout=W_LD_R,
                       ld_hist=W_LD_HIST, e=0.75, den=1.75, best_out=alloc("best_out", (1, W_S), "i32", out=True),
                       dist_out=alloc("dist_out", (1, W_S), "f64", out=True), z_out=alloc("z_out", (W_S, W_LD_Z), "f32", out=True),
                       r_out=alloc("r_out", (W_S, W_LD_R), "f32", out=True), hist_out=alloc("hist_out", (W_S, W_LD_HIST), "f32", out=True))


# (what is wrong, mutate(args) -> args or None for a NULL struct, the promised code, safe on a device)
WALK_ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("all_z NULL", S(all_z=None), E_ARG, False),
    ("r_in NULL", S(r_in=None), E_ARG, False),
    ("picked NULL", S(picked=None), E_ARG, False),
    ("workspace NULL", S(workspace=None), E_ARG, False),
    ("best_out NULL", S(best_out=None), E_ARG, False),
    ("dist_out NULL", S(dist_out=None), E_ARG, False),
    ("z_out NULL", S(z_out=None), E_ARG, False),
    ("r_out NULL", S(r_out=None), E_ARG, False),
    ("N = 0", S(N=0), E_ARG, True),
    ("N = -1", S(N=-1), E_ARG, True),
    ("S = 0", S(S=0), E_ARG, True),
    ("S = -1", S(S=-1), E_ARG, True),
    ("Z = 0", S(Z=0), E_ARG, True),
    ("Z = -1", S(Z=-1), E_ARG, True),
    ("cap = 0", S(cap=0, n_picked=0), E_ARG, True),
    ("ld_all = Z - 1", S(ld_all=W_Z - 1), E_ARG, True),
    ("ld_r = Z - 1", S(ld_r=W_Z - 1), E_ARG, True),
    ("ld_z = Z - 1", S(ld_z=W_Z - 1), E_ARG, True),
    ("ld_rout = Z - 1", S(ld_rout=W_Z - 1), E_ARG, True),
    ("ld_hist = Z - 1", S(ld_hist=W_Z - 1), E_ARG, True),
    ("ld_hist_in = Z - 1", S(ld_hist_in=W_Z - 1), E_ARG, True),
    ("n_picked = -1", S(n_picked=-1), E_ARG, False),
    ("n_picked = cap", S(n_picked=W_CAP), E_ARG, False),
    ("r_f64 = 2", S(r_f64=2), E_ARG, False),
    ("r_f64 = -1", S(r_f64=-1), E_ARG, False),
    ("hist_f64 = 2", S(hist_f64=2), E_ARG, False),
    ("hist_f64 = -1", S(hist_f64=-1), E_ARG, False),
    ("e = nan", S(e=float("nan")), E_ARG, True),
    ("e = inf", S(e=float("inf")), E_ARG, True),
    ("den = nan", S(den=float("nan")), E_ARG, True),
    ("den = -inf", S(den=float("-inf")), E_ARG, True),
    ("den = 0", S(den=0.0), E_ARG, True),
    ("Z = 4097", S(Z=4097, ld_all=4097, ld_r=4097, ld_z=4097, ld_rout=4097, ld_hist=4097, ld_hist_in=4097), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
WALK_ACCEPTED = [
    ("no history", S(hist_out=None, ld_hist=0)),
    ("a zero history, ld_hist_in unused", S(hist_in=None, ld_hist_in=0)),
    ("no history out: ld_hist_in unused", S(hist_out=None, ld_hist=0, ld_hist_in=0)),
    ("the first iteration", S(n_picked=0)),
    ("the last entry of picked", S(n_picked=W_CAP - 1)),
    ("tight rows", S(ld_all=W_Z, ld_r=W_Z, ld_z=W_Z, ld_rout=W_Z, ld_hist=W_Z, ld_hist_in=W_Z)),
    ("double codes, a double history", S(r_f64=1, hist_f64=1)),
    ("a negative e", S(e=-0.25, den=0.75)),
    ("in place", lambda a: S(z_out=a.r_in, ld_z=a.ld_r)(a)),
    ("Z = 4096", S(Z=4096, ld_all=4096, ld_r=4096, ld_z=4096, ld_rout=4096, ld_hist=4096, ld_hist_in=4096)),
]

# ---- mvae_feedback_rows --------------------------------------------------------------------------------------------------------------
F_N, F_T, F_V, F_PITCH, F_LD = 6, 12, 3, 9, 8


def feedback_baseline(alloc):
    return hl.FeedbackArgs(idx=alloc("idx", (F_N, F_T), "u8"), stride_t=1, stride_w=F_T, vel=alloc("vel", (F_N, F_T), "f32"),
                           held_idx=alloc("held_idx", (F_N, F_T), "u8"), instr=alloc("instr", (F_N, F_V), "u8"), instr_stride_v=1,
                           instr_stride_w=F_V, n=F_N, T=F_T, voices=F_V, silent=F_PITCH, n_pitch=F_PITCH, override_rules=1, threshold=0.5,
                           ld_out=F_LD, x_out=alloc("x_out", (F_T, F_LD), "u8", out=True),
                           x_rev_out=alloc("x_rev_out", (F_T, F_LD), "u8", out=True), vel_out=alloc("vel_out", (F_T, F_LD), "f32", out=True),
                           held_out=alloc("held_out", (F_T, F_LD), "u8", out=True), instr_out=alloc("instr_out", (F_V, F_LD), "u8", out=True))


FEEDBACK_ROWS = [
    ("a NULL", lambda a: None, E_ARG, False),
    ("idx NULL", S(idx=None), E_ARG, False),
    ("every output NULL", S(x_out=None, x_rev_out=None, vel_out=None, held_out=None, instr_out=None), E_ARG, True),
    ("n = 0", S(n=0), E_ARG, True),
    ("n = -1", S(n=-1), E_ARG, True),
    ("T = 0", S(T=0), E_ARG, True),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, True),
    ("stride_t = 0", S(stride_t=0), E_ARG, True),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("instr_stride_v = 0", S(instr_stride_v=0), E_ARG, True),
    ("instr_stride_w = -1", S(instr_stride_w=-1), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, False),
    ("voices = 9", S(voices=9, T=18), E_ARG, False),
    ("T % voices != 0", S(T=11), E_ARG, True),
    ("silent = -2", S(silent=-2), E_ARG, True),
    ("silent = 256", S(silent=256), E_ARG, True),
    ("override_rules = 2", S(override_rules=2), E_ARG, True),
    ("override_rules = -1", S(override_rules=-1), E_ARG, True),
    ("threshold = nan", S(threshold=float("nan")), E_ARG, True),
    ("threshold = inf", S(threshold=float("inf")), E_ARG, True),
    ("ld_out = n - 1", S(ld_out=F_N - 1), E_ARG, True),
    ("T = 65538", S(T=65538, voices=2), E_UNSUPPORTED, False),
]

FEEDBACK_ACCEPTED = [
    ("no velocity head", S(vel=None)),
    ("no held head", S(held_idx=None)),
    ("neither", S(vel=None, held_idx=None)),
    ("no instruments, strides unused", S(instr=None, instr_stride_v=0, instr_stride_w=0)),
    ("the notes alone", S(x_rev_out=None, vel_out=None, held_out=None, instr_out=None)),
    ("no silent index", S(silent=-1)),
    ("tight rows", S(ld_out=F_N)),
    ("rules off", S(override_rules=0)),
    ("T = 65536, 8 voices", S(T=65536, voices=8)),
]


def invoke(lib, entry, args, stream=None):
    return getattr(lib, entry)(None if args is None else C.byref(args), stream)
