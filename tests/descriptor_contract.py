"""The contract of include/midivae_descriptors.h as a table (no test lives here): one well-formed call of mvae_desc_windows and
every way the header says a call is refused.  tests/test_descriptors_cpu.py runs all rows on addresses nothing maps - with no
device a well-formed call fails at its first launch (MVAE_E_LAUNCH), so any other code proves the refusal came BEFORE a launch;
tests/test_descriptors_gpu.py runs the rows flagged ``safe`` on real buffers and checks that nothing was written.

``safe``: even if the library wrongly accepted the call, the kernels would stay inside the baseline's buffers (a smaller extent, a
missing output).  Rows that would index past a buffer or an LDS array, divide by zero or follow a NULL pointer are CPU-only."""
import ctypes as C

from midi_vae_amd import hiplib as hl

E_ARG, E_UNSUPPORTED = hl.E_ARG, hl.E_UNSUPPORTED
N, T, V, N_PITCH = 17, 64, 4, 60


def baseline(alloc):
    """``alloc(name, shape, kind, out=False)`` -> address; kinds 'u8', 'f32', 'f64'"""
    return hl.DescArgs(idx=alloc("idx", (N, T), "u8"), stride_t=1, stride_w=T, n=N, T=T, voices=V, silent=N_PITCH, n_pitch=N_PITCH,
                       low_crop=24, resolution=4, ld_sig=15, tonal=alloc("tonal", (6, 12), "f32"),
                       sig_out=alloc("sig", (N, 15), "f64", out=True), harm_out=alloc("harm", (N, V * V), "f64", out=True))


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
    ("both outputs NULL", S(sig_out=None, harm_out=None), E_ARG, True),
    ("n = 0", S(n=0), E_ARG, False),
    ("n = -1", S(n=-1), E_ARG, False),
    ("T = 0", S(T=0), E_ARG, False),
    ("T = -4", S(T=-4), E_ARG, False),
    ("voices = 0", S(voices=0), E_ARG, False),
    ("voices = -2", S(voices=-2), E_ARG, False),
    ("resolution = 0", S(resolution=0), E_ARG, False),
    ("resolution = -1", S(resolution=-1), E_ARG, False),
    ("voices = 1", S(voices=1), E_ARG, True),
    ("voices = 9 (T = 63)", S(voices=9, T=63), E_ARG, False),
    ("T % voices != 0 (T = 62)", S(T=62), E_ARG, True),
    ("n_pitch = 193", S(n_pitch=193, harm_out=None), E_UNSUPPORTED, False),
    ("n_pitch = 0", S(n_pitch=0), E_ARG, False),
    ("n_pitch % 12 != 0 with harm_out (61)", S(n_pitch=61), E_ARG, False),
    ("tonal NULL with harm_out", S(tonal=None), E_ARG, False),
    ("ld_sig = 14", S(ld_sig=14), E_ARG, True),
    ("stride_t = 0", S(stride_t=0), E_ARG, False),
    ("stride_w = -1", S(stride_w=-1), E_ARG, False),
    ("silent = 256", S(silent=256), E_ARG, False),
    ("silent = -2", S(silent=-2), E_ARG, False),
    ("low_crop = -1", S(low_crop=-1), E_ARG, False),
    ("low_crop = 1024", S(low_crop=1024), E_UNSUPPORTED, False),
    ("T = 2^20 + 4", S(T=(1 << 20) + 4), E_UNSUPPORTED, False),
]

# forms that stay accepted (CPU: MVAE_E_LAUNCH, i.e. past validation)
ACCEPTED = [
    ("signature only, no tonal matrix, 61 columns", S(harm_out=None, tonal=None, n_pitch=61)),
    ("harmonicity only, ld_sig unused", S(sig_out=None, ld_sig=0)),
    ("no silent index", S(silent=-1)),
    ("time-major", S(stride_t=32, stride_w=1)),
    ("8 voices, 192 columns, T = 2^20", S(voices=8, n_pitch=192, T=1 << 20)),
]


def invoke(lib, args, stream=None):
    return lib.mvae_desc_windows(None if args is None else C.byref(args), stream)
