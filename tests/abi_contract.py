"""The refusals include/midivae_hip.h promises, as data (no test lives here; test_abi_contract_cpu.py reads it without a device,
test_abi_contract_gpu.py with one).

The header makes one promise for every entry point: "0 = enqueued, negative = rejected (MVAE_E_*), nothing enqueued".  ``ENTRIES``
holds, per stream-taking entry point (some twice: one baseline per kernel family whose limits differ),

  * a BASELINE: ``build(al)`` returns a ``Call`` - a well-formed argument set at the smallest shape the entry point accepts.  ``al`` is
    the allocator: ``al(name, shape, dt, data=None, out=False, acc=False)`` returns an address.  The CPU side passes ``FakeAlloc``
    (distinct, 256-byte-aligned, never-mapped addresses: no host code dereferences a device pointer), the GPU side an allocator over
    tests/footprint.py's arena.  What the HOST reads - the argument struct, the job / problem / xpand arrays, ``host`` of the
    sampler - is real host memory (ctypes objects held by the Call) on both sides;
  * VIOLATIONS: ``V(name, mutate, code, why)`` - a named change of the baseline, the code the header promises and the header's
    sentence (or the sentence added to it with this table), and two flags:
      ``enq``  - wrongly accepted, the call would start work (nearly all);
      ``safe`` - even wrongly accepted the call stays inside the baseline's buffers: a bad enum, a refused combination of valid
                 extents, a bad job among good ones.  NEVER a NULL, a misalignment, a negative or undersized extent or stride.
                 Only these run on a device;
  * ACCEPTED: ``(name, mutate, LAUNCH | NOTHING)`` - changes of the baseline the product relies on and the header now spells out.
    They must stay accepted: LAUNCH forms enqueue (MVAE_E_LAUNCH without a device), NOTHING forms - an element count of 0 - return
    MVAE_OK and launch nothing.

Without a device a call that passes validation fails at its first launch: MVAE_E_LAUNCH.  So on the CPU "-3" reads "got past
validation, would have enqueued" - also for a refusal that comes too late, behind a fill or behind the first of several launches.

``EXEMPT``: the declared symbols that launch nothing, each with its reason.

``python -m tests.abi_contract [other_library.so]`` prints the verdict of every row with the library in the tree and, beside it,
with another build (profiles/r13_abi_contract.txt: the parent commit's library in the second column)."""
import ctypes as C
import zlib

import numpy as np

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl

E_ARG, E_UNS, E_LAUNCH = hl.E_ARG, hl.E_UNSUPPORTED, hl.E_LAUNCH
STREAM, STRUCT = object(), object()
LAUNCH, NOTHING = "enqueues", "nothing to do"      # what an accepted form does: MVAE_E_LAUNCH without a device / MVAE_OK anywhere
_ITEM = {"f32": 4, "bf16": 2, "u8": 1, "i32": 4}


class FakeAlloc:
    """addresses no one may touch: 256-byte aligned, distinct, in a range nothing maps"""

    def __init__(self):
        self.next = 0x7E5500000000

    def __call__(self, name, shape, dt, data=None, out=False, acc=False):
        n = int(np.prod(shape)) * _ITEM[dt]
        addr = self.next
        self.next += -(-n // 256) * 256 + 4096
        return addr


def default_data(name, shape, dt):
    """what an input holds when the builder does not say: small normal values; index 0; counters 0"""
    if dt in ("u8", "i32"):
        return np.zeros(shape, np.int64)
    return 0.25 * np.random.default_rng(zlib.crc32(name.encode())).standard_normal(shape)


class Call:
    """one call: ``args`` = [name, value] in the order of the C signature (STREAM: the caller's stream; STRUCT: ``host``, the argument
    struct or array the entry point reads on the host).  ``spare``: addresses of buffers the baseline owns and does not pass"""

    def __init__(self, fn, args, host=None, spare=None):
        self.fn, self.args, self.host, self.spare = fn, [list(a) for a in args], host, dict(spare or {})
        self.keep = []

    def _pos(self, name):
        for a in self.args:
            if a[0] == name:
                return a
        return None

    def set(self, name, value, i=None):
        a = self._pos(name)
        if a is not None and i is None:
            a[1] = value
        else:
            setattr(self.item(i or 0), name, value)

    def get(self, name, i=None):
        a = self._pos(name)
        return a[1] if a is not None and i is None else getattr(self.item(i or 0), name)

    def item(self, i=0):
        return self.host[i] if isinstance(self.host, C.Array) else self.host

    def argv(self, stream):
        out = []
        for (name, v), ty in zip(self.args, hl.SIGNATURES[self.fn][1]):
            if v is STREAM:
                v = stream
            elif v is STRUCT:
                v = C.addressof(self.host)
            if isinstance(v, int) and ty is not hl._vp and hasattr(ty, "contents"):
                v = C.cast(C.c_void_p(v), ty)
            out.append(v)
        return out

    def invoke(self, lib, stream=None):
        return getattr(lib, self.fn)(*self.argv(stream))


class V:
    def __init__(self, name, mutate, code, why, safe=False, enq=True):
        self.name, self.mutate, self.code, self.why, self.safe, self.enq = name, mutate, code, why, safe, enq


class Entry:
    def __init__(self, fn, build, violations, ptrs=(), dims=(), label=None, accepted=(), cpu_baseline=True):
        self.fn, self.build, self.ptrs, self.dims = fn, build, tuple(ptrs), tuple(dims)
        self.label = label or fn
        self.accepted, self.cpu_baseline = list(accepted), cpu_baseline
        self.violations = nulls(ptrs) + nonpos(dims) + list(violations)
        if any(v is STRUCT and n == "a" for n, v in build(FakeAlloc()).args):
            self.violations.insert(0, V("argument struct NULL", S("a", None), E_ARG, CONV))


CONV = "every pointer is a DEVICE pointer owned by the caller"
DIMS = "negative = rejected (MVAE_E_*), nothing enqueued"


def S(name, value, i=None):
    return lambda c: c.set(name, value, i)


def M(*fs):
    def run(c):
        for f in fs:
            f(c)
    return run


def off(name, by, i=None):
    """a pointer moved off its alignment"""
    return lambda c: c.set(name, c.get(name, i) + by, i)


def spare(name, key, i=None):
    return lambda c: c.set(name, c.spare[key], i)


def nulls(fields, i=None, why=CONV):
    return [V("%s NULL" % f, S(f, None, i), E_ARG, why) for f in fields]


def nonpos(fields, i=None, why=DIMS):
    return [V("%s = %d" % (f, v), S(f, v, i), E_ARG, why) for f in fields for v in (0, -16)]


def enum(field, last, why, i=None, code=E_ARG):
    """one past the range and -1: wrongly accepted they select no other buffers"""
    return [V("%s = %d" % (field, v), S(field, v, i), code, why, safe=True) for v in (last + 1, -1)]


# ---- recurrent layers -------------------------------------------------------------------------------------------------------
RH = 256


def _fwd_generic(al, tag="rf"):
    T, B, H, G = 2, 16, 64, 3
    return hl.RnnFwdArgs(cell=hl.GRU, dtype=hl.F32, xmode=hl.X_DENSE, T=T, B=B, H=H, u_pack=al(tag + ".u", (G * H * H,), "f32"),
                         xp=al(tag + ".xp", (T, B, G * H), "f32"), h0=al(tag + ".h0", (B, H), "f32"),
                         hs=al(tag + ".hs", (T + 1, B, H), "f32", out=True), acts=al(tag + ".acts", (T, B, G * H), "f32", out=True),
                         h_last=al(tag + ".hl", (B, H), "f32", out=True))


def _fwd_il(al, tag="ril", cell=hl.LSTM):
    """a problem of the slot-interleaved kernels (H = 256, bf16, MVAE_TILE16P), saving everything"""
    T, B, G = 2, 16, 4 if cell == hl.LSTM else 3
    a = hl.RnnFwdArgs(cell=cell, dtype=hl.BF16, xmode=hl.X_DENSE, T=T, B=B, H=RH, u_pack=al(tag + ".u", (G * RH * RH,), "bf16"),
                      xp=al(tag + ".xp", (T, B, G * RH), "bf16"), hs=al(tag + ".hs", (T + 1, B, RH), "bf16", out=True),
                      acts=al(tag + ".acts", (T, B, G * RH), "bf16", out=True), h_last=al(tag + ".hl", (B, RH), "f32", out=True),
                      seq_layout=hl.TILE16P)
    if cell == hl.LSTM:
        a.cs = al(tag + ".cs", (T + 1, B, RH), "bf16", out=True)
        a.c_last = al(tag + ".cl", (B, RH), "f32", out=True)
    return a


def _bwd_generic(al, tag="rb"):
    T, B, H, G = 2, 16, 64, 3
    return hl.RnnBwdArgs(cell=hl.GRU, dtype=hl.F32, T=T, B=B, H=H, ut_pack=al(tag + ".ut", (G * H * H,), "f32"),
                         hs=al(tag + ".hs", (T + 1, B, H), "f32"), acts=al(tag + ".acts", (T, B, G * H), "f32", data="unit"),
                         dhs_ext=al(tag + ".dhs", (T, B, H), "f32"), dh_last=al(tag + ".dhl", (B, H), "f32"),
                         da=al(tag + ".da", (T, B, G * H), "f32", out=True), rh=al(tag + ".rh", (T, B, H), "f32", out=True),
                         dh0=al(tag + ".dh0", (B, H), "f32", out=True))


def _bwd_il(al, tag="rbil", cell=hl.LSTM):
    T, B, G = 2, 16, 4 if cell == hl.LSTM else 3
    a = hl.RnnBwdArgs(cell=cell, dtype=hl.BF16, T=T, B=B, H=RH, ut_pack=al(tag + ".ut", (G * RH * RH,), "bf16"),
                      hs=al(tag + ".hs", (T + 1, B, RH), "bf16"), acts=al(tag + ".acts", (T, B, G * RH), "bf16", data="unit"),
                      dhs_ext=al(tag + ".dhs", (T, B, RH), "bf16"), dh_last=al(tag + ".dhl", (B, RH), "f32"),
                      da=al(tag + ".da", (T, B, G * RH), "bf16", out=True), dh0=al(tag + ".dh0", (B, RH), "f32", out=True),
                      seq_layout=hl.TILE16P)
    if cell == hl.LSTM:
        a.cs = al(tag + ".cs", (T + 1, B, RH), "bf16")
        a.dc0 = al(tag + ".dc0", (B, RH), "f32", out=True)
    else:
        a.rh = al(tag + ".rh", (T, B, RH), "bf16", out=True)
    return a


def _single(fn, make):
    def build(al):
        a = make(al)
        c = Call(fn, [("a", STRUCT), ("stream", STREAM)], host=a,
                 spare=dict(words=al(fn + ".words", (4,), "i32", data=np.ones(4)), idx=al(fn + ".idx", (2, 16), "u8"),
                            table=al(fn + ".table", (1, 4 * RH), "bf16")))
        return c
    return build


W_CHUNK = "With wait_ready it must be >= 2 (1: MVAE_E_ARG, also from mvae_rnn_fwd_multi)"
W_NEEDS = "hand-over fields need chunk_steps >= 1 (0 with wait_ready or signal_done: MVAE_E_ARG)"
W_HS = "needs hs (MVAE_E_ARG without)"
W_IL = "time-pipelined stacks (slot-interleaved LSTM kernels only; all NULL / 0 otherwise)"
W_LD0 = "row stride of h0 / c0 in floats (0 = H)"


def _fwd_enums(i=None):
    return (enum("cell", 2, "enum { MVAE_GRU = 0, MVAE_LSTM = 1, MVAE_RNN = 2 }", i) +
            enum("dtype", 1, "enum { MVAE_F32 = 0, MVAE_BF16 = 1 }", i) + enum("xmode", 3, "MVAE_X_DENSE .. MVAE_X_CONST", i) +
            enum("seq_layout", 3, "enum { MVAE_ROWMAJOR = 0, MVAE_TILE16 = 1, MVAE_TILE16P = 2, MVAE_TILE16Q = 3 }", i) +
            enum("table_layout", 2, "enum { MVAE_TABLE_ROWMAJOR = 0, MVAE_TABLE_PAIRED = 1, MVAE_TABLE_PAIRED8 = 2 }", i))


def _fwd_handover(i=None):
    return [V("wait_ready, chunk_steps = 0", spare("wait_ready", "words", i), E_ARG, W_NEEDS),
            V("wait_ready, chunk_steps = 1", M(spare("wait_ready", "words", i), S("chunk_steps", 1, i)), E_ARG, W_CHUNK),
            V("signal_done without hs", M(spare("signal_done", "words", i), S("chunk_steps", 2, i), S("hs", None, i)), E_ARG, W_HS),
            V("wait_ready on an indexed input", M(spare("wait_ready", "words", i), S("chunk_steps", 2, i), S("xmode", hl.X_INDEX, i),
                                                  spare("idx", "idx", i), spare("table", "table", i), S("table_layout", 1, i)),
              E_ARG, "wait_ready gates a DENSE input (xp) only: MVAE_E_ARG with any other xmode"),
            V("chunk_steps = -1", S("chunk_steps", -1, i), E_ARG, "time steps per pipeline chunk")]


def _bwd_enums(i=None):
    return (enum("cell", 2, "enum { MVAE_GRU = 0, MVAE_LSTM = 1, MVAE_RNN = 2 }", i) +
            enum("dtype", 1, "enum { MVAE_F32 = 0, MVAE_BF16 = 1 }", i) +
            enum("seq_layout", 3, "enum { MVAE_ROWMAJOR = 0, MVAE_TILE16 = 1, MVAE_TILE16P = 2, MVAE_TILE16Q = 3 }", i))


FWD_PTRS, FWD_DIMS = ("u_pack",), ("T", "B", "H")
BWD_PTRS, BWD_DIMS = ("ut_pack", "hs", "acts", "da"), ("T", "B", "H")


def _multi(fn, make, cap, xpand=False):
    """a phase launch of ONE problem in an array of cap + 1 (so that n = cap + 1 reads real host memory)"""
    def build(al):
        first = make(al)
        arr = (type(first) * (cap + 1))(*([first] * (cap + 1)))
        sp = dict(words=al(fn + ".words", (4,), "i32", data=np.ones(4)), idx=al(fn + ".idx", (2, 16), "u8"),
                  table=al(fn + ".table", (1, 4 * RH), "bf16"))
        if not xpand:
            return Call(fn, [("problems", STRUCT), ("n", 1), ("stream", STREAM)], host=arr, spare=sp)
        R, N = 32, 4 * RH
        x = hl.XpandArgs(xs=al(fn + ".xs", (R,), "f32"), w=al(fn + ".w", (N,), "f32"), bias=al(fn + ".b", (N,), "f32"),
                         out=al(fn + ".xout", (R, N), "bf16", out=True), out_kind=hl.BF16, R=R, N=N, chunk_rows=16,
                         chunk_done=al(fn + ".xdone", (2,), "i32", acc=True), blocks=1)
        xa = (hl.XpandArgs * 3)(x, x, x)
        c = Call(fn, [("problems", STRUCT), ("n", 1), ("xpand", C.addressof(xa)), ("n_xpand", 1), ("stream", STREAM)], host=arr, spare=sp)
        c.keep.append(xa)
        c.xpand = xa
        return c
    return build


def _xp(name, value):
    return lambda c: setattr(c.xpand[0], name, value)


def _xp_off(name, by):
    return lambda c: setattr(c.xpand[0], name, getattr(c.xpand[0], name) + by)


XP = "mvae_xpand_args"
XPAND_V = ([V("xpand[0].%s NULL" % f, _xp(f, None), E_ARG, CONV) for f in ("out", "chunk_done", "xs", "w", "bias")] +
           [V("xpand[0].w off 16 bytes", _xp_off("w", 4), E_ARG, "(N) f32, 16-byte aligned"),
            V("xpand[0].bias off 16 bytes", _xp_off("bias", 8), E_ARG, "(N) f32, 16-byte aligned"),
            V("xpand[0].idx off 4 bytes", M(lambda c: setattr(c.xpand[0], "idx", c.spare["idx"] + 1),
                                            lambda c: setattr(c.xpand[0], "table", c.spare["table"])), E_ARG, "or NULL (4-byte aligned)"),
            V("xpand[0].out_kind = MVAE_F32", _xp("out_kind", hl.F32), E_ARG, "(R, N) out_kind (MVAE_BF16), MVAE_TILE16"),
            V("xpand[0].R = 0", _xp("R", 0), E_ARG, DIMS), V("xpand[0].R = -32", _xp("R", -32), E_ARG, DIMS),
            V("xpand[0].N = 512", _xp("N", 512), E_ARG, "N = the consumer's G*H: 1024 (LSTM) or 768 (GRU), H = 256"),
            V("xpand[0].chunk_rows = 8", _xp("chunk_rows", 8), E_ARG, "rows per published chunk (% 16 == 0, divides R)"),
            V("xpand[0].chunk_rows = 0", _xp("chunk_rows", 0), E_ARG, "rows per published chunk (% 16 == 0, divides R)"),
            V("xpand[0].chunk_rows = 48 of R = 32", _xp("chunk_rows", 48), E_ARG, "rows per published chunk (% 16 == 0, divides R)"),
            V("xpand[0].blocks = 0", _xp("blocks", 0), E_ARG, "workgroups of this producer (<= 256)"),
            V("xpand[0].blocks = 257", _xp("blocks", 257), E_ARG, "workgroups of this producer (<= 256)"),
            V("n_xpand = 3", S("n_xpand", 3), E_ARG, "``xpand``: up to 2 expansions of a 1-feature roll", safe=True),
            V("n_xpand = -1", S("n_xpand", -1), E_ARG, "``xpand``: up to 2 expansions of a 1-feature roll"),
            V("n_xpand = 1, xpand NULL", S("xpand", None), E_ARG, CONV)])
N8 = "n <= 8 problems of the slot-interleaved kernels"


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
def _gemm_generic(al, tag="g", K=16):
    M_, N_ = 16, 16
    return hl.GemmArgs(M=M_, N=N_, K=K, a_kind=hl.F32, b_kind=hl.F32, c_kind=hl.F32, lda=K, ldb=N_, ldc=N_, split_k=1, alpha=1.0,
                       A=al(tag + ".A", (M_, K), "f32"), B=al(tag + ".B", (K, N_), "f32"), C=al(tag + ".C", (M_, N_), "f32", out=True))


def _gemm_wgrad(al, tag="gw", kstream=False):
    """C (128, 128) f32 += A^T B, bf16 operands: the fast kernel's weight-gradient form"""
    M_, N_, K = 128, 128, 64
    g = hl.GemmArgs(M=M_, N=N_, K=K, trans_a=1, a_kind=hl.BF16, b_kind=hl.BF16, c_kind=hl.F32, lda=M_, ldb=N_, ldc=N_, accumulate=1,
                    split_k=1, alpha=1.0, A=al(tag + ".A", (K, M_), "bf16"), B=al(tag + ".B", (K, N_), "bf16"),
                    C=al(tag + ".C", (M_, N_), "f32", acc=True))
    if kstream:         # the one chunk's counter is at its target already: nothing waits
        g.k_wait, g.k_wait_value, g.k_chunk_rows = al(tag + ".kw", (4,), "i32", data=np.ones(4)), 1, K
        g.chunk_status = al(tag + ".st", (1,), "i32", acc=True)
    return g


def _gemm_chunked(al, tag="gc"):
    """persistent chunked mode: C (128, 128) bf16 = A B^T, one chunk, one workgroup, its counter at the target"""
    M_, N_, K = 128, 128, 64
    return hl.GemmArgs(M=M_, N=N_, K=K, trans_b=1, a_kind=hl.BF16, b_kind=hl.BF16, c_kind=hl.BF16, lda=K, ldb=K, ldc=N_, split_k=1,
                       alpha=1.0, A=al(tag + ".A", (M_, K), "bf16"), B=al(tag + ".B", (N_, K), "bf16"),
                       C=al(tag + ".C", (M_, N_), "bf16", out=True), max_blocks=1, chunk_rows=128,
                       chunk_wait=al(tag + ".cw", (4,), "i32", data=np.ones(4)), chunk_wait_value=1,
                       chunk_done=al(tag + ".cd", (4,), "i32", acc=True), chunk_status=al(tag + ".st", (1,), "i32", acc=True))


def _gemm_call(fn, make, cap=0):
    def build(al):
        g = make(al)
        sp = dict(colsum=al(fn + ".colsum", (128,), "f32", acc=True), bias=al(fn + ".bias", (128,), "f32"),
                  words=al(fn + ".words", (4,), "i32", data=np.ones(4)))
        if not cap:
            return Call(fn, [("a", STRUCT), ("stream", STREAM)], host=g, spare=sp)
        arr = (hl.GemmArgs * (cap + 1))(*([g] * (cap + 1)))
        return Call(fn, [("problems", STRUCT), ("n", 1), ("stream", STREAM)], host=arr, spare=sp)
    return build


G_KINDS = "a_kind: MVAE_F32 / MVAE_BF16, or MVAE_A_ONEHOT ... c_kind: MVAE_F32 / MVAE_BF16"
G_LD = "Row-major with leading dimensions (each at least the length of the row it strides over)"


def _gemm_common(i=None):
    return (enum("a_kind", 2, G_KINDS, i) + enum("b_kind", 1, G_KINDS, i) + enum("c_kind", 1, G_KINDS, i) +
            [V("a_kind = 7", S("a_kind", 7, i), E_ARG, G_KINDS, safe=True), V("c_kind = 9", S("c_kind", 9, i), E_ARG, G_KINDS, safe=True),
             V("c_layout = MVAE_TILE16P", S("c_layout", hl.TILE16P, i), E_ARG, "MVAE_ROWMAJOR (ldc applies) or MVAE_TILE16", safe=True),
             V("c_layout = -1", S("c_layout", -1, i), E_ARG, "MVAE_ROWMAJOR (ldc applies) or MVAE_TILE16", safe=True)] +
            enum("act", 1, "enum { MVAE_ACT_NONE = 0, MVAE_ACT_TANH = 1 }", i) +
            [V("%s below its row" % f, lambda c, f=f: c.set(f, c.get(f, i) - 1, i), E_ARG, G_LD) for f in ("lda", "ldb", "ldc")] +
            [V("%s = 0" % f, S(f, 0, i), E_ARG, G_LD) for f in ("lda", "ldb", "ldc")])


G_PTRS, G_DIMS = ("A", "B", "C"), ("M", "N", "K")
KS = "K-streaming (fast bf16 path, trans_a = 1, accumulate = 1, row-major C)"
PERS = "persistent chunked mode (fast bf16 path only, split_k <= 1, max_blocks > 0 = the persistent grid)"
KS_V = [V("k_wait with max_blocks = 1", S("max_blocks", 1, 0), E_ARG, "(max_blocks must be 0)", safe=True),
        V("k_wait without accumulate", S("accumulate", 0, 0), E_ARG, KS, safe=True),
        V("k_wait without trans_a", M(S("trans_a", 0, 0), S("lda", 128, 0)), E_ARG, KS),
        V("k_chunk_rows = 0", S("k_chunk_rows", 0, 0), E_ARG, "The K rows come in chunks of k_chunk_rows"),
        V("k_chunk_rows = 32", S("k_chunk_rows", 32, 0), E_ARG, "k_chunk_rows / split_k a multiple of 64", safe=True),
        V("k_chunk_rows / split_k = 32", S("split_k", 2, 0), E_ARG, "k_chunk_rows / split_k a multiple of 64", safe=True),
        V("K = 96 is no multiple of k_chunk_rows = 64", S("K", 96, 0), E_ARG, "The K rows come in chunks of k_chunk_rows"),
        V("272 workgroups", M(S("M", 17 * 128, 0), S("N", 16 * 128, 0), S("lda", 17 * 128, 0), S("ldb", 16 * 128, 0), S("ldc", 16 * 128, 0)),
          E_ARG, "at most 256 workgroups in all (MVAE_E_ARG beyond)")]


# ---- everything else: positional arguments ---------------------------------------------------------------------------------------
KIND = "MVAE_F32 / MVAE_BF16"


def _head(al):
    R, H, N = 16, 16, 16
    a = hl.HeadArgs(kind=0, dtype=hl.F32, R=R, H=H, N=N, want_grad=1, hs=al("hd.hs", (R, H), "f32"), wt=al("hd.wt", (16, H), "f32"),
                    bias=al("hd.b", (N,), "f32"), target_idx=al("hd.t", (R,), "u8"), grad_scale=1.0,
                    probs=al("hd.p", (R, N), "f32", out=True), argmax=al("hd.am", (R,), "u8", out=True),
                    dlogits=al("hd.dl", (R, 16), "f32", out=True), scalars=al("hd.sc", (2,), "f32", acc=True))
    return Call("mvae_head", [("a", STRUCT), ("stream", STREAM)], host=a,
                spare=dict(dhs=al("hd.dhs", (R, H), "f32", out=True), wc=al("hd.wc", (H, 16), "f32"), tv=al("hd.tv", (R,), "f32")))


def sample_uniforms(R=16, H=16, N=16):
    """one uniform per row of the sampler's baseline, at the CENTRE of bin r % N of the row's CDF (float64, from the inputs the
    baseline is given): the draw of row r is column r % N whatever the last bits of the kernel's f32 CDF are"""
    hs, wt, bias = default_data("hs.hs", (R, H), "f32"), default_data("hs.wt", (16, H), "f32"), default_data("hs.b", (N,), "f32")
    logits = hs @ wt[:N].T + bias
    e = np.exp(logits - logits.max(1, keepdims=True))
    cdf = np.concatenate([np.zeros((R, 1)), np.cumsum(e, 1) / e.sum(1, keepdims=True)], 1)
    k = np.arange(R) % N
    return (0.5 * (cdf[np.arange(R), k] + cdf[np.arange(R), k + 1]))[:, None]


def _sample(al):
    R, H, N = 16, 16, 16
    a = hl.HeadSampleArgs(dtype=hl.F32, R=R, H=H, N=N, hs=al("hs.hs", (R, H), "f32"), wt=al("hs.wt", (16, H), "f32"),
                          bias=al("hs.b", (N,), "f32"), uniforms=al("hs.u", (R, 1), "f32", data=sample_uniforms()),
                          out=al("hs.out", (R,), "u8", out=True), T=1, u_stride=1)
    a.host.temperature, a.host.cutoff, a.host.tries = 1.0, 0.0, 1
    return Call("mvae_head_sample", [("a", STRUCT), ("stream", STREAM)], host=a)


def _host(name, value):
    return lambda c: setattr(c.host.host, name, value)


def _latent_fwd(al, Z=4, Cn=2, tag="lf"):
    B = 4
    a = hl.LatentFwdArgs(B=B, Z=Z, C=Cn, beta=1.0, prior_mean=0.0, prior_std=1.0, inv_batch=1.0 / B, mu=al(tag + ".mu", (B, Z), "f32"),
                         logvar=al(tag + ".lv", (B, Z), "f32"), eps=al(tag + ".eps", (B, Z), "f32"),
                         style_target=al(tag + ".st", (B,), "u8"), z=al(tag + ".z", (B, Z), "f32", out=True),
                         style_probs=al(tag + ".sp", (B, Cn), "f32", out=True), scalars=al(tag + ".sc", (3,), "f32", acc=True))
    return Call("mvae_latent_fwd", [("a", STRUCT), ("stream", STREAM)], host=a)


def _latent_bwd(al):
    B, Z = 4, 4
    a = hl.LatentBwdArgs(B=B, Z=Z, C=0, beta=1.0, prior_mean=0.0, prior_std=1.0, style_weight=1.0, inv_batch=1.0 / B,
                         mu=al("lb.mu", (B, Z), "f32"), logvar=al("lb.lv", (B, Z), "f32"), eps=al("lb.eps", (B, Z), "f32"),
                         dz=al("lb.dz", (B, Z), "f32"), dmu=al("lb.dmu", (B, Z), "f32", out=True),
                         dlogvar=al("lb.dlv", (B, Z), "f32", out=True))
    return Call("mvae_latent_bwd", [("a", STRUCT), ("stream", STREAM)], host=a)


def _chain_fwd(al):
    B, H, Z, zin, ni = 4, 8, 4, 4, 4
    a = hl.LatentChainFwdArgs(B=B, B_valid=B, H=H, Z=Z, C=0, ncat=1, zin=zin, n_init=ni, split=0, beta=1.0, prior_mean=0.0, prior_std=1.0,
                              inv_batch=1.0 / B, cat=al("cf.cat", (B, H), "f32"), w_mu=al("cf.wmu", (H, Z), "f32"),
                              b_mu=al("cf.bmu", (Z,), "f32"), w_lv=al("cf.wlv", (H, Z), "f32"), b_lv=al("cf.blv", (Z,), "f32"),
                              w_init=al("cf.wi", (zin, ni), "f32"), b_init=al("cf.bi", (ni,), "f32"), eps=al("cf.eps", (B, Z), "f32"),
                              mu=al("cf.mu", (B, Z), "f32", out=True), logvar=al("cf.lv", (B, Z), "f32", out=True),
                              zh=al("cf.zh", (B, zin), "f32", out=True), scalars=al("cf.sc", (3,), "f32", acc=True),
                              S=al("cf.S", (B, ni), "f32", out=True))
    return Call("mvae_latent_chain_fwd", [("a", STRUCT), ("stream", STREAM)], host=a,
                spare=dict(st=al("cf.st", (B,), "u8"), wpack=al("cf.wp", (3 * H, H), "f32")))


def _chain_bwd(al):
    B, H, Z, zin, ni = 4, 8, 4, 4, 4
    a = hl.LatentChainBwdArgs(B=B, B_valid=B, H=H, Z=Z, C=0, ncat=1, zin=zin, n_init=ni, split=0, beta=1.0, prior_mean=0.0, prior_std=1.0,
                              style_weight=1.0, inv_batch=1.0 / B, wt_mu=al("cb.wmu", (Z, H), "f32"), wt_lv=al("cb.wlv", (Z, H), "f32"),
                              wt_init=al("cb.wi", (ni, zin), "f32"), S=al("cb.S", (B, ni), "f32"), mu=al("cb.mu", (B, Z), "f32"),
                              logvar=al("cb.lv", (B, Z), "f32"), eps=al("cb.eps", (B, Z), "f32"), dS=al("cb.dS", (B, ni), "f32"),
                              dzh=al("cb.dzh", (B, zin), "f32", out=True), dmu=al("cb.dmu", (B, Z), "f32", out=True),
                              dlogvar=al("cb.dlv", (B, Z), "f32", out=True), dcat=al("cb.dcat", (B, H), "f32", out=True))
    return Call("mvae_latent_chain_bwd", [("a", STRUCT), ("stream", STREAM)], host=a)


CHAIN = "B % 4 == 0 (rows >= B_valid are padding ...); H % 8, Z % 4, zin % 4 == 0"
CHAIN_V = [V("B = 2", S("B", 2), E_ARG, CHAIN), V("H = 4", S("H", 4), E_ARG, CHAIN), V("Z = 2", S("Z", 2), E_ARG, CHAIN),
           V("zin = 6", S("zin", 6), E_ARG, CHAIN), V("zin = 0 < Z", S("zin", 0), E_ARG, "zh (B,zin): columns [0,Z) out"),
           V("ncat = 0", S("ncat", 0), E_ARG, "cat (B, ncat*H)"),
           V("ncat = 3 without the pack Dense", S("ncat", 3), E_ARG, "pack Dense (tanh, when w_pack): without it ncat must be 1"),
           V("n_init = 6", S("n_init", 6), E_ARG, "n_init /* columns of S */ a multiple of 4"),
           V("zin = 65536: more LDS than a CU has", S("zin", 1 << 16), E_UNS, "MVAE_E_UNSUPPORTED: the rows of one workgroup need more than 160 KiB of LDS")]


# ---- mvae_prepare_batch ----------------------------------------------------------------------------------------------------------
def _prep(al):
    """one job per op, each the smallest its single call accepts"""
    J, P = hl.PrepJob, "pb."
    jobs = [J(hl.PREP_PACK_RECURRENT, hl.F32, 16, 48, 0, 0, al(P + "U", (16, 48), "f32"), None, al(P + "up", (16 * 48,), "f32", out=True)),
            J(hl.PREP_MAKE_TABLE, hl.F32, 2, 256, 0, 0, al(P + "W", (2, 256), "f32"), al(P + "b", (256,), "f32"), al(P + "tab", (2, 256), "f32", out=True)),
            J(hl.PREP_TRANSPOSE_CONVERT, hl.BF16, 3, 5, 8, 0, al(P + "Wt", (3, 5), "f32"), None, al(P + "wt", (8, 3), "bf16", out=True)),
            J(hl.PREP_CONVERT, hl.BF16, 10, 1, 0, 0, al(P + "cs", (10,), "f32"), None, al(P + "cd", (10,), "bf16", out=True)),
            J(hl.PREP_ZERO, hl.F32, 6, 1, 0, 0, None, None, al(P + "z", (6,), "f32", out=True)),
            J(hl.PREP_CONVERT_PAD, hl.F32, 3, 5, 8, 0, al(P + "ps", (3, 5), "f32"), None, al(P + "pd", (3, 8), "f32", out=True)),
            J(hl.PREP_ADD_I32, hl.F32, 1, 0, 0, 0, None, None, al(P + "cnt", (1,), "i32", acc=True)),
            J(hl.PREP_BROADCAST_ROWS, hl.BF16, 3, 6, 0, 0, al(P + "row", (6,), "f32"), None, al(P + "br", (3, 6), "bf16", out=True))]
    arr = (J * len(jobs))(*jobs)
    return Call("mvae_prepare_batch", [("jobs", STRUCT), ("n_jobs", len(jobs)), ("stream", STREAM)], host=arr,
                spare=dict(latch=al(P + "latch", (1,), "i32", acc=True)))


def _many(n, bad_at):
    """n jobs - the baseline's eight, over and over (each rewrites what the last one wrote) - with op = 99 at one position"""
    def run(c):
        base = list(c.host)
        arr = (hl.PrepJob * n)(*[base[j % len(base)] for j in range(n)])
        arr[bad_at].op = 99
        c.host = arr
        c.set("n_jobs", n)
    return run


JOB = "Each job is one of the single calls above"
PK, MT, TC, CV, ZE, CP, AD, BR = range(8)
PREP_V = ([V("jobs NULL", S("jobs", None), E_ARG, "jobs /* host array */"), V("n_jobs = -1", S("n_jobs", -1), E_ARG, DIMS)] +
          [V("job %d of %d: op = 99" % (p, n), _many(n, p), E_ARG, JOB + " (all jobs are checked before the first launch)", safe=True)
           for n, p in ((65, 0), (65, 63), (65, 64), (130, 129))] +
          enum("op", 7, "enum { MVAE_PREP_PACK_RECURRENT = 0, ... MVAE_PREP_BROADCAST_ROWS = 7 }", CV) +
          enum("kind", 1, "element kind of dst (MVAE_F32 / MVAE_BF16)", ZE) +
          [V("job %d: dst NULL" % j, S("dst", None, j), E_ARG, CONV) for j in range(8)] +
          [V("job %d: src NULL" % j, S("src", None, j), E_ARG, CONV) for j in (PK, MT, TC, CV, CP, BR)] +
          [V("job %d: %s = %d" % (j, f, v), S(f, v, j), E_ARG, JOB + ": extents are positive")
           for j in (PK, MT, TC, CV, ZE, CP, BR) for f in ("a", "b") for v in (0, -5)] +
          [V("PACK_RECURRENT: a = 8", S("a", 8, PK), E_ARG, "src = U (a=H, b=G*H): multiples of 16"),
           V("PACK_RECURRENT: b = 40", S("b", 40, PK), E_ARG, "src = U (a=H, b=G*H): multiples of 16"),
           V("PACK_RECURRENT: c = 2", S("c", 2, PK), E_ARG, "c = direction (0 or 1)", safe=True),
           V("PACK_RECURRENT: c = -1", S("c", -1, PK), E_ARG, "c = direction (0 or 1)", safe=True),
           V("PACK_RECURRENT bf16: a = 16 is no multiple of 32", S("kind", hl.BF16, PK), E_ARG, "the contraction length a multiple of the MFMA's K group", safe=True),
           V("MAKE_TABLE: src2 NULL", S("src2", None, MT), E_ARG, "src2 = bias (N)"),
           V("MAKE_TABLE: c = 3", S("c", 3, MT), E_ARG, "c = layout", safe=True),
               V("MAKE_TABLE: c = -1", S("c", -1, MT), E_ARG, "c = layout", safe=True),
           V("MAKE_TABLE paired: b = 48", M(S("c", 1, MT), S("b", 48, MT)), E_ARG, "MVAE_TABLE_PAIRED (cols % 32 == 0)", safe=True),
           V("MAKE_TABLE paired8: b = 128", M(S("c", 2, MT), S("b", 128, MT)), E_ARG, "MVAE_TABLE_PAIRED8 (cols % 256 == 0)", safe=True),
           V("TRANSPOSE_CONVERT: c = 4 < b", S("c", 4, TC), E_ARG, "c = N_pad (>= N, as mvae_transpose_convert)", safe=True),
           V("TRANSPOSE_CONVERT: c = -8", S("c", -8, TC), E_ARG, "c = N_pad (>= N, as mvae_transpose_convert)"),
           V("CONVERT_PAD: c = 4 < b", S("c", 4, CP), E_ARG, "c = padded row length >= b", safe=True),
           V("ZERO bf16: a*b odd", M(S("kind", hl.BF16, ZE), S("a", 5, ZE)), E_ARG, "a*b even for bf16", safe=True),
           V("ADD_I32: a latch without a guard word", spare("src2", "latch", AD), E_ARG, "src2 = NULL or a latch word ... a non-zero *src is then moved there", safe=True),
           V("BROADCAST_ROWS: a = -5", S("a", -5, BR), E_ARG, JOB + ": extents are positive")])


def _p(fn, names, make, **kw):
    """an entry point with positional arguments: ``make(al)`` returns the values in the order of ``names`` (stream excluded) and spares"""
    def build(al):
        vals, sp = make(al)
        args = [[n, v] for n, v in zip(names, vals)]
        assert len(args) == len(names)
        return Call(fn, args, spare=sp)
    return build


def _kind_enum(field="kind"):
    return enum(field, 1, KIND)


ENTRIES = [
    Entry("mvae_rnn_fwd", _single("mvae_rnn_fwd", _fwd_generic), ptrs=FWD_PTRS, dims=FWD_DIMS, violations=_fwd_enums() + [
        V("xp NULL (MVAE_X_DENSE)", S("xp", None), E_ARG, "DENSE: (T,B,G*H) dtype"),
        V("h0_ld = H - 1", S("h0_ld", 63), E_ARG, W_LD0), V("h0_ld = -1", S("h0_ld", -1), E_ARG, W_LD0),
        V("h_last_ld = H - 1", S("h_last_ld", 63), E_ARG, "row stride of h_last (0 = H)"),
        V("H = 96: no kernel", S("H", 96), E_UNS, "MVAE_E_UNSUPPORTED (shape/dtype not built)"),
        V("wait_ready, chunk_steps = 0", spare("wait_ready", "words"), E_ARG, W_NEEDS),
        V("chunk_steps = -1", S("chunk_steps", -1), E_ARG, "time steps per pipeline chunk"),
        V("hand-over fields on a row-major layout", M(spare("signal_done", "words"), S("chunk_steps", 2)), E_UNS, W_IL, safe=True),
        V("MVAE_TILE16 at H = 64 f32", S("seq_layout", hl.TILE16), E_UNS, "The tiled layouts ... select the resident-weights kernels (H=256, bf16)", safe=True),
        V("INDEX with a paired table on the generic kernels", M(S("xmode", hl.X_INDEX), spare("idx", "idx"), spare("table", "table"), S("table_layout", 1)),
          E_ARG, "every other kernel takes the row-major table")],
          accepted=[("h0_ld = h_last_ld = H, as 0 is", M(S("h0_ld", 64), S("h_last_ld", 64)), LAUNCH)]),
    Entry("mvae_rnn_fwd", _single("mvae_rnn_fwd", _fwd_il), label="mvae_rnn_fwd[TILE16P]", ptrs=FWD_PTRS, dims=FWD_DIMS,
          violations=_fwd_enums() + _fwd_handover() + [
        V("B = 8", S("B", 8), E_UNS, "The tiled layouts need B % 16 == 0"),
        V("xp NULL (MVAE_X_DENSE)", S("xp", None), E_ARG, "DENSE: (T,B,G*H) dtype"),
        V("h_last_ld = 255", S("h_last_ld", 255), E_ARG, "row stride of h_last (0 = H)"),
        V("INDEX with a row-major table", M(S("xmode", hl.X_INDEX), spare("idx", "idx"), spare("table", "table")), E_ARG,
          "MVAE_TABLE_PAIRED ... what the slot-interleaved LSTM and GRU kernels (MVAE_TILE16P) REQUIRE"),
        V("SCALAR input without xs", S("xmode", hl.X_SCALAR), E_ARG, "SCALAR: xs, w_row, bias")]),
    Entry("mvae_rnn_bwd", _single("mvae_rnn_bwd", _bwd_generic), ptrs=BWD_PTRS, dims=BWD_DIMS, violations=_bwd_enums() + [
        V("dh_last_ld = H - 1", S("dh_last_ld", 63), E_ARG, "row stride of dh_last (0 = H)"),
        V("dh0_ld = H - 1", S("dh0_ld", 63), E_ARG, "row stride of dh0 / dc0 (0 = H)"),
        V("dh0_ld = -1", S("dh0_ld", -1), E_ARG, "row stride of dh0 / dc0 (0 = H)"),
        V("LSTM without cs", S("cell", hl.LSTM), E_ARG, "LSTM: (T+1,B,H) dtype"),
        V("H = 96: no kernel", S("H", 96), E_UNS, "MVAE_E_UNSUPPORTED (shape/dtype not built)"),
        V("wait_ready, chunk_steps = 0", spare("wait_ready", "words"), E_ARG, W_NEEDS),
        V("chunk_steps = -1", S("chunk_steps", -1), E_ARG, "chunk_steps may be 1 here"),
        V("hand-over fields on a row-major layout", M(spare("signal_done", "words"), S("chunk_steps", 1)), E_UNS, W_IL, safe=True)],
          accepted=[("dh_last_ld = dh0_ld = H, as 0 is", M(S("dh_last_ld", 64), S("dh0_ld", 64)), LAUNCH)]),
    Entry("mvae_rnn_bwd", _single("mvae_rnn_bwd", _bwd_il), label="mvae_rnn_bwd[TILE16P]", ptrs=BWD_PTRS, dims=BWD_DIMS,
          violations=_bwd_enums() + [
        V("wait_ready without dhs_ext", M(spare("wait_ready", "words"), S("chunk_steps", 1), S("dhs_ext", None)), E_ARG, "wait_ready gates dhs_ext"),
        V("LSTM without cs", S("cs", None), E_ARG, "LSTM: (T+1,B,H) dtype"),
        V("B = 8", S("B", 8), E_UNS, "The tiled layouts need B % 16 == 0")]),
    Entry("mvae_rnn_fwd_multi", _multi("mvae_rnn_fwd_multi", _fwd_il, 8, xpand=True), ptrs=("problems",), dims=(),
          violations=nulls(FWD_PTRS, 0) + nonpos(FWD_DIMS, 0) + _fwd_enums(0) + _fwd_handover(0) + XPAND_V + [
        V("n = 0", S("n", 0), E_ARG, N8), V("n = -1", S("n", -1), E_ARG, N8), V("n = 9", S("n", 9), E_ARG, N8, safe=True),
        V("B = 8", S("B", 8, 0), E_ARG, "The tiled layouts need B % 16 == 0"),
        V("xp NULL (MVAE_X_DENSE)", S("xp", None, 0), E_ARG, "DENSE: (T,B,G*H) dtype"),
        V("INDEX with a row-major table", M(S("xmode", hl.X_INDEX, 0), spare("idx", "idx", 0), spare("table", "table", 0)), E_ARG,
          "MVAE_TABLE_PAIRED ... what the slot-interleaved LSTM and GRU kernels (MVAE_TILE16P) REQUIRE"),
        V("a row-major problem", S("seq_layout", hl.ROWMAJOR, 0), E_UNS, "MVAE_E_UNSUPPORTED: some problem is not one of these kernels'", safe=True),
        V("a SCALAR input", S("xmode", hl.X_SCALAR, 0), E_UNS, "MVAE_E_UNSUPPORTED: some problem is not one of these kernels'"),
        V("mixed cell types", M(S("n", 2), S("cell", hl.GRU, 1)), E_UNS, "all of one cell type", safe=True),
        V("the bad problem is the last of 8", M(S("n", 8), S("xmode", 9, 7)), E_ARG, N8, safe=True)]),
    Entry("mvae_rnn_bwd_multi", _multi("mvae_rnn_bwd_multi", _bwd_il, 8), ptrs=("problems",), dims=(),
          violations=nulls(BWD_PTRS, 0) + nonpos(BWD_DIMS, 0) + _bwd_enums(0) + [
        V("n = 0", S("n", 0), E_ARG, N8), V("n = -1", S("n", -1), E_ARG, N8), V("n = 9", S("n", 9), E_ARG, N8, safe=True),
        V("B = 8", S("B", 8, 0), E_ARG, "The tiled layouts need B % 16 == 0"),
        V("LSTM without cs", S("cs", None, 0), E_ARG, "LSTM: (T+1,B,H) dtype"),
        V("dh0_ld = 255", S("dh0_ld", 255, 0), E_ARG, "row stride of dh0 / dc0 (0 = H)"),
        V("wait_ready without dhs_ext", M(spare("wait_ready", "words", 0), S("chunk_steps", 1, 0), S("dhs_ext", None, 0)), E_ARG, "wait_ready gates dhs_ext"),
        V("wait_ready, chunk_steps = 0", spare("wait_ready", "words", 0), E_ARG, W_NEEDS),
        V("a row-major problem", S("seq_layout", hl.ROWMAJOR, 0), E_UNS, "MVAE_E_UNSUPPORTED: some problem is not one of these kernels'", safe=True),
        V("mixed cell types", M(S("n", 2), S("cell", hl.GRU, 1)), E_UNS, "all of one cell type", safe=True),
        V("the bad problem is the last of 8", M(S("n", 8), S("cell", 9, 7)), E_ARG, N8, safe=True)]),
    Entry("mvae_pack_recurrent", _p("mvae_pack_recurrent", ("U", "out", "cell", "H", "dtype", "direction", "stream"),
                                    lambda al: ((al("pr.U", (64, 192), "f32"), al("pr.out", (192 * 64,), "f32", out=True), hl.GRU, 64, hl.F32, 0, STREAM), {})),
          ptrs=("U", "out"), dims=(),
              violations=enum("cell", 2, "cell") + _kind_enum("dtype") + enum("direction", 1, "direction 0: forward ... direction 1: backward") + [
              V("H = 0", S("H", 0), E_ARG, "U (H, G*H): H a positive multiple of 64"),
                  V("H = -64", S("H", -64), E_ARG, "U (H, G*H): H a positive multiple of 64"),
              V("H = 32", S("H", 32), E_ARG, "U (H, G*H): H a positive multiple of 64")]),
    Entry("mvae_gemm", _gemm_call("mvae_gemm", _gemm_generic), ptrs=G_PTRS, dims=G_DIMS, violations=_gemm_common() + [
        V("split_k = 2 without accumulate", S("split_k", 2), E_ARG, "accumulate: 0 store, 1 atomic add into f32 C (split-K allowed)", safe=True),
        V("accumulate into bf16", M(S("accumulate", 1), S("c_kind", hl.BF16)), E_ARG, "1 atomic add into f32 C", safe=True),
        V("act with accumulate", M(S("accumulate", 1), S("act", hl.ACT_TANH)), E_ARG, "[-> tanh] of a stored C only", safe=True),
        V("TILE16 store with accumulate", M(S("accumulate", 1), S("c_layout", hl.TILE16)), E_ARG, "MVAE_TILE16 (store only, M%16==0, N%16==0)", safe=True),
        V("TILE16 store, M = 8", M(S("c_layout", hl.TILE16), S("M", 8)), E_ARG, "MVAE_TILE16 (store only, M%16==0, N%16==0)"),
        V("TILE16 store, N = 8", M(S("c_layout", hl.TILE16), S("N", 8)), E_ARG, "MVAE_TILE16 (store only, M%16==0, N%16==0)"),
        V("MVAE_A_ONEHOT without trans_a", S("a_kind", hl.ONEHOT), E_ARG, "(requires trans_a = 1)", safe=True),
        V("colsum_b off its path", spare("colsum_b", "colsum"), E_UNS, "Fast bf16 path with trans_a = 1, trans_b = 0 and accumulate only (else MVAE_E_UNSUPPORTED)", safe=True),
        V("k_wait off the fast path", M(spare("k_wait", "words"), S("k_chunk_rows", 16)), E_ARG, KS, safe=True),
        V("chunk_rows off the fast path", M(S("chunk_rows", 128), S("max_blocks", 1), S("M", 128), S("lda", 16)), E_UNS, PERS),
        V("split_k = -1", S("split_k", -1), E_ARG, "split_k"),
            V("max_blocks = -1", S("max_blocks", -1), E_ARG, "max_blocks: 0 = one workgroup per output tile; >0")],
          accepted=[("a one-hot A with lda = 0 (not read)", M(S("a_kind", hl.ONEHOT), S("trans_a", 1), S("lda", 0)), LAUNCH)]),
    Entry("mvae_gemm", _gemm_call("mvae_gemm",
        lambda al: _gemm_generic(al, "gs", 512)), label="mvae_gemm[self-splitting store]", ptrs=G_PTRS, dims=G_DIMS,
          violations=[V("a_kind = 7", S("a_kind", 7), E_ARG, G_KINDS + " (nothing enqueued: not the fill of C either)", safe=True),
                      V("b_kind = 7", S("b_kind", 7), E_ARG, G_KINDS + " (nothing enqueued: not the fill of C either)", safe=True)]),
    Entry("mvae_gemm", _gemm_call("mvae_gemm", lambda al: _gemm_wgrad(al, "gk", True)), label="mvae_gemm[K-streaming]", ptrs=G_PTRS, dims=G_DIMS,
          violations=_gemm_common() + KS_V +
              [V("colsum_b with a narrow N", M(spare("colsum_b", "colsum"), S("N", 64)), E_UNS, "colsum_b: Fast bf16 path ... (else MVAE_E_UNSUPPORTED)")]),
    Entry("mvae_gemm", _gemm_call("mvae_gemm", _gemm_chunked), label="mvae_gemm[persistent chunks]", ptrs=G_PTRS, dims=G_DIMS, violations=[
        V("chunk_rows = 64", S("chunk_rows", 64), E_ARG, "chunks of chunk_rows (multiple of 128)", safe=True),
        V("chunk_rows = -128", S("chunk_rows", -128), E_ARG, "chunks of chunk_rows (multiple of 128)"),
        V("chunk_rows = 256 does not divide M", S("chunk_rows", 256), E_ARG, "the M rows are processed in chunks of chunk_rows"),
        V("split_k = 2", S("split_k", 2), E_ARG, PERS, safe=True), V("max_blocks = 0", S("max_blocks", 0), E_ARG, PERS, safe=True),
        V("max_blocks = 257", S("max_blocks", 257), E_ARG, "max_blocks > 0 = the persistent grid (at most 256 workgroups)", safe=True),
        V("accumulate", M(S("accumulate", 1), S("c_kind", hl.F32)), E_ARG, PERS)]),
    Entry("mvae_gemm_kstream_multi", _gemm_call("mvae_gemm_kstream_multi", lambda al: _gemm_wgrad(al, "gkm", True), 8), ptrs=("problems",), dims=(),
          violations=nulls(G_PTRS, 0) + nonpos(G_DIMS, 0) + _gemm_common(0) + KS_V + [
        V("n = 0", S("n", 0), E_ARG, "n <= 8 K-streaming problems"), V("n = -1", S("n", -1), E_ARG, "n <= 8 K-streaming problems"),
        V("n = 9", S("n", 9), E_ARG, "n <= 8 K-streaming problems", safe=True),
        V("a problem without k_wait", S("k_wait", None, 0), E_ARG, "K-streaming problems (k_wait set, ...)"),
        V("trans_b", M(S("trans_b", 1, 0), S("ldb", 64, 0)), E_ARG, "(k_wait set, trans_a = 1, trans_b = 0, accumulate, no bias)"),
        V("a bias", spare("bias", "bias", 0), E_ARG, "(k_wait set, trans_a = 1, trans_b = 0, accumulate, no bias)", safe=True),
        V("the bad problem is the last of 8", M(S("n", 8), S("a_kind", 7, 7)), E_ARG, G_KINDS, safe=True)]),
    Entry("mvae_gemm_multi", _gemm_call("mvae_gemm_multi", lambda al: _gemm_wgrad(al, "gm"), 16), ptrs=("problems",), dims=(),
          violations=nulls(G_PTRS, 0) + nonpos(G_DIMS, 0) + _gemm_common(0) + [
        V("n = 0", S("n", 0), E_ARG, "n <= 16 ORDINARY weight-gradient GEMMs"),
            V("n = -1", S("n", -1), E_ARG, "n <= 16 ORDINARY weight-gradient GEMMs"),
        V("n = 17", S("n", 17), E_ARG, "n <= 16 ORDINARY weight-gradient GEMMs", safe=True),
        V("a bias", spare("bias", "bias", 0), E_ARG, "every problem C (M,N) f32 row-major += A^T B", safe=True),
        V("trans_a = 0", M(S("trans_a", 0, 0), S("lda", 64, 0)), E_UNS, "every problem C (M,N) f32 row-major += A^T B with trans_a = 1"),
        V("a storing problem", S("accumulate", 0, 0), E_UNS, "MVAE_E_UNSUPPORTED: a problem is not of this form", safe=True),
        V("k_wait set", spare("k_wait", "words", 0), E_UNS, "none of the chunk_* / k_wait fields", safe=True),
        V("max_blocks = 4", S("max_blocks", 4, 0), E_UNS, "MVAE_E_UNSUPPORTED: a problem is not of this form", safe=True),
        V("f32 operands", M(S("a_kind", hl.F32, 0), S("b_kind", hl.F32, 0)), E_UNS, "bf16 or MVAE_A_ONEHOT A, bf16 B"),
        V("the bad problem is the last of 16", M(S("n", 16), S("c_kind", 9, 15)), E_ARG, G_KINDS, safe=True)]),
    Entry("mvae_stream_wait_value32", _p("mvae_stream_wait_value32", ("stream", "addr", "value"),
                                         lambda al: ((STREAM, al("sw.w", (1,), "i32", data=np.ones(1)), 1), {})), ptrs=("addr",), violations=[]),
    Entry("mvae_stream_write_value32", _p("mvae_stream_write_value32", ("stream", "addr", "value"),
                                          lambda al: ((STREAM, al("sv.w", (1,), "i32", acc=True), 5), {})), ptrs=("addr",), violations=[]),
    Entry("mvae_streams_alias", _p("mvae_streams_alias", ("stream_a", "stream_b", "scratch", "tag"),
                                   lambda al: ((STREAM, STREAM, al("sa.w", (2,), "i32", acc=True), 7), {})), ptrs=("scratch",), cpu_baseline=False,
          violations=[V("tag = 0", S("tag", 0), E_ARG, "`tag` != 0 a value not used before on them", safe=True)]),
    Entry("mvae_occupancy", _p("mvae_occupancy", ("which",), lambda al: ((0,), {})), cpu_baseline=False,
          violations=[V("which = 3", S("which", 3), E_ARG, "which = 0 ... 1 ... 2", safe=True, enq=False),
                      V("which = -1", S("which", -1), E_ARG, "which = 0 ... 1 ... 2", safe=True, enq=False)]),
    Entry("mvae_colsum", _p("mvae_colsum", ("X", "kind", "R", "N", "ldx", "out", "stream"),
                            lambda al: ((al("cs.X", (16, 16), "f32"), hl.F32, 16, 16, 16, al("cs.out", (16,), "f32", acc=True), STREAM), {})),
          ptrs=("X", "out"), dims=("R", "N"), violations=_kind_enum() + [V("ldx = N - 1", S("ldx", 15), E_ARG, "ldx elements between rows (>= N)")]),
    Entry("mvae_colsum_weighted", _p("mvae_colsum_weighted", ("X", "kind", "wgt", "R", "N", "ldx", "out", "stream"),
                                     lambda al: ((al("cw.X", (16, 16), "f32"), hl.F32, al("cw.w", (16,), "f32"), 16, 16, 16, al("cw.out", (16,), "f32", acc=True), STREAM), {})),
          ptrs=("X", "wgt", "out"), dims=("R", "N"),
              violations=_kind_enum() +
              [V("ldx = N - 1", S("ldx", 15), E_ARG, "ldx elements between rows (>= N)")]),
    Entry("mvae_sum_over_time", _p("mvae_sum_over_time", ("X", "kind", "T", "BN", "out", "accumulate", "stream"),
                                   lambda al: ((al("st.X", (2, 16), "f32"), hl.F32, 2, 16, al("st.out", (16,), "f32", out=True), 0, STREAM), {})),
          ptrs=("X", "out"), dims=("T", "BN"), violations=_kind_enum() + [
              V("kind = 7, accumulate = 0", S("kind", 7), E_ARG, KIND + " (nothing enqueued: not the fill of out either)", safe=True)]),
    Entry("mvae_head", _head, ptrs=("hs", "wt", "bias"), dims=("R", "H", "N"),
        violations=enum("kind", 1, "kind 0: softmax ... kind 1: sigmoid") + _kind_enum("dtype") + [
        V("kind = 2, N = 61", M(S("kind", 2), S("N", 61)), E_ARG, "kind 0: softmax ... kind 1: sigmoid"),
        V("want_grad without dlogits", S("dlogits", None), E_ARG, "required if want_grad"),
        V("kind 1 with N = 16", S("kind", 1), E_ARG, "kind 1: sigmoid + squared error (targets f32 per row), N must be 1", safe=True),
        V("N = 193", S("N", 193), E_UNS, "< 0 = too wide: mvae_head then returns MVAE_E_UNSUPPORTED and launches nothing"),
        V("H = 8", S("H", 8), E_UNS, "MVAE_E_UNSUPPORTED: H a multiple of 16 (f32) / 32 (bf16)"),
        V("dhs without wc", spare("dhs", "dhs"), E_ARG, "(needs wc, want_grad, R % 16 == 0, H <= 256)"),
        V("dhs without want_grad", M(spare("dhs", "dhs"), spare("wc", "wc"), S("want_grad", 0)), E_ARG, "(needs wc, want_grad, R % 16 == 0, H <= 256)", safe=True),
        V("dhs with R = 8", M(spare("dhs", "dhs"), spare("wc", "wc"), S("R", 8)), E_ARG, "(needs wc, want_grad, R % 16 == 0, H <= 256)"),
        V("dhs with H = 320", M(spare("dhs", "dhs"), spare("wc", "wc"), S("H", 320)), E_UNS, "(needs wc, want_grad, R % 16 == 0, H <= 256)")],
        accepted=[("decode: target_idx, target_val, row_weight and scalars NULL, no gradient",
                   M(S("target_idx", None), S("scalars", None), S("want_grad", 0), S("dlogits", None)), LAUNCH),
                  ("scalars NULL with targets", S("scalars", None), LAUNCH), ("row_weight given", spare("row_weight", "tv"), LAUNCH)]),
    Entry("mvae_head_sample", _sample, ptrs=("hs", "wt", "bias", "out"), dims=("R", "H", "N"), violations=_kind_enum("dtype") + [
        V("temperature = 0", _host("temperature", 0.0), E_ARG, "temperature <= 0 MVAE_E_ARG", safe=True),
        V("temperature = -1", _host("temperature", -1.0), E_ARG, "temperature <= 0 MVAE_E_ARG", safe=True),
        V("cutoff = -1", _host("cutoff", -1.0), E_ARG, ">= 0 (cutoff_sample_threshold)", safe=True),
        V("tries = 0", _host("tries", 0), E_ARG, "1..4 (number_of_tries)", safe=True),
            V("tries = 5", _host("tries", 5), E_UNS, "tries > 4 MVAE_E_UNSUPPORTED", safe=True),
        V("N = 193", S("N", 193), E_UNS, "NP = mvae_head_np(N)"),
            V("H = 8", S("H", 8), E_UNS, "MVAE_E_UNSUPPORTED: H a multiple of 16 (f32) / 32 (bf16)"),
        V("u_stride = 1 < tries = 2", _host("tries", 2), E_ARG, "values per row of `uniforms` (>= tries)"),
        V("u_stride = 0", S("u_stride", 0), E_ARG, "values per row of `uniforms` (>= tries)"),
        V("row0 = -1", S("row0", -1), E_ARG, "device row of this launch's first row"), V("b_stride = -1", S("b_stride", -1), E_ARG, "b_stride"),
        V("b_stride = 16 with T = 0", M(S("b_stride", 16), S("T", 0)), E_ARG, "steps per window", safe=True)]),
    Entry("mvae_latent_fwd", _latent_fwd, ptrs=("mu", "logvar", "eps", "z", "scalars"), dims=("B", "Z"), violations=[
        V("C = 0 with a style target", S("C", 0), E_ARG, "style classifier on z[:, :C]", safe=True),
        V("C = 65", S("C", 65), E_ARG, "C <= 64, C <= Z"), V("C = 5 > Z = 4", S("C", 5), E_ARG, "C <= 64, C <= Z"),
        V("ldz = Z - 1", S("ldz", 3), E_ARG, "row stride of z (0 = Z)"), V("ldz = -4", S("ldz", -4), E_ARG, "row stride of z (0 = Z)")],
          accepted=[("ldz = Z, as 0 is", S("ldz", 4), LAUNCH)]),
    Entry("mvae_latent_bwd", _latent_bwd, ptrs=("mu", "logvar", "eps", "dz", "dmu", "dlogvar"), dims=("B", "Z"), violations=[
        V("lddz = Z - 1", S("lddz", 3), E_ARG, "row stride of dz (0 = Z)"), V("lddz = -4", S("lddz", -4), E_ARG, "row stride of dz (0 = Z)")],
          accepted=[("lddz = Z, as 0 is", S("lddz", 4), LAUNCH)]),
    Entry("mvae_latent_chain_fwd", _chain_fwd, ptrs=("cat", "w_mu", "w_lv", "mu", "logvar", "eps", "zh", "scalars"), dims=("B", "H", "Z"),
          violations=CHAIN_V + [V("w_init without S", S("S", None), E_ARG, "S (B,n_init) out"),
                                V("w_pack without pack", spare("w_pack", "wpack"), E_ARG, "pack, extra (B,H) out (kept for backward)"),
                                V("C = 65 with a style target", M(spare("style_target", "st"), S("C", 65)), E_ARG, "as mvae_latent_fwd_args"),
                                V("C = 0 with a style target", spare("style_target", "st"), E_ARG, "as mvae_latent_fwd_args")]),
    Entry("mvae_latent_chain_bwd", _chain_bwd, ptrs=("S", "dS", "wt_init", "wt_mu", "wt_lv", "mu", "logvar", "eps", "dzh", "dmu", "dlogvar", "dcat"),
          dims=("B", "H", "Z", "n_init"), violations=CHAIN_V),
    Entry("mvae_prepare_batch", _prep, violations=PREP_V),
    Entry("mvae_outer_bias_tile16", _p("mvae_outer_bias_tile16", ("xs", "w", "bias", "out", "out_kind", "R", "N", "stream"),
                                       lambda al: ((al("ob.xs", (16,), "f32"), al("ob.w", (16,), "f32"), al("ob.b", (16,), "f32"), al("ob.out", (16, 16), "f32", out=True), hl.F32, 16, 16, STREAM), {})),
          ptrs=("xs", "w", "bias", "out"), dims=("R", "N"), violations=_kind_enum("out_kind") + [
              V("R = 8", S("R", 8), E_ARG, "(R % 16 == 0, N % 16 == 0, w and bias 16-byte aligned)"),
                  V("N = 8", S("N", 8), E_ARG, "(R % 16 == 0, N % 16 == 0, w and bias 16-byte aligned)"),
              V("w off 16 bytes", off("w", 4), E_ARG, "w and bias 16-byte aligned"),
                  V("bias off 16 bytes", off("bias", 8), E_ARG, "w and bias 16-byte aligned")]),
    Entry("mvae_gather2_tile16", _p("mvae_gather2_tile16", ("idx", "idx2", "table", "table2", "out", "kind", "R", "N", "layout", "stream"),
                                    lambda al: ((al("g2.i", (16,), "u8"), al("g2.j", (16,), "u8"), al("g2.t", (1, 16), "f32"), al("g2.u", (1, 16), "f32"), al("g2.out", (16, 16), "f32", out=True), hl.F32, 16, 16, hl.TILE16, STREAM), {})),
          ptrs=("idx", "idx2", "table", "table2", "out"), dims=("R", "N"), violations=_kind_enum() + [
              V("R = 8", S("R", 8), E_ARG, "(R, N % 16 == 0)"), V("N = 8", S("N", 8), E_ARG, "(R, N % 16 == 0)"),
              V("layout = MVAE_TILE16P", S("layout", hl.TILE16P), E_ARG, "`layout` (MVAE_TILE16 / MVAE_ROWMAJOR)", safe=True),
              V("layout = -1", S("layout", -1), E_ARG, "`layout` (MVAE_TILE16 / MVAE_ROWMAJOR)", safe=True)]),
    Entry("mvae_relayout", _p("mvae_relayout", ("src", "dst", "kind", "rows", "cols", "to_tile16", "stream"),
                              lambda al: ((al("rl.s", (16, 256), "f32"), al("rl.d", (16, 256), "f32", out=True), hl.F32, 16, 256, 1, STREAM), {})),
          ptrs=("src", "dst"), dims=("rows", "cols"), violations=_kind_enum() + enum("to_tile16", 5, "to_tile16: 0 ... 5") + [
              V("rows = 8", S("rows", 8), E_ARG, "rows and cols in tiles of 16"), V("cols = 8", S("cols", 8), E_ARG, "rows and cols in tiles of 16"),
              V("TILE16P with cols = 48", M(S("to_tile16", 3), S("cols", 48)), E_ARG, "(cols % 32 == 0)"),
              V("TILE16Q with cols = 128", M(S("to_tile16", 5), S("cols", 128)), E_ARG, "(cols % 256 == 0)")]),
    Entry("mvae_tanh_bwd", _p("mvae_tanh_bwd", ("y", "dy", "dx", "n", "stream"),
                              lambda al: ((al("tb.y", (16,), "f32"), al("tb.dy", (16,), "f32"), al("tb.dx", (16,), "f32", out=True), 16, STREAM), {})),
          ptrs=("y", "dy", "dx"), violations=[],
          accepted=[("n = 0", S("n", 0), NOTHING)]),
    Entry("mvae_convert", _p("mvae_convert", ("src", "src_kind", "dst", "dst_kind", "n", "stream"),
                             lambda al: ((al("cv.s", (16,), "f32"), hl.F32, al("cv.d", (16,), "bf16", out=True), hl.BF16, 16, STREAM), {})),
          ptrs=("src", "dst"), violations=_kind_enum("src_kind") + _kind_enum("dst_kind"),
          accepted=[("n = 0", S("n", 0), NOTHING)]),
    Entry("mvae_make_table", _p("mvae_make_table", ("W", "bias", "table", "K", "N", "dst_kind", "stream"),
                                lambda al: ((al("mt.W", (2, 16), "f32"), al("mt.b", (16,), "f32"), al("mt.t", (2, 16), "f32", out=True), 2, 16, hl.F32, STREAM), {})),
          ptrs=("W", "bias", "table"), dims=("K", "N"), violations=_kind_enum("dst_kind")),
    Entry("mvae_transpose_convert", _p("mvae_transpose_convert", ("W", "out", "K", "N", "N_pad", "dst_kind", "stream"),
                                       lambda al: ((al("tc.W", (3, 5), "f32"), al("tc.o", (8, 3), "f32", out=True), 3, 5, 8, hl.F32, STREAM), {})),
          ptrs=("W", "out"), dims=("K", "N"),
              violations=_kind_enum("dst_kind") +
              [V("N_pad = 4 < N", S("N_pad", 4), E_ARG, "rows N..N_pad-1 zero", safe=True)]),
    Entry("mvae_adam_step", _p("mvae_adam_step", ("p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "t", "grad_scale", "stream"),
                               lambda al: ((al("ad.p", (16,), "f32", acc=True), al("ad.g", (16,), "f32"), al("ad.m", (16,), "f32", acc=True), al("ad.v", (16,), "f32", acc=True), 16, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, STREAM), {})),
          ptrs=("p", "g", "m", "v"),
              violations=[V("t = 0", S("t", 0), E_ARG, "lr_t = lr*sqrt(1-b2^t)/(1-b1^t): t >= 1", safe=True),
              V("t = -1", S("t", -1), E_ARG, "t >= 1", safe=True)],
          accepted=[("n = 0", S("n", 0), NOTHING)]),
    Entry("mvae_adam_step_dev", _p("mvae_adam_step_dev", ("p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "t_done", "grad_scale", "zero_grad", "guard", "stream"),
                                   lambda al: ((al("dd.p", (16,), "f32", acc=True), al("dd.g", (16,), "f32"), al("dd.m", (16,), "f32", acc=True), al("dd.v", (16,), "f32", acc=True), 16, 1e-3, 0.9, 0.999, 1e-8, al("dd.t", (1,), "i32", acc=True), 1.0, 0, None, STREAM), {})),
          ptrs=("p", "g", "m", "v", "t_done"), violations=[]),
    Entry("mvae_rmsprop_step", _p("mvae_rmsprop_step", ("p", "g", "v", "n", "lr", "rho", "eps", "grad_scale", "zero_grad", "guard", "stream"),
                                  lambda al: ((al("rp.p", (16,), "f32", acc=True), al("rp.g", (16,), "f32"), al("rp.v", (16,), "f32", acc=True), 16, 1e-3, 0.9, 1e-7, 1.0, 0, None, STREAM), {})),
          ptrs=("p", "g", "v"), violations=[],
          accepted=[("n = 0", S("n", 0), NOTHING)]),
    Entry("mvae_scalars_accumulate", _p("mvae_scalars_accumulate", ("acc", "x", "n", "alpha", "plain_mask", "stream"),
                                        lambda al: ((al("sc.a", (32,), "f32", acc=True), al("sc.x", (32,), "f32"), 4, 0.5, 1, STREAM), {})),
          ptrs=("acc", "x"), violations=[V("n = 33", S("n", 33), E_ARG, "n <= 32"), V("n = -1", S("n", -1), E_ARG, "n <= 32")],
          accepted=[("n = 0", S("n", 0), NOTHING)]),
    Entry("mvae_copy2d_f32", _p("mvae_copy2d_f32", ("dst", "ldd", "src", "lds", "rows", "cols", "src_row0", "zero_rows", "stream"),
                                lambda al: ((al("c2.d", (4, 8), "f32", out=True), 8, al("c2.s", (4, 8), "f32"), 8, 4, 8, 0, 1, STREAM), {})),
          ptrs=("dst", "src"), violations=[V("rows = -1", S("rows", -1), E_ARG, DIMS), V("cols = -1", S("cols", -1), E_ARG, DIMS),
                                          V("ldd = cols - 1", S("ldd", 7), E_ARG, "row stride ldd"),
                                              V("lds = cols - 1", S("lds", 7), E_ARG, "row stride lds"),
                                          V("zero_rows = -1", S("zero_rows", -1), E_ARG, "the first zero_rows rows of dst are ZERO"),
                                          V("src_row0 = -2 with one zero row", S("src_row0", -2), E_ARG, "(their source row index may be negative): only theirs")],
          accepted=[("rows = 0", S("rows", 0), NOTHING), ("cols = 0", S("cols", 0), NOTHING)]),
    Entry("mvae_history_from_latent", _p("mvae_history_from_latent", ("mu", "logvar", "eps2", "B", "B_pad", "Z", "hist", "ldh", "prev", "z_out", "ldo", "stream"),
                                         lambda al: ((al("hf.mu", (4, 4), "f32"), al("hf.lv", (4, 4), "f32"), al("hf.e", (4, 4), "f32"), 4, 4, 4, al("hf.h", (4, 4), "f32", out=True), 4, None, al("hf.z", (4, 4), "f32", out=True), 4, STREAM), {})),
          ptrs=("mu", "logvar", "eps2", "hist"), dims=("B", "Z"), violations=[
              V("B_pad = 3 < B", S("B_pad", 3), E_ARG, "hist[b] = 0 for B <= b < B_pad", safe=True),
                  V("ldh = Z - 1", S("ldh", 3), E_ARG, "rows of stride ldh"),
              V("ldo = Z - 1", S("ldo", 3), E_ARG, "rows of stride ldo")]),
    Entry("mvae_signature_head_fwd", _p("mvae_signature_head_fwd", ("zh", "ldz", "off", "SD", "B", "target", "row_weight", "out", "scalars", "stream"),
                                        lambda al: ((al("sf.zh", (4, 8), "f32"), 8, 4, 4, 4, None, None, al("sf.o", (4, 4), "f32", out=True), None, STREAM), {})),
          ptrs=("zh", "out"), dims=("SD", "B"),
              violations=[V("off = -1", S("off", -1), E_ARG, "zh[:, off:off+SD]"),
              V("ldz = 7 < off + SD", S("ldz", 7), E_ARG, "zh[:, off:off+SD]")]),
    Entry("mvae_signature_head_bwd", _p("mvae_signature_head_bwd", ("dz", "lddz", "off", "SD", "B", "out", "target", "row_weight", "weight", "stream"),
                                        lambda al: ((al("sb.dz", (4, 8), "f32", acc=True), 8, 4, 4, 4, al("sb.o", (4, 4), "f32"), al("sb.t", (4, 4), "f32"), al("sb.rw", (4,), "f32"), 1.0, STREAM), {})),
          ptrs=("dz", "out", "target", "row_weight"), dims=("SD", "B"),
              violations=[V("off = -1", S("off", -1), E_ARG, "dz[b, off+j]"),
              V("lddz = 7 < off + SD", S("lddz", 7), E_ARG, "dz[b, off+j]")]),
    Entry("mvae_softmax_bwd_add", _p("mvae_softmax_bwd_add", ("probs", "dprobs", "dlogits", "kind", "R", "N", "NP", "stream"),
                                     lambda al: ((al("sm.p", (4, 5), "f32", data="half"), al("sm.dp", (4, 5), "f32"), al("sm.dl", (4, 16), "f32", acc=True), hl.F32, 4, 5, 16, STREAM), {})),
          ptrs=("probs", "dprobs", "dlogits"), dims=("R", "N"),
              violations=_kind_enum() +
              [V("NP = 4 < N", S("NP", 4), E_ARG, "dlogits (R,NP)", safe=True)]),
    Entry("mvae_bi_concat", _p("mvae_bi_concat", ("f", "r", "cat", "cat_rev", "kind", "T", "B", "H", "stream"),
                               lambda al: ((al("bc.f", (2, 2, 4), "f32"), al("bc.r", (2, 2, 4), "f32"), al("bc.c", (2, 2, 8), "f32", out=True), al("bc.cr", (2, 2, 8), "f32", out=True), hl.F32, 2, 2, 4, STREAM), {})),
          ptrs=("f", "r", "cat"), dims=("T", "B", "H"), violations=_kind_enum() + [V("H = 2 (f32)", S("H", 2), E_ARG, "H*elemsize % 16 == 0")]),
    Entry("mvae_add_time_reversed", _p("mvae_add_time_reversed", ("dst", "a", "b", "kind", "T", "slab", "stream"),
                                       lambda al: ((al("tr.d", (2, 8), "f32", out=True), al("tr.a", (2, 8), "f32"), al("tr.b", (2, 8), "f32"), hl.F32, 2, 8, STREAM), {})),
          ptrs=("dst", "b"), dims=("T",), violations=_kind_enum() + [V("slab = 0", S("slab", 0), E_ARG, "`slab` elements (% 4 == 0)"),
                                                                     V("slab = 6", S("slab", 6), E_ARG, "`slab` elements (% 4 == 0)", safe=True)]),
]

EXEMPT = {
    "mvae_abi_version": "a constant", "mvae_build_info": "a constant string", "mvae_head_np": "arithmetic on N (test_wide_onehot_cpu.py)",
    "mvae_rnn_producer_waves": "arithmetic on the layout",
    "mvae_event_create": "event API, no launch (test_plan_cpu.py)", "mvae_event_create_timed": "event API, no launch (test_plan_cpu.py)",
    "mvae_event_elapsed_ms": "event API, no launch", "mvae_event_destroy": "event API, no launch", "mvae_event_record": "event API, no launch",
    "mvae_event_synchronize": "event API, no launch", "mvae_stream_wait_event": "event API, no launch",
    "mvae_plan_create": "host-side recording (test_plan_cpu.py)", "mvae_plan_destroy": "host-side recording (test_plan_cpu.py)",
    "mvae_plan_add_call": "host-side recording (test_plan_cpu.py)", "mvae_plan_set_blob": "host-side recording (test_plan_cpu.py)",
    "mvae_plan_add_patch": "host-side recording (test_plan_cpu.py)", "mvae_plan_run": "replays entry points of this table (test_plan_cpu.py)",
    "mvae_plan_size": "host-side recording", "mvae_plan_failed_call": "host-side recording",
    "mvae_host_threads": "host packer (test_hostpack_cpu.py)", "mvae_host_onehot_to_index_tm": "host packer (test_hostpack_cpu.py)",
    "mvae_host_index_to_tm": "host packer (test_hostpack_cpu.py)", "mvae_host_twohot_to_index_tm": "host packer (test_hostpack_cpu.py)",
    "mvae_host_rows_to_tm_f32": "host packer (test_hostpack_cpu.py)",
}


# What the completeness test derives from the signatures and the argument structs (hiplib): every pointer the baseline passes must be
# NULLed by some row, every integer it passes must be changed by some row - or stand here, with the header's word for why not.
OPTIONAL = {        # pointers the header marks "or NULL" / "when ..." (NULL is a form of the call, not a violation)
    "mvae_rnn_fwd": {"h0": "or NULL = zeros", "hs": "or NULL", "cs": "or NULL", "acts": "or NULL (inference)", "h_last": "or NULL",
                     "c_last": "or NULL"},
    "mvae_rnn_fwd_multi": {"cs": "or NULL", "acts": "or NULL (all saving activations or none)", "h_last": "or NULL", "c_last": "or NULL"},
    "mvae_rnn_bwd": {"dhs_ext": "or NULL", "dh_last": "or NULL", "rh": "GRU only; skipped when NULL", "dh0": "or NULL", "dc0": "or NULL"},
    "mvae_rnn_bwd_multi": {"dh_last": "or NULL", "dh0": "or NULL", "dc0": "or NULL"},
    "mvae_gemm": {"k_wait": "NULL = not K-streaming", "chunk_wait": "NULL = no wait", "chunk_done": "NULL = nothing published",
                  "chunk_status": "NULL = time-outs not reported"},
    "mvae_gemm_kstream_multi": {"chunk_status": "NULL = time-outs not reported"},
    "mvae_head": {"target_idx": "or NULL (no target)", "probs": "or NULL", "argmax": "or NULL", "scalars": "or NULL"},
    "mvae_head_sample": {"uniforms": "or NULL = generated"},
    "mvae_latent_fwd": {"style_target": "or NULL (no style head)", "style_probs": "or NULL"},
    "mvae_latent_chain_fwd": {"w_init": "S only when w_init", "b_mu": "bias, not checked", "b_lv": "bias, not checked", "b_init": "bias, not checked"},
    "mvae_history_from_latent": {"z_out": "may be NULL"},
    "mvae_bi_concat": {"cat_rev": "(optional)"},
    "mvae_add_time_reversed": {"a": "a ? a[t] : 0"},
}
UNLIMITED = {       # integers the header puts no limit on
    "mvae_gemm": {"trans_b": "a flag: 0 / non-zero"},
    "mvae_gemm_multi": {"split_k": "optional colsum_b and split_k"},
    "mvae_stream_wait_value32": {"value": "any"}, "mvae_stream_write_value32": {"value": "any"},
    "mvae_latent_chain_fwd": {"B_valid": "rows >= B_valid are padding"}, "mvae_latent_chain_bwd": {"B_valid": "rows >= B_valid are padding"},
    "mvae_tanh_bwd": {"n": "size_t; 0 = nothing to do"}, "mvae_convert": {"n": "size_t; 0 = nothing to do"},
    "mvae_adam_step": {"n": "size_t; 0 = nothing to do"}, "mvae_adam_step_dev": {"n": "size_t"}, "mvae_rmsprop_step": {"n": "size_t; 0 = nothing to do"},
    "mvae_scalars_accumulate": {"plain_mask": "any bits"},
}


def slots(call):
    """{(where, name): ("ptr" | "int", value)} of everything a call hands over: the positional arguments by the types of
    hiplib.SIGNATURES, the fields of the first struct of ``host`` and of the first xpand by their ctypes types"""
    out = {}
    for (name, v), ty in zip(call.args, hl.SIGNATURES[call.fn][1]):
        if v is STREAM or v is STRUCT or name.startswith("stream") or name == "xpand":
            continue
        kind = "ptr" if (ty is hl._vp or hasattr(ty, "contents")) else "int" if ty in (hl._i32, hl._sz, C.c_uint32) else None
        if kind:
            out[("arg", name)] = (kind, v)
    items = [("a", call.item(0))] if call.host is not None else []
    if getattr(call, "xpand", None) is not None:
        items.append(("xpand", call.xpand[0]))
    for where, x in items:
        for f, t in x._fields_:
            if t is hl._vp or t is hl._i32:
                out[(where, f)] = ("ptr" if t is hl._vp else "int", getattr(x, f))
    return out


def rows():
    """(entry, violation) for every row of the table"""
    return [(e, v) for e in ENTRIES for v in e.violations]


def run_baseline(lib, entry, al=None, stream=None):
    return entry.build(al or FakeAlloc()).invoke(lib, stream)


def run_violation(lib, entry, v, al=None, stream=None):
    c = entry.build(al or FakeAlloc())
    v.mutate(c)
    return c.invoke(lib, stream)


def check_library(lib):
    """every failure of ``lib`` against the table, without a device: [(label, what, message)]"""
    bad = []
    for e in ENTRIES:
        if e.cpu_baseline:
            rc = run_baseline(lib, e)
            if rc != E_LAUNCH:
                bad.append((e.label, "baseline", "%s: the baseline returned %d, not MVAE_E_LAUNCH (-3): it is not well-formed" % (e.label, rc)))
            for name, mut, does in e.accepted:
                c = e.build(FakeAlloc())
                mut(c)
                rc = c.invoke(lib)
                if rc != (E_LAUNCH if does is LAUNCH else 0):
                    bad.append((e.label, name, "%s: '%s' must stay accepted (%s), returned %d" % (e.label, name, does, rc)))
        for v in e.violations:
            rc = run_violation(lib, e, v)
            if rc != v.code:
                how = "got past validation (would have enqueued)" if rc in (E_LAUNCH, 0) else "the wrong code"
                bad.append((e.label, v.name, "%s, %s: returned %d, promised %d - %s.  Header: \"%s\"" % (e.label, v.name, rc, v.code, how, v.why)))
    return bad


def _load(path):
    lib = C.CDLL(path)
    for name, (res, args) in hl.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


if __name__ == "__main__":
    import sys
    libs = [("final", hl.load())] + [("parent", _load(p)) for p in sys.argv[1:2]]
    print("# entry point | violation | promised | " + " | ".join(n for n, _ in reversed(libs)) + "   (no device: -3 = got past validation)")
    wrong = {n: 0 for n, _ in libs}
    for e, v in rows():
        got = [(n, run_violation(lib, e, v)) for n, lib in reversed(libs)]
        for n, rc in got:
            wrong[n] += rc != v.code
        print("%s | %s | %d | %s" % (e.label, v.name, v.code, " | ".join("%d%s" % (rc, "" if rc == v.code else " FAIL") for _, rc in got)))
    print("# rows: %d; failing: %s" % (len(rows()), ", ".join("%s %d" % (n, wrong[n]) for n, _ in reversed(libs))))
