"""Scale-aware parity bounds: a kernel's output against the float64 oracle, block by block (no GPU needed to import).

``close(got, want, tol)`` in test_ops_gpu.py passes when |err| <= tol * (1 + |want|): the ``1 +`` is an absolute floor, and
most bf16 gradients checked there (gate gradients ~ 2.5e-3, dh0 / dc0 without an upstream gradient, head d(logits) ~ 1/R) lie
far below it - a zero gradient passes.  Here every block (a time step's gate, a time step, a row, a whole tensor) is checked
at its own scale, two ways:

  elementwise   |err| <= rtol * |want| + floor * RMS(want over the block)
  normwise      ||err|| / ||want|| <= nw                                      (2-norms over the block)

A block whose ``want`` is all zero must come back exactly zero.  The constants are one table per arithmetic mode (BOUNDS);
forward values (``values=True``: hs, cs, acts, h_last, probabilities) have a normwise bound of their own, since they carry
no backward accumulation.  bf16: a float64 model of a correct bf16 kernel (U, each step's matmul operand and the stored
sequences rounded to bf16, everything else float64: test_parity_cpu.py) stays within 2.1e-3 normwise forward and 6.5e-3
in BPTT at the test shapes - 1.7e-2 for SimpleRNN at T = 33 with only dh_last, a gradient that shrinks through 33 tanh
steps - and within 0.1 x block RMS elementwise.  The defects test_parity_cpu.py plants are 1.8e-2 (a GRU's U scaled by
0.9, forward) to 1.0 normwise in at least one block.  The margins measured on the MI355X against these bounds are in
profiles/r08_parity_margins.txt.  f32: the recurrent kernels stay within 1.1e-6 normwise; the heads' d(logits) within
9e-5 - p - 1 of a well-predicted row cancels in f32 - which sets the f32 gradient bound.

Matrix products and reductions (``assert_product``).  The GEMM, column-sum and time-sum kernels are handed operands that are
ALREADY rounded to their storage type, and the float64 reference is formed on those, so what is left is the f32 accumulation.
Its natural unit is known per element:

  unit[i, j] = 2^-24 * sqrt( sum_k (alpha a[i,k] b[k,j])^2 + bias[j]^2 + c0[i,j]^2 )       (c0: what an accumulating call adds to)

  elementwise   |err| <= c_acc * unit + h(want)               h = 0 (f32 output) or HALF AN ULP of bf16 at want (bf16 output):
                                                              2^(floor(log2 |want|) - 8), i.e. between 2^-9 and 2^-8 of |want| -
                                                              what separates round-to-nearest-even from truncation (a whole
                                                              ulp).  A flat 2^-9 |want| cannot hold: bf16_round itself is up
                                                              to 2^-8 |want| off in the lower half of every binade
  normwise      ||err|| / ||want|| <= nw                      over the whole output (+ 2^-7 / sqrt(12) for a bf16 output: the
                                                              RMS of rounding errors spread over +- half an ulp; truncation
                                                              is 2^-7 / sqrt(3) x 0.7 = 3.2e-3 and fails it)
  zero          an element whose unit is 0 (pad columns, rows of a one-hot A that are never hot, untouched column blocks)
                must come back exactly as it was

c_acc and nw come from a CPU model of a CORRECT kernel (``product_models``), never from a kernel: float32 accumulation of the
products in three orders - sequential over k; 64-row k tiles summed sequentially; the call's split-K partitions, each
sequential, added onto C in a random order (atomics) - at every shape the GPU tests use (``GEMM_SHAPES``; outputs of more than
128 columns are sampled by their first 128, the errors of different columns being independent).  bf16 x bf16 products are exact
in float32; on the f32-operand path (v_mfma_f32_16x16x4_f32) the model is run twice, with float32 products and with exact
products rounded once per accumulation (a fused multiply-add), and the worse counts.  The sequential order is the pessimistic
one: its error grows like sqrt(K / 2) units, and the matrix cores add 32 (bf16) or 4 (f32) products per accumulation.

  model, worst of all orders and shapes (test_parity_gemm_cpu.py prints them with -s):
      bf16 operands   199 units   9.6e-7 normwise      (K = 8192, sequential; 64-row tiles: 28 units, 2.1e-7)
      f32 operands     96 units   8.3e-7 normwise      (K = 2304, sequential, either product rounding)
      column sums     142 units   1.7e-6 normwise      (R = 8192 rows, f32 and bf16, plain and weighted)
  chosen (x 4, rounded up):  PRODUCT[...] below.  A single dropped product is about 1e5 units.

Exact operations (concatenations, copies, relayouts, a two-term f32 sum, conversions) and every product or sum of small
integers (``integer_operands``: |a|, |b| <= 8, alpha a power of two - every partial sum is an integer below 2^24 / alpha, so
every summation order, split-K partition and atomic arrival order gives the same f32 bits) are asserted BIT-equal to the
float64 result cast to the storage type (``assert_bits``).

Elementwise f32 functions (the GEMM's tanh epilogue, the latent block and chain, the optimizers' update) are bounded by
rtol |want| + floor * RMS(want) (``ELEMWISE_F32`` / ``assert_elementwise``): numpy float32 evaluation of the same expressions
(tests/latent_ref.py in float32 at every chain case, the tanh of the float32 accumulation models; test_parity_gemm_cpu.py) is
within 1.85 x (1e-5 |want| + 1e-5 RMS) - d(logvar) of a row with eps = 60, 0.45 x otherwise; x 4: rtol = floor = 8e-5.
The margins measured on the MI355X against all of these are in profiles/r09_op_parity_margins.txt.
"""
import os

import numpy as np

from oracle import vae_oracle as vo

F32, BF16 = 0, 1                   # = midi_vae_amd.hiplib.F32 / BF16 (the arithmetic mode of a kernel call)

BOUNDS = {
    F32: dict(nw=2e-4, nw_values=1e-5, rtol=2e-5, floor=4e-4),
    BF16: dict(nw=2e-2, nw_values=1e-2, rtol=2.0 ** -6, floor=0.25),
}

# relative bound on a head's loss scalar (f32 sums over rows in both modes; the oracle is given the kernel's rounded hs and W)
LOSS_RTOL = 1e-4

GATE_NAMES = {"LSTM": "ifgo", "GRU": "zrh", "SimpleRNN": "h"}


def bf16_round(a):
    """float64 -> bf16 (round to nearest even through f32, as the device conversions) -> float64"""
    b = np.ascontiguousarray(a, np.float64).astype(np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> 16) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


# ---- blocks: a block maker turns an array into (blocks, elements per block) and names block i ---------------------------
def gate_blocks(cellname):
    """acts / da (T, B, G*H): one block per (time step, gate)"""
    names = GATE_NAMES[cellname]
    G = len(names)

    def split(a):
        T, B, GH = a.shape
        return (a.reshape(T, B, G, GH // G).transpose(0, 2, 1, 3).reshape(T * G, -1),
                lambda i: "t=%d, gate %s" % (i // G, names[i % G]))
    return split


def step_blocks(a):
    """hs / cs (T + 1, B, H): one block per time step (index 0 = the initial state)"""
    return a.reshape(a.shape[0], -1), lambda i: "t=%d" % i


def whole(a):
    """h_last, dh0, dc0: the whole tensor"""
    return a.reshape(1, -1), lambda i: "all"


def row_blocks(a):
    """head d(logits), probabilities and dhs (R, N): one block per row"""
    return a.reshape(a.shape[0], -1), lambda i: "row %d" % i


def _ratio(num, den):
    """num / den, with 0 / 0 = 0 and x / 0 = inf"""
    safe = np.where(den > 0, den, 1.0)
    return np.where(den > 0, num / safe, np.where(num > 0, np.inf, 0.0))


def parity_ratios(got, want, dtype, blocks, values=False):
    """the worst elementwise and normwise error of any block, each as a multiple of its bound (<= 1 passes), and where;
    ``elem_rms`` (max |err| / block RMS) and ``norm_rel`` (||err|| / ||want||) are the same errors without the bounds"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bd = BOUNDS[dtype]
    g, name = blocks(got)
    w, _ = blocks(want)
    err = np.abs(g - w)
    err[~np.isfinite(err)] = np.inf
    rms = np.sqrt(np.mean(w * w, axis=1, keepdims=True))
    elem = _ratio(err, bd["rtol"] * np.abs(w) + bd["floor"] * rms).max(axis=1)
    norm_rel = _ratio(np.sqrt(np.sum(err * err, axis=1)), np.sqrt(np.sum(w * w, axis=1)))
    norm = norm_rel / bd["nw_values" if values else "nw"]
    ie, i_n = int(np.argmax(elem)), int(np.argmax(norm))
    return dict(elem=float(elem[ie]), elem_at=name(ie), norm=float(norm[i_n]), norm_at=name(i_n),
                elem_rms=float(_ratio(err, rms).max()), norm_rel=float(norm_rel[i_n]))


def assert_parity(got, want, dtype, blocks, what, values=False):
    """fail with the block's name and the worst ratio; return the ratios (for calibration)"""
    r = parity_ratios(got, want, dtype, blocks, values)
    assert r["elem"] <= 1.0, "%s, %s: elementwise error %.3g x the bound" % (what, r["elem_at"], r["elem"])
    assert r["norm"] <= 1.0, "%s, %s: normwise error %.3g x the bound (%.2e)" % (what, r["norm_at"], r["norm"], r["norm_rel"])
    return r


def assert_rel(got, want, rtol, what):
    """a scalar within rtol of the oracle's; returns |err| / (rtol |want|)"""
    r = float(_ratio(np.abs(np.float64(got) - np.float64(want)), rtol * np.abs(np.float64(want))))
    assert r <= 1.0, "%s: %.9g vs %.9g (%.3g x the bound %.0e)" % (what, got, want, r, rtol)
    return r


# ---- problem builders shared by the GPU tests and test_parity_cpu.py (same seeds, same scales) ---------------------------
def rnn_problem(cellname, H, T, B, seed, K=7):
    rng = np.random.default_rng(seed)
    G = vo.GATES[cellname]
    U = rng.standard_normal((H, G * H)) * (0.5 / np.sqrt(H))
    W = rng.standard_normal((K, G * H)) * 0.4
    b = rng.standard_normal((G * H,)) * 0.2
    h0 = rng.standard_normal((B, H)) * 0.3
    c0 = rng.standard_normal((B, H)) * 0.3
    return rng, G, U, W, b, h0, c0


def rnn_backward_problem(cellname, H, T, B, ext, rnd):
    """the BPTT inputs of test_ops_gpu._rnn_backward_case: the oracle's forward sequences (rounded by ``rnd`` as the kernel
    stores them), an upstream gradient at every step if ``ext``, and one at the final state"""
    rng, G, U, W, b, h0, c0 = rnn_problem(cellname, H, T, B, seed=11 + H)
    xp = rng.standard_normal((T, B, G * H)) * 0.5
    hs_o, cs_o, acts_o = vo.rnn_forward(cellname, xp, U, h0, c0 if cellname == "LSTM" else None)
    hs_o, acts_o = rnd(hs_o), rnd(acts_o)
    if cs_o is not None:
        cs_o = rnd(cs_o)
    dext = rnd(rng.standard_normal((T, B, H)) * 0.1) if ext else None
    dlast = rng.standard_normal((B, H)) * 0.1
    return U, hs_o, cs_o, acts_o, dext, dlast


def softmax_head_problem(N, H, R, seed, two_hot=False):
    """hs (R, H), W (H, N) (logits of the same spread at every H), bias, target index per row (row 5: all-zero target), row
    weights ~ 1/R; ``two_hot``: a second target index per row (255 = none on about a third of the rows and on row 5), never
    equal to the first"""
    rng = np.random.default_rng(seed)
    hs = rng.standard_normal((R, H))
    W = rng.standard_normal((H, N)) * (0.3 * np.sqrt(64.0 / H))
    bias = rng.standard_normal((N,)) * 0.1
    tgt = rng.integers(0, N, (R,))
    tgt[5] = 255
    rw = rng.random((R,)) / R
    tgt2 = None
    if two_hot:
        tgt2 = (tgt + rng.integers(1, N, (R,))) % N
        tgt2[rng.random(R) < 0.3] = 255
        tgt2[5] = 255
    return rng, hs, W, bias, tgt, rw, tgt2


def softmax_head_oracle(hs, Wq, bias, tgt, rw, grad_scale, tgt2=None):
    """float64 probabilities, loss (sum rw * CE), d(logits) and the one- / two-hot target matrix of a softmax head"""
    R, N = hs.shape[0], Wq.shape[1]
    p = vo.softmax(hs @ Wq + bias)
    y = np.zeros((R, N))
    for t in (tgt, tgt2) if tgt2 is not None else (tgt,):
        ok = t < N
        y[np.nonzero(ok)[0], t[ok]] = 1
    return p, np.sum(rw * vo._cce(p, y)), grad_scale * rw[:, None] * vo._cce_grad_logits(p, y), y


def fused_head_problem(kind, N, H, R, seed):
    """test_ops_gpu.test_head_fused_input_gradient's data: hs (R, H), W (H, N), row weights, bias, targets (kind 0: class
    index per row; kind 1: a value per row)"""
    rng = np.random.default_rng(seed)
    hs = rng.standard_normal((R, H)) * 0.5
    W = rng.standard_normal((H, N)) * 0.3
    rw = rng.random((R,)) / R
    if kind == 0:
        bias = rng.standard_normal((N,)) * 0.1
        return hs, W, rw, bias, rng.integers(0, N, (R,))
    return hs, W, rw, np.array([0.1]), rng.random(R)


# ---- matrix products and reductions: the f32 accumulation unit ------------------------------------------------------------
U_ACC = 2.0 ** -24                 # unit roundoff of the f32 accumulators
NW_BF16 = 2.0 ** -7 / np.sqrt(12.0)     # normwise allowance of a bf16 output


def half_ulp_bf16(x):
    """half the spacing of bf16 (8 significant bits) at |x|: the most a correctly rounded store is off; 0 at 0"""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.where(np.asarray(x) != 0, np.ldexp(1.0, e - 9), 0.0)

# c_acc (units), nw (normwise) per accumulation kind: 4 x the worst of the CPU model (module docstring)
PRODUCT = {
    "bf16": dict(c_acc=800.0, nw=4e-6),
    "f32": dict(c_acc=400.0, nw=3.5e-6),
    "sum": dict(c_acc=600.0, nw=7e-6),
}
ELEMWISE_F32 = dict(rtol=8e-5, floor=8e-5)

_RECORD = os.environ.get("MVAE_PARITY_RECORD")       # a file: every check appends its figures (profiles/r09_op_parity_margins.txt)


def _record(kind, what, **figs):
    if _RECORD:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]
        with open(_RECORD, "a") as f:
            f.write("%s\t%s\t%s\t%s\n" % (kind, test, what, " ".join("%s=%.3g" % kv for kv in figs.items())))


def product_unit(A, B, alpha=1.0, extra=()):
    """unit (M, N) of alpha * A (M, K) @ B (K, N) + extras (bias row, initial C: anything that broadcasts to (M, N))"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s = (alpha * alpha) * ((A * A) @ (B * B))
    for e in extra:
        s = s + np.asarray(e, np.float64) ** 2
    return U_ACC * np.sqrt(s)


def sum_unit(X, wgt=None, extra=()):
    """unit (N,) of sum_r wgt[r] X[r, n] + extras: a product with a row of ones (or the row weights) on the left"""
    X = np.asarray(X, np.float64)
    w = np.ones(X.shape[0]) if wgt is None else np.asarray(wgt, np.float64)
    return product_unit(w[None, :], X, extra=extra)[0]


def product_ratios(got, want, unit, kind, out_bf16=False):
    """``units``: the worst (|err| - u_out |want|) / unit; ``norm_rel``: ||err|| / ||want||; ``elem`` / ``norm``: both as a
    multiple of their bound (<= 1 passes); an element whose unit is zero must be exact (its ratio is 0 or inf)"""
    got, want, unit = (np.asarray(a, np.float64) for a in (got, want, unit))
    assert got.shape == want.shape == unit.shape, (got.shape, want.shape, unit.shape)
    bd = PRODUCT[kind]
    err = np.abs(got - want)
    err[~np.isfinite(err)] = np.inf
    h_out = half_ulp_bf16(want) if out_bf16 else 0.0
    units = _ratio(np.maximum(err - h_out, 0.0), unit)
    elem = _ratio(err, bd["c_acc"] * unit + h_out)
    norm_rel = float(_ratio(np.sqrt(np.sum(err * err)), np.sqrt(np.sum(want * want))))
    at = np.unravel_index(int(np.argmax(elem)), elem.shape) if elem.size else ()
    nw = bd["nw"] + (NW_BF16 if out_bf16 else 0.0)
    return dict(units=float(units.max(initial=0.0)), norm_rel=norm_rel, elem=float(elem.max(initial=0.0)), elem_at=at,
                norm=norm_rel / nw)


def assert_product(got, want, unit, kind, what, out_bf16=False):
    """the three bounds of a product / reduction output (module docstring); returns the ratios"""
    r = product_ratios(got, want, unit, kind, out_bf16)
    _record("product:" + kind + (":bf16out" if out_bf16 else ""), what, units=r["units"], norm_rel=r["norm_rel"], elem=r["elem"],
            norm=r["norm"])
    assert r["elem"] <= 1.0, "%s at %s: elementwise error %.3g x the bound (%.3g units)" % (what, r["elem_at"], r["elem"], r["units"])
    assert r["norm"] <= 1.0, "%s: normwise error %.3g x the bound (%.2e)" % (what, r["norm"], r["norm_rel"])
    return r


def cast(a, storage):
    """float64 -> the storage type ("f32" / "bf16") -> float64"""
    a = np.asarray(a, np.float64)
    return bf16_round(a) if storage == "bf16" else a.astype(np.float32).astype(np.float64)


def assert_bits(got, want, storage, what):
    """an exact operation: ``got`` (the device output, as float64) is bit-equal to the float64 result cast to its storage type"""
    got, want = np.asarray(got, np.float64), cast(want, storage)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got == want) & (np.signbit(got) == np.signbit(want))
    _record("bits:" + storage, what, mismatches=float(np.sum(~same)))
    assert np.all(same), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, np.sum(~same), same.size, np.unravel_index(int(np.argmax(~same)), same.shape), got[~same][0], want[~same][0])


def elementwise_ratios(got, want, out_bf16=False, floor_of=None):
    """``floor_of``: the tensor whose RMS scales the floor when ``want`` is an increment onto existing content (default: want)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    err[~np.isfinite(err)] = np.inf
    ref = want if floor_of is None else np.asarray(floor_of, np.float64)
    rms = np.sqrt(np.mean(ref * ref)) if ref.size else 0.0
    elem = _ratio(err, ELEMWISE_F32["rtol"] * np.maximum(np.abs(want), np.abs(ref) if floor_of is not None else 0.0) +
                  ELEMWISE_F32["floor"] * rms + (half_ulp_bf16(want) if out_bf16 else 0.0))
    big = np.abs(want) >= 0.1 * rms
    return dict(elem=float(elem.max(initial=0.0)), elem_at=np.unravel_index(int(np.argmax(elem)), elem.shape) if elem.size else (),
                rel=float(_ratio(err, np.abs(want))[big].max(initial=0.0)), rms=float(_ratio(err, rms).max(initial=0.0)))


def assert_elementwise(got, want, what, out_bf16=False, floor_of=None):
    """an elementwise f32 function: |err| <= rtol |want| + floor RMS(want) (plus half an ulp of bf16 for a bf16 output); all-zero ``want``
    must come back exactly zero"""
    r = elementwise_ratios(got, want, out_bf16, floor_of)
    _record("elementwise" + (":bf16out" if out_bf16 else ""), what, rel=r["rel"], rms=r["rms"], elem=r["elem"])
    assert r["elem"] <= 1.0, "%s at %s: elementwise error %.3g x the bound (%.3g relative, %.3g x RMS)" % (
        what, r["elem_at"], r["elem"], r["rel"], r["rms"])
    return r


# ---- the CPU model of a correct accumulation ------------------------------------------------------------------------------
def split_ranges(K, splits, tile=32):
    """the k range of every split-K partition, as gemm_k cuts them (whole k tiles; trailing partitions may be empty)"""
    per = -(-(-(-K // splits)) // tile) * tile
    return [(p * per, min(K, (p + 1) * per)) for p in range(splits) if p * per < K]


def _accumulate(A32, B32, k0, k1, fused, start=None):
    """float32 accumulation of the products of k rows [k0, k1) onto ``start``; fused: one rounding per accumulation"""
    acc = np.zeros((A32.shape[0], B32.shape[1]), np.float32) if start is None else start.astype(np.float32)
    if fused:
        A64, B64 = A32.astype(np.float64), B32.astype(np.float64)
        for k in range(k0, k1):
            acc = (acc.astype(np.float64) + A64[:, k, None] * B64[None, k, :]).astype(np.float32)
    else:
        for k in range(k0, k1):
            acc += A32[:, k, None] * B32[None, k, :]
    return acc


def product_models(A, B, split_k=1, alpha=1.0, bias=None, c0=None, fused=False, seed=0, tile=64):
    """what a correct kernel may return for alpha * A @ B + bias + c0 on operands that are f32-representable: a dict
    order name -> float64 array.  Orders: "sequential", "tiles" (64-row k tiles, then the tiles), "split" (the call's
    partitions, scaled, added onto c0 in a random order, the bias with partition 0)"""
    A32, B32 = np.asarray(A, np.float32), np.asarray(B, np.float32)
    assert np.array_equal(A32.astype(np.float64), A) and np.array_equal(B32.astype(np.float64), B), "operands must be rounded"
    M, K = A32.shape
    N = B32.shape[1]
    al = np.float32(alpha)
    b32 = None if bias is None else np.asarray(bias, np.float32)
    c32 = np.zeros((M, N), np.float32) if c0 is None else np.broadcast_to(np.asarray(c0, np.float32), (M, N)).copy()

    def epilogue(acc, with_bias=True):
        v = acc * al
        return v + b32 if (b32 is not None and with_bias) else v

    out = {"sequential": c32 + epilogue(_accumulate(A32, B32, 0, K, fused))}
    t = np.zeros((M, N), np.float32)
    for k0 in range(0, K, tile):
        t = t + _accumulate(A32, B32, k0, min(K, k0 + tile), fused)
    out["tiles"] = c32 + epilogue(t)
    parts = [epilogue(_accumulate(A32, B32, k0, k1, fused), with_bias=(i == 0)) for i, (k0, k1) in
             enumerate(split_ranges(K, max(1, split_k)))]
    c = c32.copy()
    for i in np.random.default_rng(seed).permutation(len(parts)):
        c = c + parts[i]
    out["split"] = c
    return {k: v.astype(np.float64) for k, v in out.items()}


def integer_operands(rng, shape, lim=8):
    """small integers as float64: exact in bf16, and so are their products and every partial sum over K <= 8192"""
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


# (M, N, K, split_k, operand scale) of every product the GPU tests check with the unit bound (test_ops_gpu.py): the CPU model runs
# at each of them (test_parity_gemm_cpu.py).  bf16 operands, then f32 operands; column sums: (R, N, scale)
GEMM_SHAPES = {
    "bf16": [(50, 61, 33, 3, 1.0), (300, 192, 256, 3, 1.0), (128, 128, 1000, 3, 1.0), (256, 384, 1024, 3, 1.0), (512, 128, 192, 3, 1.0),
             (61, 256, 1024, 4, 1.0), (256, 61, 4096, 4, 1.0), (256, 1024, 4096, 16, 0.5), (256, 512, 2048, 8, 0.5),
             (128, 256, 1024, 1, 0.5), (256, 512, 8192, 2, 0.5), (256, 512, 6144, 4, 0.5), (128, 512, 6144, 2, 0.5),
             (256, 768, 4096, 4, 0.5), (256, 61, 4096, 16, 0.5), (128, 1024, 256, 1, 0.3), (384, 256, 512, 1, 1.0),
             (256, 256, 1024, 1, 1.0), (256, 256, 768, 1, 1.0), (256, 120, 1024, 4, 1.0), (256, 8, 1024, 4, 1.0),
             (256, 256, 512, 4, 1.0), (384, 256, 128, 1, 1.0), (512, 512, 40, 1, 1.0), (16, 64, 576, 4, 1.0), (16, 64, 2304, 16, 1.0),
             (5, 9, 7, 1, 1.0), (1, 1, 1, 1, 1.0), (50, 61, 33, 8, 1.0)],
    "f32": [(50, 61, 33, 3, 1.0), (300, 192, 256, 3, 1.0), (128, 128, 1000, 3, 1.0), (256, 384, 1024, 3, 1.0), (512, 128, 192, 3, 1.0),
            (64, 64, 200, 2, 1.0), (61, 256, 1024, 4, 1.0), (16, 64, 576, 4, 1.0), (16, 64, 2304, 16, 1.0), (1, 1, 1, 1, 1.0),
            (5, 9, 7, 1, 1.0), (512, 512, 40, 1, 1.0), (50, 61, 33, 8, 1.0), (320, 192, 128, 1, 1.0), (504, 512, 40, 1, 1.0)],
    "sum": [(4099, 128, 1.0), (8192, 128, 0.5), (1000, 192, 1.0), (96, 128, 1.0), (15, 64, 1.0), (1, 64, 1.0)],
}
