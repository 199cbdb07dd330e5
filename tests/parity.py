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

The saturated and clipped regime.  The default problems sit in the smooth interior of every non-linearity (no gate clipped, no
target probability near a clip of the cross-entropy).  ``rnn_saturated_problem`` (inputs of standard deviation 2, planted rows at
+-60), ``softmax_head_clipped_problem`` (target probabilities below 1e-9 / above 1 - 1e-9, one-hot and two-hot) and
``sigmoid_head_saturated_problem`` (logits +-100 and exactly 0) sit on the kinks, with the SAME bounds: the bf16 rounding model
stays below 0.4 x every bound on them (test_parity_cpu.py), a derivative of 0.2 at a clipped gate, unclipped gates, a NaN from
tanh, a leaking or dropped gradient of a clipped target and an unclipped loss all fail.  Where Keras' derivative is zero the
kernels must return exactly zero (``assert_clipped_gates_have_no_gradient``, all-zero blocks of ``assert_parity``).  Margins on
the MI355X: profiles/r10_saturation_margins.txt.
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
    _record("parity:" + ("bf16" if dtype == BF16 else "f32") + (":values" if values else ""), what, elem=r["elem"], norm=r["norm"],
            norm_rel=r["norm_rel"])
    assert r["elem"] <= 1.0, "%s, %s: elementwise error %.3g x the bound" % (what, r["elem_at"], r["elem"])
    assert r["norm"] <= 1.0, "%s, %s: normwise error %.3g x the bound (%.2e)" % (what, r["norm_at"], r["norm"], r["norm_rel"])
    return r


def assert_rel(got, want, rtol, what):
    """a scalar within rtol of the oracle's; returns |err| / (rtol |want|)"""
    r = float(_ratio(np.abs(np.float64(got) - np.float64(want)), rtol * np.abs(np.float64(want))))
    _record("rel", what, ratio=r)
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


# ---- hand-over, carried state and phase launches (test_rnn_handover_gpu.py; the CPU side of it: test_parity_cpu.py) ---------
# States as column blocks: ld = 3 H, the block at column H, every other column a finite sentinel.
STATE_LD_FACTOR, STATE_SENTINEL, WORD_SENTINEL = 3, -777.25, 0x5A5A5A5A
# A sequence as consecutive launches: T -> the chunk lengths.  T = 8 as 3 + 5: an odd first chunk shifts the two-step unrolling of the
# slot-interleaved and two-waves-per-SIMD GRU kernels.
TIME_SPLITS = {7: [(3, 4), (1, 6)], 8: [(3, 5)]}
# (H, B, arithmetic mode) of the generic kernels' cases (T = 7); the resident families run H = 256, B = 32, bf16
GENERIC_SHAPES = [(64, 5, F32), (128, 20, BF16)]
RES_H, RES_B, HANDOVER_T = 256, 32, 7


def rnn_forward_inputs(cellname, H, T, B, xmode, seed, rnd=None, K=7):
    """test_ops_gpu.test_rnn_forward's problem as a Problem: ``rnn_problem``'s U, h0, c0 and the inputs of one input mode ("dense": xp
    (T, B, GH); "index": idx (T, B) into table (K, GH) = W + b; "scalar": xs (T, B), w_row, bias; "const": xp0 (B, GH)), ``rnd``
    rounding what the kernel is handed in its storage type; xp = the pre-activation inputs the oracle gets, and the oracle's hs, cs,
    acts on them (float64, unrounded)."""
    rnd = rnd or (lambda a: a)
    rng, G, U, W, b, h0, c0 = rnn_problem(cellname, H, T, B, seed, K)
    GH = G * H
    pb = Problem(cellname=cellname, H=H, T=T, B=B, G=G, xmode=xmode, U=U, h0=h0, c0=c0 if cellname == "LSTM" else None, idx=None,
                 table=None, xs=None, w_row=None, bias=None, xp0=None, rng=rng)
    if xmode == "dense":
        pb.xp = rnd(rng.standard_normal((T, B, GH)) * 0.5)
    elif xmode == "index":
        pb.idx, pb.table = rng.integers(0, K, (T, B)), rnd(W + b)
        pb.xp = pb.table[pb.idx]
    elif xmode == "scalar":
        pb.xs, pb.w_row, pb.bias = rng.random((T, B)), W[0], b
        pb.xp = pb.xs[..., None] * W[0] + b
    else:
        assert xmode == "const", xmode
        pb.xp0 = rnd(rng.standard_normal((B, GH)) * 0.5)
        pb.xp = np.broadcast_to(pb.xp0[None], (T, B, GH)).copy()
    pb.hs, pb.cs, pb.acts = vo.rnn_forward(cellname, pb.xp, U, pb.h0, pb.c0)
    return pb


def carried_cell_gradient(H, B):
    """a gradient arriving at the final CELL state of an LSTM (dc_last), at the scale of ``rnn_backward_problem``'s dh_last"""
    return np.random.default_rng(1000 + H + B).standard_normal((B, H)) * 0.1


def split_bounds(lengths):
    """chunk lengths -> [(t0, t1)] in time order"""
    t, out = 0, []
    for n in lengths:
        out.append((t, t + n))
        t += n
    return out


def forward_in_chunks(cellname, xp, U, h0, c0, lengths):
    """the oracle's forward pass as consecutive runs over time chunks, chunk k + 1 starting from the final h (and c) of chunk k; the
    assembled hs (T + 1, B, H), cs, acts.  Slot t0 of hs / cs is written by both neighbours, the later one last."""
    T, B, GH = xp.shape
    H = U.shape[0]
    hs, acts = np.full((T + 1, B, H), np.nan), np.full((T, B, GH), np.nan)
    cs = np.full((T + 1, B, H), np.nan) if cellname == "LSTM" else None
    h, c = h0, c0
    for t0, t1 in split_bounds(lengths):
        hs_k, cs_k, acts_k = vo.rnn_forward(cellname, xp[t0:t1], U, h, c)
        hs[t0:t1 + 1], acts[t0:t1] = hs_k, acts_k
        h = hs_k[-1]
        if cs is not None:
            cs[t0:t1 + 1], c = cs_k, cs_k[-1]
    return hs, cs, acts


def backward_in_chunks(cellname, hs, cs, acts, U, dext, dlast, lengths, dclast=None):
    """the oracle's BPTT from the last time chunk to the first, dh_last / dc_last of a chunk = dh0 / dc0 of the chunk behind it;
    the assembled da and the first chunk's dh0, dc0"""
    da = np.full(acts.shape, np.nan)
    dh, dc = dlast, dclast
    for t0, t1 in reversed(split_bounds(lengths)):
        da[t0:t1], _, dh, dc = vo.rnn_backward(cellname, hs[t0:t1 + 1], cs[t0:t1 + 1] if cs is not None else None, acts[t0:t1], U,
                                               dext[t0:t1] if dext is not None else None, dh, dc_last=dc)
    return da, dh, dc


# Chunk counters of the time-pipelined kernels: chunk k = steps [k cs, (k + 1) cs) (the last one may be short).  Forward: hs slot
# t + 1 belongs to step t; chunk k is published behind slot min((k + 1) cs, T), chunks in ascending order.  Backward: steps run from
# T - 1 down; chunk k is published behind da of its FIRST step k cs, chunks in descending order.  Every producer wave adds 1:
# mvae_rnn_producer_waves(layout) * B / 16 per chunk and launch.
def chunk_count(T, cs):
    return -(-T // cs)


def chunk_of_step(t, cs):
    return t // cs


def chunk_steps_of(k, T, cs):
    """(first step, one past the last step) of chunk k"""
    return k * cs, min((k + 1) * cs, T)


def publish_order(T, cs, forward):
    """[(chunk, the step behind which it is published)] in the kernel's own order"""
    n = chunk_count(T, cs)
    if forward:
        return [(k, chunk_steps_of(k, T, cs)[1] - 1) for k in range(n)]
    return [(k, k * cs) for k in range(n - 1, -1, -1)]


def expected_counters(T, cs, waves, B, launches=1):
    """the increments of counters 0 .. chunk_count - 1 after ``launches`` launches"""
    return [launches * waves * (B // 16)] * chunk_count(T, cs)


COUNTER_CS = [1, 2, 3, 16]        # (1: publishing alone and the backward kernels; the forward kernels refuse it with wait_ready)


def counter_lengths(cs):
    """T of the chunk-counter cases of one chunk length: 1, cs - 1, cs, cs + 1, 2 cs, 2 cs + 1 (T >= 1)"""
    return sorted({T for T in (1, cs - 1, cs, cs + 1, 2 * cs, 2 * cs + 1) if T >= 1})


LIVE_T, LIVE_CS_FWD, LIVE_CS_BWD = [8, 9], [2, 4], [1, 2, 4]
COUNTER_T_MAX = 33


def handover_t_cs():
    """every (T, chunk_steps) the GPU tests run a counter rule at"""
    out = {(T, cs) for cs in COUNTER_CS for T in counter_lengths(cs)}
    out |= {(T, cs) for T in LIVE_T for cs in LIVE_CS_FWD + LIVE_CS_BWD}
    out |= {(XPAND_T, XPAND_CS)}
    return sorted(out)


# Phase launches: (T, B, input mode, upstream gradient?) of the problems of one launch - three row-tile counts, so every base[] differs
PHASE_PROBLEMS = [(4, 16, "index", False), (16, 32, "const", True), (33, 48, "dense", True), (16, 16, "dense", False)]
XPAND_T, XPAND_CS, XPAND_B, XPAND_BLOCKS = 16, 4, 32, [2, 16]


def phase_seed(i, cellname):
    return 300 + 10 * i + len(cellname)


def xpand_problem(GH, R, seed, K=61):
    """the inputs of an expansion producer: a 1-feature roll xs (R), w and bias (GH); or index rows idx (R) into a table (K, GH)"""
    rng = np.random.default_rng(seed)
    return Problem(xs=rng.random(R), w=rng.standard_normal(GH) * 0.4, bias=rng.standard_normal(GH) * 0.2,
                   idx=rng.integers(0, K, R), table=rng.standard_normal((K, GH)) * 0.5)


# ---- the saturated regime: clipped hard-sigmoid gates, tanh far out, a cell state past the range of e^{2c} ------------------
SAT_STD, SAT_BIG = 2.0, 60.0       # spread of the pre-activation inputs; the planted rows' value (exact in bf16)


def plant_saturated_rows(x):
    """x (..., B, GH), in place: batch row 1 = +60, row 2 = -60, row 3 = +60 / -60 alternating by column (only when B > 3).
    GH / G is even, so a unit's gates share their sign: an LSTM unit of row 1 has i = f = o = g = 1 and its cell state grows
    by one every step; a unit of row 2 has i = f = o = 0 and c = h = 0."""
    B, GH = x.shape[-2:]
    if B > 3:
        x[..., 1, :], x[..., 2, :] = SAT_BIG, -SAT_BIG
        x[..., 3, :] = np.where(np.arange(GH) % 2 == 0, SAT_BIG, -SAT_BIG)
    return x


def saturated_seed(H, T, B):
    """one seed per saturated shape, the same for the GPU tests and the CPU model (test_parity_cpu.py)"""
    return 7 + H + 3 * T + B


class Problem(dict):
    """a dict whose keys read as attributes"""
    __getattr__ = dict.__getitem__


def rnn_saturated_problem(cellname, H, T, B, seed, rnd=None, xmode="dense"):
    """``rnn_problem``'s U, h0, c0 with pre-activation inputs of standard deviation 2 (hard_sigmoid clips beyond +-2.5) and the
    planted rows of ``plant_saturated_rows``.  xmode "dense": xp (T, B, GH); "index": a table of 7 random rows and the three
    planted ones (rows 7, 8, 9), gathered by idx (T, B); "const": one xp0 (B, GH) for every step.  ``rnd`` rounds what the kernel
    is handed in its storage type.  Returns the forward inputs, the oracle's forward sequences on them (hs, cs, acts: float64,
    unrounded) and what BPTT needs: those sequences rounded (hs_r, cs_r, acts_r), an upstream gradient per step (dext, rounded)
    and one at the final state (dlast), at the scales of ``rnn_backward_problem``."""
    rnd = rnd or (lambda a: a)
    rng, G, U, W, b, h0, c0 = rnn_problem(cellname, H, T, B, seed)
    GH = G * H
    c0 = c0 if cellname == "LSTM" else None
    pb = Problem(U=U, h0=h0, c0=c0, G=G, idx=None, table=None, xp0=None)
    if xmode == "dense":
        pb.xp = rnd(plant_saturated_rows(rng.standard_normal((T, B, GH)) * SAT_STD))
    elif xmode == "index":
        pb.table = rnd(np.concatenate([rng.standard_normal((7, GH)) * SAT_STD, plant_saturated_rows(np.zeros((4, GH)))[1:]]))
        pb.idx = rng.integers(0, 7, (T, B))
        if B > 3:
            pb.idx[:, 1], pb.idx[:, 2], pb.idx[:, 3] = 7, 8, 9
        pb.xp = pb.table[pb.idx]
    else:
        assert xmode == "const", xmode
        pb.xp0 = rnd(plant_saturated_rows(rng.standard_normal((B, GH)) * SAT_STD))
        pb.xp = np.broadcast_to(pb.xp0[None], (T, B, GH)).copy()
    pb.hs, pb.cs, pb.acts = vo.rnn_forward(cellname, pb.xp, U, h0, c0)
    pb.hs_r, pb.acts_r, pb.cs_r = rnd(pb.hs), rnd(pb.acts), (rnd(pb.cs) if pb.cs is not None else None)
    pb.dext = rnd(rng.standard_normal((T, B, H)) * 0.1)
    pb.dlast = rng.standard_normal((B, H)) * 0.1
    return pb


def hard_sigmoid_gates(cellname, acts):
    """the hard-sigmoid gates of acts / da (T, B, G*H) as (T, B, n, H): LSTM i, f, o; GRU z, r; SimpleRNN has none"""
    T, B, GH = acts.shape
    G = len(GATE_NAMES[cellname])
    a = acts.reshape(T, B, G, GH // G)
    return a[:, :, {"LSTM": [0, 1, 3], "GRU": [0, 1], "SimpleRNN": []}[cellname]]


def clipped_share(cellname, acts):
    """(share of hard-sigmoid gate values that are exactly 0, share that are exactly 1)"""
    g = hard_sigmoid_gates(cellname, acts)
    return float(np.mean(g == 0.0)), float(np.mean(g == 1.0))


def assert_clipped_gates_have_no_gradient(cellname, acts, da, what=""):
    """wherever the SAVED gate value a BPTT kernel was handed is exactly 0 or 1, its pre-activation gradient is exactly zero
    (Keras: the gradient of clip() outside the range); returns the number of such elements"""
    g, d = hard_sigmoid_gates(cellname, np.asarray(acts, np.float64)), hard_sigmoid_gates(cellname, np.asarray(da, np.float64))
    clipped = (g == 0.0) | (g == 1.0)
    bad = clipped & (d != 0.0)
    assert not bad.any(), "%s: %d of %d clipped gates carry a gradient, first at (t, b, gate, unit) = %s: %r" % (
        what, bad.sum(), clipped.sum(), tuple(np.argwhere(bad)[0]), d[bad][0])
    return int(clipped.sum())


# (H, B) of the saturated forward cases (T = 9) and BPTT cases (T = 8): a ragged generic shape, a ragged and a whole-tile batch at
# the resident kernels' H = 256; the wider generic kernels (test_hidden_sizes_gpu.py); the long LSTM window whose cell state leaves
# the range of e^{2c}
SAT_FWD_SHAPES = [(64, 5), (256, 21), (256, 32)]
SAT_BWD_SHAPES = [(64, 5), (256, 19), (256, 32)]
SAT_WIDE_SHAPES = [(384, 21), (512, 16)]
SAT_T_FWD, SAT_T_BWD, SAT_LONG = 9, 8, (256, 64, 16)           # SAT_LONG: (H, T, B)


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


SHARED_LOGIT, SHARED_DROP = 10.0, 36.0
CE_FAR, CE_NEAR = 1e-9, 1e-6      # a target probability is beyond a clip by a factor 100, or inside it by a factor 10


def ce_bands(hs, Wq, bias, tgt, tgt2=None):
    """float64 target probabilities of a softmax head problem, on the rounded operands the oracle gets: every one must be below
    1e-9, above 1 - 1e-9 or inside [1e-6, 1 - 1e-6], so that no f32 evaluation (relative error ~1e-6) can land on the other side
    of Keras' clip at 1e-7.  Returns boolean (R, 2) arrays low, high, inside (all False where there is no target)."""
    z = hs @ Wq + bias
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    p = e / e.sum(1, keepdims=True)
    N = Wq.shape[1]
    q = np.stack([np.delete(e, c, 1).sum(1) for c in range(N)], 1) / e.sum(1, keepdims=True)     # 1 - p without cancellation
    R = hs.shape[0]
    low, high, inside = (np.zeros((R, 2), bool) for _ in range(3))
    for s, t in enumerate((tgt, tgt2)):
        if t is None:
            continue
        rows = np.nonzero(np.asarray(t) < N)[0]
        pt, qt = p[rows, np.asarray(t)[rows]], q[rows, np.asarray(t)[rows]]
        low[rows, s], high[rows, s] = pt < CE_FAR, qt < CE_FAR
        inside[rows, s] = (pt >= CE_NEAR) & (qt >= CE_NEAR)
        bad = ~(low[rows, s] | high[rows, s] | inside[rows, s])
        assert not bad.any(), "rows %s: target probabilities %s are too close to a clip of the cross-entropy" % (rows[bad], pt[bad])
    return low, high, inside


def softmax_head_clipped_problem(N, H, R, seed, two_hot=False, rnd=None, s=12.0):
    """``softmax_head_problem`` with rows whose target probabilities lie beyond Keras' clip [1e-7, 1 - 1e-7] (no gradient from such a
    target, each target of a two-hot row on its own; -log(1e-7) as its loss).  hs[row] = s W[:, j] lifts column j by more than 30
    in logit over every other column ("high" = j, "low" = any other); hs[row] = a W[:, j] + b W[:, m] + c W[:, low] with logits of
    10, 10 and -26 at those columns leaves j and m "inside" and column ``low`` 36 below them.  j = N - 1 (the last column of the
    last tile), m = N // 2, low = column 0.  Planted rows: 0 high, 1 low; two-hot: 2 (low, inside), 3 (inside, low), 4 (low, high), 6 (high, low), 7 (low, low), R - 3 (low, inside); one-hot:
    6 high, 7 low; R - 2: low (one-hot in both - a fully clipped row in the last, partial 16-row tile).  Rows 6 and 7 are padding
    positions under b_stride = 8, b_valid = 5; row 5 keeps its all-zero target.  ``rnd`` rounds to the kernel's storage type: hs comes
    back rounded, W does not (the device converts it), and the conditions of ``ce_bands`` are asserted on rnd(hs), rnd(W).
    Returns softmax_head_problem's tuple and a dict case name -> row."""
    rnd = rnd or (lambda a: a)
    assert N >= 3 and R >= 24
    rng, hs, W, bias, tgt, rw, tgt2 = softmax_head_problem(N, H, R, seed, two_hot)
    Wq = rnd(W)
    j, m, lo = N - 1, N // 2, 0
    dominant = s * Wq[:, j]
    # the "inside" rows keep their logits SMALL: an f32 logit near 70 carries rounding errors of several 1e-6 (half an ulp is 3.8e-6
    # there), which is the relative error of a probability that is not 0 or 1 - more than the f32 bound on forward values allows a
    # correct kernel.  So columns j and m sit at a logit of 10 and the low column is pushed DOWN to -26 (test_parity_cpu.py runs a
    # float32 model of a correct head on these problems: it must stay below half of every bound)
    trio = Wq[:, [j, m, lo]]
    shared = trio @ np.linalg.solve(trio.T @ trio, np.array([SHARED_LOGIT, SHARED_LOGIT, SHARED_LOGIT - SHARED_DROP]))
    NONE = 255
    if two_hot:
        plan = {"high": (0, dominant, j, NONE), "low": (1, dominant, lo, NONE), "low_inside": (2, shared, lo, j),
                "inside_low": (3, shared, j, lo), "low_high": (4, dominant, lo, j), "high_low": (6, dominant, j, lo),
                "low_low": (7, dominant, lo, m), "low_inside_last_tile": (R - 3, shared, lo, m),
                "low_last_tile": (R - 2, dominant, lo, NONE)}
    else:
        plan = {"high": (0, dominant, j, NONE), "low": (1, dominant, lo, NONE), "high_padding": (6, dominant, j, NONE),
                "low_padding": (7, dominant, lo, NONE), "low_last_tile": (R - 2, dominant, lo, NONE)}
    for row, h, t1, t2 in plan.values():
        hs[row], tgt[row] = h, t1
        if two_hot:
            tgt2[row] = t2
    hs = rnd(hs)
    low, high, inside = ce_bands(hs, Wq, bias, tgt, tgt2)
    for name, (row, _, t1, t2) in plan.items():              # every planted target is in the band its name says
        kinds = name.replace("_last_tile", "").replace("_padding", "").split("_")
        for slot, kind in enumerate(kinds):
            assert dict(low=low, high=high, inside=inside)[kind][row, slot], (name, row, slot)
    assert tgt[5] == NONE and (tgt2 is None or tgt2[5] == NONE)
    return rng, hs, W, bias, tgt, rw, tgt2, {name: v[0] for name, v in plan.items()}


# (N, H, R, two_hot) -> seed of every clipped head case the GPU tests run: the first seed >= N at which the float64 oracle meets the
# conditions of ``ce_bands`` on unrounded, f32-rounded and bf16-rounded operands (found on the CPU; test_parity_cpu.py re-asserts)
CLIPPED_HEAD_SEEDS = {(3, 64, 40, False): 3, (3, 64, 40, True): 3, (3, 64, 48, False): 3, (3, 64, 48, True): 3, (3, 256, 48, False): 3,
                      (3, 256, 48, True): 3, (61, 64, 40, False): 61, (61, 64, 40, True): 62, (61, 64, 48, False): 61,
                      (61, 64, 48, True): 61, (61, 256, 48, False): 61, (61, 256, 48, True): 61, (145, 64, 40, False): 145,
                      (145, 64, 40, True): 145, (145, 64, 48, False): 146, (145, 64, 48, True): 146, (145, 256, 48, False): 146,
                      (145, 256, 48, True): 145}


def retarget_padding_rows(hs, Wq, bias, tgt, tgt2, counted, keep):
    """in place, as test_ops_gpu._softmax_head_case does: a padding row (not ``counted``) gets its own argmax as its only target - a
    hit if it were counted - except the planted rows ``keep``"""
    rows = np.setdiff1d(np.nonzero(~counted)[0], list(keep))
    tgt[rows] = np.argmax(hs[rows] @ Wq + bias, 1)
    if tgt2 is not None:
        tgt2[rows] = 255
    return rows


def fully_clipped_rows(low, high, inside):
    """rows of a softmax head problem with a target and none inside the clip range: d(logits) and dhs must be exactly zero"""
    return np.nonzero((low | high).any(1) & ~inside.any(1))[0]


def sigmoid_head_saturated_problem(R, H, seed, rnd=None):
    """test_sigmoid_head's problem with zero bias and planted rows: logits of +100 (rows 0, 1: targets 1, 0) and -100 (rows 2, 3:
    targets 0, 1) - exp(-100) is below half an ulp of 1 and exp(100) above the f32 range, so pr is exactly 1 / 0 and the gradient
    2 (pr - y) pr (1 - pr) exactly zero - and all-zero hs rows (4 and R - 1, targets 0 and 1): the logit is exactly 0, pr exactly
    1/2, which Keras' binary accuracy rounds half-to-even to 0.  Returns hs (rounded), W (H, 1), bias, y, rw and the planted rows."""
    rnd = rnd or (lambda a: a)
    rng = np.random.default_rng(seed)
    hs = rng.standard_normal((R, H))
    W = rng.standard_normal((H, 1)) * 0.3
    y = np.where(rng.random(R) < 0.5, 0.0, 0.5 + 0.5 * rng.random(R))
    rw = rng.random((R,)) / R
    Wq = rnd(W)[:, 0]
    big = (100.0 / (Wq @ Wq)) * Wq
    rows = dict(plus=[0, 1], minus=[2, 3], half=[4, R - 1])
    hs[0], hs[1], hs[2], hs[3], hs[4], hs[R - 1] = big, big, -big, -big, 0.0, 0.0
    y[[0, 1, 2, 3, 4, R - 1]] = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    hs = rnd(hs)
    z = hs @ Wq
    assert np.all(np.abs(z[rows["plus"]] - 100.0) < 5.0) and np.all(np.abs(z[rows["minus"]] + 100.0) < 5.0) and np.all(z[rows["half"]] == 0)
    return hs, W, np.array([0.0]), y, rw, rows


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
