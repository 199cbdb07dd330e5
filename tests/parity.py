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
"""
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
