"""The scale-aware parity bounds of tests/parity.py, checked on the CPU against what they are for (no GPU).

Specificity: a float64 model of a CORRECT bf16 kernel - U, the h (GRU candidate: r * h) or da operand of each step's matmul
and the stored sequences rounded to bf16, state and accumulation kept in float64 - passes the bf16 bounds against the plain
oracle at the kernel tests' shapes.  Sensitivity: the float64 oracle's outputs on the GPU tests' own problems (same builders,
seeds and scales), changed the way a broken kernel would change them, fail the bounds - every one of these passes the
``close(got, want, 4e-2 / 2e-2)`` checks of test_ops_gpu.py, whose ``1 + |want|`` floor is far above these gradients.
"""
import numpy as np
import pytest

from oracle import vae_oracle as vo
from tests import parity as par

bf = par.bf16_round
BF16 = par.BF16


# ---- the bf16 rounding model -------------------------------------------------------------------------------------------
def model_forward(cellname, xp, U, h0, c0):
    """hs, cs, acts as stored (bf16) and the final h (f32 output) of a correct bf16 forward kernel"""
    T, B, GH = xp.shape
    H = U.shape[0]
    Ub = bf(U)
    hs, acts = np.zeros((T + 1, B, H)), np.zeros((T, B, GH))
    cs = np.zeros((T + 1, B, H)) if cellname == "LSTM" else None
    h, c = h0.copy(), (c0.copy() if cs is not None else None)
    hs[0] = h
    if cs is not None:
        cs[0] = c
    hsig = vo.hard_sigmoid
    for t in range(T):
        if cellname == "GRU":
            a = xp[t, :, :2 * H] + bf(h) @ Ub[:, :2 * H]
            z, r = hsig(a[:, :H]), hsig(a[:, H:])
            hh = np.tanh(xp[t, :, 2 * H:] + bf(r * h) @ Ub[:, 2 * H:])
            h = z * h + (1.0 - z) * hh
            acts[t] = np.concatenate([z, r, hh], 1)
        elif cellname == "LSTM":
            a = xp[t] + bf(h) @ Ub
            i, f, g, o = hsig(a[:, :H]), hsig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), hsig(a[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            cs[t + 1] = c
            acts[t] = np.concatenate([i, f, g, o], 1)
        else:
            h = np.tanh(xp[t] + bf(h) @ Ub)
            acts[t] = h
        hs[t + 1] = h
    return bf(hs), (bf(cs) if cs is not None else None), bf(acts), h


def model_backward(cellname, hs, cs, acts, U, dext, dlast):
    """da as stored (bf16), dh0 and dc0 (f32 outputs) of a correct bf16 BPTT kernel on the same (stored) forward sequences"""
    T, B, GH = acts.shape
    H = U.shape[0]
    Ub = bf(U)
    da = np.zeros_like(acts)
    dh, dc = dlast.copy(), np.zeros((B, H))
    dsig = vo._dhs
    for t in range(T - 1, -1, -1):
        d = dh + (dext[t] if dext is not None else 0.0)
        hp = hs[t]
        if cellname == "GRU":
            z, r, hh = acts[t, :, :H], acts[t, :, H:2 * H], acts[t, :, 2 * H:]
            da_h = d * (1.0 - z) * (1.0 - hh * hh)
            drh = bf(da_h) @ Ub[:, 2 * H:].T
            da[t] = np.concatenate([d * (hp - hh) * dsig(z), drh * hp * dsig(r), da_h], 1)
            dh = d * z + drh * r + bf(da[t, :, :2 * H]) @ Ub[:, :2 * H].T
        elif cellname == "LSTM":
            i, f, g, o = acts[t, :, :H], acts[t, :, H:2 * H], acts[t, :, 2 * H:3 * H], acts[t, :, 3 * H:]
            tc = np.tanh(cs[t + 1])
            dct = dc + d * o * (1.0 - tc * tc)
            da[t] = np.concatenate([dct * g * dsig(i), dct * cs[t] * dsig(f), dct * i * (1.0 - g * g), d * tc * dsig(o)], 1)
            dc = dct * f
            dh = bf(da[t]) @ Ub.T
        else:
            da[t] = d * (1.0 - acts[t] ** 2)
            dh = bf(da[t]) @ Ub.T
    return bf(da), dh, dc


# ---- the checks the GPU tests make ---------------------------------------------------------------------------------------
def check_forward(cellname, got, want, dtype=BF16):
    """test_rnn_forward's parity checks: got / want = (hs, cs, acts, h_last)"""
    worst = []
    for k, name, blocks in ((0, "hs", par.step_blocks), (1, "cs", par.step_blocks), (2, "acts", par.gate_blocks(cellname)),
                            (3, "h_last", par.whole)):
        if want[k] is not None:
            worst.append(par.assert_parity(got[k], want[k], dtype, blocks, name, values=True))
    return worst


def check_backward(cellname, got, want, dtype=BF16):
    """_rnn_backward_case's parity checks: got / want = (da, dh0, dc0)"""
    worst = [par.assert_parity(got[0], want[0], dtype, par.gate_blocks(cellname), "da"),
             par.assert_parity(got[1], want[1], dtype, par.whole, "dh0")]
    if cellname == "LSTM":
        worst.append(par.assert_parity(got[2], want[2], dtype, par.whole, "dc0"))
    return worst


def _oracle_backward(cellname, H, T, B, ext):
    U, hs, cs, acts, dext, dlast = par.rnn_backward_problem(cellname, H, T, B, ext, bf)
    da, _, dh0, dc0 = vo.rnn_backward(cellname, hs, cs, acts, U, dext, dlast)
    return (U, hs, cs, acts, dext, dlast), (da, dh0, dc0)


# ---- specificity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cellname", ["LSTM", "GRU", "SimpleRNN"])
@pytest.mark.parametrize("H", [64, 256, 512])
def test_bf16_rounding_model_passes_the_bf16_bounds(cellname, H):
    """every B in {5, 16, 32, 37} x T in {1, 3, 8, 33}, forward and BPTT with and without an upstream gradient per step.  The
    model's worst blocks: 0.21 x the bounds forward, 0.33 in BPTT, 0.85 (1.7e-2 normwise) for SimpleRNN at T = 33 with no
    upstream gradient but dh_last: the gradient shrinks through 33 tanh steps while each step's rounding stays relative to
    its own size."""
    for B in (5, 16, 32, 37):
        for T in (1, 3, 8, 33):
            rng, G, U, W, b, h0, c0 = par.rnn_problem(cellname, H, T, B, seed=H + B + T)
            xp = bf(rng.standard_normal((T, B, G * H)) * 0.5)
            c0 = c0 if cellname == "LSTM" else None
            hs_o, cs_o, acts_o = vo.rnn_forward(cellname, xp, U, h0, c0)
            check_forward(cellname, model_forward(cellname, xp, U, h0, c0), (hs_o, cs_o, acts_o, hs_o[-1]))
            for ext in (True, False):
                (U_, hs, cs, acts, dext, dlast), want = _oracle_backward(cellname, H, T, B, ext)
                check_backward(cellname, model_backward(cellname, hs, cs, acts, U_, dext, dlast), want)


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _zero(a, idx):
    a = a.copy()
    a[idx] = 0.0
    return a


@pytest.mark.parametrize("B", [32, 16])
def test_lstm_backward_defects_fail(B):
    H = 256
    for ext in (True, False):
        _, (da, dh0, dc0) = _oracle_backward("LSTM", H, 8, B, ext)
        want = (da, dh0, dc0)
        check_backward("LSTM", (bf(da), dh0, dc0), want)
        ifo_zero = _zero(_zero(da, np.s_[:, :, :2 * H]), np.s_[:, :, 3 * H:])           # input, forget and output gates
        for bad in (ifo_zero, _zero(da, np.s_[:, :, :16]), _zero(da, np.s_[:, 3])):      # ... the first 16 columns, a batch row
            _fails(check_backward, "LSTM", (bad, dh0, dc0), want)
        if not ext:
            _fails(check_backward, "LSTM", (_zero(da, np.s_[0]), dh0, dc0), want)       # time step 0
            for bad_dh0 in (0.0 * dh0, 0.5 * dh0, 1.3 * dh0):
                _fails(check_backward, "LSTM", (da, bad_dh0, dc0), want)
            _fails(check_backward, "LSTM", (da, dh0, 0.0 * dc0), want)


def test_gru_backward_defects_fail():
    H = 256
    for B, ext in ((19, True), (32, True), (33, False), (16, False)):
        _, (da, dh0, dc0) = _oracle_backward("GRU", H, 8, B, ext)
        want = (da, dh0, dc0)
        check_backward("GRU", (bf(da), dh0, dc0), want)
        _fails(check_backward, "GRU", (_zero(da, np.s_[:, :, H:2 * H]), dh0, dc0), want)      # reset gate
        _fails(check_backward, "GRU", (_zero(da, np.s_[:, B - 1]), dh0, dc0), want)           # a batch row
        if not ext:
            _fails(check_backward, "GRU", (_zero(da, np.s_[0]), dh0, dc0), want)
            _fails(check_backward, "GRU", (da, 0.0 * dh0, dc0), want)


@pytest.mark.parametrize("B", [21, 32])
def test_gru_forward_with_scaled_recurrent_weights_fails(B):
    """test_rnn_forward's GRU H=256 problem (dense input) with U scaled by 0.9"""
    H, T = 256, 9
    rng, G, U, W, b, h0, c0 = par.rnn_problem("GRU", H, T, B, seed=H + B)
    xp = bf(rng.standard_normal((T, B, G * H)) * 0.5)
    hs, _, acts = vo.rnn_forward("GRU", xp, U, h0)
    hs_b, _, acts_b = vo.rnn_forward("GRU", xp, 0.9 * U, h0)
    check_forward("GRU", (bf(hs), None, bf(acts), hs[-1]), (hs, None, acts, hs[-1]))
    _fails(check_forward, "GRU", (bf(hs_b), None, bf(acts_b), hs_b[-1]), (hs, None, acts, hs[-1]))


# ---- heads ---------------------------------------------------------------------------------------------------------------
def check_softmax_head(got, want, dtype=BF16):
    """test_softmax_head's parity checks: got / want = (probs, dlogits, loss)"""
    return [par.assert_parity(got[0], want[0], dtype, par.row_blocks, "probs", values=True),
            par.assert_parity(got[1], want[1], dtype, par.row_blocks, "dlogits"),
            par.assert_rel(got[2], want[2], par.LOSS_RTOL, "loss")]


@pytest.mark.parametrize("N", [61, 16, 3, 77, 128])
@pytest.mark.parametrize("two_hot", [False, True])
def test_softmax_head_defects_fail(N, two_hot):
    rng, hs, W, bias, tgt, rw, tgt2 = par.softmax_head_problem(N, 64, 333, seed=N, two_hot=two_hot)
    p, loss, dl, _ = par.softmax_head_oracle(bf(hs), bf(W), bias, tgt, rw, 0.7, tgt2)
    want = (p, dl, loss)
    check_softmax_head((p.astype(np.float32), bf(dl), np.float32(loss)), want)       # a correct bf16 head
    _fails(check_softmax_head, (p, 0.0 * dl, loss), want)
    _fails(check_softmax_head, (p, dl, 1.1 * loss), want)
    _fails(check_softmax_head, (p, dl, 1.01 * loss), want)
    row = int(np.argmax(np.abs(dl).sum(1) > 0))
    scaled = dl.copy()
    scaled[row] *= 1.1
    _fails(check_softmax_head, (p, scaled, loss), want)


def test_sigmoid_head_defects_fail():
    """test_sigmoid_head's problem: d(logit) all zero"""
    rng = np.random.default_rng(2)
    R, H = 150, 64
    hs = bf(rng.standard_normal((R, H)))
    W = rng.standard_normal((H, 1)) * 0.3
    y = np.where(rng.random(R) < 0.5, 0.0, 0.5 + 0.5 * rng.random(R))
    y[:10] = 1.0
    rw = rng.random((R,)) / R
    p = vo.sigmoid(hs @ bf(W) + 0.1)[:, 0]
    dl = (rw * 2 * (p - y) * p * (1 - p))[:, None]
    par.assert_parity(bf(dl), dl, BF16, par.row_blocks, "dlogits")
    _fails(par.assert_parity, 0.0 * dl, dl, BF16, par.row_blocks, "dlogits")


@pytest.mark.parametrize("kind,N", [(0, 61), (0, 16), (1, 1)])
def test_fused_head_input_gradient_defects_fail(kind, N):
    """test_head_fused_input_gradient's bf16 problem: dhs = dlogits W^T all zero, or one 16-column tile of it zero"""
    R, H = 320, 256
    hs, W, rw, bias, tgt = par.fused_head_problem(kind, N, H, R, seed=N + kind)
    hs, W = bf(hs), bf(W)
    if kind == 0:
        _, _, dl, _ = par.softmax_head_oracle(hs, W, bias, tgt, rw, 0.7)
    else:
        p = vo.sigmoid(hs @ W + bias)[:, 0]
        dl = (rw * 2 * (p - tgt) * p * (1 - p))[:, None]
    want = bf(dl) @ W.T
    par.assert_parity(bf(want), want, BF16, par.row_blocks, "dhs")
    _fails(par.assert_parity, 0.0 * want, want, BF16, par.row_blocks, "dhs")
    _fails(par.assert_parity, _zero(want, np.s_[:, 32:48]), want, BF16, par.row_blocks, "dhs")


# ---- the helper itself ---------------------------------------------------------------------------------------------------
def test_assert_parity_names_the_block_and_returns_the_ratios():
    want = np.ones((3, 2, 8))
    got = want.copy()
    got[2, :, 2:4] *= 1.5
    with pytest.raises(AssertionError, match="da, t=2, gate f"):
        par.assert_parity(got, want, BF16, par.gate_blocks("LSTM"), "da")
    r = par.assert_parity(want * (1 + 2 ** -8), want, BF16, par.gate_blocks("LSTM"), "da")
    assert 0 < r["elem"] < 1 and 0 < r["norm"] < 1
    zero = np.zeros((4, 16))                                   # a block that is zero must come back exactly zero
    par.assert_parity(zero, zero, BF16, par.row_blocks, "dlogits")
    bad = zero.copy()
    bad[1, 0] = 1e-30
    with pytest.raises(AssertionError, match="row 1"):
        par.assert_parity(bad, zero, BF16, par.row_blocks, "dlogits")
    with pytest.raises(AssertionError):
        par.assert_parity(np.full((2, 2), np.nan), np.ones((2, 2)), BF16, par.whole, "dh0")


# ---- the saturated regime: clipped gates, tanh far out, clipped cross-entropy rows ------------------------------------------
# The problems of parity.rnn_saturated_problem / softmax_head_clipped_problem at every shape the GPU tests run them at.  BOUNDS is
# the table the smooth problems use: the same rounding model decides, and must stay below HALF of every bound here.
SAT_CELLS = ["LSTM", "GRU", "SimpleRNN"]


def f32r(a):
    """float64 -> f32 -> float64"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _sat(cellname, H, T, B, rnd=bf, xmode="dense"):
    return par.rnn_saturated_problem(cellname, H, T, B, par.saturated_seed(H, T, B), rnd, xmode)


def _sat_backward(cellname, pb, ext, seqs=None):
    """(inputs of a BPTT run on the problem's rounded sequences - or on ``seqs`` - , the oracle's da, dh0, dc0)"""
    hs, cs, acts = seqs if seqs is not None else (pb.hs_r, pb.cs_r, pb.acts_r)
    args = (hs, cs, acts, pb.U, pb.dext if ext else None, pb.dlast)
    da, _, dh0, dc0 = vo.rnn_backward(cellname, *args)
    return args, (da, dh0, dc0)


def check_backward_saturated(cellname, got, want, acts, dtype=BF16):
    """what test_ops_gpu._rnn_backward_case checks on a saturated problem: the parity bounds and exact zeros at clipped gates"""
    worst = check_backward(cellname, got, want, dtype)
    par.assert_clipped_gates_have_no_gradient(cellname, acts, got[0], "da")
    return worst


def _sat_backward_cases(cellname):
    """(H, T, B, ext) of every saturated BPTT case of test_ops_gpu.py / test_hidden_sizes_gpu.py"""
    cases = [(H, par.SAT_T_BWD, B, ext) for H, B in par.SAT_BWD_SHAPES + par.SAT_WIDE_SHAPES for ext in (True, False)]
    cases += [(256, T, 32, ext) for T in (3, 7) for ext in (True, False)]
    if cellname in ("LSTM", "GRU"):
        cases.append((par.SAT_LONG[0], par.SAT_LONG[1], par.SAT_LONG[2], True))
    return cases


def _worst(ratios):
    return max(max(r["elem"], r["norm"]) if isinstance(r, dict) else r for r in ratios)


@pytest.mark.parametrize("cellname", SAT_CELLS)
def test_bf16_rounding_model_passes_the_bounds_on_saturated_problems(cellname):
    """forward (dense and index input; the LSTM's long window with dense and constant input), BPTT on the oracle's rounded sequences,
    and BPTT on the model's OWN forward sequences (the hand-over test).  Measured: profiles/r10_saturation_margins.txt."""
    worst = {}
    for H, B in par.SAT_FWD_SHAPES + par.SAT_WIDE_SHAPES:
        for xmode in ("dense", "index"):
            pb = _sat(cellname, H, par.SAT_T_FWD, B, xmode=xmode)
            worst["forward H=%d B=%d %s" % (H, B, xmode)] = _worst(check_forward(
                cellname, model_forward(cellname, pb.xp, pb.U, pb.h0, pb.c0), (pb.hs, pb.cs, pb.acts, pb.hs[-1])))
    if cellname == "LSTM":
        H, T, B = par.SAT_LONG
        for xmode in ("dense", "const"):
            pb = _sat(cellname, H, T, B, xmode=xmode)
            worst["forward H=%d T=%d B=%d %s" % (H, T, B, xmode)] = _worst(check_forward(
                cellname, model_forward(cellname, pb.xp, pb.U, pb.h0, pb.c0), (pb.hs, pb.cs, pb.acts, pb.hs[-1])))
    for H, T, B, ext in _sat_backward_cases(cellname):
        pb = _sat(cellname, H, T, B)
        args, want = _sat_backward(cellname, pb, ext)
        worst["BPTT H=%d T=%d B=%d ext=%d" % (H, T, B, ext)] = _worst(check_backward_saturated(
            cellname, model_backward(cellname, *args), want, pb.acts_r))
    if cellname != "SimpleRNN":
        pb = _sat(cellname, 256, par.SAT_T_FWD, 32)
        hs, cs, acts, _ = model_forward(cellname, pb.xp, pb.U, pb.h0, pb.c0)
        args, want = _sat_backward(cellname, pb, True, (hs, cs, acts))
        worst["hand-over H=256 T=9 B=32"] = _worst(check_backward_saturated(cellname, model_backward(cellname, *args), want, acts))
    for k, v in worst.items():                           # (pytest -s shows them)
        print("saturated model %-9s %-34s %.3f x the bound" % (cellname, k, v))
    assert max(worst.values()) <= 0.5, max(worst.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("cellname", ["LSTM", "GRU"])
@pytest.mark.parametrize("rnd", [bf, f32r])
def test_saturated_problems_are_saturated(cellname, rnd):
    """at least 10 % of the hard-sigmoid gate values clipped at 0, and as many at 1, at every shape; the LSTM cell state of the long
    window beyond 45 (e^{2c} leaves the f32 range at c = 44.4)"""
    shapes = {(H, par.SAT_T_FWD, B) for H, B in par.SAT_FWD_SHAPES + par.SAT_WIDE_SHAPES} | {(H, T, B) for H, T, B, _ in _sat_backward_cases(cellname)}
    for H, T, B in sorted(shapes):
        for xmode in ("dense", "index"):
            pb = _sat(cellname, H, T, B, rnd, xmode)
            lo, hi = par.clipped_share(cellname, pb.acts_r)
            print("clipped share %-4s %-5s H=%d T=%d B=%d %s: %.3f at 0, %.3f at 1" % (cellname, rnd.__name__, H, T, B, xmode, lo, hi))
            assert lo >= 0.10 and hi >= 0.10, (H, T, B, xmode, lo, hi)
    if cellname == "LSTM":
        H, T, B = par.SAT_LONG
        for xmode in ("dense", "const"):
            pb = _sat(cellname, H, T, B, rnd, xmode)
            assert np.abs(pb.cs).max() > 45 and np.all(np.isfinite(pb.hs)), (xmode, np.abs(pb.cs).max())


@pytest.mark.parametrize("cellname", ["LSTM", "GRU"])
def test_saturated_backward_defects_fail(cellname, monkeypatch):
    """the derivative 0.2 at a clipped gate, at every BPTT shape: the parity bounds see it, and so does the exact-zero check"""
    for H, T, B, ext in _sat_backward_cases(cellname):
        pb = _sat(cellname, H, T, B)
        args, want = _sat_backward(cellname, pb, ext)
        check_backward_saturated(cellname, (bf(want[0]), want[1], want[2]), want, pb.acts_r)
        with monkeypatch.context() as mp:
            mp.setitem(vo._REC_ACT, "hard_sigmoid", (vo.hard_sigmoid, lambda y: 0.2 + 0.0 * y))
            da, _, dh0, dc0 = vo.rnn_backward(cellname, *args)
        _fails(check_backward, cellname, (da, dh0, dc0), want)
        _fails(par.assert_clipped_gates_have_no_gradient, cellname, pb.acts_r, da)
        _fails(par.assert_clipped_gates_have_no_gradient, cellname, pb.acts_r, da + 1e-30)


@pytest.mark.parametrize("cellname", SAT_CELLS)
def test_saturated_forward_defects_fail(cellname, monkeypatch):
    """gates left unclipped; NaN where tanh of a planted row is +-1 (e^{2x} overflowing to inf / inf)"""
    cases = [(H, par.SAT_T_FWD, B) for H, B in par.SAT_FWD_SHAPES + par.SAT_WIDE_SHAPES] + ([par.SAT_LONG] if cellname == "LSTM" else [])
    for H, T, B in cases:
        pb = _sat(cellname, H, T, B)
        want = (pb.hs, pb.cs, pb.acts, pb.hs[-1])
        check_forward(cellname, (bf(pb.hs), bf(pb.cs) if pb.cs is not None else None, bf(pb.acts), pb.hs[-1]), want)
        if cellname != "SimpleRNN":
            with monkeypatch.context() as mp:
                mp.setitem(vo._REC_ACT, "hard_sigmoid", (lambda x: 0.2 * x + 0.5, vo._dhs))
                hs, cs, acts = vo.rnn_forward(cellname, pb.xp, pb.U, pb.h0, pb.c0)
            with np.errstate(over="ignore"):                  # (an unclipped LSTM cell state runs away)
                _fails(check_forward, cellname, (hs, cs, acts, hs[-1]), want)
        if B > 3:
            tanh_gate = {"LSTM": np.s_[:, 1, 2 * H:3 * H], "GRU": np.s_[:, 1, 2 * H:], "SimpleRNN": np.s_[:, 1]}[cellname]
            acts = pb.acts.copy()
            assert np.all(acts[tanh_gate] == 1.0)
            acts[tanh_gate] = np.nan
            _fails(check_forward, cellname, (pb.hs, pb.cs, acts, pb.hs[-1]), want)
            hs = pb.hs.copy()
            hs[1:, 1] = np.nan                                   # ... or the state: tanh(c) of a cell state past 44.4
            _fails(check_forward, cellname, (hs, pb.cs, pb.acts, hs[-1]), want)


@pytest.mark.parametrize("key", sorted(par.CLIPPED_HEAD_SEEDS))
@pytest.mark.parametrize("rnd", [bf, f32r])
def test_clipped_softmax_head_problem_and_its_defects(key, rnd):
    """the builder's probability bands hold at every case of the GPU tests (asserted inside the builder, on rounded operands); a
    correct head passes test_softmax_head's checks and the planted defects fail them.  The HIGH clip changes a row's loss by
    -log(1 - 1e-7) = 1e-7, which no loss check can see: that branch is covered by the gradient (exactly zero on such a row)."""
    N, H, R, two_hot = key
    rng, hs, W, bias, tgt, rw, tgt2, rows = par.softmax_head_clipped_problem(N, H, R, par.CLIPPED_HEAD_SEEDS[key], two_hot, rnd)
    Wq = rnd(W)
    low, high, inside = par.ce_bands(hs, Wq, bias, tgt, tgt2)
    clipped = par.fully_clipped_rows(low, high, inside)
    assert set(clipped) >= {rows["high"], rows["low"], rows["low_last_tile"]} and rows["low_last_tile"] >= 16 * ((R - 1) // 16)
    assert low.any() and high.any() and inside.sum() > R // 2
    if two_hot:
        assert {"low_inside", "inside_low", "low_high", "high_low", "low_low"} <= set(rows)
        assert set(clipped) >= {rows["low_high"], rows["high_low"], rows["low_low"]}
    if R == 40:                    # the padding-rows variant (b_stride = 8, b_valid = 5) keeps the bands and the planted rows
        t1, t2 = tgt.copy(), (tgt2.copy() if two_hot else None)
        moved = par.retarget_padding_rows(hs, Wq, bias, t1, t2, np.arange(R) % 8 < 5, [5] + list(rows.values()))
        bands = par.ce_bands(hs, Wq, bias, t1, t2)
        assert len(moved) >= R // 4 and np.all(bands[2][moved, 0]) and set(par.fully_clipped_rows(*bands)) == set(clipped)
    p, loss, dl, y = par.softmax_head_oracle(hs, Wq, bias, tgt, rw, 0.7, tgt2)
    assert np.all(dl[clipped] == 0) and np.all(dl[5] == 0)
    want = (p, dl, loss)
    check_softmax_head((p.astype(np.float32), rnd(dl), np.float32(loss)), want, BF16 if rnd is bf else par.F32)
    for dtype in (BF16, par.F32):
        leak = 0.7 * rw[:, None] * (p * y.sum(1, keepdims=True) - y)                 # p - y on a clipped row
        for row in clipped:
            bad = dl.copy()
            bad[row] = leak[row]
            _fails(check_softmax_head, (p, bad, loss), want, dtype)
        if two_hot:                                                                    # one target clipped: both dropped
            for row in (rows["low_inside"], rows["inside_low"], rows["low_inside_last_tile"]):
                assert np.abs(dl[row]).max() > 0
                _fails(check_softmax_head, (p, _zero(dl, row), loss), want, dtype)
        row = rows["low"]                                                             # loss from the unclipped log p
        unclipped = loss + rw[row] * (-np.log(p[row, tgt[row]]) + np.log(vo.CE_EPS))
        assert p[row, tgt[row]] < par.CE_FAR
        _fails(check_softmax_head, (p, dl, unclipped), want, dtype)


def model_head_f32(hs, Wq, bias, tgt, rw, grad_scale, tgt2, order):
    """a correct head in float32: logits accumulated in float32 in one of par.product_models' orders, softmax, Keras' clipped
    cross-entropy and its gradient evaluated in numpy float32.  Returns (probs, dlogits, loss)."""
    f = np.float32
    z = par.product_models(hs, Wq, bias=bias)[order].astype(f)
    e = np.exp(z - z.max(1, keepdims=True), dtype=f)
    p = e / e.sum(1, keepdims=True, dtype=f)
    R, N = p.shape
    dl, loss = np.zeros((R, N), f), f(0)
    for t in (tgt, tgt2) if tgt2 is not None else (tgt,):
        rows = np.nonzero(t < N)[0]
        pt = p[rows, t[rows]]
        inside = (pt >= f(vo.CE_EPS)) & (pt <= f(1) - f(vo.CE_EPS))
        y = np.zeros((R, N), f)
        y[rows[inside], t[rows[inside]]] = 1
        g = np.zeros((R, N), f)
        g[rows[inside]] = p[rows[inside]]
        dl += f(grad_scale) * rw.astype(f)[:, None] * (g - y)
        loss += np.sum(rw[rows].astype(f) * -np.log(np.clip(pt, f(vo.CE_EPS), f(1) - f(vo.CE_EPS)), dtype=f), dtype=f)
    return p.astype(np.float64), dl.astype(np.float64), float(loss)


@pytest.mark.parametrize("key", sorted(par.CLIPPED_HEAD_SEEDS))
@pytest.mark.parametrize("rnd", [bf, f32r])
def test_float32_model_of_a_correct_head_passes_the_bounds_on_clipped_rows(key, rnd):
    """the f32 bound on forward values is 1e-5 normwise per row, and the relative error of a probability is the absolute error of
    its logit: the planted rows must not ask more of an f32 kernel than f32 gives.  Worst of the accumulation orders: below half of
    every f32 bound (f32-rounded operands; bf16-rounded ones, whose products are exact, as well)."""
    N, H, R, two_hot = key
    rng, hs, W, bias, tgt, rw, tgt2, rows = par.softmax_head_clipped_problem(N, H, R, par.CLIPPED_HEAD_SEEDS[key], two_hot, rnd)
    Wq = rnd(W)
    p, loss, dl, _ = par.softmax_head_oracle(hs, Wq, bias, tgt, rw, 0.7, tgt2)
    for order in ("sequential", "tiles"):
        got = model_head_f32(hs, Wq, bias, tgt, rw, 0.7, tgt2, order)
        worst = _worst(check_softmax_head(got, (p, dl, loss), par.F32))
        print("clipped head f32 model %s %s %s: %.3f x the bound" % (key, rnd.__name__, order, worst))
        assert worst <= 0.5, (order, worst)


@pytest.mark.parametrize("rnd", [bf, f32r])
def test_saturated_sigmoid_head_problem(rnd):
    """float64 on the planted rows: sigmoid(+100) is 1 to the last bit, sigmoid(-100) = 3.7e-44 (the f32 kernel returns exactly 0:
    e^100 is inf), the zero-logit rows exactly 1/2 - rounded half-to-even to 0"""
    hs, W, bias, y, rw, rows = par.sigmoid_head_saturated_problem(40, 64, 2, rnd)
    p = vo.sigmoid(hs @ rnd(W) + bias)[:, 0]
    assert np.all(p[rows["plus"]] == 1.0) and np.all(p[rows["minus"]] < 1e-40) and np.all(p[rows["half"]] == 0.5)
    assert np.all(np.round(p[rows["half"]]) == 0.0) and list(y[rows["half"]]) == [0.0, 1.0]


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_engine_saturated_problem_keeps_its_distance_from_the_clips(cell):
    """test_engine_gpu's saturated problem: every pre-clip gate value of the float64 oracle at least 1e-4 from 0 and from 1, and at
    least 5 % of the gate values of each of the 8 recurrences clipped"""
    from tests import test_engine_gpu as eng_t
    margins = eng_t._oracle_gate_margins(*eng_t._saturated_problem(cell))
    assert len(margins) == 8
    for share, dist in margins:
        assert share >= eng_t.SATURATED_MIN_SHARE and dist >= eng_t.SATURATED_MIN_DISTANCE, margins


# ---- hand-over, carried state and chunk counters (the CPU side of test_rnn_handover_gpu.py) ------------------------------
def _handover_shapes():
    """(H, B, arithmetic mode, T) of every carried-state case of the GPU tests"""
    return [(H, B, dt, par.HANDOVER_T) for H, B, dt in par.GENERIC_SHAPES] + [(par.RES_H, par.RES_B, BF16, T) for T in sorted(par.TIME_SPLITS)]


def _rnd(dt):
    return bf if dt == BF16 else (lambda a: a)


@pytest.mark.parametrize("cellname", ["GRU", "LSTM", "SimpleRNN"])
def test_oracle_in_time_chunks_with_carried_state_equals_the_whole_sequence(cellname):
    """the slicing and carry plumbing of the GPU tests' part 2, on their own inputs: the oracle run chunk by chunk (h0 = h_last,
    c0 = c_last forward; dh_last = dh0, dc_last = dc0 from the last chunk to the first) equals its whole-sequence run to 1e-12"""
    for H, B, dt, T in _handover_shapes():
        if cellname == "SimpleRNN" and H == par.RES_H:
            continue
        for xmode in ("dense", "index"):
            pb = par.rnn_forward_inputs(cellname, H, T, B, xmode, seed=H + B + T, rnd=_rnd(dt))
            for lengths in par.TIME_SPLITS[T]:
                assert sum(lengths) == T
                hs, cs, acts = par.forward_in_chunks(cellname, pb.xp, pb.U, pb.h0, pb.c0, lengths)
                np.testing.assert_allclose(hs, pb.hs, rtol=0, atol=1e-12)
                np.testing.assert_allclose(acts, pb.acts, rtol=0, atol=1e-12)
                if cs is not None:
                    np.testing.assert_allclose(cs, pb.cs, rtol=0, atol=1e-12)
        for ext in (True, False):
            U, hs_o, cs_o, acts_o, dext, dlast = par.rnn_backward_problem(cellname, H, T, B, ext, _rnd(dt))
            dclast = par.carried_cell_gradient(H, B) if cellname == "LSTM" else None
            da_w, _, dh0_w, dc0_w = vo.rnn_backward(cellname, hs_o, cs_o, acts_o, U, dext, dlast, dc_last=dclast)
            for lengths in par.TIME_SPLITS[T]:
                da, dh0, dc0 = par.backward_in_chunks(cellname, hs_o, cs_o, acts_o, U, dext, dlast, lengths, dclast)
                np.testing.assert_allclose(da, da_w, rtol=0, atol=1e-12)
                np.testing.assert_allclose(dh0, dh0_w, rtol=0, atol=1e-12)
                if cellname == "LSTM":
                    np.testing.assert_allclose(dc0, dc0_w, rtol=0, atol=1e-12)


def test_oracle_dc_last_defaults_to_zero_and_reaches_dc0():
    """rnn_backward(dc_last=None) is what it was; a dc_last changes da and dc0 of an LSTM and nothing of a GRU"""
    U, hs_o, cs_o, acts_o, dext, dlast = par.rnn_backward_problem("LSTM", 64, 7, 5, True, lambda a: a)
    base = vo.rnn_backward("LSTM", hs_o, cs_o, acts_o, U, dext, dlast)
    zero = vo.rnn_backward("LSTM", hs_o, cs_o, acts_o, U, dext, dlast, dc_last=np.zeros((5, 64)))
    for a, b in zip(base, zero):
        np.testing.assert_array_equal(a, b)
    dcl = par.carried_cell_gradient(64, 5)
    with_dc = vo.rnn_backward("LSTM", hs_o, cs_o, acts_o, U, dext, dlast, dc_last=dcl)
    twice = vo.rnn_backward("LSTM", hs_o, cs_o, acts_o, U, dext, dlast, dc_last=2.0 * dcl)
    for k in (0, 2, 3):                                           # BPTT is linear in the gradients that arrive: da, dh0, dc0
        np.testing.assert_allclose(twice[k] - with_dc[k], with_dc[k] - base[k], rtol=0, atol=1e-12)
        assert np.abs(with_dc[k] - base[k]).max() > 1e-4
    Ug, hs_g, _, acts_g, dext_g, dlast_g = par.rnn_backward_problem("GRU", 64, 7, 5, True, lambda a: a)
    for a, b in zip(vo.rnn_backward("GRU", hs_g, None, acts_g, Ug, dext_g, dlast_g)[:3],
                    vo.rnn_backward("GRU", hs_g, None, acts_g, Ug, dext_g, dlast_g, dc_last=dcl)[:3]):        # (da, dU, dh0)
        np.testing.assert_array_equal(a, b)


def _walk_forward(T, cs):
    """a step-by-step walk that MIRRORS the forward kernels' own bookkeeping (pk / phi, advanced at a chunk's first step) - it pins
    the closed forms of tests/parity.py to the code's logic, it is not a second derivation; the independent checks are the ones
    beside it (floor(t / cs) per step, the chunks' step ranges covering range(T) once).  Returns (chunk of every step, [(chunk,
    step behind which it is published)])"""
    pk, phi, of, pub = 0, cs, [], []
    for t in range(T):
        if t == phi:            # the first step of the next chunk: the previous chunk's last hs slot is written during it
            pub.append((pk, t - 1))
            pk, phi = pk + 1, phi + cs
        of.append(pk)
    pub.append((pk, T - 1))
    return of, pub


def _walk_backward(T, cs):
    """the same for the backward kernels (pk / plo, from the last step down): a mirror of their bookkeeping"""
    pk = (T - 1) // cs
    plo, of, pub = pk * cs, {}, []
    for t in range(T - 1, -1, -1):
        of[t] = pk
        if t == plo:
            pub.append((pk, t))
            pk, plo = pk - 1, plo - cs
    return [of[t] for t in range(T)], pub


def test_chunk_counter_rule_against_a_walk_over_the_steps():
    """parity.chunk_count / chunk_of_step / chunk_steps_of / publish_order at every (T, chunk_steps) the GPU tests use"""
    cases = par.handover_t_cs()
    assert (8, 2) in cases and (33, 16) in cases and (1, 16) in cases and (9, 1) in cases
    for T, cs in cases:
        for forward, walk in ((True, _walk_forward), (False, _walk_backward)):
            of, pub = walk(T, cs)
            assert of == [par.chunk_of_step(t, cs) for t in range(T)] == [int(np.floor(t / cs)) for t in range(T)], (T, cs)
            assert pub == par.publish_order(T, cs, forward), (T, cs, forward)
            assert len(pub) == par.chunk_count(T, cs) == max(of) + 1
        steps = [t for k in range(par.chunk_count(T, cs)) for t in range(*par.chunk_steps_of(k, T, cs))]
        assert steps == list(range(T)), (T, cs)
        assert par.expected_counters(T, cs, 8, 48, launches=2) == [48] * par.chunk_count(T, cs)
    for cs in par.COUNTER_CS:
        assert all(1 <= T <= par.COUNTER_T_MAX for T in par.counter_lengths(cs))


def test_phase_launch_problems_stay_small():
    """the resident kernels wait for each other inside one launch: the GPU tests' phase launches stay under 24 workgroups"""
    assert sum(B // 16 for _, B, _, _ in par.PHASE_PROBLEMS) < 24
    assert max(par.XPAND_BLOCKS) + par.XPAND_B // 16 < 24 and par.XPAND_T % par.XPAND_CS == 0
    assert sorted({B for _, B, _, _ in par.PHASE_PROBLEMS}) == [16, 32, 48] and {T for T, _, _, _ in par.PHASE_PROBLEMS} == {4, 16, 33}
