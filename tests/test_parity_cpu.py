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
