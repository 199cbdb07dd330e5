"""One-hot rows of 129 .. 192 columns (inputs up to 255) on the GPU: the 9..12-tile softmax head, the fast GEMM with a narrow last
N tile (the head's dW) and with a one-hot A of two M tiles (the table gradient) - single, batched and K-streaming launches -, the
engine against OracleVAE, the Keras surface with and without step plans, and the index-mode classifier.  Tolerances: the
scale-aware bounds of tests/parity.py and the engine bounds of test_hidden_sizes_gpu.py / test_engine_gpu.py, unchanged."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
import tests.test_ops_gpu as ops_t
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from midi_vae_amd import packers as pk
from midi_vae_amd.classifier import ClassifierEngine
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.engine import Engine
from midi_vae_amd.model import VAE
from oracle.classifier_oracle import OracleClassifier
from oracle.vae_oracle import OracleVAE, make_cfg
from tests import parity as par
from tests.test_classifier_gpu import _problem as _cls_problem
from tests.test_engine_gpu import _onehot, _problem, _rel_l2, _stage

pytestmark = pytest.mark.gpu

DEV = ops_t.DEV
dev, host, close, tile16 = ops_t.dev, ops_t.host, ops_t.close, ops_t.tile16
HEAD_MODES = [(hl.F32, 2e-5, 64), (hl.BF16, 2e-2, 256)]
WIDE_N = [129, 145, 192]


# ---- head kernel -----------------------------------------------------------------------------------------------------------
def _head_buffers(W, N, H, td):
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=td, device=DEV)
    wc = torch.full((H, NP), 7.0, dtype=td, device=DEV)
    pb = ops.PrepBatch()
    pb.transpose_convert(dev(W), wt, n_pad=NP); pb.convert_pad(dev(W), wc, NP)
    pb.run()
    return NP, wt, wc


@pytest.mark.parametrize("dtype,tol,H", HEAD_MODES)
@pytest.mark.parametrize("N,two_hot", [(129, False), (145, False), (192, False), (145, True), (192, True)])
def test_wide_softmax_head_every_output(dtype, tol, H, N, two_hot):
    """R = 320 rows: 20 row tiles = 5 workgroups of 4 waves; targets in columns 127, 128 and N - 1, rows without a target (255), a
    second hot column >= 129 (two_hot); probabilities, loss, accuracy, first-maximum argmax, d(logits) with zero pad columns and
    the fused dhs = d(logits) W^T - against float64 on the kernel's rounded hs and W"""
    R = 320
    rng, hs_h, W, bias, tgt, rw, tgt2 = par.softmax_head_problem(N, H, R, seed=N, two_hot=two_hot)
    tgt[[0, 17, 100]] = (127, 128, N - 1)
    tgt[[5, 33, 319]] = 255
    if two_hot:
        tgt2 = np.where(tgt2 == 255, 255, 129 + tgt2 % (N - 129))
        tgt2[[0, 17]] = (N - 1, 129)
        tgt2[tgt2 == tgt] = 255
        assert np.all(tgt2 >= 129) and np.sum(tgt2 < N) > R // 2
    td = ops.torch_dtype(dtype)
    hs = dev(hs_h, td)
    NP, wt, wc = _head_buffers(W, N, H, td)
    assert NP >= N and NP % 16 == 0
    assert np.array_equal(host(wc)[:, :N], host(wt)[:N].T) and np.all(host(wc)[:, N:] == 0) and np.all(host(wt)[N:] == 0)
    Wq = host(wt)[:N].T
    p, want_loss, want_dl, y = par.softmax_head_oracle(host(hs), Wq, bias, tgt, rw, 0.7, tgt2)
    probs = torch.zeros((R, N), device=DEV)
    am = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    dl = torch.full((R, NP), 3.0, dtype=td, device=DEV)
    dhs = torch.zeros((R, H), dtype=td, device=DEV)
    sc = torch.zeros((2,), device=DEV)
    ops.head(0, dtype, R, H, N, hs, wt, dev(bias), target_idx=dev(tgt, torch.uint8), row_weight=dev(rw), grad_scale=0.7,
             probs=probs, argmax=am, dlogits=dl, scalars=sc, wc=wc, dhs=dhs,
             target_idx2=dev(tgt2, torch.uint8) if two_hot else None)
    torch.cuda.synchronize()
    close(host(probs), p, tol, "probs")
    close(host(dl)[:, :N], want_dl, tol, "dlogits")
    assert np.all(host(dl)[:, N:] == 0)
    close(host(sc)[0], want_loss, tol * 5, "loss")
    par.assert_parity(host(probs), p, dtype, par.row_blocks, "probs", values=True)
    par.assert_parity(host(dl)[:, :N], want_dl, dtype, par.row_blocks, "dlogits")
    par.assert_rel(host(sc)[0], want_loss, par.LOSS_RTOL, "loss")
    # argmax: the first maximum of the probabilities the kernel returned; a hit = the target row's first hot column (0 if none)
    pk_ = probs.cpu().numpy()
    assert np.array_equal(am.cpu().numpy(), np.argmax(pk_, axis=1).astype(np.uint8))
    assert host(sc)[1] == np.sum(np.argmax(pk_, 1) == np.argmax(y, 1))
    # the fused input gradient, from the d(logits) of the same launch
    want_dhs = host(dl) @ host(wc).T
    got_dhs = host(tile16(dhs, R, H, False))
    assert np.abs(want_dhs).max() > 0
    close(got_dhs, want_dhs, tol, "dhs")
    par.assert_parity(got_dhs, want_dhs, dtype, par.row_blocks, "dhs")


@pytest.mark.parametrize("dtype,tol,H", HEAD_MODES)
@pytest.mark.parametrize("N", WIDE_N)
def test_wide_softmax_head_argmax_planted_winner_on_every_row(dtype, tol, H, N):
    """row r is built along weight column r % N (every column wins somewhere, the tiles beyond 128 included), so that its logit
    leads by a margin no rounding of the bf16 operands closes: the fused argmax must equal the oracle's on ALL rows, and the
    accuracy count with it"""
    rng = np.random.default_rng(200 + N)
    R = 320
    W = rng.standard_normal((H, N)) * 0.3
    bias = rng.standard_normal((N,)) * 0.1
    win = np.arange(R) % N
    hs_h = 0.05 * rng.standard_normal((R, H)) + 12.0 * (W[:, win] / np.sum(W[:, win] ** 2, 0)).T
    td = ops.torch_dtype(dtype)
    hs = dev(hs_h, td)
    NP, wt, _ = _head_buffers(W, N, H, td)
    lg = host(hs) @ host(wt)[:N].T + bias                      # float64 on the rounded operands
    top2 = np.sort(lg, 1)[:, -2:]
    assert np.array_equal(np.argmax(lg, 1), win) and np.all(top2[:, 1] - top2[:, 0] > 1.0)      # decisive on every row
    am = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    sc = torch.zeros((2,), device=DEV)
    tgt = np.where(np.arange(R) % 3 == 0, win, (win + 1) % N)
    ops.head(0, dtype, R, H, N, hs, wt, dev(bias), target_idx=dev(tgt, torch.uint8), argmax=am, scalars=sc)
    torch.cuda.synchronize()
    assert np.array_equal(am.cpu().numpy(), win.astype(np.uint8))
    assert host(sc)[1] == np.sum(tgt == win)


@pytest.mark.parametrize("dtype,tol,H", HEAD_MODES)
@pytest.mark.parametrize("N,c,c2", [(129, 5, 128), (145, 127, 128), (192, 100, 191)])
def test_wide_softmax_head_argmax_tie_across_the_128_column_boundary(dtype, tol, H, N, c, c2):
    """two bit-identical weight columns c < 128 <= c2, lifted above every other column: the first maximum is c"""
    rng = np.random.default_rng(7 + N)
    R = 16 * 9 + 5
    hs_h = rng.standard_normal((R, H))
    W = rng.standard_normal((H, N)) * 0.3
    bias = rng.standard_normal((N,)) * 0.1
    W[:, c2] = W[:, c]
    bias[c2] = bias[c] = bias[c] + 5.0 * np.abs(hs_h @ W + bias).max()
    td = ops.torch_dtype(dtype)
    NP, wt, _ = _head_buffers(W, N, H, td)
    probs = torch.zeros((R, N), device=DEV)
    am = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    ops.head(0, dtype, R, H, N, dev(hs_h, td), wt, dev(bias), probs=probs, argmax=am)
    torch.cuda.synchronize()
    p = probs.cpu().numpy()
    assert np.array_equal(p[:, c], p[:, c2]) and np.all(p[:, c] == p.max(1))          # the tie is exact on the device
    assert np.all(am.cpu().numpy() == c)


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16])
def test_head_refuses_more_than_192_columns(dtype):
    """N = 193: no padded width, MVAE_E_UNSUPPORTED, nothing launched - dlogits and dhs keep what they held"""
    rng = np.random.default_rng(43)
    R, H, N, NP = 320, 64, 193, 208
    assert ops.head_np(N) == -1 and ops.head_np(192) == 192
    td = ops.torch_dtype(dtype)
    wt = dev(rng.standard_normal((NP, H)) * 0.1, td)
    wc = dev(rng.standard_normal((H, NP)) * 0.1, td)
    dl = torch.full((R, NP), 3.0, dtype=td, device=DEV)
    dhs = torch.full((R, H), 5.0, dtype=td, device=DEV)
    with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):
        ops.head(0, dtype, R, H, N, dev(rng.standard_normal((R, H)), td), wt, dev(np.zeros(N)),
                 target_idx=dev(rng.integers(0, N, (R,)), torch.uint8), grad_scale=1.0, dlogits=dl, wc=wc, dhs=dhs)
    torch.cuda.synchronize()
    assert torch.all(dhs == 5.0) and torch.all(dl == 3.0)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------
GK = 1024
GEMM_CASES = [("dense", 256, N) for N in WIDE_N] + [("onehot", M, 256) for M in (129, 200, 255)]
# (mode, split-K counts).  A K-streaming problem's partitions are whole 64-row k tiles of a chunk: 3 does not divide one - 2 and 16
# there; ``kstream`` = (partitions, chunk rows)
GEMM_MODES = [("gemm", (3, 16)), ("multi", (3, 16)), ("kstream", ((2, 256), (16, 1024)))]


def _wide_operands(kind, M, N, integer, rng):
    """A (K, M) bf16 or one-hot indices hitting rows 127, 128 and M - 1; B (K, ldb) bf16 with data in its pad columns too"""
    ldb = ops.head_np(N) if kind == "dense" else N
    if kind == "onehot":
        idx = rng.integers(0, M, (GK,))
        idx[[3, 500, 1023]] = (127, 128, M - 1)
        A = dev(idx, torch.uint8)
        A64 = np.zeros((GK, M))
        A64[np.arange(GK), idx] = 1.0
    else:
        A = dev(par.integer_operands(rng, (GK, M)) if integer else rng.standard_normal((GK, M)) * 0.5, torch.bfloat16)
        A64 = host(A)
    Bd = dev(par.integer_operands(rng, (GK, ldb)) if integer else rng.standard_normal((GK, ldb)) * 0.5, torch.bfloat16)
    return A, A64, Bd, host(Bd)[:, :N], ldb


def _launch(mode, sk, A, Bd, C, M, N, ldb, ldc, onehot, alpha, keep):
    kw = dict(trans_a=True, ldb=ldb, ldc=ldc, accumulate=True, a_kind=hl.ONEHOT if onehot else None, alpha=alpha)
    if mode == "gemm":
        ops.gemm(A, Bd, C, M, N, GK, split_k=sk, **kw)
    elif mode == "multi":            # the full count: the fast family took it
        assert ops.gemm_multi([ops.gemm(A, Bd, C, M, N, GK, split_k=sk, build_only=True, **kw)]) == 1
    else:
        P, rows = sk
        counters = torch.full((GK // rows,), 10, dtype=torch.int32, device=DEV)       # (already published: the non-live variant)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        keep += [counters, status]
        ops.gemm(A, Bd, C, M, N, GK, split_k=P, k_wait=counters, k_wait_value=7, k_chunk_rows=rows, k_reverse=True,
                 chunk_status=status, **kw)
        torch.cuda.synchronize()
        assert int(status.item()) == 0


@pytest.mark.parametrize("mode,splits", GEMM_MODES)
@pytest.mark.parametrize("kind,M,N", GEMM_CASES)
def test_fast_gemm_narrow_last_n_tile_and_two_tile_onehot(kind, M, N, mode, splits):
    """C (M, N) += alpha A^T B into an oversized, pre-filled C: against float64 (assert_product), bit-equal on small integers, and
    every element outside the M x N block unchanged"""
    rng = np.random.default_rng(1000 + M + N)
    onehot = kind == "onehot"
    rows_c, ldc = M + 9, N + 24
    for sk in splits:
        for integer in (False, True):
            A, A64, Bd, B64, ldb = _wide_operands(kind, M, N, integer, rng)
            c0 = host(dev(par.integer_operands(rng, (rows_c, ldc)) if integer else rng.standard_normal((rows_c, ldc))))
            C = dev(c0)
            keep = []
            _launch(mode, sk, A, Bd, C, M, N, ldb, ldc, onehot, 0.5, keep)
            torch.cuda.synchronize()
            got = host(C)
            what = "%s M=%d N=%d %s split %s" % (kind, M, N, mode, sk)
            want = c0[:M, :N] + 0.5 * (A64.T @ B64)
            if integer:
                par.assert_bits(got[:M, :N], want, "f32", what + " (integers)")
            else:
                par.assert_product(got[:M, :N], want, par.product_unit(A64.T, B64, 0.5, [c0[:M, :N]]), "bf16", what)
            par.assert_bits(got[:M, N:], c0[:M, N:], "f32", what + ": columns beyond N")
            par.assert_bits(got[M:], c0[M:], "f32", what + ": rows beyond M")


def test_wide_gradient_gemms_share_the_batched_and_the_k_streaming_launch():
    """all six shapes as problems of ONE mvae_gemm_multi launch (the full count is returned) and of ONE mvae_gemm_kstream_multi
    launch, equal to float64"""
    rng = np.random.default_rng(77)
    ops_, outs = [], {}
    for kind, M, N in GEMM_CASES:
        ops_.append((kind, M, N) + _wide_operands(kind, M, N, False, rng))
    counters = torch.full((4,), 10, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for name, extra in (("multi", dict(split_k=3)), ("kstream", dict(split_k=4, k_wait=counters, k_wait_value=7, k_chunk_rows=256,
                                                                    k_reverse=True, chunk_status=status))):
        probs, Cs = [], []
        for kind, M, N, A, A64, Bd, B64, ldb in ops_:
            C = torch.zeros((M, N), device=DEV)
            Cs.append(C)
            probs.append(ops.gemm(A, Bd, C, M, N, GK, trans_a=True, ldb=ldb, accumulate=True,
                                  a_kind=hl.ONEHOT if kind == "onehot" else None, build_only=True, **extra))
        if name == "multi":
            assert ops.gemm_multi(probs) == len(probs)
        else:
            ops.gemm_kstream_multi(probs)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        for (kind, M, N, A, A64, Bd, B64, ldb), C in zip(ops_, Cs):
            par.assert_product(host(C), A64.T @ B64, par.product_unit(A64.T, B64), "bf16", "%s %s M=%d N=%d" % (name, kind, M, N))


# ---- engine ----------------------------------------------------------------------------------------------------------------
def _check_engine(spec, params, batch, raw, dtype, B, stage=None):
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    m_o, cache = orc.forward(p64, batch, raw["eps"].astype(np.float64))
    g_o = orc.backward(p64, cache)
    eng = Engine(spec, max_batch=32, dtype=dtype, seed=0)
    eng.set_params(params)
    (stage or _stage)(eng, raw, B)
    eng.forward_backward(B)
    eng.check_pipeline()
    m = eng.metrics(B)
    g = eng.get_grads()
    tol = 2e-4 if dtype == "f32" else 3e-2
    for k in m_o:
        if k.endswith("_acc"):
            if dtype == "f32":
                assert abs(m[k] - m_o[k]) < 1e-9, (k, m[k], m_o[k])
            continue
        assert abs(m[k] - m_o[k]) <= tol * (1 + abs(m_o[k])), (k, m[k], m_o[k])
    for k in g_o:
        if dtype == "f32":
            err = np.abs(g[k] - g_o[k])
            assert np.all(err <= 2e-6 + 2e-4 * np.abs(g_o[k]) + 2e-4 * np.abs(g_o[k]).max()), (k, err.max())
        elif np.linalg.norm(g_o[k]) < 1e-9:
            assert np.linalg.norm(g[k]) < 1e-6, k
        else:
            assert _rel_l2(g[k], g_o[k]) < 6e-2, (k, _rel_l2(g[k], g_o[k]))


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
@pytest.mark.parametrize("dtype,H", [("f32", 64), ("bf16", 256)])
@pytest.mark.parametrize("D", [145, 192])
def test_engine_forward_backward_matches_oracle_wide_rows(cell, dtype, H, D):
    """bf16 at H = 256: the resident / two-waves-per-SIMD kernels gather rows >= 128 of their (paired) input tables"""
    B = 7
    spec, params, batch, raw = _problem(cell, B, seed=B, H=H, Din=D, Dout=D)
    assert raw["x_idx"].max() >= 128
    _check_engine(spec, params, batch, raw, dtype, B)


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
@pytest.mark.parametrize("dtype,H", [("f32", 64), ("bf16", 256)])
@pytest.mark.parametrize("kw", [dict(Din=149, Dout=145, ID=130, meta_instrument=True), dict(Din=145, Dout=145, comp_notes=True, meta_next=True)],
                         ids=["instrument_head_130", "comp_notes_next_notes"])
def test_engine_wide_side_heads_and_classifier_on_the_notes_output(cell, dtype, H, kw):
    B = 7
    spec, params, batch, raw = _problem(cell, B, seed=11, H=H, **kw)
    _check_engine(spec, params, batch, raw, dtype, B)


@pytest.mark.parametrize("cell,dtype,H,T", [("GRU", "f32", 64, 12), ("LSTM", "f32", 64, 12), ("LSTM", "bf16", 256, 64)])
def test_attach_instruments_two_hot_rows_match_oracle_at_145_columns(cell, dtype, H, T):
    """test_engine_gpu.test_attach_instruments_two_hot_rows_match_oracle at 129 + 16 columns: the second hot column is >= 129"""
    B, A = 16, 16
    spec, params, batch, raw = _problem(cell, B, seed=91, H=H, Z=32, T=T, Din=145, Dout=145, attach=A)
    D0 = spec.Din - A
    rng = np.random.default_rng(4)
    x_idx = rng.integers(0, D0, (B, T)).astype(np.uint8)
    x_idx[0, :2] = (127, 128)
    xa_idx = np.tile(raw["i_idx"][:, np.arange(T) % spec.V], 1).astype(np.uint8)
    X = np.concatenate([_onehot(x_idx, D0), _onehot(xa_idx, A)], -1)
    batch = dict(batch, X=X, Y=X)
    raw = dict(raw, x_idx=x_idx)
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    m_o, cache = orc.forward(p64, batch, raw["eps"].astype(np.float64))
    g_o = orc.backward(p64, cache)
    eng = Engine(spec, max_batch=B, dtype=dtype)
    eng.set_params(params)
    eng.stage_encoder_inputs(x_idx, raw["i_idx"], raw["vel"], raw["eps"], d_idx=raw["d_idx"], xa_idx=xa_idx)
    eng.stage_decoder_inputs(B, hist=raw["hist"], add=raw["add"])
    eng.stage_targets(B, x_idx, raw["c_idx"], w_notes=raw["w_notes"], n_idx=raw["n_idx"], sig=raw["sig"], ya_idx=xa_idx)
    eng.forward_backward(B)
    eng.check_pipeline()
    m, g = eng.metrics(B), eng.get_grads()
    tol_l, tol_g = (2e-4, 2e-3) if dtype == "f32" else (3e-2, 6e-2)
    for k in m_o:
        assert abs(m[k] - m_o[k]) <= tol_l * (1 + abs(m_o[k])) + (1e-6 if k.endswith("_acc") else 0), (k, m[k], m_o[k])
    for k in g_o:
        n = np.linalg.norm(g_o[k])
        if n < 1e-12:
            assert np.linalg.norm(g[k]) < 1e-6, k
        else:
            assert _rel_l2(g[k], g_o[k]) < tol_g, (k, _rel_l2(g[k], g_o[k]))


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_three_adam_steps_at_145_columns_match_oracle_f32(cell):
    B = 16
    spec, params, batch, raw = _problem(cell, B, seed=3, Din=145, Dout=145)
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    st = orc.new_opt_state(p64)
    eng = Engine(spec, max_batch=B, dtype="f32")
    eng.set_params(params)
    _stage(eng, raw, B)
    for step in range(3):
        m_o = orc.train_step(p64, st, batch, raw["eps"].astype(np.float64))
        eng.train_step(B)
        m = eng.metrics(B)
        assert abs(m["loss"] - m_o["loss"]) < 1e-3, (step, m["loss"], m_o["loss"])
    got = eng.get_params()
    for k in p64:
        assert np.allclose(got[k], p64[k], rtol=1e-3, atol=2e-5), k


# ---- Keras surface ---------------------------------------------------------------------------------------------------------
EPOCHS = 3        # minibatches 8, 8, 4 per epoch: a step is recorded three times, then replayed


def wide_settings(cell):
    return build_settings(cell_type=cell, high_crop=128, low_crop=0, lstm_size=64, input_length=4, output_length=4, batch_size=8,
                          learning_rate=1e-2)


def wide_windows(s, n=20, seed=5):
    """a small song in the TOP of the range: pitches 120 .. 127 and, on 60 % of the rows, the silent column 128 - what the fitted
    decoder then answers with on most rows (checked on the CPU with the oracle's trajectory: every decoded row is 128)"""
    rng = np.random.default_rng(seed)
    T, D = s["output_length"], s["output_dim"]
    x_idx = np.where(rng.random((n, T)) < 0.6, D - 1, rng.integers(120, 128, (n, T))).astype(np.uint8)
    X = np.eye(D)[x_idx.astype(np.int64)]
    I = np.eye(s["meta_instrument_dim"])[rng.integers(0, s["meta_instrument_dim"], s["max_voices"])]
    V = np.where((x_idx != D - 1) & (rng.random((n, T)) >= 0.5), 0.5 + 0.5 * rng.random((n, T)), 0.0)
    return X, X.copy(), 0, I, V, np.zeros((n, T))


def _model_run(monkeypatch, plans, cell):
    monkeypatch.setenv("MVAE_PLANS", plans)
    s = wide_settings(cell)
    assert s["input_dim"] == s["output_dim"] == 129
    m = VAE().create(compute_dtype="f32", seed=0, **create_kwargs(s))
    X, Y, C, I, V, D = wide_windows(s)
    n = X.shape[0]
    Hh = np.zeros((n, s["latent_dim"]))
    S = np.zeros((n, s["signature_vector_length"]))
    x, y, sw = pk.prepare_autoencoder_input_and_output_list(s, X, Y, C, I, V, D, S, Hh, return_sample_weight=True)
    hist = m.autoencoder.fit(x, y, epochs=EPOCHS, batch_size=s["batch_size"], shuffle=False, sample_weight=sw, verbose=False)
    out = dict(loss=np.array(hist.history["loss"]))
    out["evaluate"] = np.array(m.autoencoder.evaluate(x, y, batch_size=s["batch_size"], verbose=False), dtype=np.float64)
    m._shared.rng = np.random.default_rng(0)
    z = m.encoder.predict(pk.prepare_encoder_input_list(s, X, I, V, D), batch_size=s["batch_size"], verbose=False)
    out["z"] = z
    dec_in = pk.prepare_decoder_input(s, z, C, S, None)
    dec = m.decoder.predict(dec_in, batch_size=s["batch_size"])
    out["decoded"] = dec[0]
    idx = m.decoder.predict_note_indices(dec_in, batch_size=s["batch_size"])
    out["idx"] = np.asarray(idx)
    assert np.array_equal(np.asarray(idx).ravel(), np.argmax(np.asarray(dec[0]).reshape(-1, 129), 1))
    assert np.array_equal(pk.notes_from_indices(s, idx, 129), pk.process_decoder_outputs(s, dec, "argmax")[0])
    return m, s, (X, Y, C, I, V, Hh), out, dict(m._shared.engine.plan_stats)


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_vae_full_midi_range_fit_evaluate_decode_with_and_without_plans(cell, monkeypatch):
    m, s, (X, Y, C, I, V, Hh), on, stats_on = _model_run(monkeypatch, "1", cell)
    assert stats_on["recorded"] >= 1 and stats_on["replayed"] >= 1, stats_on
    spec = m.spec
    assert spec.Din == spec.Dout == 129
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    from midi_vae_amd.layout import init_params
    p = {k: v.astype(np.float64) for k, v in init_params(spec, 0).items()}
    st = orc.new_opt_state(p)
    rng = np.random.default_rng(1)
    n, bs = X.shape[0], s["batch_size"]
    Coh = np.eye(s["num_classes"])[np.full(n, C)]
    It = np.tile(I[None], (n, 1, 1))
    for e in range(EPOCHS):
        tot = 0.0
        for lo in range(0, n, bs):
            hi = min(n, lo + bs)
            eps = (rng.standard_normal((hi - lo, spec.Z)) * spec.epsilon_std).astype(np.float32).astype(np.float64)
            b = dict(X=X[lo:hi], I=It[lo:hi], Vel=V[lo:hi, :, None], Hist=Hh[lo:hi], Y=Y[lo:hi], C=Coh[lo:hi])
            tot += orc.train_step(p, st, b, eps)["loss"] * (hi - lo)
        assert abs(on["loss"][e] - tot / n) < 1e-3, (e, on["loss"][e], tot / n)
    assert np.all(np.isfinite(on["evaluate"])) and np.all(np.isfinite(on["z"]))
    assert on["idx"].max() > 127, np.unique(on["idx"])           # a decoded column beyond the old ceiling
    del m
    torch.cuda.synchronize()
    _, _, _, off, stats_off = _model_run(monkeypatch, "0", cell)
    assert stats_off["replayed"] == 0, stats_off
    np.testing.assert_allclose(off["loss"], on["loss"], rtol=3e-5, atol=3e-6)
    np.testing.assert_allclose(off["evaluate"], on["evaluate"], rtol=3e-5, atol=3e-6)
    for k in ("z", "decoded"):
        assert np.linalg.norm(off[k] - on[k]) <= 1e-3 * np.linalg.norm(on[k]) + 1e-5, (k, np.linalg.norm(off[k] - on[k]))
    assert np.array_equal(off["idx"], on["idx"])


# ---- style classifier ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_classifier_index_mode_145_columns_matches_oracle(dtype):
    B = 21
    spec, params, x, X, c, Y = _cls_problem("index", B, 12, 145, 3, 64, 2, seed=6)
    assert x.max() >= 128
    orc = OracleClassifier(spec.oracle_cfg())
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    probs_o, m_o, cache = orc.forward(p64, X, Y)
    g_o = orc.backward(p64, cache)
    eng = ClassifierEngine(spec, max_batch=32, dtype=dtype)
    eng.set_params(params)
    eng.stage(x, c)
    eng.grads.zero_()
    eng.forward(B, want_probs=True)
    eng.backward(B)
    m = eng.metrics(B)
    g = eng.get_grads()
    if dtype == "f32":
        assert abs(m["loss"] - m_o["loss"]) <= 2e-4 * (1 + abs(m_o["loss"])) and abs(m["acc"] - m_o["acc"]) < 1e-9
        np.testing.assert_allclose(eng.probs(B), probs_o, rtol=2e-4, atol=2e-6)
        for k in g_o:
            err = np.abs(g[k] - g_o[k])
            assert np.all(err <= 2e-6 + 2e-4 * np.abs(g_o[k]) + 2e-4 * np.abs(g_o[k]).max()), (k, err.max())
    else:
        assert abs(m["loss"] - m_o["loss"]) <= 3e-2 * (1 + abs(m_o["loss"]))
        np.testing.assert_allclose(eng.probs(B), probs_o, rtol=3e-2, atol=3e-3)
        for k in g_o:
            if np.linalg.norm(g_o[k]) > 1e-9:
                assert _rel_l2(g[k], g_o[k]) < 6e-2, (k, _rel_l2(g[k], g_o[k]))
