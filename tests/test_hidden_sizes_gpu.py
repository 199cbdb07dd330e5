"""lstm_size = 192 .. 512 (64 k) on the GPU: the generic recurrent kernels at the new widths against the float64 oracle (the
tolerances of test_ops_gpu), the engine's forward / backward and Adam steps against OracleVAE, the Keras surface (fit / evaluate /
predict / decode / weight files, with and without step plans) and the style classifier."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
import tests.test_ops_gpu as ops_t
from midi_vae_amd import packers as pk
from midi_vae_amd.classifier import ClassifierEngine, StyleClassifier
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.engine import Engine
from midi_vae_amd.model import VAE
from midi_vae_amd.synth import make_windows, to_reference_format
from oracle.classifier_oracle import OracleClassifier
from oracle.vae_oracle import OracleVAE, make_cfg
from tests import parity as par
from tests.test_classifier_gpu import _problem as _cls_problem
from tests.test_engine_gpu import _problem, _rel_l2, _stage

pytestmark = pytest.mark.gpu

NEW_H = [192, 320, 384, 448, 512]
RAGGED_B = {192: 5, 320: 37, 384: 21, 448: 5, 512: 37}


# ---- kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cellname,cell", ops_t.CELLS)
@pytest.mark.parametrize("dtype,tol", ops_t.DTYPES)
@pytest.mark.parametrize("H,xmode", [(H, "dense") for H in NEW_H] + [(H, m) for H in (384, 512) for m in ("index", "scalar", "const")])
def test_rnn_forward_new_sizes(cellname, cell, dtype, tol, H, xmode):
    ops_t.test_rnn_forward(cellname, cell, dtype, tol, xmode, H, RAGGED_B[H])


@pytest.mark.parametrize("cellname,cell", ops_t.CELLS)
@pytest.mark.parametrize("dtype,tol", ops_t.DTYPES)
@pytest.mark.parametrize("H", NEW_H)
@pytest.mark.parametrize("ext", [True, False])
def test_rnn_backward_new_sizes(cellname, cell, dtype, tol, H, ext):
    ops_t._rnn_backward_case(cellname, cell, dtype, tol, H, RAGGED_B[H] if ext else 16, ext, T=8)


@pytest.mark.parametrize("cellname,cell", ops_t.CELLS)
@pytest.mark.parametrize("dtype,tol", ops_t.DTYPES)
@pytest.mark.parametrize("xmode", ["dense", "index"])
@pytest.mark.parametrize("H,B", par.SAT_WIDE_SHAPES)
def test_rnn_forward_saturated_new_sizes(cellname, cell, dtype, tol, xmode, H, B):
    """clipped gates and the planted +-60 rows (tests/parity.py rnn_saturated_problem) at the wide generic kernels"""
    ops_t._rnn_forward_saturated_case(cellname, cell, dtype, tol, xmode, H, B, par.SAT_T_FWD)


@pytest.mark.parametrize("cellname,cell", ops_t.CELLS)
@pytest.mark.parametrize("dtype,tol", ops_t.DTYPES)
@pytest.mark.parametrize("H,B", par.SAT_WIDE_SHAPES)
@pytest.mark.parametrize("ext", [True, False])
def test_rnn_backward_saturated_new_sizes(cellname, cell, dtype, tol, H, B, ext):
    ops_t._rnn_backward_case(cellname, cell, dtype, tol, H, B, ext, T=par.SAT_T_BWD, saturated=True)


# ---- engine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H", [384, 512])
def test_engine_forward_backward_matches_oracle(cell, dtype, H):
    B = 7
    spec, params, batch, raw = _problem(cell, B, seed=B, H=H)
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    m_o, cache = orc.forward(p64, batch, raw["eps"].astype(np.float64))
    g_o = orc.backward(p64, cache)
    eng = Engine(spec, max_batch=32, dtype=dtype, seed=0)
    eng.set_params(params)
    _stage(eng, raw, B)
    eng.forward_backward(B)
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
def test_three_adam_steps_h512_match_oracle_f32(cell):
    B = 16
    spec, params, batch, raw = _problem(cell, B, seed=3, H=512)
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


def _model_run(monkeypatch, tmp_path, plans, cell):
    """VAE.create(lstm_size=512) at the reference's default heads and latent width: fit three epochs of a small song, evaluate,
    encode, decode (probabilities and the fused argmax), save and reload the weights"""
    monkeypatch.setenv("MVAE_PLANS", plans)
    s = build_settings(cell_type=cell, lstm_size=512, input_length=4, output_length=4, batch_size=8, learning_rate=1e-3)
    m = VAE().create(compute_dtype="f32", seed=0, **create_kwargs(s))
    n = 20
    w = make_windows(n, s["output_length"], s["output_dim"], s["max_voices"], 16, s["num_classes"], s["latent_dim"], seed=5)
    X, Y, C, I, V, D = to_reference_format(w)
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
    out["decoded"] = m.decoder.predict(dec_in, batch_size=s["batch_size"])[0]
    idx = m.decoder.predict_note_indices(dec_in, batch_size=s["batch_size"])
    Yd = pk.process_decoder_outputs(s, m.decoder.predict(dec_in, batch_size=s["batch_size"]), "argmax")[0]
    assert np.array_equal(pk.notes_from_indices(s, idx, 61), Yd)
    path = str(tmp_path / ("w_%s.npz" % plans))
    m.autoencoder.save_weights(path)
    m2 = VAE().create(compute_dtype="f32", seed=1, **create_kwargs(s))
    m2.autoencoder.load_weights(path)
    for a, b in zip(m.autoencoder.get_weights(), m2.autoencoder.get_weights()):
        assert np.array_equal(a, b)
    m2._shared.rng = np.random.default_rng(0)
    out["z_reloaded"] = m2.encoder.predict(pk.prepare_encoder_input_list(s, X, I, V, D), batch_size=s["batch_size"], verbose=False)
    stats = dict(m._shared.engine.plan_stats)
    return m, s, (X, Y, C, I, V, Hh), out, stats


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_vae_h512_fit_evaluate_decode_with_and_without_plans(cell, monkeypatch, tmp_path):
    m, s, (X, Y, C, I, V, Hh), on, stats_on = _model_run(monkeypatch, tmp_path, "1", cell)
    assert stats_on["recorded"] >= 1 and stats_on["replayed"] >= 1, stats_on
    # the fitted epochs against the oracle's Adam trajectory (same init, minibatches and epsilon stream)
    spec = m.spec
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
    np.testing.assert_allclose(on["z_reloaded"], on["z"], rtol=0, atol=0)
    del m
    torch.cuda.synchronize()
    _, _, _, off, stats_off = _model_run(monkeypatch, tmp_path, "0", cell)
    assert stats_off["replayed"] == 0, stats_off
    np.testing.assert_allclose(off["loss"], on["loss"], rtol=3e-5, atol=3e-6)
    np.testing.assert_allclose(off["evaluate"], on["evaluate"], rtol=3e-5, atol=3e-6)
    for k in ("z", "decoded", "z_reloaded"):
        assert np.linalg.norm(off[k] - on[k]) <= 1e-3 * np.linalg.norm(on[k]) + 1e-5, (k, np.linalg.norm(off[k] - on[k]))


# ---- style classifier ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xmode,K,T", [("index", 61, 12), ("scalar", 1, 12)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_classifier_h512_matches_oracle(xmode, K, T, dtype):
    B = 21
    spec, params, x, X, c, Y = _cls_problem(xmode, B, T, K, 3, 512, 2, seed=4)
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


def test_style_classifier_h512_fit_and_evaluate():
    rng = np.random.default_rng(2)
    n, T = 24, 16
    X = np.eye(61)[rng.integers(0, 61, (n, T))]
    Y = np.eye(2)[rng.integers(0, 2, n)]
    clf = StyleClassifier(kind="pitch", input_dim=61, num_classes=2, lstm_size=512, learning_rate=1e-3, compute_dtype="f32")
    before = clf.evaluate(X, Y, batch_size=8)
    hist = clf.fit(X, Y, epochs=2, batch_size=8)
    after = clf.evaluate(X, Y, batch_size=8)
    assert len(hist.history["loss"]) == 2 and np.all(np.isfinite(hist.history["loss"])) and np.all(np.isfinite(after))
    assert after[0] != before[0]                                   # the fit moved the 2 x GRU(512) weights
