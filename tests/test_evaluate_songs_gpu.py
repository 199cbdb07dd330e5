"""autoencoder.evaluate_windows / evaluate_songs (GPU box only): per-window losses summed on the device, many songs as one
chip-filling pass.

Models: (a) GRU, f32, H = 64, Z = 16, T = 8, V = 4, C = 2 with the instrument, velocity and style heads - and a variant that adds
the held-notes head, the next-notes head and the classifier on the notes output; (b) LSTM, bf16, H = 256, T = 32, the default
graph: the resident recurrent kernels.  Songs of 1, 17 and 40 windows for (a), 3 and 20 for (b); batch_size = 16, so the longer
songs span Keras batches (epsilon is drawn per batch); epsilon_std = 1.

  - evaluate_songs on one model equals the loop of evaluate on a second model built from the same seed: accuracy columns exactly,
    loss columns within n_addends x 2^-23 relative - both sides are f32 sums of the same positive addends in another order
    (n_addends: the song's windows x the steps of the heads behind the column);
  - evaluate_windows rows equal the oracle's forward pass on one-window batches with the same epsilon rows, to the bounds the suite
    holds evaluate to: 2e-4 (1 + |want|) in f32 (test_model_gpu.py), 3e-2 (1 + |want|) on the losses in bf16 (the accuracies of a
    bf16 run are not compared with the float64 oracle: a near-tie may round the other way);
  - evaluate before and after gives what it gave, a second evaluate_songs repeats the first: the step plans stay apart - decisive
    for the one-window song, where both steps are normalised by one window and only ``per_window`` tells their plan keys apart;
  - signature_decoder=True raises NotImplementedError, a DeviceLatent history raises TypeError."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import packers as pk
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.layout import init_params
from midi_vae_amd.model import VAE
from midi_vae_amd.synth import make_windows, to_reference_format
from oracle.vae_oracle import OracleVAE, make_cfg

pytestmark = pytest.mark.gpu

BS = 16
MODELS = {
    "a": (dict(cell_type="GRU", lstm_size=64, latent_dim=16, input_length=2, output_length=2), "f32", (1, 17, 40)),
    "a+": (dict(cell_type="GRU", lstm_size=64, latent_dim=16, input_length=2, output_length=2, meta_held_notes=True,
                meta_next_notes=True, composer_decoder_at_notes_output=True), "f32", (1, 17, 40)),
    "b": (dict(cell_type="LSTM", lstm_size=256, input_length=8, output_length=8), "bf16", (3, 20)),
}


def _settings(key, **over):
    kw, dtype, lengths = MODELS[key]
    return build_settings(batch_size=BS, epsilon_std=1.0, **dict(kw, **over)), dtype, lengths


def _model(s, dtype, seed=4):
    return VAE().create(compute_dtype=dtype, seed=seed, **create_kwargs(s))


def _songs(s, lengths, seed=30):
    """(xs, ys): the reference's lists of every song; songs differ in windows, instruments, style class and history"""
    xs, ys = [], []
    rng = np.random.default_rng(seed)
    for i, n in enumerate(lengths):
        raw = n + int(bool(s["meta_next_notes"]))            # (the next-notes head drops the last window of a song)
        w = make_windows(raw, s["output_length"], s["output_dim"], s["max_voices"], 16, s["num_classes"], s["latent_dim"], seed=seed + i)
        X, Y, _, I, V, D = to_reference_format(w)
        D = (rng.random(D.shape) < 0.4).astype(np.float64)
        H = rng.standard_normal((raw, s["latent_dim"])) * 0.1
        S = np.zeros((raw, s["signature_vector_length"]))
        x, y = pk.prepare_autoencoder_input_and_output_list(s, X, Y, i % s["num_classes"], I, V, D, S, H)
        assert x[0].shape[0] == n
        if n == 1:          # (the reference's list builder squeezes the one-hot style rows of a one-window song to a vector)
            y = [np.asarray(a).reshape(1, -1) if np.ndim(a) == 1 else a for a in y]
        xs.append(x)
        ys.append(y)
    return xs, ys


def _steps(m):
    """engine metric name -> addends per window behind it"""
    sp = m.spec
    st = dict(notes=sp.T, instr=sp.V, vel=sp.T, held=sp.T, next=sp.T, style=1, cnotes=1, cinstr=1)
    cols = m.autoencoder._metric_columns()
    heads = {c.rsplit("_", 1)[0] for c in cols if c != "loss"}
    st["loss"] = sum(st[h] for h in heads) + 1               # (every head's rows and the KL term)
    return cols, st


def _reseed(*models, seed=11):
    for m in models:
        m._shared.rng = np.random.default_rng(seed)


def _assert_songs_equal_loop(m, got, want, lengths):
    cols, st = _steps(m)
    for n, g, w in zip(lengths, got, want):
        assert len(g) == len(w) == len(cols) == len(m.autoencoder.metrics_names)
        for c, a, b in zip(cols, g, w):
            if c.endswith("_acc"):
                assert a == b, (n, c, a, b)
            else:
                head = c if c == "loss" else c.rsplit("_", 1)[0]
                tol = n * st[head] * 2.0 ** -23
                print("song of %d windows, %s: %.9g vs %.9g, %.3g of the bound" % (n, c, a, b, abs(a - b) / (tol * abs(b))))
                assert abs(a - b) <= tol * abs(b), (n, c, a, b, tol)


@pytest.mark.parametrize("key", list(MODELS))
def test_evaluate_songs_equals_the_loop_of_evaluate(key):
    s, dtype, lengths = _settings(key)
    m1, m2 = _model(s, dtype), _model(s, dtype)
    xs, ys = _songs(s, lengths)
    _reseed(m1, m2)
    got = m1.autoencoder.evaluate_songs(xs, ys, batch_size=BS)
    want = [m2.autoencoder.evaluate(x, y, batch_size=BS, verbose=False) for x, y in zip(xs, ys)]
    _assert_songs_equal_loop(m1, got, want, lengths)
    # both consumed the same number of draws: the next one is the same on both
    assert np.array_equal(m1._shared.epsilon(3), m2._shared.epsilon(3))


def _oracle_batch(s, x, y):
    i = 2 + int(bool(s["history"]))
    b = dict(X=x[0], Hist=x[2], I=x[i + 1], Vel=x[i + 3], Y=y[0])
    k = 3
    if s["meta_held_notes"]:
        b["Held"] = x[i + 5]
        k += 1
    if s["meta_next_notes"]:
        b["Next"] = y[k]
        k += 1
    b["C"] = y[k]
    return b


@pytest.mark.parametrize("key,song", [("a", 1), ("a+", 1), ("b", 0)])
def test_evaluate_windows_equals_the_oracle_on_one_window_batches(key, song):
    s, dtype, lengths = _settings(key)
    m = _model(s, dtype)
    xs, ys = _songs(s, lengths)
    x, y, n = xs[song], ys[song], lengths[song]
    _reseed(m, seed=12)
    rows = m.autoencoder.evaluate_windows(x, y, batch_size=BS)
    cols = m.autoencoder._metric_columns()
    assert rows.shape == (n, len(m.autoencoder.metrics_names)) and rows.dtype == np.float64
    spec = m.spec
    eps = (np.random.default_rng(12).standard_normal((n, spec.Z)) * spec.epsilon_std).astype(np.float32).astype(np.float64)
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    p = {k: v.astype(np.float64) for k, v in init_params(spec, 4).items()}
    b = _oracle_batch(s, x, y)
    tol = 2e-4 if dtype == "f32" else 3e-2
    for i in range(n):
        mo, _ = orc.forward(p, {k: v[i:i + 1] for k, v in b.items()}, eps[i:i + 1])
        for j, c in enumerate(cols):
            if dtype != "f32" and c.endswith("_acc"):
                continue
            assert abs(rows[i, j] - mo[c]) <= tol * (1 + abs(mo[c])), (i, c, rows[i, j], mo[c])
    # and the song's metrics are the means of its windows' rows
    _reseed(m, seed=12)
    song_vals = m.autoencoder.evaluate_songs([x], [y], batch_size=BS)[0]
    np.testing.assert_allclose(song_vals, rows.mean(0), rtol=1e-6, atol=0)


def test_evaluate_and_per_window_plans_stay_apart():
    """evaluate, evaluate_songs and evaluate_windows alternate until every step plan is armed and replayed (three recordings arm a
    plan): each call repeats its first result.  The one-window song is normalised by one window in both modes."""
    s, dtype, lengths = _settings("a")
    m = _model(s, dtype)
    xs, ys = _songs(s, lengths)
    first = {}
    for rnd in range(5):
        for name, call in (("evaluate 1", lambda: m.autoencoder.evaluate(xs[0], ys[0], batch_size=BS, verbose=False)),
                           ("windows 1", lambda: m.autoencoder.evaluate_windows(xs[0], ys[0], batch_size=BS)[0]),
                           ("evaluate 17", lambda: m.autoencoder.evaluate(xs[1], ys[1], batch_size=BS, verbose=False)),
                           ("songs", lambda: np.concatenate(m.autoencoder.evaluate_songs(xs, ys, batch_size=BS)))):
            _reseed(m, seed=13)
            got = np.asarray(call(), np.float64)
            assert np.all(np.isfinite(got))
            if rnd == 0:
                first[name] = got
            else:       # (the sums are f32 atomics: equal to the last bits, not bit for bit)
                np.testing.assert_allclose(got, first[name], rtol=2e-6, atol=0, err_msg="%s, round %d" % (name, rnd))
    np.testing.assert_allclose(first["windows 1"], first["evaluate 1"], rtol=2e-6, atol=0)       # (one window: the same numbers)
    stats = m._shared.infer.plan_stats
    assert stats["replayed"] > 0, stats


def test_refusals_signature_head_and_device_history():
    s, dtype, lengths = _settings("a", signature_decoder=True, latent_dim=32)        # (the signature columns need room)
    m = _model(s, dtype)
    xs, ys = _songs(s, (3,))
    with pytest.raises(NotImplementedError, match="signature_decoder"):
        m.autoencoder.evaluate_songs(xs, ys, batch_size=BS)
    with pytest.raises(NotImplementedError, match="signature_decoder"):
        m.autoencoder.evaluate_windows(xs[0], ys[0], batch_size=BS)
    with pytest.raises(NotImplementedError, match="signature_decoder"):
        eng = m._shared.get_infer(16)
        eng.eval_step(3, per_window=True)
    s, dtype, lengths = _settings("a")
    m = _model(s, dtype)
    n = 5
    w = make_windows(n, s["output_length"], s["output_dim"], s["max_voices"], 16, s["num_classes"], s["latent_dim"], seed=3)
    X, Y, C, I, V, D = to_reference_format(w)
    lat = m.encoder.predict(pk.prepare_encoder_input_list(s, X, I, V, D), batch_size=BS, verbose=False, device=True)
    x, y = pk.prepare_autoencoder_input_and_output_list(s, X, Y, C, I, V, D, np.zeros((n, s["signature_vector_length"])), lat)
    with pytest.raises(TypeError, match="host array"):
        m.autoencoder.evaluate_songs([x], [y], batch_size=BS)
    with pytest.raises(TypeError, match="host array"):
        m.autoencoder.evaluate_windows(x, y, batch_size=BS)
