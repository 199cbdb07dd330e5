"""'choice' decode on the device (csrc/sample.hip, Engine.decode(sample=...), decoder.predict_note_indices / predict_indices).

Kernel level, on small-integer hs / W / bias (logits exact in f32 and bf16, the project's practice for GEMM parity):
  * DESIGNED uniforms - the midpoint of a float64 CDF bin at least 1e-3 wide - must give exactly that bin on every row;
  * GENERATED uniforms (Philox in the kernel) must give what the NumPy mirror gives (midi_vae_amd/sampling.py), except on rows
    whose uniform lies within delta = (2N + 16) 2^-23 of a float64 CDF boundary; those rows are named by the oracle alone and
    their share is capped at 3 % (the seeds meet the cap on the mirror: tests/test_choice_decode_cpu.py);
  * the counts of 65536 draws from one row stay within 6 sigma + 1 of the float64 probabilities.
Model level: the public calls against the float64 CDF of the device's OWN probabilities (decoder.predict) with designed
uniforms, chunking / batch-size / seed behaviour, the untouched argmax default and plan replay.
"""
import functools

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops, sampling
from midi_vae_amd import packers as pk
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE
from test_choice_decode_cpu import (DISTRIBUTION_SEED, GENERATED_CASES, distribution_row, excluded_rows, integer_problem)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {hl.F32: torch.float32, hl.BF16: torch.bfloat16}
MIN_BIN = 1e-3


def dev(a, td=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(td)


@functools.lru_cache(maxsize=None)
def problem(R, H, N):
    """hs, W, bias, float64 logits - computed once per shape, shared by every case that uses it (never modified)"""
    out = integer_problem(R, H, N, seed=1000 * N + H)
    for a in out:
        a.setflags(write=False)
    return out


def designed(cdf, seed):
    """per row: a bin of the normalised float64 CDF at least MIN_BIN wide (drawn among those) and the f32 uniform at its middle"""
    rng = np.random.default_rng(seed)
    lo = np.concatenate([np.zeros((cdf.shape[0], 1)), cdf[:, :-1]], axis=1)
    ok = (cdf - lo) >= MIN_BIN
    assert ok.any(axis=1).all()
    score = np.where(ok, rng.random(cdf.shape), -1.0)
    k = np.argmax(score, axis=1)
    rows = np.arange(cdf.shape[0])
    u = (0.5 * (lo[rows, k] + cdf[rows, k])).astype(np.float32)
    assert np.all(u < 1)
    return k, u


def run_sampler(dtype, hs, W, bias, N, **kw):
    R, H = hs.shape
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=TD[dtype], device=DEV)
    ops.transpose_convert(dev(W), wt, n_pad=NP)
    out = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    u = kw.pop("uniforms", None)
    ud = None
    if u is not None:
        ud = dev(np.asarray(u, np.float32).reshape(R, -1))
        kw["u_stride"] = ud.shape[1]
    ops.head_sample(dtype, R, H, N, dev(hs, TD[dtype]), wt, dev(bias), out, uniforms=ud, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- kernel, designed uniforms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 16, 17, 61, 129, 145, 192])
def test_designed_uniforms_give_their_bin_on_every_row(N, dtype):
    for H in (64, 256):
        for R in (1, 37, 4100):
            hs, W, bias, logits = problem(R, H, N)
            for tau in (0.5, 1.0, 2.0):
                k, u = designed(sampling.cdf_bins(logits, tau, from_logits=True), seed=R + N)
                got = run_sampler(dtype, hs, W, bias, N, uniforms=u, temperature=tau)
                bad = np.nonzero(got != k)[0]
                assert bad.size == 0, (H, R, tau, bad[:8], got[bad[:8]], k[bad[:8]])


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16], ids=["f32", "bf16"])
def test_more_rows_than_one_pass_of_the_grid(dtype):
    """the launch caps its grid (1024 workgroups of 64 rows; 512 of 128 where a wave holds two row tiles: bf16 up to 4 column
    tiles), so one pass covers 65536 / 131072 rows and a 4 M-row decode walks the rest in the kernel's row loop: 131172 rows take
    three passes in f32 and a second, partial one in bf16 - designed uniforms, every row exact"""
    N, H, R = 61, 64, 2 * 65536 + 100
    hs, W, bias, logits = problem(R, H, N)
    k, u = designed(sampling.cdf_bins(logits, 1.0, from_logits=True), seed=9)
    got = run_sampler(dtype, hs, W, bias, N, uniforms=u)
    bad = np.nonzero(got != k)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], k[bad[:8]])
    # generated uniforms depend on the row alone: the tail of the long launch equals a launch of its own at that row offset
    gen = run_sampler(dtype, hs, W, bias, N, seed=5, T=4)
    tail = run_sampler(dtype, hs[131072:], W, bias, N, seed=5, T=4, row0=131072)
    assert np.array_equal(gen[131072:], tail) and len(np.unique(gen)) > 10


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16], ids=["f32", "bf16"])
def test_padded_batch_and_sliced_launch_equal_the_unsliced_one(dtype):
    """time-major rows with pad windows (b_stride 48, 40 real): a launch over rows [r0, r1) with row0 = r0 gives the bytes of the
    launch over all rows - with supplied uniforms (the slice of the array) and with generated ones (the global row decides)"""
    N, H, T, Bp, Bv = 61, 64, 12, 48, 40
    R = T * Bp
    hs, W, bias, logits = problem(R, H, N)
    k, u = designed(sampling.cdf_bins(logits, 1.0, from_logits=True), seed=3)
    valid = (np.arange(R) % Bp) < Bv
    geo = dict(b_stride=Bp, b_valid=Bv, T=T)
    whole = run_sampler(dtype, hs, W, bias, N, uniforms=u, **geo)
    assert np.array_equal(whole[valid], k[valid])
    gen = run_sampler(dtype, hs, W, bias, N, seed=99, window0=7, head_id=2, **geo)
    # the generated uniforms of the valid rows are the mirror's, in the caller's (window, t) order
    um = sampling.uniforms(99, 2, Bv, T, 1, first_window=7)[:, :, 0]                  # (window, t)
    lg = logits.reshape(T, Bp, N)[:, :Bv].transpose(1, 0, 2).reshape(-1, N)       # caller order
    want = sampling.choice_index_rows(lg, um.reshape(-1), 1.0, from_logits=True)
    ex = excluded_rows(sampling.cdf_bins(lg, 1.0, from_logits=True), um.reshape(-1), N)
    got = gen.reshape(T, Bp)[:, :Bv].T.reshape(-1)
    assert ex.mean() <= 0.03 and np.array_equal(got[~ex], want[~ex])
    r0, r1 = 5 * Bp, 9 * Bp + 16          # (a slice that ends inside a time step)
    part = run_sampler(dtype, hs[r0:r1], W, bias, N, uniforms=u[r0:r1], row0=r0, **geo)
    assert np.array_equal(part[valid[r0:r1]], whole[r0:r1][valid[r0:r1]])
    part = run_sampler(dtype, hs[r0:r1], W, bias, N, seed=99, window0=7, head_id=2, row0=r0, **geo)
    assert np.array_equal(part, gen[r0:r1])


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16], ids=["f32", "bf16"])
def test_cold_temperature_is_the_heads_argmax(dtype):
    """temperature 1/64 on rows whose two largest logits are >= 1 apart: the draw is the first-maximum index mvae_head writes"""
    N, H, R = 61, 64, 4100
    hs, W, bias, logits = problem(R, H, N)
    srt = np.sort(logits, axis=1)
    rows = (srt[:, -1] - srt[:, -2]) >= 1
    assert rows.sum() > R // 4
    rng = np.random.default_rng(4)
    u = np.maximum(rng.random(R).astype(np.float32), np.float32(2.0 ** -24))
    u = np.minimum(u, np.float32(1 - 2.0 ** -24))
    got = run_sampler(dtype, hs, W, bias, N, uniforms=u, temperature=1.0 / 64)
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=TD[dtype], device=DEV)
    ops.transpose_convert(dev(W), wt, n_pad=NP)
    am = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    ops.head(0, dtype, R, H, N, dev(hs, TD[dtype]), wt, dev(bias), argmax=am)
    torch.cuda.synchronize()
    am = am.cpu().numpy()
    assert np.array_equal(am[rows], np.argmax(logits, axis=1)[rows])
    assert np.array_equal(got[rows], am[rows])


def test_tries_and_cutoff_on_the_device():
    """two supplied uniforms per row: a first draw whose probability is below the cutoff is replaced by the second; when both
    are below, the second is kept - the mirror's rule, on designed uniforms (both in the middle of a bin)"""
    N, H, R = 61, 64, 700
    hs, W, bias, logits = problem(R, H, N)
    cdf = sampling.cdf_bins(logits, 1.0, from_logits=True)
    k1, u1 = designed(cdf, seed=5)
    k2, u2 = designed(cdf, seed=6)
    q = np.diff(np.concatenate([np.zeros((R, 1)), cdf], axis=1), axis=1)
    cutoff = 0.05
    p1, p2 = q[np.arange(R), k1], q[np.arange(R), k2]
    clear = (np.abs(p1 - cutoff) > 1e-4) & (np.abs(p2 - cutoff) > 1e-4)          # (the comparison itself is not at its edge)
    want = np.where(p1 > cutoff, k1, k2)
    assert (p1 <= cutoff).sum() > 20 and ((p1 <= cutoff) & (p2 <= cutoff)).sum() > 5 and (p1 > cutoff).sum() > 20
    u = np.stack([u1, u2], axis=1)
    assert np.array_equal(sampling.choice_index_rows(logits, u, 1.0, tries=2, cutoff=cutoff, from_logits=True), want)
    got = run_sampler(hl.F32, hs, W, bias, N, uniforms=u, tries=2, cutoff=cutoff)
    assert np.array_equal(got[clear], want[clear])
    got1 = run_sampler(hl.F32, hs, W, bias, N, uniforms=u, tries=1, cutoff=cutoff)
    assert np.array_equal(got1, k1)


# ---- kernel, generated uniforms ---------------------------------------------------------------------------------------------

def _time_major(rows_caller, n, T, Bp):
    """(n * T, ...) rows in the caller's (window, t) order -> (T * Bp, ...) device rows, pad windows zero"""
    a = rows_caller.reshape((n, T) + rows_caller.shape[1:])
    out = np.zeros((T, Bp) + a.shape[2:], a.dtype)
    out[:, :n] = np.swapaxes(a, 0, 1)
    return out.reshape((T * Bp,) + a.shape[2:])


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,R,H,seed,head,window0", GENERATED_CASES)
def test_generated_uniforms_match_the_mirror(N, R, H, seed, head, window0, dtype):
    T, n = 4, R // 4
    Bp = (n + 15) // 16 * 16
    hs, W, bias, logits = integer_problem(n * T, H, N, seed=N)
    hs_tm = _time_major(hs, n, T, Bp)
    for tau in (0.5, 1.0, 2.0):
        u = sampling.uniforms(seed, head, n, T, 1, first_window=window0).reshape(-1)
        want = sampling.choice_index_rows(logits, u, tau, from_logits=True)
        ex = excluded_rows(sampling.cdf_bins(logits, tau, from_logits=True), u, N)
        assert ex.mean() <= 0.03
        got = run_sampler(dtype, hs_tm, W, bias, N, seed=seed, window0=window0, head_id=head, temperature=tau, b_stride=Bp, b_valid=n, T=T)
        got = got.reshape(T, Bp)[:, :n].T.reshape(-1)
        bad = np.nonzero((got != want) & ~ex)[0]
        assert bad.size == 0, (tau, bad[:8], got[bad[:8]], want[bad[:8]])
        if tau == 1.0:
            # the same windows as two launches with the matching window offsets: the same bytes
            n1 = n // 3
            a = run_sampler(dtype, _time_major(hs[:n1 * T], n1, T, Bp), W, bias, N, seed=seed, window0=window0, head_id=head,
                            b_stride=Bp, b_valid=n1, T=T).reshape(T, Bp)[:, :n1].T.reshape(-1)
            b = run_sampler(dtype, _time_major(hs[n1 * T:], n - n1, T, Bp), W, bias, N, seed=seed, window0=window0 + n1, head_id=head,
                            b_stride=Bp, b_valid=n - n1, T=T).reshape(T, Bp)[:, :n - n1].T.reshape(-1)
            assert np.array_equal(np.concatenate([a, b]), got)


def test_control_block_in_device_memory_equals_host_values():
    N, H, R = 61, 64, 700
    hs, W, bias, _ = problem(R, H, N)
    want = run_sampler(hl.F32, hs, W, bias, N, seed=(3 << 32) + 11, window0=5, head_id=1, temperature=0.5, T=4)
    ctl = torch.from_numpy(sampling.control_words((3 << 32) + 11, 5, 0.5, 0.0, 1)).to(DEV)
    got = run_sampler(hl.F32, hs, W, bias, N, ctl=ctl, head_id=1, T=4, temperature=123.0, seed=1)      # (the host values are not read)
    assert np.array_equal(got, want)


def test_distribution_of_generated_draws():
    R, N, H = 65536, 61, 64
    lg = distribution_row()
    hs = np.zeros((R, H), np.float32)
    hs[:, 0] = 1
    W = np.zeros((H, N), np.float32)
    W[0] = lg
    got = run_sampler(hl.F32, hs, W, np.zeros(N, np.float32), N, seed=DISTRIBUTION_SEED, head_id=0, T=16)
    e, S = sampling.tempered(lg[None], 1.0, from_logits=True)
    q = e[0] / S[0]
    cnt = np.bincount(got, minlength=N)
    assert cnt.sum() == R and np.all(np.abs(cnt - R * q) <= 6 * np.sqrt(R * q * (1 - q)) + 1), (cnt, R * q)


# ---- model ----------------------------------------------------------------------------------------------------------------

def _model(cell, dtype, seed=0, **over):
    s = build_settings(cell_type=cell, lstm_size=64, latent_dim=32, input_length=4, output_length=4, batch_size=8, **over)
    m = VAE().create(compute_dtype=dtype, seed=seed, **create_kwargs(s))
    m.decoder.sample_settings = s
    return s, m


def _dec_in(s, n, seed=1):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, s["latent_dim"])) * 2.0
    return pk.prepare_decoder_input(s, z, 0, np.zeros((n, s["signature_vector_length"])), None)


def _designed_for(P, tau, seed):
    P = np.asarray(P, np.float64)
    k, u = designed(sampling.cdf_bins(P.reshape(-1, P.shape[-1]), tau), seed)
    return k.reshape(P.shape[:-1]), u.reshape(P.shape[:-1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
@pytest.mark.parametrize("n", [8, 40])
def test_model_designed_uniforms_against_the_devices_own_probabilities(cell, dtype, n):
    s, m = _model(cell, dtype)
    dec_in = _dec_in(s, n)
    outs = m.decoder.predict(dec_in, batch_size=8)
    before = m.decoder.predict_note_indices(dec_in, 8)
    assert np.array_equal(before, pk.note_indices(s, outs[0], "argmax").reshape(n, -1))
    for tau in (1.0, 0.5):
        k, u = _designed_for(outs[0], tau, seed=n)
        got = m.decoder.predict_note_indices(dec_in, batch_size=8, sample_method="choice", temperature=tau, uniforms=u)
        assert got.dtype == np.uint8 and got.shape == k.shape and np.array_equal(got, k)
    # the default call is what it was, after a 'choice' call too
    after = m.decoder.predict_note_indices(dec_in, 8)
    assert np.array_equal(after, before)


@pytest.mark.parametrize("over", [dict(meta_held_notes=True, meta_next_notes=True), dict(high_crop=128, low_crop=0)], ids=["all-heads", "wide"])
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_predict_indices_every_softmax_head(cell, over):
    s, m = _model(cell, "f32", **over)
    n = 8
    dec_in = _dec_in(s, n)
    outs = m.decoder.predict(dec_in, batch_size=8)
    names = m._shared.head_names()
    assert s["output_dim"] == (129 if "high_crop" in over else 61)
    ks, us = {}, {}
    for name, P in zip(names, outs):
        if name != "vel":
            ks[name], us[name] = _designed_for(P, 1.0, seed=len(name))
    got = m.decoder.predict_indices(dec_in, batch_size=8, sample_method="choice", uniforms=us)
    assert set(got) == set(ks) | ({"velocity"} if "vel" in names else set())
    for name in ks:
        assert got[name].dtype == np.uint8 and np.array_equal(got[name], ks[name]), name
    if "vel" in names:
        assert got["velocity"].dtype == np.float32 and np.array_equal(got["velocity"], outs[names.index("vel")][:, :, 0])
    # argmax through the same call, and the host decode from indices alone
    am = m.decoder.predict_indices(dec_in, batch_size=8)
    for name, P in zip(names, outs):
        if name != "vel":
            assert np.array_equal(am[name], np.argmax(P, axis=-1)), name
    want = pk.process_decoder_outputs(s, outs, "argmax")
    for g, w in zip(pk.process_decoder_indices(s, am), want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_seeded_results_do_not_depend_on_chunking_or_batch_size(cell, monkeypatch):
    n = 40
    s, m = _model(cell, "bf16")
    dec_in = _dec_in(s, n)
    whole = m.decoder.predict_indices(dec_in, batch_size=8, sample_method="choice", seed=1234)
    again = m.decoder.predict_indices(dec_in, batch_size=32, sample_method="choice", seed=1234)
    other = m.decoder.predict_indices(dec_in, batch_size=8, sample_method="choice", seed=1235)
    for name in whole:
        assert np.array_equal(whole[name], again[name]), name
    assert not np.array_equal(whole["notes"], other["notes"])
    # the mirror's uniforms on the device's own probabilities: the same draws (rows at a CDF boundary aside)
    P = np.asarray(m.decoder.predict(dec_in, batch_size=8)[0], np.float64)
    u = sampling.uniforms(1234, sampling.HEAD_IDS["notes"], n, P.shape[1], 1)[:, :, 0]
    want = sampling.choice_index_rows(P, u, s["temperature"])
    near = (np.abs(sampling.cdf_bins(P.reshape(-1, P.shape[-1]), s["temperature"]) - u.reshape(-1, 1).astype(np.float64)) <= 5e-4).any(axis=1)
    assert near.mean() < 0.1 and np.array_equal(whole["notes"].reshape(-1)[~near], want.reshape(-1)[~near])
    # a model whose forward-only engine holds 16 windows decodes the 40 in three engine batches: the same bytes
    monkeypatch.setenv("MVAE_INFER_BATCH", "16")
    s2, m2 = _model(cell, "bf16")
    assert m2._shared.infer_cap == 16
    chunked = m2.decoder.predict_indices(dec_in, batch_size=8, sample_method="choice", seed=1234)
    assert m2._shared.infer.maxB == 16
    for name in whole:
        assert np.array_equal(whole[name], chunked[name]), name
    # seed=None: the model's own key stream - two calls differ, and the epsilon stream is not touched
    state = repr(m._shared.rng.bit_generator.state)
    a = m.decoder.predict_note_indices(dec_in, 8, sample_method="choice")
    b = m.decoder.predict_note_indices(dec_in, 8, sample_method="choice")
    assert not np.array_equal(a, b) and repr(m._shared.rng.bit_generator.state) == state


def test_a_choice_decode_with_another_seed_is_replayed():
    s, m = _model("LSTM", "bf16")
    dec_in = _dec_in(s, 24)
    # (the first call also prepares the weights - a plan key of its own; three recordings of the steady call arm its plan)
    res = [m.decoder.predict_note_indices(dec_in, 8, sample_method="choice", seed=i) for i in range(5)]
    eng = m._shared.infer
    rep, rec = eng.plan_stats["replayed"], eng.plan_stats["recorded"]
    assert eng.plan_stats["refused"] == {}, eng.plan_stats
    res += [m.decoder.predict_note_indices(dec_in, 8, sample_method="choice", seed=i) for i in (5, 0)]
    assert eng.plan_stats["replayed"] == rep + 2 and eng.plan_stats["recorded"] == rec, eng.plan_stats
    assert np.array_equal(res[6], res[0]) and not np.array_equal(res[5], res[0])
    # the argmax decode has plans of its own: recorded now, untouched by the sample mode
    am = m.decoder.predict_note_indices(dec_in, 8)
    assert eng.plan_stats["recorded"] == rec + 1
    assert np.array_equal(am, pk.note_indices(s, m.decoder.predict(dec_in, 8)[0], "argmax").reshape(24, -1))
