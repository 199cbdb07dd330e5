"""decoder.latent_sweep: the statistics kernel behind the decode against the host route - predict_indices on the same decoder inputs,
then the NumPy mirror and the host summaries of midi_vae_amd.sweep (tests/test_sweep_stats_cpu.py pins both to the reference).

The device reads the very bytes predict_indices brings to the host, so the table obeys the split of test_sweep_stats_gpu.py: the stds
within 1e-12, everything else bit-equal; the summaries are host functions of the table latent_sweep returns and must be EQUAL to
those functions applied to it."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import sweep as sw
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE
from tests.sweep_contract import assert_table

pytestmark = pytest.mark.gpu
N, PER_DIM = 2, 3


@pytest.fixture(scope="module")
def small_model():
    """the small model of test_descriptors_gpu.py; its forward-only engine holds 128 windows, so the 320 of the sweep take three
    engine batches"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MVAE_INFER_BATCH", "128")
        s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=32, input_length=8, output_length=8, max_voices=2, batch_size=8)
        m = VAE().create(compute_dtype="f32", seed=4, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z) == (16, 2, 32) and m._shared.infer_cap == 128
    assert s["meta_velocity"] and s["meta_instrument"] and s["instrument_attach_method"] == "1hot-category"
    z = np.random.default_rng(24).standard_normal((N, 32)) * 2.0
    return s, m, z


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_latent_sweep(small_model, method, kw):
    s, m, z = small_model
    dec = m.decoder
    values = sw.sweep_values(1.0, 1.0, PER_DIM, True)
    K, Z, T, V = len(values), 32, 16, 2
    assert K == 5
    dec_in = dec.sweep_inputs(z, values, s)
    assert dec_in[1].shape == (N * Z * K, Z)
    grid = dec_in[1].reshape(N, Z, K, Z)
    assert np.array_equal(grid[1, 7, :, 7], values) and np.array_equal(grid[1, 7, 2, np.arange(Z) != 7], z[1, np.arange(Z) != 7])
    notes_before = dec.predict_note_indices(dec_in, 8, sample_method=method, **kw)

    got = dec.latent_sweep(z, evaluations_per_dimension=PER_DIM, batch_size=8, sample_method=method, **kw)
    assert m._shared.infer.maxB == 128          # three engine batches
    assert sorted(got) == ["influence", "most_peaked", "overall_best", "programs", "summaries", "table", "values"]
    assert got["table"].shape == (N, Z, K, 22) and got["programs"].shape == (N, Z, K, V) and np.array_equal(got["values"], values)

    # the host route on the same decoder inputs
    host = dec.predict_indices(dec_in, 8, sample_method=method, **kw)
    assert np.array_equal(host["notes"], notes_before)
    want = sw.window_statistics(host["notes"], host["velocity"], s, device=False)
    print("windows with a pitch: %.0f %%, with a note start: %.0f %%" % (100 * (want[:, 0] > 0).mean(), 100 * (want[:, 9] > 0).mean()))
    assert (want[:, 0] > 0).any(), "the model decodes nothing to take statistics of"
    assert_table(got["table"].reshape(-1, 22), want, "latent_sweep (%s) against the mirror" % method)
    assert np.array_equal(got["programs"].reshape(-1, V), host["instr"].astype(np.int64) * 8)

    # the summaries: the host functions on that table
    summaries, infl, peaked, best = sw.summarize_sweep(got["table"], got["programs"])
    assert len(got["summaries"]) == N and len(got["summaries"][0]) == Z
    for i in range(N):
        for d in range(Z):
            a, b = got["summaries"][i][d], summaries[i][d]
            assert set(a) == set(b) and all(_same(a[k][0], b[k][0]) and _same(a[k][1], b[k][1]) for k in a), (i, d)
            assert "total_change_of_instruments" in a
    assert set(got["influence"]) == set(infl) and got["most_peaked"] == peaked and got["overall_best"] == best
    for key in infl:
        assert got["influence"][key].shape == (Z,) and np.array_equal(got["influence"][key], infl[key], equal_nan=True), key

    # a second call replays the recorded decode: the same result; the rolls ride along on request; the decode is as it was
    again = dec.latent_sweep(z, evaluations_per_dimension=PER_DIM, batch_size=8, sample_method=method, return_rolls=True, **kw)
    assert np.array_equal(again["table"], got["table"], equal_nan=True) and np.array_equal(again["programs"], got["programs"])
    assert again["most_peaked"] == got["most_peaked"] and again["overall_best"] == got["overall_best"]
    assert np.array_equal(again["notes"].reshape(-1, T), host["notes"])
    rules = sw.window_statistics(host["notes"], host["velocity"], s, device=False, return_velocity=True)[1]
    assert np.array_equal(again["velocity"].reshape(-1, T).view(np.uint32), rules.view(np.uint32))
    assert np.array_equal(dec.predict_note_indices(dec_in, 8, sample_method=method, **kw), notes_before)


def test_latent_sweep_refuses_what_it_cannot_do(small_model):
    s, m, z = small_model
    with pytest.raises(ValueError):
        m.decoder.latent_sweep(z[:, :31])
    m.decoder.sample_settings = dict(s, max_voices=4)
    try:
        with pytest.raises(ValueError):
            m.decoder.latent_sweep(z)
    finally:
        m.decoder.sample_settings = s
