"""The six public decodes of model.Decoder go through one loop (Decoder._run) and one sink each (midi_vae_amd.decode_sinks), and every
sink reads the same time-major device views (Engine.decoded): the same windows must come out of all of them.

Everything compared here is a copy of the same bytes of the same decode - indices, instrument bytes - or, for the velocities, the
NumPy mirror's input floats and zeros (tests/test_sweep_stats_cpu.py pins it): EQUAL, no tolerance.  300 windows on an engine of 128
are two full engine batches and a ragged third of 44 - no multiple of 16, so the padded columns of the views are in play - and the
songs of 1, 5, 130, 60 and 104 windows straddle both batch edges."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import decode_sinks as sinks
from midi_vae_amd import packers
from midi_vae_amd import sweep as sw
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE

pytestmark = pytest.mark.gpu
LENGTHS = [1, 5, 130, 60, 104]
N, T, V = 300, 16, 2


@pytest.fixture(scope="module")
def small_model():
    """the small model of test_latent_sweep_gpu.py; its forward-only engine holds 128 windows"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MVAE_INFER_BATCH", "128")
        s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=32, input_length=8, output_length=8, max_voices=2, batch_size=8)
        m = VAE().create(compute_dtype="f32", seed=4, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z) == (T, V, 32) and m._shared.infer_cap == 128 and sum(LENGTHS) == N
    assert s["meta_velocity"] and s["meta_instrument"]
    rng = np.random.default_rng(31)
    xs = [packers.prepare_decoder_input(s, rng.standard_normal((n, 32)) * 2.0, 0, np.zeros((n, s["signature_vector_length"])), None)
          for n in LENGTHS]
    x_all = [np.concatenate([x[k] for x in xs], 0) for k in range(len(xs[0]))]
    return s, m, xs, x_all


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_every_path_decodes_the_same_windows(small_model, method, kw):
    s, m, xs, x_all = small_model
    dec = m.decoder
    notes = dec.predict_note_indices(x_all, 8, sample_method=method, **kw)
    assert m._shared.infer.maxB == 128          # two full engine batches and one of 44
    assert notes.shape == (N, T) and notes.dtype == np.uint8

    indices = dec.predict_indices(x_all, 8, sample_method=method, **kw)
    assert sorted(indices) == ["instr", "notes", "velocity"] and np.array_equal(indices["notes"], notes)
    assert indices["instr"].shape == (N, V) and indices["velocity"].shape == (N, T) and indices["velocity"].dtype == np.float32

    described = dec.predict_descriptors(x_all, 8, sample_method=method, **kw)
    assert np.array_equal(described["notes"], notes) and described["signature"].shape == (N, 15)

    sample = dec._sample_spec(N, method, None, kw.get("seed"), None, dec._softmax_heads())
    swept = dec._run(x_all, 8, sinks.SweepStatistics(p=sw.params(s), T=T, return_rolls=True), sample)
    assert sorted(swept) == ["instr", "notes", "table", "velocity"] and swept["table"].shape == (N, 22)
    assert np.array_equal(swept["notes"], notes) and np.array_equal(swept["instr"], indices["instr"])
    rules = sw.window_statistics(indices["notes"], indices["velocity"], s, device=False, return_velocity=True)[1]
    assert swept["velocity"].dtype == np.float32 and np.array_equal(swept["velocity"].view(np.uint32), rules.view(np.uint32))

    songs = dec.predict_songs(xs, 8, sample_method=method, **kw)
    assert [len(d["notes"]) for d in songs] == LENGTHS
    assert np.array_equal(np.concatenate([d["notes"] for d in songs], 0), notes)
    assert np.array_equal(np.concatenate([d["instr"] for d in songs], 0), indices["instr"])
    assert (notes != s["high_crop"] - s["low_crop"]).any(), "the model decodes no note: the comparison shows little"


def test_no_windows(small_model):
    s, m, xs, x_all = small_model
    dec = m.decoder
    none = [a[:0] for a in x_all]
    notes = dec.predict_note_indices(none, 8)
    assert notes.shape == (0, T) and notes.dtype == np.uint8
    described = dec.predict_descriptors(none, 8)
    assert sorted(described) == ["harmonicity", "notes", "signature"]
    assert described["notes"].shape == (0, T) and described["notes"].dtype == np.uint8
    assert described["signature"].shape == (0, 15) and described["harmonicity"].shape == (0, V, V)
    assert dec.predict_songs([]) == []
    assert dec.predict_indices(none, 8) == {}
