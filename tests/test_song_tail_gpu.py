"""The one tail of the song decodes (song_decodes.finish_rolls) on the device: the velocity roll mvae_recon_songs writes without a song
structure is bit for bit what mvae_sweep_windows writes - switch_styles moved from the one to the other - and the one real difference
between switch_styles and predict_songs, what stands in for a velocity head the model lacks, stays."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import reconstruction as rec
from midi_vae_amd import sweep as sw
from tests import song_tail_contract as stc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def on_device(a, layout):
    """the (n, T) device view of a host roll: contiguous, or of a time-major (T, Bp) buffer whose pad columns hold what nobody may read"""
    if layout == "window-major":
        return torch.from_numpy(a).to(DEV)
    n, T = a.shape
    Bp = -(-n // 16) * 16 + 16
    t = torch.full((T, Bp), 7 if a.dtype == np.uint8 else float("nan"), dtype=torch.from_numpy(a).dtype, device=DEV)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)
    return t[:, :n].t()


@pytest.mark.parametrize("override", [True, False], ids=["rules_on", "rules_off"])
@pytest.mark.parametrize("layout", ["window-major", "time-major"])
@pytest.mark.parametrize("n,T,V", stc.SHAPES, ids=lambda x: str(x))
def test_sweep_and_recon_kernels_write_the_same_velocities(n, T, V, layout, override):
    """mvae_sweep_windows with stats_out = NULL against mvae_recon_songs with first_window = NULL, and both against the mirror"""
    s = stc.settings(V, override)
    idx, vel, _ = stc.planted_rolls(n, T, V)
    idx_d, vel_d = on_device(idx, layout), on_device(vel, layout)
    assert idx_d.shape == (n, T) and idx_d.stride() == vel_d.stride()
    stream = torch.cuda.current_stream().cuda_stream
    of_sweep = torch.full((n, T), -7.0, dtype=torch.float32, device=DEV)
    of_recon = torch.full((n, T), -9.0, dtype=torch.float32, device=DEV)
    starts = torch.empty((n, T), dtype=torch.uint8, device=DEV)
    counts = torch.empty((n, rec.N_COUNTS), dtype=torch.int32, device=DEV)
    sw.enqueue(idx_d, vel_d, sw.params(s), None, of_sweep, stream)
    rec.enqueue(idx_d, vel_d, None, None, None, rec.params(s), None, of_recon, starts, counts, stream)
    of_sweep, of_recon = of_sweep.cpu().numpy(), of_recon.cpu().numpy()
    assert np.array_equal(of_sweep.view(np.uint32), of_recon.view(np.uint32))
    want = rec._mirror(idx, vel, None, None, np.arange(n), rec.params(s))
    assert np.array_equal(of_recon.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(starts.cpu().numpy(), want[1])          # (the NaN row: no note start)


# ---- a model without the velocity head -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def headless():
    """the tiny VAE of test_style_scores_gpu.py (GRU, H = 64, Z = 16, T = 16, 4 voices, 3 style classes, songs of 2, 5 and 3
    windows) with the instrument head and WITHOUT the velocity head"""
    from midi_vae_amd.config import build_settings, create_kwargs
    from midi_vae_amd.model import VAE
    s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=16, input_length=4, output_length=4, max_voices=4, batch_size=8,
                       classes=("a", "b", "c"), meta_velocity=False)
    m = VAE().create(compute_dtype="f32", seed=8, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z, m.spec.C) == (16, 4, 16, 3) and not m.spec.meta_velocity and m.spec.meta_instrument
    assert not m.spec.meta_held
    rng = np.random.default_rng(88)
    zs = [rng.standard_normal((m_i, 16)) * 2.0 for m_i in (2, 5, 3)]
    return s, m, zs, [2, 0, 1]


def test_without_the_velocity_head_the_two_decodes_keep_their_own_stand_in(headless):
    """switch_styles: velocity 80 on every note and the default velocity reported from the host; predict_songs: the notes carry the
    velocity of the default-filled roll the reconstruction returned"""
    from midi_vae_amd import packers as pk
    from midi_vae_amd import style as st
    s, m, zs, classes = headless
    dec, T, bs = m.decoder, 16, 8
    thr = s["velocity_threshold_such_that_it_is_a_played_note"]
    got = dec.switch_styles(zs, classes, note_events=True, batch_size=bs)
    pairs = st.switch_pairs(classes, 3)
    assert [(d["song"], d["C"], d["C_switch"]) for d in got["pairs"]] == pairs and len(pairs) == 6
    switched_records = []
    for d, (song, _, _) in zip(got["pairs"], pairs):
        m_k = zs[song].shape[0]
        assert "starts" not in d and "counts" not in d
        assert d["velocity"].dtype == np.float32 and d["velocity"].shape == (m_k, T)
        assert np.array_equal(d["velocity"].view(np.uint32), np.full((m_k, T), thr + (1 - thr) * 0.5, np.float32).view(np.uint32))
        want = ev.note_events(d["notes"], None, np.ones((m_k, T), np.uint8), [m_k], s, device=False)[0]
        assert np.array_equal(d["events"], want)
        switched_records.append(d["events"])
    switched_records = np.concatenate(switched_records)
    assert len(switched_records) and np.all(switched_records["velocity"] == ev.DEFAULT_VELOCITY)

    xs = [pk.prepare_decoder_input(s, z, C, np.zeros((z.shape[0], s["signature_vector_length"])), None) for z, C in zip(zs, classes)]
    songs = dec.predict_songs(xs, batch_size=bs, note_events=True)
    song_records = []
    for d, z in zip(songs, zs):
        m_i = z.shape[0]
        filled = np.full((m_i, T), rec.default_velocity(rec.params(s)), np.float32)
        assert np.array_equal(d["velocity"].view(np.uint32), filled.view(np.uint32)) and np.all(d["starts"] == 1)
        want = ev.note_events(d["notes"], filled, np.ones((m_i, T), np.uint8), [m_i], s, device=False)[0]
        assert np.array_equal(d["events"], want)
        song_records.append(d["events"])
    song_records = np.concatenate(song_records)
    assert len(song_records) and np.all(song_records["velocity"] != ev.DEFAULT_VELOCITY)
    assert set(song_records["velocity"].tolist()).isdisjoint(switched_records["velocity"].tolist())
