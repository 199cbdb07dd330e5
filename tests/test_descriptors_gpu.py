"""Window descriptors on the device (csrc/descriptors.hip, mvae_desc_windows) against the NumPy mirror of midi_vae_amd.descriptors -
which tests/test_descriptors_cpu.py pins to the reference's own outputs - and against those outputs themselves.

Bounds (derived, not measured; the same as in test_descriptors_cpu.py).  Counts, ratios, max, min and mean are exact integer sums
and the same one or two double divisions on both sides: BIT-EQUAL.  The three stds: both sides take sqrt((c * sum(x^2) - sum(x)^2)
/ c^2) from exact integers, the reference the two-pass form; values <= 127, at most T terms, 1.1e-16 per rounding: 1e-12 absolute.
Harmonicity: values <= 3, fewer than 100 roundings separate sum-of-columns / count (device) from tonal . (chroma / sum) (mirror):
1e-12 absolute, NaN in exactly the same places.  Two layouts of the same windows run the same arithmetic per lane: bit-equal."""
import itertools
import os

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import descriptors as de
from midi_vae_amd import hiplib as hl
from midi_vae_amd import packers as pk
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE
from tests import descriptor_contract as dc
from tests import footprint as fp
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD_COLUMNS = [6, 10, 14]
EXACT_COLUMNS = [c for c in range(15) if c not in STD_COLUMNS]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "descriptors.npz"))
    s = {k[2:]: z[k].item() for k in z.files if k.startswith("s_")}
    idx = z["idx"]
    return dict(s=s, idx=idx, signature=z["signature"], harmonicity=z["harmonicity"],
                mirror_sig=de.signature_vectors(idx, s, device=False), mirror_harm=de.harmonicity(idx, s, device=False))


def _assert_signature(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    bad = np.argwhere(got[:, EXACT_COLUMNS] != want[:, EXACT_COLUMNS])
    assert bad.size == 0, "%s: %d entries differ, first window %d entry %d: %r vs %r" % (
        what, len(bad), bad[0][0], EXACT_COLUMNS[bad[0][1]], got[bad[0][0], EXACT_COLUMNS[bad[0][1]]], want[bad[0][0], EXACT_COLUMNS[bad[0][1]]])
    err = np.abs(got[:, STD_COLUMNS] - want[:, STD_COLUMNS]).max()
    print("%s: largest std difference %.3g" % (what, err))
    assert err <= 1e-12, what


def _assert_harmonicity(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN in other places (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(want).sum())
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
    print("%s: largest harmonicity difference %.3g" % (what, err))
    assert err <= 1e-12, what
    V = want.shape[1]
    assert np.all(got[:, np.arange(V), np.arange(V)] == 0) and np.array_equal(got, got.transpose(0, 2, 1), equal_nan=True), what


def _walks(rng, n, T, V, n_pitch, p_silent, p_hold):
    """voice-wise random walks: steps of -4..4 columns, a rest with p_silent, else the last note again with p_hold"""
    ticks = T // V
    rest, hold = rng.random((n, ticks, V)) < p_silent, rng.random((n, ticks, V)) < p_hold
    step = np.where(hold, 0, rng.integers(-4, 5, (n, ticks, V)))
    step[rest] = 0
    q = np.clip(rng.integers(0, n_pitch, (n, 1, V)) + np.cumsum(step, 1), 0, n_pitch - 1)
    return np.where(rest, n_pitch, q).astype(np.uint8).reshape(n, T)


# ---- every window of 3 ticks x 2 voices over four pitches and silence ---------------------------------------------------------------
@pytest.mark.parametrize("n_pitch,columns", [(12, (0, 1, 5, 7)), (24, (0, 1, 10, 15))], ids=["12 columns", "24 columns"])
def test_exhaustive_smallest_windows(n_pitch, columns):
    """5^6 = 15 625 windows in one launch, resolution 1 (three segments): the skipped deletion, unequal note sets with ties, the
    doubled pitch, the flush on silence and empty segments all occur.  On 12 columns every column is a chroma bin of its own; on 24
    (two columns a bin) columns 0 and 1 share a bin, 10 and 15 do not - the smallest roll on which two pitches can share one."""
    alphabet = np.array(columns + (n_pitch,), np.uint8)
    idx = alphabet[np.array(list(itertools.product(range(5), repeat=6)))]
    assert idx.shape == (15625, 6)
    s = dict(max_voices=2, low_crop=24, high_crop=24 + n_pitch, include_silent_note=True, SMALLEST_NOTE=4)
    assert de.params(s)["resolution"] == 1
    _assert_signature(de.signature_vectors(idx, s), de.signature_vectors(idx, s, device=False), "exhaustive signature")
    want = de.harmonicity(idx, s, device=False)
    nan = np.isnan(want[:, 0, 1])
    assert nan.any() and not nan.all() and np.any(want[:, 0, 1] == 0) and np.any(want[:, 0, 1] > 0.5)
    _assert_harmonicity(de.harmonicity(idx, s), want, "exhaustive harmonicity")
    tidy = de.signature_vectors(idx, s, device=False, _tidy=True)
    assert np.any(tidy != de.signature_vectors(idx, s, device=False)), "no window exercises the skipped deletion"


# ---- the reference's windows ---------------------------------------------------------------------------------------------------
def test_fixture_windows_window_major(fx):
    sig, harm = de.signature_vectors(fx["idx"], fx["s"]), de.harmonicity(fx["idx"], fx["s"])
    _assert_signature(sig, fx["signature"], "device against the reference")
    _assert_harmonicity(harm, fx["harmonicity"], "device against the reference")
    _assert_signature(sig, fx["mirror_sig"], "device against the mirror")
    _assert_harmonicity(harm, fx["mirror_harm"], "device against the mirror")
    onehot = np.eye(61)[fx["idx"][:40]]
    assert np.array_equal(de.signature_vectors(onehot, fx["s"]), sig[:40])
    dev = torch.from_numpy(fx["idx"]).to(DEV)
    assert np.array_equal(de.signature_vectors(dev, fx["s"]), sig)
    assert np.array_equal(de.harmonicity(dev.t().contiguous().t(), fx["s"]), harm, equal_nan=True)       # a strided view: time-major memory
    assert np.array_equal(de.song_harmonicity(fx["idx"], fx["s"]), de.nanmean_windows(harm), equal_nan=True)


def _f64(buf):
    """the float64 reading of a buffer carved as pairs of 32-bit words (the arena has no 64-bit element type)"""
    return np.ascontiguousarray(buf.bits()).view(np.uint64).view(np.float64)


def test_fixture_windows_time_major_padded(fx):
    """17 windows in a (T, 32) buffer as the engine keeps them: bit-equal to the window-major run, rows 17..31 of both outputs and
    every guard untouched"""
    B, Bp, T, V = 17, 32, 64, 4
    p = de.params(fx["s"])
    pick = np.r_[0:4, 64:68, 128:132, 192:195, 256:258]
    idx = fx["idx"][pick]
    tm = np.random.default_rng(7).integers(0, 61, (T, Bp)).astype(np.uint8)          # (valid notes in the pad columns)
    tm[:, :B] = idx.T
    ar = fp.Arena(DEV)
    b_idx = ar.carve("idx", (T, Bp), torch.uint8, data=tm, guard="zero")
    b_ton = ar.carve("tonal", (6, 12), torch.float32, data=torch.from_numpy(de.tonal_matrix()))
    b_sig = ar.carve("sig", (Bp, 30), torch.float32)
    b_harm = ar.carve("harm", (Bp, 2 * V * V), torch.float32)
    ar.commit()
    sig, harm = b_sig.t.view(torch.float64), b_harm.t.view(torch.float64)
    assert sig.shape == (Bp, 15) and harm.shape == (Bp, V * V) and sig.data_ptr() == b_sig.t.data_ptr()
    de.enqueue(b_idx.t[:, :B].t(), p, sig, harm, b_ton.t, torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    for b in (b_sig, b_harm):
        ar.assert_written(b, np.s_[:B])
        ar.assert_untouched(b, np.s_[B:])
    assert np.array_equal(b_idx.bits(), tm)
    want_sig, want_harm = de.signature_vectors(idx, fx["s"]), de.harmonicity(idx, fx["s"])
    got_sig, got_harm = _f64(b_sig)[:B], _f64(b_harm)[:B].reshape(B, V, V)
    assert np.array_equal(got_sig.view(np.uint64), want_sig.view(np.uint64)), "signature: time-major differs from window-major"
    assert np.array_equal(got_harm.view(np.uint64), want_harm.view(np.uint64)), "harmonicity: time-major differs from window-major"
    _assert_signature(got_sig, fx["signature"][pick], "time-major against the reference")
    _assert_harmonicity(got_harm, fx["harmonicity"][pick], "time-major against the reference")


# ---- more than one wave, more than one chunk of ticks ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_windows(fx):
    rng = np.random.default_rng(512)
    base = np.concatenate([_walks(rng, 11, 512, 4, 60, ps, ph) for ps, ph in ((0.35, 0.0), (0.3, 0.6), (0.2, 0.8))], 0)
    idx = np.concatenate([base, np.roll(base[:32], 4, axis=1)], 0)          # 33 walks, 32 of them again one tick later
    assert idx.shape == (65, 512)
    return idx, de.signature_vectors(idx, fx["s"], device=False), de.harmonicity(idx, fx["s"], device=False)


@pytest.mark.parametrize("n", [1, 65])
def test_across_a_wave_and_a_chunk(fx, long_windows, n):
    """T = 512 (128 ticks: eight chunks of the staged path), 65 windows (a second, one-lane workgroup) and a single window"""
    idx, want_sig, want_harm = long_windows
    _assert_signature(de.signature_vectors(idx[:n], fx["s"]), want_sig[:n], "T = 512 window-major")
    _assert_harmonicity(de.harmonicity(idx[:n], fx["s"]), want_harm[:n], "T = 512 window-major")
    tm = torch.from_numpy(np.ascontiguousarray(idx[:n].T)).to(DEV)            # (T, n) time-major memory, seen as (n, T)
    _assert_signature(de.signature_vectors(tm.t(), fx["s"]), want_sig[:n], "T = 512 time-major")
    _assert_harmonicity(de.harmonicity(tm.t(), fx["s"]), want_harm[:n], "T = 512 time-major")


# ---- the decode ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=32, input_length=8, output_length=8, max_voices=2, batch_size=8)
    m = VAE().create(compute_dtype="f32", seed=4, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V) == (16, 2)
    z = np.random.default_rng(24).standard_normal((24, s["latent_dim"])) * 2.0
    return s, m, pk.prepare_decoder_input(s, z, 0, np.zeros((24, s["signature_vector_length"])), None)


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_predict_descriptors(small_model, method, kw):
    s, m, dec_in = small_model
    notes = m.decoder.predict_note_indices(dec_in, 8, sample_method=method, **kw)
    got = m.decoder.predict_descriptors(dec_in, 8, sample_method=method, **kw)
    assert sorted(got) == ["harmonicity", "notes", "signature"]
    assert got["notes"].dtype == np.uint8 and np.array_equal(got["notes"], notes)
    assert got["signature"].shape == (24, 15) and got["harmonicity"].shape == (24, 2, 2)
    _assert_signature(got["signature"], de.signature_vectors(notes, s, device=False), "predict_descriptors (%s)" % method)
    _assert_harmonicity(got["harmonicity"], de.harmonicity(notes, s, device=False), "predict_descriptors (%s)" % method)
    assert np.array_equal(m.decoder.predict_note_indices(dec_in, 8, sample_method=method, **kw), notes)      # the decode itself is as it was


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing(fx):
    """the safe rows of tests/descriptor_contract.py on real buffers: the promised code, and every byte of the arena - the rolls, the
    sentinel-filled outputs, the guards - as planted; the baseline itself then runs inside its buffers"""
    ar, bufs = fp.Arena(DEV), {}

    def carve(name, shape, kind, out=False):
        if kind == "f64":
            bufs[name] = ar.carve(name, (shape[0], 2 * shape[1]), torch.float32)
        elif kind == "u8":
            bufs[name] = ar.carve(name, shape, torch.uint8, data=fx["idx"][:shape[0]], guard="zero")
        else:
            bufs[name] = ar.carve(name, shape, torch.float32, data=torch.from_numpy(de.tonal_matrix()))
        return 0x1000

    dc.baseline(carve)
    ar.commit()
    resolve = lambda name, shape, kind, out=False: bufs[name].t.data_ptr()
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in dc.ROWS if r[3]]
    assert len(safe) >= 4
    for name, mutate, code, _ in safe:
        rc = dc.invoke(lib, mutate(dc.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert dc.invoke(lib, dc.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(bufs["sig"])
    ar.assert_written(bufs["harm"])
    _assert_signature(_f64(bufs["sig"]), fx["signature"][:dc.N], "baseline")
    _assert_harmonicity(_f64(bufs["harm"]).reshape(dc.N, dc.V, dc.V), fx["harmonicity"][:dc.N], "baseline")
