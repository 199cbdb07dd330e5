"""Window descriptors without a device: the NumPy mirror and the ``data_class`` shim against the reference's own outputs
(tests/golden/descriptors.npz, written by tests/golden/make_descriptor_fixtures.py), the second header's hygiene, the refusals of
mvae_desc_windows as a table (tests/descriptor_contract.py), and the normalisation of ``vae_training.py --signatures``.

Bounds (derived, not measured).  With ``_np_std`` the mirror takes max / min / mean / std through the same NumPy calls on the same
lists in the same order as the reference: all 15 entries bit-equal.  In its default form the three stds come from exact integer
sums, sqrt((c * sum(x^2) - sum(x)^2) / c^2): values <= 127, at most T terms, every double rounding 1.1e-16 relative - under 1e-13
from NumPy's two-pass form; the bound is 1e-12 absolute, the other twelve entries stay bit-equal (exact sums, the same one or two
divisions).  Harmonicity: values <= 3, fewer than 100 roundings between the two evaluation orders: 1e-12 absolute, NaN in the same
places."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import descriptors as de
from midi_vae_amd import hiplib as hl
from midi_vae_amd import rolls
from tests import descriptor_contract as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD_COLUMNS = [6, 10, 14]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "descriptors.npz"))
    s = {k[2:]: z[k].item() for k in z.files if k.startswith("s_")}
    return dict(s=s, idx=z["idx"], signature=z["signature"], harmonicity=z["harmonicity"], generator=z["generator"])


# ---- the mirror against the reference ----------------------------------------------------------------------------------------
def test_fixture_is_the_shipped_shape(fx):
    assert fx["idx"].shape == (258, 64) and fx["idx"].dtype == np.uint8
    assert fx["s"] == dict(max_voices=4, low_crop=24, high_crop=84, include_silent_note=True, SMALLEST_NOTE=16)
    assert de.params(fx["s"]) == dict(voices=4, n_pitch=60, silent=60, low_crop=24, resolution=4)


def test_mirror_signature_is_the_reference_bit_for_bit(fx):
    got = de.signature_vectors(fx["idx"], fx["s"], device=False, _np_std=True)
    assert got.shape == (258, 15) and got.dtype == np.float64
    bad = np.argwhere(got != fx["signature"])
    assert bad.size == 0, "first difference at window %d entry %d: %r vs %r" % (
        bad[0][0], bad[0][1], got[tuple(bad[0])], fx["signature"][tuple(bad[0])])


def test_mirror_signature_from_integer_sums(fx):
    """the form the device computes: twelve entries bit-equal, the stds within 1e-12"""
    got = de.signature_vectors(fx["idx"], fx["s"], device=False)
    rest = [c for c in range(15) if c not in STD_COLUMNS]
    assert np.array_equal(got[:, rest], fx["signature"][:, rest])
    err = np.abs(got[:, STD_COLUMNS] - fx["signature"][:, STD_COLUMNS]).max()
    print("largest std difference, integer sums against np.std: %.3g" % err)
    assert err <= 1e-12


def test_mirror_harmonicity_is_the_reference(fx):
    got = de.harmonicity(fx["idx"], fx["s"], device=False)
    want = fx["harmonicity"]
    assert got.shape == (258, 4, 4)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = np.nanmax(np.abs(got - want))
    print("largest harmonicity difference: %.3g" % err)
    assert err <= 1e-12
    assert np.all(got[:, np.arange(4), np.arange(4)] == 0) and np.array_equal(got, got.transpose(0, 2, 1), equal_nan=True)


def test_fixture_exercises_the_quirks(fx):
    """the skipped deletion changes at least a quarter of the windows, a useful share of the harmonicity entries is NaN, the
    unequal-set case occurs, and the two hand-made windows give what their description says"""
    tidy = de.signature_vectors(fx["idx"], fx["s"], device=False, _tidy=True, _np_std=True)
    assert np.mean(np.any(tidy != fx["signature"], axis=1)) >= 0.25
    off = ~np.eye(4, dtype=bool)
    share = np.isnan(fx["harmonicity"][:, off]).mean()
    assert 0.05 <= share <= 0.60, share
    on = rolls.sounding(fx["idx"], de.params(fx["s"])).reshape(258, 16, 4)
    counts = np.array([[len(set(fx["idx"][w].reshape(16, 4)[k][on[w, k]])) for k in range(16)] for w in range(258)])
    assert np.any((counts[:, 1:] != counts[:, :-1]) & (counts[:, 1:] > 0) & (counts[:, :-1] > 0))
    assert np.all(fx["signature"][256] == 0) and np.all(np.isnan(fx["harmonicity"][256][off]))
    single = fx["signature"][257]
    assert single[0] == 1 / 16 and single[1] == 1 / 16 and single[2] == 0 and single[3] == single[4] == single[5] == 55 / 127
    assert single[6] == 0 and np.all(single[7:11] == 0) and list(single[11:]) == [1, 1, 1, 0]


def test_inputs_one_hot_rolls_and_wide_indices(fx):
    idx = fx["idx"][:9]
    onehot = np.eye(61)[idx]
    assert np.array_equal(de.signature_vectors(onehot, fx["s"], device=False), de.signature_vectors(idx, fx["s"], device=False))
    assert np.array_equal(de.harmonicity(idx.astype(np.int64), fx["s"], device=False), de.harmonicity(idx, fx["s"], device=False),
                          equal_nan=True)
    with pytest.raises(ValueError):
        de.signature_vectors(idx[:, :63], fx["s"], device=False)
    with pytest.raises(ValueError):
        de.harmonicity(idx, dict(fx["s"], high_crop=85), device=False)
    song = de.song_harmonicity(fx["idx"][:64], fx["s"], device=False)
    assert song.shape == (4, 4) and np.allclose(song, np.nanmean(fx["harmonicity"][:64], axis=0), atol=1e-12, rtol=0)


def test_tonal_matrix():
    tm = de.tonal_matrix()
    assert tm.shape == (6, 12) and tm.dtype == np.float32
    k = np.arange(12)
    assert np.array_equal(tm[0], np.sin(k * (7. / 6.) * np.pi).astype(np.float32))
    assert np.array_equal(tm[5], (0.5 * np.cos(k * (2. / 3.) * np.pi)).astype(np.float32))
    assert np.allclose(np.hypot(tm[0], tm[1]), 1) and np.allclose(np.hypot(tm[4], tm[5]), 0.5)


# ---- the data_class shim through the reference's call shapes ---------------------------------------------------------------------
def test_data_class_shim_against_the_fixture(fx):
    import data_class
    import settings
    assert (settings.max_voices, settings.low_crop, settings.high_crop, settings.include_silent_note) == (4, 24, 84, True)
    rolls = np.eye(61)[fx["idx"]]
    for w in list(range(0, 256, 9)) + [256, 257]:
        sig = data_class.signature_form_unrolled_pianoroll(rolls[w], 4, True)
        assert isinstance(sig, list) and len(sig) == 15 and np.array_equal(np.asarray(sig, np.float64), fx["signature"][w]), w
        khot = data_class.monophonic_to_khot_pianoroll(rolls[w], 4)[:, :-1]
        assert np.array_equal(np.asarray(data_class.signature_from_pianoroll(khot), np.float64), fx["signature"][w])
        h = data_class.get_harmonicity_scores_for_each_track_combination(rolls[w][:, :60])
        assert np.array_equal(np.isnan(h), np.isnan(fx["harmonicity"][w]))
        assert np.all(np.abs(h - fx["harmonicity"][w])[~np.isnan(h)] <= 1e-12)
    stack = data_class.get_harmonicity_scores_for_each_track_combination(rolls[:64, :, :60])
    assert np.allclose(stack, np.nanmean(fx["harmonicity"][:64], axis=0), atol=1e-12, rtol=0)
    assert np.array_equal(data_class.get_tonal_matrix(), de.tonal_matrix())


def test_mahalanobis_helpers():
    import data_class
    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((40, 5)) @ rng.standard_normal((5, 5))
    vecs[:, 4] = vecs[:, 0] + vecs[:, 1]          # a singular covariance: the pseudo-inverse still gives a distance
    mean, cov = data_class.get_mean_and_cov_from_vector_list(vecs)
    assert np.allclose(mean, vecs.mean(0)) and np.allclose(cov, np.cov(vecs.T))
    d = data_class.mahalanobis_distance(vecs[0], mean, cov)
    diff = vecs[0] - mean
    assert np.isfinite(d) and np.isclose(d, np.sqrt(diff @ np.linalg.pinv(cov) @ diff))
    assert data_class.mahalanobis_distance(mean, mean, cov) == 0


# ---- the second header ----------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_descriptors.h")
    assert declared == {"mvae_desc_abi_version", "mvae_desc_windows"} == set(hl.DESC_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert name not in hl.SIGNATURES and name not in _declared("midivae_hip.h")
    assert lib.mvae_desc_abi_version() == 1 == hl.DESC_ABI_VERSION
    assert lib.mvae_abi_version() == hl.ABI_VERSION


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_descriptors.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_desc_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_desc_args, %s));' % (f, f) for f, _ in hl.DescArgs._fields_]
    lines += ['printf("MVAE_DESC_SIGNATURE_LENGTH %d\\n", (int)MVAE_DESC_SIGNATURE_LENGTH);', 'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.DescArgs) and ctypes.sizeof(hl.DescArgs) % 8 == 0
    for f, _ in hl.DescArgs._fields_:
        assert int(got[f]) == getattr(hl.DescArgs, f).offset, f
    assert int(got["MVAE_DESC_SIGNATURE_LENGTH"]) == de.SIGNATURE_LENGTH


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_descriptors_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert dc.invoke(lib, dc.baseline(dc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in dc.ACCEPTED:
        assert dc.invoke(lib, mutate(dc.baseline(dc.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("row", dc.ROWS, ids=[r[0] for r in dc.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = dc.invoke(hl.load(), mutate(dc.baseline(dc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_covers_every_documented_limit():
    names = " | ".join(r[0] for r in dc.ROWS)
    for what in ("a NULL", "idx NULL", "both outputs NULL", "n = 0", "T = 0", "voices = 0", "resolution = 0", "voices = 1", "voices = 9",
                 "T % voices", "n_pitch = 193", "n_pitch % 12", "tonal NULL", "ld_sig = 14"):
        assert what in names, what
    assert {r[0] for r in dc.ROWS if r[3]} == {"both outputs NULL", "voices = 1", "T % voices != 0 (T = 62)", "ld_sig = 14"}


# ---- vae_training --signatures -----------------------------------------------------------------------------------------------------
def test_training_signatures_are_normalised_with_the_training_statistics(default_settings):
    import vae_training
    s = default_settings
    train, test = vae_training.synthetic_songs(3, s, seed=1), vae_training.synthetic_songs(1, s, seed=999)
    assert all(not song["S"].any() for song in train + test)          # 'zeros': what the songs come with
    raw = [de.signature_vectors(song["Y"], s, device=False) for song in train + test]
    mean, std = vae_training.attach_signatures(train, test, s, "host")
    seen = np.concatenate(raw[:3], 0)
    assert np.array_equal(mean, seen.mean(0)) and np.all(std > 0)
    assert np.array_equal(std == 1e-10, seen.std(0) == 0)
    for song, r in zip(train + test, raw):
        assert song["S"].shape == (song["X"].shape[0], s["signature_vector_length"]) == r.shape
        assert np.array_equal(song["S"], (r - mean) / std)
    S = np.concatenate([song["S"] for song in train], 0)
    live = seen.std(0) > 0
    assert live.sum() >= 10 and np.allclose(S[:, live].mean(0), 0, atol=1e-9) and np.allclose(S[:, live].std(0), 1, atol=1e-9)
    assert np.all(S[:, ~live] == 0)
    assert np.abs(test[0]["S"][:, live].mean(0)).max() > 1e-6          # the test song is measured with the TRAINING statistics
