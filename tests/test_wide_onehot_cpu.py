"""One-hot rows up to 192 columns (the full MIDI range: 128 pitches + the silent column + 16 instrument categories; inputs up to
255 with the composer columns) through the settings surface, the head kernel's padded width and the host packers (no GPU)."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import packers as pk
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.layout import spec_from_create_kwargs
from midi_vae_amd.staging import host_onehot_to_index, host_onehot_to_index_tm


def test_full_midi_range_is_accepted():
    spec = spec_from_create_kwargs(create_kwargs(build_settings(high_crop=128, low_crop=0)))
    assert spec.Din == 129 and spec.Dout == 129


def test_full_midi_range_with_instrument_and_composer_columns_is_accepted():
    """129 + 16 instrument-category columns (+ 2 composer columns on the input): 147 / 145.  (The create call of the reference carries
    no attach_dim; VAE.create(attach_dim=16) selects the two-hot rows, which need input_dim == output_dim - no composer columns -
    whatever the width: the case below.)"""
    s = build_settings(high_crop=128, low_crop=0, attach_instruments=True, include_composer_feature=True)
    assert s["instrument_dim"] == 16
    spec = spec_from_create_kwargs(create_kwargs(s))
    assert (spec.Din, spec.Dout) == (147, 145)


def test_full_midi_range_two_hot_rows_are_accepted():
    s = build_settings(high_crop=128, low_crop=0, attach_instruments=True)
    spec = spec_from_create_kwargs(dict(create_kwargs(s), attach_dim=s["instrument_dim"]))
    assert (spec.Din, spec.Dout, spec.attach) == (145, 145, 16)


@pytest.mark.parametrize("name,value", [("output_dim", 193), ("meta_instrument_dim", 193), ("input_dim", 256)])
def test_wider_rows_are_still_refused_naming_the_limit_and_the_setting(name, value):
    kw = dict(create_kwargs(build_settings(high_crop=128, low_crop=0)))
    kw[name] = value
    with pytest.raises(NotImplementedError, match=r"%s=%d.*192" % (name, value)):
        spec_from_create_kwargs(kw)


def test_one_hot_instrument_attach_does_not_fit_a_byte_and_stays_refused():
    s = build_settings(high_crop=128, low_crop=0, attach_instruments=True, instrument_attach_method="1hot-instrument")
    with pytest.raises(NotImplementedError, match="192"):
        spec_from_create_kwargs(create_kwargs(s))


def test_padded_head_width():
    np_of = hl.load().mvae_head_np
    for N in (129, 144, 145, 192):
        assert np_of(N) >= N and np_of(N) % 16 == 0, (N, np_of(N))
    assert np_of(193) == -1
    assert [np_of(N) for N in (1, 16, 17, 32, 33, 61, 64, 65, 77, 128)] == [16, 16, 32, 32, 64, 64, 64, 128, 128, 128]


@pytest.mark.parametrize("K", [192, 255])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
def test_host_packers_round_trip_wide_rows(K, dtype):
    """the wire format: one byte per row, every column up to K - 1 = 254 representable (255 stays the 'no target' fill)"""
    rng = np.random.default_rng(K)
    n, T = 5, 2 * K
    idx = rng.integers(0, K, (n, T))
    idx[0, :K] = np.arange(K)                      # every column once
    idx[1, :3] = (127, 128, K - 1)
    X = np.eye(K, dtype=dtype)[idx]
    got = host_onehot_to_index(X)
    assert got.dtype == np.uint8 and np.array_equal(got, idx)
    assert np.array_equal(pk.onehot_to_index(X), idx)
    assert np.array_equal(host_onehot_to_index_tm(X, 1, 4), idx[1:4].T)
    assert np.array_equal(np.eye(K)[got.astype(np.int64)], X.astype(np.float64))
