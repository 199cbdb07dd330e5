"""lstm_size = 64 k for k = 1..8 through the model surface: accepted by VAE.create for every cell, refused elsewhere, and laid
out / packed exactly as the oracle names and shapes its parameters (no GPU)."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.layout import LSTM_SIZES, ParamLayout, init_params, spec_from_create_kwargs
from midi_vae_amd.model import VAE
from oracle.vae_oracle import make_cfg, param_shapes

CELLS = ["GRU", "LSTM", "SimpleRNN"]


def _kw(**over):
    return create_kwargs(build_settings(**over))


def test_accepted_sizes_are_the_multiples_of_64_up_to_512():
    assert LSTM_SIZES == (64, 128, 192, 256, 320, 384, 448, 512)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("H", [192, 320, 384, 448, 512])
def test_create_accepts_the_new_sizes(cell, H):
    m = VAE().create(**_kw(cell_type=cell, lstm_size=H))
    assert m.lstm_size == H and m.cell_type == cell
    spec = spec_from_create_kwargs(_kw(cell_type=cell, lstm_size=H))
    assert m.autoencoder.count_params() == sum(int(np.prod(s)) for s in param_shapes(make_cfg(**spec.oracle_cfg())).values())


@pytest.mark.parametrize("H", [100, 32, 576, 640, 1024])
def test_other_sizes_are_refused_naming_the_accepted_set(H):
    with pytest.raises(NotImplementedError, match="64, 128, 192, 256, 320, 384, 448, 512"):
        VAE().create(**_kw(lstm_size=H))


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("H", [192, 384, 512])
def test_layout_matches_the_oracle_and_roundtrips(cell, H):
    spec = spec_from_create_kwargs(_kw(cell_type=cell, lstm_size=H))
    assert spec.H == H
    L = ParamLayout.build(spec)
    o = param_shapes(make_cfg(**spec.oracle_cfg()))
    assert set(o) == set(L.oracle_names())
    for k, shp in o.items():
        assert tuple(shp) == L.entries[k].shape, k
    p = init_params(spec, 5)
    back = L.unpack(L.pack(p))
    assert all(np.array_equal(p[k], back[k]) for k in p)
