"""The song decodes' surface and the rule their one tail rests on, without a GPU: the Decoder methods that moved to song_decodes keep
their signatures and docstrings, and the two NumPy mirrors of the velocity post-rule with every window starting afresh - the latent
sweep's and the song-level decode's without a song structure - give the same bits."""
import inspect
import json
import os

import numpy as np
import pytest

from midi_vae_amd import reconstruction as rec
from midi_vae_amd import sweep as sw
from midi_vae_amd.model import Decoder
from tests import song_tail_contract as stc

SURFACE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decoder_song_surface.json")))
PUBLIC = ("latent_sweep", "sweep_inputs", "predict_songs", "decode_paths", "interpolation_songs", "medleys", "random_songs",
          "class_knob_codes", "class_knob_songs", "long_songs", "switch_styles")


@pytest.mark.parametrize("name", PUBLIC)
def test_decoder_keeps_signature_and_docstring(name):
    """tests/golden/decoder_song_surface.json was written from the commit before the methods' bodies moved"""
    method = getattr(Decoder, name)
    assert str(inspect.signature(method)) == SURFACE[name]["signature"]
    assert method.__doc__ == SURFACE[name]["doc"]


def test_surface_table_is_complete_and_the_private_tail_is_gone():
    assert sorted(SURFACE) == sorted(PUBLIC)
    assert not hasattr(Decoder, "_finish_songs") and not hasattr(Decoder, "_check_song_extras")


def test_class_knob_codes_is_callable_on_the_class():
    got = Decoder.class_knob_codes(np.arange(5, dtype=np.float32), 3)
    assert got.dtype == np.float32 and got.tolist() == [[1, -1, -1, 3, 4], [-1, 1, -1, 3, 4], [-1, -1, 1, 3, 4]]


@pytest.mark.parametrize("override", [True, False], ids=["rules_on", "rules_off"])
@pytest.mark.parametrize("n,T,V", stc.SHAPES, ids=lambda x: str(x))
def test_the_two_mirrors_agree_window_by_window(n, T, V, override):
    s = stc.settings(V, override)
    idx, vel, plants = stc.planted_rolls(n, T, V)
    of_sweep = sw._mirror(idx, vel, sw.params(s))[1]
    of_recon = rec._mirror(idx, vel, None, None, np.arange(n), rec.params(s))[0]
    assert of_sweep.dtype == of_recon.dtype == np.float32
    assert np.array_equal(of_sweep.view(np.uint32), of_recon.view(np.uint32))
    if override:
        for w, row, want in plants:
            if want is None:
                assert np.isnan(of_recon[w, row]), (w, row)
            else:
                assert of_recon[w, row] == want, (w, row)
        assert not np.array_equal(of_recon.view(np.uint32), np.where(rec.sounding(idx, rec.params(s)), vel, np.float32(0)).view(np.uint32))
