"""Per-window evaluation, the parts that need no GPU: the fields appended to the argument structs under ABI 9 sit at the end of
their structs in the header and in the ctypes mirrors; the per-song reduction of the per-window block; the argument refusals of
``autoencoder.evaluate_songs`` / ``evaluate_windows``, which come before anything touches a device."""
import os
import re

import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import packers as pk
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE, DeviceLatent, song_means
from midi_vae_amd.staging import Norm
from midi_vae_amd.synth import make_windows, to_reference_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

APPENDED = {"mvae_head_args": (hl.HeadArgs, ["row_out"]),
            "mvae_latent_fwd_args": (hl.LatentFwdArgs, ["kl_rows", "style_rows"]),
            "mvae_latent_chain_fwd_args": (hl.LatentChainFwdArgs, ["kl_rows", "style_rows"])}


def _header_fields(struct):
    """field names of ``struct`` in include/midivae_hip.h, in declaration order (comments stripped)"""
    text = open(os.path.join(ROOT, "include", "midivae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():            # "const float *w_mu, *b_mu" / "int32_t B, Z, C" / "float* S": the last identifier of every part
            names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    return names


@pytest.mark.parametrize("struct", list(APPENDED))
def test_appended_fields_are_the_last_fields_of_their_structs(struct):
    cls, fields = APPENDED[struct]
    assert [n for n, _ in cls._fields_][-len(fields):] == fields
    assert _header_fields(struct)[-len(fields):] == fields
    assert all(t is hl._vp for _, t in cls._fields_[-len(fields):])
    # NULL is what a caller that does not know the fields passes: a struct built by keyword holds it
    assert all(getattr(cls(), f) is None for f in fields)
    assert hl.ABI_VERSION == 9


def test_header_and_integration_notes_say_the_fields_were_appended_under_abi_9():
    header = open(os.path.join(ROOT, "include", "midivae_hip.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (header, notes):
        for f in ("row_out", "kl_rows", "style_rows"):
            assert f in text
        assert re.search(r"appended\s+under\s+ABI\s+9", text, flags=re.I)


def test_song_means_hand_written():
    rows = np.array([[1.0, 0.5],                         # song 0: one window
                     [2.0, 1.0], [4.0, 0.0], [6.0, 0.5],           # song 1: three windows
                     [1.0, 0.25], [3.0, 0.75]])                     # song 2: two windows
    got = song_means(rows, [1, 3, 2])
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([[1.0, 0.5], [4.0, 0.5], [2.0, 0.5]]))


def test_song_means_of_songs_that_are_no_multiple_of_the_batch_size():
    """a song's metric is the mean over its windows whatever batch_size cut it into (17 = 16 + 1, 40 = 16 + 16 + 8): Keras' mean of
    batch means weighted by the batch sizes is the same number"""
    rng = np.random.default_rng(0)
    lengths = [1, 17, 40, 16]
    rows = rng.random((sum(lengths), 3))
    got = song_means(rows, lengths)
    lo = 0
    for i, n in enumerate(lengths):
        song = rows[lo:lo + n]
        keras = sum(song[b:b + 16].mean(0) * len(song[b:b + 16]) for b in range(0, n, 16)) / n
        np.testing.assert_allclose(got[i], keras, rtol=1e-14, atol=0)
        np.testing.assert_allclose(got[i], song.mean(0), rtol=1e-14, atol=0)
        lo += n
    assert np.array_equal(got[0], rows[0])              # (the one-window song: its row)


def test_song_means_refuses_lengths_that_do_not_fit():
    with pytest.raises(ValueError):
        song_means(np.zeros((4, 2)), [2, 3])
    with pytest.raises(ValueError):
        song_means(np.zeros((4, 2)), [4, 0])


def test_one_window_normalisers():
    """the row weights of a per-window step: 1 / steps of the head, a batch of one"""
    nm = Norm.one_window(64)
    assert (nm.B, nm.nz_notes, nm.nz_instr, nm.nz_vel, nm.nz_style, nm.nz_held, nm.nz_next, nm.nz_cnotes, nm.nz_cinstr) == \
        (1, 64, 1, 1, 1, 1, 1, 1, 1)


def _lists(s, n, seed=1, hist=None):
    w = make_windows(n, s["output_length"], s["output_dim"], s["max_voices"], 16, s["num_classes"], s["latent_dim"], seed=seed)
    X, Y, C, I, V, D = to_reference_format(w)
    H = np.zeros((n, s["latent_dim"])) if hist is None else hist
    return pk.prepare_autoencoder_input_and_output_list(s, X, Y, C, I, V, D, np.zeros((n, s["signature_vector_length"])), H)


def test_evaluate_songs_refusals_say_what_to_pass():
    s = build_settings(lstm_size=64, latent_dim=16, input_length=2, output_length=2, batch_size=16)
    m = VAE().create(compute_dtype="f32", **create_kwargs(s))
    x, y = _lists(s, 3)
    assert m.autoencoder.evaluate_songs([], []) == []
    with pytest.raises(ValueError, match="one x and one y per song"):
        m.autoencoder.evaluate_songs([x, x], [y])
    x0, y0 = [a[:0] for a in x], [a[:0] for a in y]
    with pytest.raises(ValueError, match="song 1 has no windows"):
        m.autoencoder.evaluate_songs([x, x0], [y, y0])
    lat = DeviceLatent.__new__(DeviceLatent)            # (a device-resident history: only its type matters here)
    xd = list(x)
    xd[2] = lat
    with pytest.raises(TypeError, match="host array"):
        m.autoencoder.evaluate_songs([x, xd], [y, y])
    with pytest.raises(TypeError, match="host array"):
        m.autoencoder.evaluate_windows(xd, y)
    ss = build_settings(lstm_size=64, latent_dim=32, input_length=2, output_length=2, batch_size=16, signature_decoder=True)
    ms = VAE().create(compute_dtype="f32", **create_kwargs(ss))
    with pytest.raises(NotImplementedError, match="signature_decoder"):
        ms.autoencoder.evaluate_songs([x], [y])
    assert m._shared.infer is None and ms._shared.infer is None          # (no engine was built for any of this)
