"""Drop-in for the descriptor helpers of the reference's ``data_class`` module (reference data_class.py:25-88, 96-252), bound to
the flat ``settings`` namespace at call time like ``vae_definition``.  These take host piano rolls window by window, as the
reference's callers do, and run the NumPy mirror of ``midi_vae_amd.descriptors``; whole batches of index rolls, and rolls that are
already on the device, go through ``descriptors.signature_vectors`` / ``descriptors.harmonicity`` instead.  The plots of the
reference's module are not reproduced."""
import numpy as np

import midi_vae_amd  # noqa: F401
import settings as _settings
from midi_vae_amd import descriptors as _de
from midi_vae_amd import packers as _pk


def _s():
    return vars(_settings)


def monophonic_to_khot_pianoroll(pianoroll, max_voices, set_all_nonzero_to_1=True):
    return _pk.monophonic_to_khot_pianoroll(pianoroll, max_voices, set_all_nonzero_to_1)


def get_tonal_matrix(r1=1.0, r2=1.0, r3=0.5):
    return _de.tonal_matrix(r1, r2, r3)


def signature_from_pianoroll(pianoroll):
    """15 numbers from a (ticks, pitches) k-hot roll: every nonzero column of a row sounds at that tick"""
    low = int(_s()["low_crop"])
    song = [tuple((np.nonzero(step)[0] + low).tolist()) for step in np.asarray(pianoroll)]
    return signature_from_index(song)


def signature_from_index(song):
    """15 numbers from a sequence of ascending pitch tuples, one per tick"""
    return _de.signature_from_note_sets([tuple(int(p) for p in notes) for notes in song], _np_std=True)


def signature_form_unrolled_pianoroll(pianoroll, voices, include_silent_note):
    """(the reference's spelling) 15 numbers from an unrolled (T, columns) roll, one row per voice and tick; like the reference it
    folds by settings.max_voices and drops the last column when it is the silent one"""
    poly = monophonic_to_khot_pianoroll(np.asarray(pianoroll), int(_s()["max_voices"]))
    if include_silent_note:
        poly = poly[:, :-1]
    return signature_from_pianoroll(poly)


def _unrolled_to_index(rolls):
    """(n, T, pitches) rolls of one-hot or all-zero rows -> (n, T) uint8, 255 where nothing sounds"""
    rolls = np.asarray(rolls)
    if rolls.shape[-1] > 192:
        raise NotImplementedError("piano rolls wider than 192 columns are not supported")
    nz = rolls != 0
    if np.any(nz.sum(-1) > 1) or np.any(rolls[nz] != 1):
        raise NotImplementedError("harmonicity takes unrolled rolls: at most one note per row, written as 1")
    return np.where(nz.any(-1), nz.argmax(-1), 255).astype(np.uint8)


def get_harmonicity_scores_for_each_track_combination(unrolled_pianoroll):
    """(max_voices, max_voices) tonal distance between the voices of an unrolled (T, pitches) roll without a silent column; a
    (n, T, pitches) stack gives the mean over the windows that have a value"""
    rolls = np.asarray(unrolled_pianoroll)
    s = dict(_s())
    s.update(low_crop=0, high_crop=rolls.shape[-1], include_silent_note=False)       # every column of the roll is a pitch
    if rolls.ndim > 2:
        return _de.song_harmonicity(_unrolled_to_index(rolls), s, device=False)
    return _de.harmonicity(_unrolled_to_index(rolls[None]), s, device=False)[0]


def mahalanobis_distance(x, mean, cov):
    diff = x - mean
    return np.sqrt(np.dot(np.dot(diff, np.linalg.pinv(cov)), diff.T))


def get_mean_and_cov_from_vector_list(vector_list):
    return np.mean(vector_list, axis=0), np.cov(np.transpose(vector_list))
