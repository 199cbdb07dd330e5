#!/usr/bin/env python3
"""Generate tests/golden/descriptors.npz: signature vectors and harmonicity matrices from the reference's own functions.

Runs ONLY where the reference is present (make_fixtures.REF); its Keras / pretty_midi imports are replaced by the stub modules
of make_fixtures.py.  Only data is written: the index rolls, the reference's outputs for them and the settings it ran with.

  python tests/golden/make_descriptor_fixtures.py

Pinned functions (reference file:line):
  data_class.py:217-221  signature_form_unrolled_pianoroll   (-> :208-215 signature_from_pianoroll, :116-206 signature_from_index)
  data_class.py:65-88    get_harmonicity_scores_for_each_track_combination   (-> :25-63)

Windows: the shipped shape (T = 64 rows = 16 ticks x 4 voices, 60 pitch columns + the silent one, low_crop 24); 64 each from four
voice-wise random walks with (silent probability, hold probability) = (0.35, 0), (0.3, 0.6), (0.2, 0.8), (0.9, 0.5), then one
all-silent window and one with a single note.  Two assertions keep the fixture from going soft: the mirror with ``_tidy=True``
(held notes dropped from a copy of the list) must DIFFER from the reference on at least a quarter of the windows, and between 5 %
and 60 % of the off-diagonal harmonicity entries must be NaN.

The reference picks the nearest notes with ``np.argsort`` of at most 8 distances and relies on the order it gives to equal ones:
the insertion sort NumPy runs on short arrays, which is stable.  NumPy 2 on a machine with AVX2 / AVX-512 sorts 64-bit keys with a
vectorised network that orders ties differently (3 of these 258 windows change).  The fixture pins the reference as written, so
this script runs itself again with those CPU features disabled for NumPy, and checks that ties come out in input order.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402

GENERATORS = ((0.35, 0.0), (0.3, 0.6), (0.2, 0.8), (0.9, 0.5))
PER_GENERATOR = 64


def random_walk_windows(rng, n, T, V, n_pitch, p_silent, p_hold):
    """(n, T) uint8: every voice walks in steps of -4..4 columns, rests with p_silent, else repeats its last note with p_hold"""
    idx = np.full((n, T), n_pitch, np.uint8)
    for w in range(n):
        for v in range(V):
            q = int(rng.integers(0, n_pitch))
            for k in range(T // V):
                if rng.random() < p_silent:
                    continue
                if not rng.random() < p_hold:
                    q = int(np.clip(q + rng.integers(-4, 5), 0, n_pitch - 1))
                idx[w, k * V + v] = q
    return idx


def _with_scalar_sort():
    """run this script again with NumPy's vectorised sorts off (NPY_DISABLE_CPU_FEATURES is read when NumPy is imported)"""
    import subprocess
    from numpy._core._multiarray_umath import __cpu_features__ as features
    off = sorted(k for k, on in features.items() if on and k.startswith(("AVX2", "AVX512")))
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=" ".join(off), MVAE_FIXTURE_CHILD="1")
    raise SystemExit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=env))


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    if not os.environ.get("MVAE_FIXTURE_CHILD"):
        _with_scalar_sort()
    ties = np.argsort([np.int64(x) for x in (3, 3, 0, 0, 3, 0, 1, 1)])
    assert ties.tolist() == [2, 3, 5, 6, 7, 0, 1, 4], "np.argsort does not keep ties in input order here: %s" % ties
    mfx._stub_modules()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings
    import data_class as dc
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions"):   # the project's own modules of these names are importable again
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)
    sys.path.insert(0, ROOT)
    from midi_vae_amd import descriptors as de

    s = dict(max_voices=int(settings.max_voices), low_crop=int(settings.low_crop), high_crop=int(settings.high_crop),
             include_silent_note=bool(settings.include_silent_note), SMALLEST_NOTE=int(settings.SMALLEST_NOTE))
    V, T, D = s["max_voices"], int(settings.output_length), int(settings.output_dim)
    n_pitch = s["high_crop"] - s["low_crop"]
    assert (T, V, D, n_pitch, s["low_crop"], s["include_silent_note"]) == (64, 4, 61, 60, 24, True)

    rng = np.random.default_rng(20261019)
    parts = [random_walk_windows(rng, PER_GENERATOR, T, V, n_pitch, ps, ph) for ps, ph in GENERATORS]
    silent = np.full((1, T), n_pitch, np.uint8)
    single = silent.copy()
    single[0, 5 * V + 2] = 31
    idx = np.concatenate(parts + [silent, single], 0)
    n = idx.shape[0]

    onehot = np.zeros((n, T, D))
    onehot[np.arange(n)[:, None], np.arange(T)[None, :], idx] = 1
    with np.errstate(all="ignore"):
        import warnings
        warnings.simplefilter("ignore", RuntimeWarning)
        sig = np.array([dc.signature_form_unrolled_pianoroll(onehot[w], V, s["include_silent_note"]) for w in range(n)], np.float64)
        harm = np.array([dc.get_harmonicity_scores_for_each_track_combination(onehot[w][:, :n_pitch]) for w in range(n)], np.float64)

    tidy = de.signature_vectors(idx, s, device=False, _tidy=True, _np_std=True)
    differs = np.any(tidy != sig, axis=1)
    per_gen = [float(differs[i * PER_GENERATOR:(i + 1) * PER_GENERATOR].mean()) for i in range(len(GENERATORS))]
    print("windows on which dropping held notes from a copy changes the signature: %.1f %% (per generator %s)"
          % (100 * differs.mean(), ", ".join("%.0f %%" % (100 * f) for f in per_gen)))
    assert differs.mean() >= 0.25, "the fixture no longer exercises the skipped deletion"
    off = ~np.eye(V, dtype=bool)
    nan = np.isnan(harm[:, off])
    print("off-diagonal harmonicity entries that are NaN: %.1f %% (per generator %s)" % (
        100 * nan.mean(), ", ".join("%.0f %%" % (100 * nan[i * PER_GENERATOR:(i + 1) * PER_GENERATOR].mean()) for i in range(len(GENERATORS)))))
    assert 0.05 <= nan.mean() <= 0.60, "the fixture's NaN share left the band"

    out = dict(idx=idx, signature=sig, harmonicity=harm, generator=np.repeat(np.arange(len(GENERATORS)), PER_GENERATOR),
               **{"s_" + k: np.asarray(v) for k, v in s.items()})
    path = os.path.join(HERE, "descriptors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "windows:", n)


if __name__ == "__main__":
    main()
