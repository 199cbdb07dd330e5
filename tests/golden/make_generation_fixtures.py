#!/usr/bin/env python3
"""Generate tests/golden/generation.npz: the decoder's latent rows of interpolation songs and medleys from the reference's own
``linear_interpolation`` and ``slerp``, and piano-roll images from its own ``prepare_for_drawing`` and
``monophonic_to_khot_pianoroll``.

Runs ONLY where the reference is present (make_fixtures.REF).  The reference's vae_evaluation.py is a script, so it is never imported:
the three functions (:578-584, :619-642) are picked out of its syntax tree, ``monophonic_to_khot_pianoroll`` out of data_class.py's
(:241-252), and executed in a namespace that holds the globals they read.  The two generation loops (:731-822 medleys, :864-874
random interpolation songs) are inline script code there; ``medley`` and ``interpolation_song`` below restate them line by line with a
stand-in decoder that records the z and the history it is handed, cast to float32 as the engine's staging casts them.  Only data is
written: anchors, recipes' results, rolls, velocities and the recorded arrays.

  python tests/golden/make_generation_fixtures.py

Paths, once with float32 codes (what encoder.predict returns) and once with float64 codes (np.random.normal): a run of 75 windows,
Z = 32, in four songs - a medley of one song of one window; a random interpolation song of length 10 (11 windows); a medley at the
reference's defaults, 3 songs of 8 windows and bridges of 4 (32 windows); a medley of songs of 9, 7 and 5 windows with bridges of 5
blended by ``slerp`` (31 windows).  Some coordinates of the anchors are -0.0.
Images: case ``a`` T = 16 / 2 voices, 20 pitches, songs of 1, 3, 40 and 5 windows - the song of 40 holds one note per voice
throughout, both on one cell; case ``b`` T = 12 / 3 voices, 9 pitches, songs of 2, 1 and 6 windows.  Velocities are float32 values handed to the
reference as float64, which keeps NumPy's scalar promotion out of the fixture.
Assertions keep the fixture sharp; ``main`` prints what each one counted.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402

Z = 32
THRESHOLD, MAX_VELOCITY = 0.5, 127.0


def _pick(path, names, ns):
    tree = ast.parse(open(os.path.join(mfx.REF, path)).read())
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
    assert sorted(n.name for n in picked) == sorted(names), (path, names)
    exec(compile(ast.Module(body=picked, type_ignores=[]), "<pinned>", "exec"), ns)
    return ns


def reference_functions(max_voices):
    khot = _pick("data_class.py", ["monophonic_to_khot_pianoroll"], dict(np=np))

    class data_class:          # what prepare_for_drawing calls through the module's name
        monophonic_to_khot_pianoroll = staticmethod(khot["monophonic_to_khot_pianoroll"])

    ns = dict(np=np, arccos=np.arccos, dot=np.dot, sin=np.sin, data_class=data_class, max_voices=max_voices,
              velocity_threshold_such_that_it_is_a_played_note=THRESHOLD, MAX_VELOCITY=MAX_VELOCITY)
    return _pick("vae_evaluation.py", ["linear_interpolation", "slerp", "prepare_for_drawing"], ns)


# ---- the two generation loops, restated ---------------------------------------------------------------------------------------------
class Recorder:
    """the stand-in decoder: keeps the z and the history of every call as the float32 rows the engine's staging makes of them"""

    def __init__(self):
        self.z, self.hist = [], []

    def predict(self, z, previous_latent_rep):
        self.z.append(np.asarray(z, np.float32).reshape(-1).copy())
        self.hist.append(np.asarray(previous_latent_rep, np.float32).reshape(-1).copy())


def medley(Rs, interpolation_length, blend, latent_dim):
    decoder = Recorder()
    previous_medley_z = None                                                           # :725
    previous_latent_rep = np.zeros((1, latent_dim))                                    # :727
    for medley_song_num in range(len(Rs)):                                             # :731
        R = Rs[medley_song_num]                                                        # :790
        if previous_medley_z is not None:                                              # :792
            for i in range(interpolation_length):                                      # :794
                z = blend(previous_medley_z, R[0], i / float(interpolation_length))    # :795
                z = np.expand_dims(z, axis=0)                                          # :796
                decoder.predict(z, previous_latent_rep)                                # :797-798
                previous_latent_rep = z                                                # :807
        for i in range(R.shape[0]):                                                    # :809
            z = R[i]                                                                   # :810
            z = np.expand_dims(z, axis=0)                                              # :811
            decoder.predict(z, previous_latent_rep)                                    # :812-813
            previous_latent_rep = z                                                    # :820
        previous_medley_z = R[-1]                                                      # :822
    return np.stack(decoder.z), np.stack(decoder.hist)


def interpolation_song(random_code_1, random_code_2, interpolation_song_length, blend, latent_dim):
    decoder = Recorder()
    previous_latent_rep = np.zeros((1, latent_dim))                                    # :860
    for i in range(interpolation_song_length + 1):                                     # :864
        R = blend(random_code_1, random_code_2, i / float(interpolation_song_length))  # :865
        decoder.predict(R, previous_latent_rep)                                        # :866-867
        previous_latent_rep = R                                                        # :874
    return np.stack(decoder.z), np.stack(decoder.hist)


def _fma_rows(A, a0, a1, c0, c1, z):
    """windows whose float32 blend changes when either product is fused into the sum (a float32 product is exact in double and the
    double sum rounds at 2^-53, so rounding it to float32 is the fused result up to a 2^-29 chance)"""
    rows = 0
    for w in np.nonzero(a1 >= 0)[0]:
        x, y = A[a0[w]], A[a1[w]]
        k0, k1 = np.float32(c0[w]), np.float32(c1[w])
        f1 = (y.astype(np.float64) * np.float64(k1) + (x * k0).astype(np.float64)).astype(np.float32)
        f2 = (x.astype(np.float64) * np.float64(k0) + (y * k1).astype(np.float64)).astype(np.float32)
        rows += bool((f1.view(np.uint32) != z[w].view(np.uint32)).any() or (f2.view(np.uint32) != z[w].view(np.uint32)).any())
    return rows


def build_paths(rng, ref, dtype, tag):
    """the run of 75 windows and, beside what the reference's loops hand the decoder, the anchors and the recipe that describe it"""
    lerp, slerp = ref["linear_interpolation"], ref["slerp"]
    codes = lambda m: (rng.standard_normal((m, Z)) * 1.5).astype(dtype)
    one = [codes(1)]
    pair = codes(2)
    pair[0, [3, 9]] = -0.0
    pair[1, 3], pair[1, 9] = abs(pair[1, 3]) + dtype(0.25), -abs(pair[1, 9]) - dtype(0.25)
    defaults = [codes(8) for _ in range(3)]
    defaults[0][-1, [0, 5]] = -0.0
    defaults[1][0, 0], defaults[1][0, 5] = dtype(0.75), dtype(-0.75)
    ragged = [codes(m) for m in (9, 7, 5)]
    songs = [medley(one, 4, lerp, Z), interpolation_song(pair[0:1], pair[1:2], 10, lerp, Z), medley(defaults, 4, lerp, Z),
             medley(ragged, 5, slerp, Z)]
    lengths = [len(z) for z, _ in songs]
    assert lengths == [1, 11, 32, 31]
    z = np.concatenate([s[0] for s in songs])
    hist = np.concatenate([s[1] for s in songs])
    assert z.dtype == np.float32 and hist.dtype == np.float32

    # the anchors and the recipe, by hand: rows of `one`, `pair`, `defaults`, `ragged` in this order
    anchors = np.concatenate(one + [pair] + defaults + ragged)
    a0, a1, c0, c1 = [0], [-1], [1.0], [0.0]
    for i in range(11):
        t = i / float(10)
        a0.append(1), a1.append(2), c0.append(1.0 - t), c1.append(t)
    off = 3
    for group, L, mode in ((defaults, 4, "lerp"), (ragged, 5, "slerp")):
        for k, R in enumerate(group):
            if k:
                p0, p1 = anchors[off - 1], anchors[off]
                for i in range(L):
                    t = i / float(L)
                    if mode == "lerp":
                        k0, k1 = 1.0 - t, t
                    else:          # the two factors of the reference's slerp, evaluated as it evaluates them
                        omega = np.arccos(np.dot(p0 / np.linalg.norm(p0), p1 / np.linalg.norm(p1)))
                        so = np.sin(omega)
                        k0, k1 = float(np.sin((1.0 - t) * omega) / so), float(np.sin(t * omega) / so)
                    a0.append(off - 1), a1.append(off), c0.append(k0), c1.append(k1)
            for r in range(len(R)):
                a0.append(off + r), a1.append(-1), c0.append(1.0), c1.append(0.0)
            off += len(R)
    a0, a1, c0, c1 = np.asarray(a0, np.int32), np.asarray(a1, np.int32), np.asarray(c0), np.asarray(c1)
    assert off == len(anchors) == 48 and len(a0) == 75

    fma = _fma_rows(anchors, a0, a1, c0, c1, z) if dtype is np.float32 else 0
    neg_zero_kept = int(((z == 0) & np.signbit(z)).sum())
    blended = np.nonzero((a1 >= 0) & (c1 == 0.0))[0]
    neg_zero_lost = int(sum(((anchors[a0[w]] == 0) & np.signbit(anchors[a0[w]]) & ~np.signbit(z[w])).sum() for w in blended))
    print("paths %s: %d anchors, %d windows, %d rows change under FMA, %d coordinates keep -0.0, %d lose it in a blend at t = 0"
          % (tag, len(anchors), len(a0), fma, neg_zero_kept, neg_zero_lost))
    assert dtype is not np.float32 or fma >= 10
    assert neg_zero_kept >= 3 and neg_zero_lost >= 2
    out = dict(anchors=anchors, a0=a0, a1=a1, c0=c0, c1=c1, lengths=np.asarray(lengths, np.int64), z=z, hist=hist, fma_rows=np.int64(fma))
    return {"paths_%s_%s" % (tag, k): v for k, v in out.items()}


# ---- images ----------------------------------------------------------------------------------------------------------------------
def _voice_rows(rng, ticks, n_pitch, held_throughout=None):
    """one voice of one song: (index, velocity) per tick.  Runs of one pitch - pitch index 0 and the silent index n_pitch among them -
    struck on their first tick and mostly held after it"""
    idx, vel = np.zeros(ticks, np.uint8), np.zeros(ticks, np.float32)
    if held_throughout is not None:
        first, pitch = held_throughout
        idx[:] = pitch
        vel[:] = rng.uniform(0.05, 0.45, ticks)
        vel[first] = 0.9
        return idx, vel
    t = 0
    while t < ticks:
        run = int(rng.integers(1, 7))
        pitch = int(rng.choice([0, 0, n_pitch, n_pitch, rng.integers(1, 4), rng.integers(1, n_pitch)]))
        for k in range(min(run, ticks - t)):
            idx[t + k] = pitch
            struck = rng.random() < (0.55 if k == 0 else 0.1)
            vel[t + k] = rng.uniform(0.55, 1.0) if struck else rng.uniform(0.0, 0.5)
        t += run
    return idx, vel


def restated_newY(Y, V, max_voices):
    """prepare_for_drawing's loop (:621-637), restated to look at the rows before they are folded"""
    newY = np.copy(Y)
    for step in range(V.shape[0]):
        if V[step] > THRESHOLD:
            velocity = (V[step] - THRESHOLD) * MAX_VELOCITY
            newY[step, :] *= velocity
        else:
            if step > max_voices:
                previous_pitch = np.argmax(newY[step - max_voices])
                current_pitch = np.argmax(newY[step])
                if current_pitch != previous_pitch:
                    newY[step, :] = 0
                else:
                    newY[step, :] = newY[step - max_voices, :]
            else:
                newY[step, :] = 0
    return newY


def build_images(rng, case):
    name, T, V, n_pitch, lengths = case["name"], case["T"], case["V"], case["n_pitch"], case["lengths"]
    ref = reference_functions(V)
    ticks = T // V
    idx_songs, vel_songs, with_v, without_v = [], [], [], []
    seen = dict.fromkeys(("pitch0_continues", "step_equals_voices", "shared_cell", "broken_chain", "struck_silent", "crosses_window"), 0)
    for s, m in enumerate(lengths):
        L = m * ticks
        voices = []
        for v in range(V):
            held = None
            if s == case.get("held_song"):          # one note per voice through the whole song: the longest look-back
                held = (1, 4) if v == 0 else (0, 4)          # (both on one cell: their levels add up)
            voices.append(_voice_rows(rng, L, n_pitch, held))
        if s in (0, 1):          # voice 0 strikes a note on the song's first tick and holds it: the row at step == V must not inherit
            voices[0][0][:2] = 3
            voices[0][1][:2] = (0.8, 0.2)
        idx = np.stack([a for a, _ in voices], 1).reshape(m, T)          # row t of a window: voice t % V of tick t // V
        vel = np.stack([b for _, b in voices], 1).reshape(m, T)
        Y = np.zeros((m * T, n_pitch))
        rows = idx.reshape(-1)
        Y[np.nonzero(rows < n_pitch)[0], rows[rows < n_pitch]] = 1.0
        V64 = vel.reshape(-1).astype(np.float64)
        image = ref["prepare_for_drawing"](Y, V64)
        binary = ref["prepare_for_drawing"](Y)
        assert image.shape == binary.shape == (n_pitch, L) and image.dtype == np.float64

        newY = restated_newY(Y, V64, V)
        folded = np.zeros((L, n_pitch))
        for step in range(m * T):
            folded[step // V] += newY[step]
        assert np.array_equal(folded.T, image), "the restated loop is not the reference's"
        sounds, struck = Y.any(1), V64 > THRESHOLD
        for step in range(m * T):
            shown = newY[step].any()
            if not struck[step] and not sounds[step] and shown and newY[step, 0] != 0:
                seen["pitch0_continues"] += 1
            if not struck[step] and step == V and newY[step - V].any() and np.argmax(newY[step - V]) == np.argmax(Y[step]):
                assert not shown
                seen["step_equals_voices"] += 1
            if not struck[step] and step > V and newY[step - V].any() and np.argmax(newY[step - V]) != np.argmax(Y[step]):
                assert not shown
                seen["broken_chain"] += 1
            if struck[step] and not sounds[step]:
                assert not shown
                seen["struck_silent"] += 1
            if not struck[step] and shown and step >= T and step % T < V:
                seen["crosses_window"] += 1
        per_tick = (newY.reshape(L, V, n_pitch) != 0).sum(1)
        seen["shared_cell"] += int((per_tick > 1).sum())
        idx_songs.append(idx), vel_songs.append(vel), with_v.append(image.T), without_v.append(binary.T)
    print("image case %s: %s" % (name, ", ".join("%s %d" % kv for kv in seen.items())))
    assert all(count >= 2 for count in seen.values()), seen
    assert 1 in lengths
    out = dict(idx=np.concatenate(idx_songs), vel=np.concatenate(vel_songs), lengths=np.asarray(lengths, np.int64),
               voices=np.int64(V), n_pitch=np.int64(n_pitch), threshold=np.float64(THRESHOLD), max_velocity=np.float64(MAX_VELOCITY),
               image=np.concatenate(with_v), binary=np.concatenate(without_v))          # both tick-major: (all ticks, n_pitch)
    if "held_song" in case:
        out["held_song"] = np.int64(case["held_song"])
        lo = sum(lengths[:case["held_song"]]) * ticks
        held = out["image"][lo:lo + lengths[case["held_song"]] * ticks]
        assert (held[2:, 4] > 0).all() and np.count_nonzero(held[2:]) == len(held) - 2, "the held song's notes do not last"
    return {"image_%s_%s" % (name, k): v for k, v in out.items()}


IMAGE_CASES = (dict(name="a", T=16, V=2, n_pitch=20, lengths=[1, 3, 40, 5], held_song=2),
               dict(name="b", T=12, V=3, n_pitch=9, lengths=[2, 1, 6]))


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    rng = np.random.default_rng(20261022)
    ref = reference_functions(2)
    out = {}
    out.update(build_paths(rng, ref, np.float32, "f32"))
    out.update(build_paths(rng, ref, np.float64, "f64"))
    for case in IMAGE_CASES:
        out.update(build_images(rng, case))
    path = os.path.join(HERE, "generation.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
