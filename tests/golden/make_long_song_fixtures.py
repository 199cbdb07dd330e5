#!/usr/bin/env python3
"""Generate tests/golden/long_songs.npz: the long-song generator's search-and-pull loop and its decode-to-encode feedback, from the
reference's own functions.

Runs ONLY where the reference is present (make_fixtures.REF), on the CPU.  vae_definition.process_decoder_outputs and
prepare_encoder_input_list are imported with the stub modules of make_fixtures.py and their settings patched per case, as
make_recon_fixtures.py patches them.  The search loop lives in vae_evaluation.py, a script that cannot be imported: it is restated, as it
stands, in midi_vae_amd.longsongs.walk_reference, which this file drives with a scripted table of codes in place of decode and encode.
Only data is written.

  python tests/golden/make_long_song_fixtures.py

(a) Walk cases ``walk_<name>_*``: all_z (N, Z) float32, start (S, Z) float64 the first code, script (S, L-1, Z) float32 the codes the
"encoder" returns, e (float32; the reference's np.std(all_z)) and den = 1 + e as NumPy forms it; results picked (S, L), z (S, L, Z)
float32 the pulled codes as the decoder reads them, r0 (S, Z) float64 the first pull unrounded, dist (S, L) the reference's own norms.
Scripted codes aim at a row of all_z plus a little noise, so every search is DECISIVE against the reference's float32 BLAS norm whose
summation order is not the kernel's: the winner's distance is below every other candidate's by a relative margin of 1e-4 (well above
Z * 2^-24 at Z = 257), or ties exactly with a duplicate row; this file asserts it and writes nothing otherwise.  It also asserts that
the NumPy mirror (longsongs.nearest_walk(device=False)) repeats the reference bit for bit and counts the elements on which a fused
multiply-add would change the pull.

(b) Feedback cases, flat arrays ``fb_*`` with one row of ``fb_cases`` per case (voices, T, n, silent, vel, held, override, first
instrument byte, first row, threshold * 1000): decoded windows through process_decoder_outputs ONE WINDOW A CALL, the silent column of
vae_evaluation.py:1878-1884 and prepare_encoder_input_list; recorded are X (as indices), V, D and I as the encoder receives them.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_fixtures as mfx  # noqa: E402

MARGIN = 1e-4
N_PITCH, LOW_CROP, ID = 12, 24, 5


# ---- (a) walks ---------------------------------------------------------------------------------------------------------------------
def walk_case(ls, rng, name, N, Z, S, L, targets=None, all_z=None, spread=1.0, first=None):
    """targets (S, L-1): the row every scripted code aims at (None: random rows); first (S,): the row the start code aims at (None: a
    random code, as the reference draws it)"""
    if all_z is None:
        all_z = (rng.standard_normal((N, Z)) * spread).astype(np.float32)
    N = all_z.shape[0]
    e = np.std(all_z)
    if not e > 0:
        e = np.float32(0.5)
    assert isinstance(e, np.float32)
    den = 1 + e
    start = rng.standard_normal((S, Z)) * float(e)
    if first is not None:
        start = all_z[np.asarray(first)].astype(np.float64) + start * 1e-3
    if targets is None:
        targets = rng.integers(0, N, (S, max(L - 1, 0)))
    targets = np.asarray(targets).reshape(S, max(L - 1, 0))
    noise = (rng.standard_normal((S, max(L - 1, 0), Z)) * 1e-3).astype(np.float32)
    script = (all_z[targets] + noise).astype(np.float32)
    picked, z, dist = np.zeros((S, L), np.int32), np.zeros((S, L, Z), np.float32), np.zeros((S, L))
    r0 = np.zeros((S, Z))
    fused = 0
    for s in range(S):
        ref = ls.walk_reference(all_z, start[s], L, e, step=lambda it, R, prev: script[s, it] if it < L - 1 else R)
        assert ref["rows"][0].dtype == np.float64 and all(r.dtype == np.float32 for r in ref["rows"][1:])
        picked[s], z[s], dist[s], r0[s] = ref["picked"], ref["z"], ref["distances"], ref["rows"][0][0]
        # the mirror, iteration by iteration, and how decisive every search is
        for it in range(L):
            R = start[s][None] if it == 0 else script[s, it - 1][None]
            got = ls.nearest_walk(all_z, R, picked[s:s + 1, :it], e, device=False)
            assert got["best"][0] == picked[s, it], (name, s, it)
            assert got["z"].tobytes() == z[s, it].tobytes(), (name, s, it)
            d = np.sqrt(np.cumsum((all_z.astype(np.float64) - R.astype(np.float64)) ** 2, axis=1)[:, -1])
            w = picked[s, it]
            cand = np.ones(N, bool)
            cand[picked[s, :it]] = False
            cand[0] = True
            cand[w] = False
            twin = np.all(all_z == all_z[w], axis=1)
            close = cand & ~(d >= d[w] * (1 + MARGIN))
            assert not np.any(close & ~twin), "%s: song %d iteration %d is not decisive" % (name, s, it)
            assert not np.any(close & twin & (np.arange(N) < w))
            assert abs(ref["distances"][it] - d[w]) <= 1e-5 * max(d[w], 1e-30)
            # a fused multiply-add: r + z * e with the product exact (a float32 product is exact in double)
            prod = all_z[w].astype(np.float64) * np.float64(e)
            if R.dtype == np.float32:
                fused += int(np.sum((R[0].astype(np.float64) + prod).astype(np.float32) != (R[0] + all_z[w] * e)))
            else:
                fused += int(np.sum((R[0] + prod) != (R[0] + (all_z[w] * e).astype(np.float64))))
    out = {"all_z": all_z, "start": start, "script": script, "e": np.float32(e), "den": np.float64(float(den)), "picked": picked, "z": z,
           "r0": r0, "dist": dist}
    return {"walk_%s_%s" % (name, k): v for k, v in out.items()}, fused


def walks(ls):
    rng = np.random.default_rng(20261022)
    data, fused = {}, {}

    def add(name, *a, **k):
        d, f = walk_case(ls, rng, name, *a, **k)
        data.update(d)
        fused[name] = f

    add("n1", 1, 8, 1, 3)
    add("runout", 5, 8, 2, 8, first=[0, 3], targets=[[1, 2, 3, 4, 2, 3, 4], [4, 2, 1, 0, 1, 0, 2]])   # the candidates run out: index 0 again and again
    base = (rng.standard_normal((6, 8))).astype(np.float32)
    dup = np.concatenate([base, base[[1, 3]], base[[1]]], 0)     # rows 6, 8 repeat row 1, row 7 repeats row 3: exact ties
    add("dups", 9, 8, 2, 6, first=[0, 5], targets=[[1, 1, 1, 3, 3], [3, 3, 1, 1, 1]], all_z=dup)
    add("zero", 7, 8, 2, 5, first=[0, 4], targets=[[0, 0, 3, 0], [2, 0, 0, 0]])          # index 0 picked before and nearest again
    add("z1", 9, 1, 2, 4, spread=4.0)
    add("z3", 9, 3, 17, 4)
    add("z256", 24, 256, 2, 4)
    add("z257", 24, 257, 1, 4)
    for N in (63, 64, 65, 255, 256, 257):
        add("n%d" % N, N, 3, 2, 4, targets=[[N - 1, 0, N // 2], [N - 2, N - 1, 1]], spread=3.0)
    for S in (7, 8, 9):
        add("s%d" % S, 40, 4, S, 3, spread=3.0)
    add("n3000", 3000, 3, 3, 5, targets=[[2999, 256, 1023, 2048], [255, 257, 2999, 512], [1, 2, 3, 2998]], spread=6.0)
    print("elements a fused multiply-add would change:", fused)
    assert sum(fused.values()) >= 50 and fused["z256"] > 0 and fused["z3"] > 0
    # what the cases promise
    assert data["walk_runout_picked"].tolist() == [[0, 1, 2, 3, 4, 0, 0, 0], [3, 4, 2, 1, 0, 0, 0, 0]]
    assert data["walk_dups_picked"][0, 1:4].tolist() == [1, 6, 8] and data["walk_dups_picked"][0, 4:].tolist() == [3, 7]
    assert data["walk_zero_picked"].tolist() == [[0, 0, 0, 3, 0], [4, 2, 0, 0, 0]]
    return data


# ---- (b) feedback ------------------------------------------------------------------------------------------------------------------
FLAGS = ((1, 1, 0, 1), (0, 1, 1, 0), (1, 0, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (1, 1, 0, 0))          # silent, vel, held, override


def feedback(vd):
    rng = np.random.default_rng(20261023)
    cases, flat = [], {k: [] for k in ("idx", "vel", "held", "instr", "X", "V", "D", "I")}
    w0 = r0 = 0
    for V in (2, 4, 8):
        for ticks in (1, 3, 16):
            T = V * ticks
            for k, (silent, has_vel, has_held, override) in enumerate(FLAGS):
                thr = (0.5, 0.25)[k % 2]
                n = 4
                D_out = N_PITCH + silent
                idx = rng.integers(0, N_PITCH, (n, T))
                for w in range(n):          # runs of one pitch, as a decode makes them
                    for v in range(V):
                        col = idx[w, v::V]
                        keep = rng.random(ticks) < 0.5
                        for t in range(1, ticks):
                            if keep[t]:
                                col[t] = col[t - 1]
                if silent:
                    idx[rng.random((n, T)) < 0.25] = N_PITCH
                    idx[n - 1] = N_PITCH                                                   # a window that is all silent
                if ticks > 1:
                    idx[0, 0], idx[0, V] = 0, 5                                            # the `previous_pitch > 0` quirk: a pitch-index-0 note
                vel = rng.random((n, T))
                vel = np.where(rng.random((n, T)) < 1 / 3, np.round(vel * 8) / 8, vel).astype(np.float32)
                vel[rng.random((n, T)) < 0.15] = np.float32(thr)                           # exactly at the threshold
                if ticks > 1:
                    vel[0, 0], vel[0, V] = 0.875, 0.125
                held = (rng.random((n, T)) < 0.6).astype(np.uint8)
                instr = rng.integers(0, ID, (n, V))
                vd.max_voices, vd.output_length, vd.input_length = V, T, T
                vd.low_crop, vd.high_crop, vd.include_silent_note = LOW_CROP, LOW_CROP + N_PITCH, bool(silent)
                vd.output_dim = vd.input_dim = D_out
                vd.meta_instrument, vd.meta_instrument_dim = True, ID
                vd.meta_velocity, vd.meta_held_notes, vd.meta_next_notes = bool(has_vel), bool(has_held), False
                vd.override_sampled_pitches_based_on_velocity_info = bool(override)
                vd.velocity_threshold_such_that_it_is_a_played_note = thr
                vd.combine_velocity_and_held_notes = False

                def onehot(a, width):
                    out = np.zeros(a.shape + (width,))
                    np.put_along_axis(out, a[..., None].astype(np.int64), 1, axis=-1)
                    return out

                X_all, V_all, D_all, I_all = [], [], [], []
                for w in range(n):          # one window a call, as the long-song loop decodes
                    outputs = [onehot(idx[w:w + 1], D_out), onehot(instr[w:w + 1], ID)]
                    if has_vel:
                        outputs.append(vel[w:w + 1].astype(np.float64).reshape(1, T, 1))
                    if has_held:
                        outputs.append(onehot(held[w:w + 1], 2))
                    Y, I, Vp, Dp, _ = vd.process_decoder_outputs(outputs, "argmax")
                    X = np.copy(Y)                                                          # vae_evaluation.py:1878-1884
                    if silent:
                        X = np.append(X, np.zeros((X.shape[0], 1)), axis=1)
                        for step in range(X.shape[0]):
                            if np.sum(X[step]) == 0:
                                X[step, -1] = 1
                    X = np.asarray([X])
                    lst = vd.prepare_encoder_input_list(X, I[0], np.expand_dims(Vp, axis=0), np.expand_dims(Dp, axis=0))
                    assert isinstance(lst, list) and np.all(lst[0].sum(-1) == 1)
                    X_all.append(np.argmax(lst[0][0], -1))
                    I_all.append(np.argmax(lst[1][0], -1))
                    pos = 2
                    v_enc = np.asarray(Vp, np.float64)
                    if has_vel:
                        v_enc = lst[pos][0, :, 0]
                        pos += 1
                    d_enc = (np.asarray(Dp) != 0).astype(np.int64)
                    if has_held:
                        d_enc = np.argmax(lst[pos][0], -1)
                    assert np.array_equal(d_enc, (np.asarray(Dp) != 0).astype(np.int64))
                    assert np.array_equal(v_enc.astype(np.float32).astype(np.float64), v_enc)          # inputs, zeros, the default: nothing rounds
                    V_all.append(v_enc)
                    D_all.append(d_enc)
                assert np.array_equal(np.asarray(X_all), idx)                                           # the index byte, unchanged
                cases.append((V, T, n, silent, has_vel, has_held, override, w0, r0, int(round(thr * 1000))))
                for key, arr, dt in (("idx", idx, np.uint8), ("vel", vel, np.float32), ("held", held, np.uint8), ("instr", instr, np.uint8),
                                     ("X", np.asarray(X_all), np.uint8), ("V", np.asarray(V_all), np.float32), ("D", np.asarray(D_all), np.uint8),
                                     ("I", np.asarray(I_all), np.uint8)):
                    flat[key].append(np.asarray(arr).astype(dt).reshape(-1))
                w0 += n * V
                r0 += n * T
    data = {"fb_" + k: np.concatenate(v) for k, v in flat.items()}
    data["fb_cases"] = np.asarray(cases, np.int32)
    data["fb_n_pitch"] = np.int32(N_PITCH)
    # the fixture stays hard: the rule changes velocities, threshold-equal velocities occur on sounding rows, D differs from "all held"
    c = data["fb_cases"]
    changed = 0
    for V, T, n, silent, has_vel, has_held, override, w_lo, r_lo, _ in c.tolist():
        if has_vel and override:
            changed += int(np.sum(data["fb_V"][r_lo:r_lo + n * T] != np.where(data["fb_idx"][r_lo:r_lo + n * T] < N_PITCH, data["fb_vel"][r_lo:r_lo + n * T], 0)))
    print("feedback: %d cases, %d rows, %d velocities changed by the rule" % (len(c), len(data["fb_idx"]), changed))
    assert changed >= 20
    return data


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    mfx._stub_modules()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings  # noqa: F401
    import vae_definition as vd
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions", "vae_definition"):
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)
    import midi_vae_amd  # noqa: F401
    from midi_vae_amd import longsongs as ls

    data = walks(ls)
    data.update(feedback(vd))
    path = os.path.join(HERE, "long_songs.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "long_songs.npz")
    print("wrote %s: %d bytes (largest other fixture: %d)" % (path, size, largest))
    assert size <= largest, "the fixture outgrew the largest one already there"


if __name__ == "__main__":
    main()
