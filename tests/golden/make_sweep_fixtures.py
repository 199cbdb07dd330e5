#!/usr/bin/env python3
"""Generate tests/golden/sweep_stats.npz: the latent sweep's window statistics and summaries from the reference's own functions.

Runs ONLY where the reference is present (make_fixtures.REF).  The reference's vae_evaluation.py is a script - it reads names nobody
defines and waits on input() - so it is never imported: the function definitions named in PINNED are picked out of its syntax tree
and executed in a namespace that holds NumPy, SciPy, the reference's data_class, the reference's settings values and a stand-in for
the three style classifiers (predict -> zeros; the '*style' keys they feed are dropped).  vae_definition.process_decoder_outputs -
imported with the stub modules of make_fixtures.py - turns ONE window at a time into the rolls those functions read, as the
reference's sweep does.  Only data is written: the inputs, the outputs and the settings.

  python tests/golden/make_sweep_fixtures.py

Windows: the shipped shape (T = 64 rows = 16 ticks x 4 voices, 60 pitch columns + the silent one, threshold 0.5, rules on), in groups
of K = 9 (one (sample, dimension) pair of a sweep): four groups from each of the four random-walk generators of the descriptor
fixture, then four hand-made groups - every window silent; no velocity above the threshold; a single window that is not empty
(one-element statistic lists: strength NaN); and one whose first window has a voice with previous pitch column 0 (the rule's
``previous_pitch > 0``).  Velocities are float32 in [0, 1], a third of them multiples of 1/8 (ties in the median); instrument
indices 0..15.  Per window the table holds the statistics of the reference's OWN lists, taken through NumPy as the reference takes
them (np.mean, np.median, np.std, ...).  Assertions keep the fixture from going soft: at least a quarter of the windows change
velocity between rules on and off, and even and odd list lengths both occur for each of the three medians.
"""
import ast
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402
from make_descriptor_fixtures import GENERATORS, random_walk_windows  # noqa: E402

PINNED = ("get_normal_distributed_values", "save_to_summary", "get_strength_probability_direction_for_value_list",
          "evaluate_statistic_value", "evaluate_count_of_values", "evaluate_change_of_values", "run_all_statistics",
          "evaluate_velocityroll", "evaluate_pitchroll", "evaluate_instrumentlist")
K, GROUPS_PER_GENERATOR = 9, 4
SWEEPS = ((1.0, 1.0, 5, True), (2.0, 0.5, 4, False))


class _Zeros:
    def predict(self, x):
        return np.zeros((len(x), 2))


def _pinned_namespace(settings, dc):
    import scipy
    import scipy.stats
    tree = ast.parse(open(os.path.join(mfx.REF, "vae_evaluation.py")).read())
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in PINNED]
    assert sorted(f.name for f in picked) == sorted(PINNED), [f.name for f in picked]
    ns = {k: getattr(settings, k) for k in dir(settings) if not k.startswith("__")}
    ns.update(np=np, scipy=scipy, data_class=dc, velocity_classifier_model=_Zeros(), pitches_classifier_model=_Zeros(),
              instrument_classifier_model=_Zeros())
    exec(compile(ast.Module(body=picked, type_ignores=[]), "<pinned>", "exec"), ns)
    return ns


def _row(values, counted=None):
    """count, mean, median, min, max, range, std (and the two specific counts) of one of the reference's lists, through NumPy"""
    values = list(values)
    row = [float(len(values))]
    row += ([np.mean(values), np.median(values), np.min(values), np.max(values), np.max(values) - np.min(values), np.std(values)]
            if values else [np.nan] * 6)
    if counted:
        row += [float(values.count(c)) for c in counted]
    return [float(v) for v in row]


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    mfx._stub_modules()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings
    import data_class as dc
    import vae_definition as vd
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions", "vae_definition"):
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)
    ns = _pinned_namespace(settings, dc)

    V, T, D, ID = int(settings.max_voices), int(settings.output_length), int(settings.output_dim), int(settings.meta_instrument_dim)
    thr = float(settings.velocity_threshold_such_that_it_is_a_played_note)
    s = dict(max_voices=V, low_crop=int(settings.low_crop), high_crop=int(settings.high_crop),
             include_silent_note=bool(settings.include_silent_note), velocity_threshold_such_that_it_is_a_played_note=thr,
             override_sampled_pitches_based_on_velocity_info=bool(settings.override_sampled_pitches_based_on_velocity_info),
             instrument_attach_method=str(settings.instrument_attach_method))
    n_pitch = s["high_crop"] - s["low_crop"]
    assert (T, V, D, n_pitch, ID, thr, s["include_silent_note"], s["override_sampled_pitches_based_on_velocity_info"],
            s["instrument_attach_method"]) == (64, 4, 61, 60, 16, 0.5, True, True, "1hot-category")
    assert settings.meta_instrument and settings.meta_velocity and not settings.meta_held_notes and not settings.meta_next_notes

    rng = np.random.default_rng(20261020)

    def velocities(n):
        v = rng.random((n, T))
        v = np.where(rng.random((n, T)) < 1 / 3, np.round(v * 8) / 8, v)
        return v.astype(np.float32)

    parts_idx, parts_vel = [], []
    for ps, ph in GENERATORS:
        parts_idx.append(random_walk_windows(rng, K * GROUPS_PER_GENERATOR, T, V, n_pitch, ps, ph))
        parts_vel.append(velocities(K * GROUPS_PER_GENERATOR))
    # every window silent
    parts_idx.append(np.full((K, T), n_pitch, np.uint8))
    parts_vel.append(velocities(K))
    # no velocity above the threshold
    parts_idx.append(random_walk_windows(rng, K, T, V, n_pitch, 0.3, 0.3))
    parts_vel.append((velocities(K) * np.float32(0.5)).astype(np.float32))
    # a single window that is not empty
    lone = np.full((K, T), n_pitch, np.uint8)
    lone[4] = random_walk_windows(rng, 1, T, V, n_pitch, 0.3, 0.3)[0]
    parts_idx.append(lone)
    parts_vel.append(velocities(K))
    # previous pitch column 0: voice 0 goes 0 -> 5 with a silent velocity (stays), voice 1 goes 3 -> 7 with one (inherits 0.8125)
    quirk_idx, quirk_vel = random_walk_windows(rng, K, T, V, n_pitch, 0.3, 0.3), velocities(K)
    quirk_idx[0, :2 * V] = [0, 3, n_pitch, n_pitch, 5, 7, n_pitch, n_pitch]
    quirk_vel[0, :2 * V] = [0.9375, 0.8125, 0.25, 0.25, 0.125, 0.1875, 0.25, 0.25]
    parts_idx.append(quirk_idx)
    parts_vel.append(quirk_vel)

    idx, vel = np.concatenate(parts_idx, 0), np.concatenate(parts_vel, 0)
    n = idx.shape[0]
    G = n // K
    assert n == G * K and vel.dtype == np.float32 and vel.min() >= 0 and vel.max() <= 1
    instr = rng.integers(0, ID, (n, V)).astype(np.uint8)
    instr[K:2 * K] = instr[K]                                   # one group without a change of instruments
    instr[2 * K:3 * K, 0] = np.arange(K) % 2 * 3                # and one whose first voice alternates piano / not

    def decode(w, override):
        vd.override_sampled_pitches_based_on_velocity_info = override
        onehot = np.zeros((1, T, D))
        onehot[0, np.arange(T), idx[w]] = 1
        I = np.zeros((1, V, ID))
        I[0, np.arange(V), instr[w]] = 1
        Y, I_pred, V_pred, _, _ = vd.process_decoder_outputs([onehot, I, vel[w].astype(np.float64).reshape(1, T, 1)], "argmax")
        vd.override_sampled_pitches_based_on_velocity_info = s["override_sampled_pitches_based_on_velocity_info"]
        return Y, I_pred, V_pred

    rolls_on = np.zeros((n, T))
    rolls_off = np.zeros((n, T))
    table = np.full((n, 22), np.nan)
    table[:, [0, 7, 8, 9]] = 0
    keys, group_of_key, numbers, programs = [], [], [], np.zeros((n, V), np.int64)
    recorded = {}
    run_all = ns["run_all_statistics"]

    def recording(list_of_lists, name, d):
        recorded[name] = [list(values) for values in list_of_lists]
        return run_all(list_of_lists, name, d)

    ns["run_all_statistics"] = recording
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)
    for g in range(G):
        Y_list, I_list, V_list = [], [], []
        for w in range(g * K, (g + 1) * K):
            Y, I_pred, V_pred = decode(w, True)
            rolls_on[w] = V_pred
            rolls_off[w] = decode(w, False)[2]
            Y_list.extend(Y)
            I_list.extend(I_pred)
            V_list.extend(V_pred)
            programs[w] = dc.instrument_representation_to_programs(I_pred[0], s["instrument_attach_method"])
        Y_list, I_list, V_list = np.asarray(Y_list), np.asarray(I_list), np.asarray(V_list)
        recorded.clear()
        summary = dict()
        summary.update(ns["evaluate_pitchroll"](Y_list))
        summary.update(ns["evaluate_velocityroll"](V_list))
        summary.update(ns["evaluate_instrumentlist"](I_list))
        for key, (strength, probability) in summary.items():
            if "style" in key:
                continue
            keys.append(key)
            group_of_key.append(g)
            numbers.append((float(strength), float(probability)))
        for k in range(K):
            w = g * K + k
            if "pitch" in recorded:
                table[w, 0:9] = _row([int(v) for v in recorded["pitch"][k]], counted=(35, 39))
            if "velocity" in recorded:
                table[w, 9:16] = _row([float(v) for v in recorded["velocity"][k]])
                table[w, 16:22] = _row([int(v) for v in recorded["note_starts"][k]])[1:]

    assert np.array_equal(rolls_on.astype(np.float32).astype(np.float64), rolls_on)          # input values and zeros: nothing rounds
    changed = np.any(rolls_on != rolls_off, axis=1)
    print("windows whose velocities change under the rules: %.1f %%" % (100 * changed.mean()))
    assert changed.mean() >= 0.25, "the fixture no longer exercises the velocity rules"
    assert rolls_on[n - K, V] == 0.125 and rolls_on[n - K, V + 1] == 0.8125, "the previous-pitch-0 window lost its point"
    for what, counts in (("pitch", table[:, 0]), ("velocity / note start", table[:, 9])):
        counts = counts[counts > 0]
        assert np.any(counts % 2 == 0) and np.any(counts % 2 == 1), "even and odd %s lists must both occur" % what
    per_group = [sum(1 for h in group_of_key if h == g) for g in range(G)]
    print("keys per group:", per_group)
    assert per_group[G - 4] == 2 and min(per_group[:G - 4]) == 24, per_group
    assert any(np.isnan(numbers[i][0]) for i in range(len(keys)) if group_of_key[i] == G - 2), "no one-element list in the lone group"

    out = dict(idx=idx, vel=vel, instr=instr, programs=programs, table=table, velocity_rules_on=rolls_on.astype(np.float32),
               velocity_rules_off=rolls_off.astype(np.float32), summary_key=np.array(keys), summary_group=np.array(group_of_key, np.int64),
               summary_value=np.array(numbers, np.float64), K=np.int64(K),
               **{"s_" + k: np.asarray(v) for k, v in s.items()})
    import scipy.stats
    for i, (stds, sigma, per_dim, both) in enumerate(SWEEPS):
        range_end = scipy.stats.norm.cdf(stds * sigma, loc=0.0, scale=sigma) - 0.5
        out["sweep_args_%d" % i] = np.array([stds, sigma, per_dim, both], np.float64)
        out["sweep_values_%d" % i] = np.array(ns["get_normal_distributed_values"](range_end, per_dim, sigma, both), np.float64)
    path = os.path.join(HERE, "sweep_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "windows:", n, "groups:", G, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
