"""The latent sweep's statistics without a device: the NumPy mirror and the host summaries of midi_vae_amd.sweep against the
reference's own outputs (tests/golden/sweep_stats.npz, written by tests/golden/make_sweep_fixtures.py), the third header's hygiene,
the layout of SweepArgs, and the refusals of mvae_sweep_windows as a table (tests/sweep_contract.py).

Bounds (derived, not measured).  Counts, min, max, range and the three medians are integers or input floats and one exact halving:
BIT-EQUAL.  Pitch and position means are an exact integer sum and one double division on both sides: bit-equal.  The velocity mean
is bit-equal HERE because the fixture's threshold is 0.5: every note-start velocity is a float32 in (0.5, 1], a multiple of 2^-24, and
at T <= 2^16 terms the partial sums stay below 2^16 - exact multiples of 2^-24 under 2^53 of them - so the double sum is exact in any
order, NumPy's pairwise one and the mirror's row order alike.  The three stds: integer sums or a two-pass sum against np.std, values
<= 64 (pitches, positions) or <= 1, at most 64 terms, 1.1e-16 relative a rounding: far under the descriptor tests' 1e-12 absolute.
The post-rule velocities are input values or zeros: bit-equal."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import sweep as sw
from tests import sweep_contract as sc
from tests.sweep_contract import STD_COLUMNS, assert_table, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


# ---- the mirror against the reference ------------------------------------------------------------------------------------------
def test_fixture_is_the_shipped_shape(fx):
    assert fx["idx"].shape == (180, 64) and fx["idx"].dtype == np.uint8 and fx["vel"].dtype == np.float32 and fx["K"] == 9
    assert fx["s"] == dict(max_voices=4, low_crop=24, high_crop=84, include_silent_note=True,
                           velocity_threshold_such_that_it_is_a_played_note=0.5, override_sampled_pitches_based_on_velocity_info=True,
                           instrument_attach_method="1hot-category")
    assert sw.params(fx["s"]) == dict(voices=4, n_pitch=60, silent=60, threshold=0.5, default_velocity=0.75, override=True,
                                      count_a=35, count_b=39)
    assert len(sw.COLUMNS) == 22 == sw.N_COLUMNS and len(set(sw.COLUMNS)) == 22


def test_mirror_table_and_velocities_are_the_reference(fx):
    table, roll = sw.window_statistics(fx["idx"], fx["vel"], fx["s"], device=False, return_velocity=True)
    assert roll.dtype == np.float32 and np.array_equal(roll.view(np.uint32), fx["velocity_rules_on"].view(np.uint32))
    assert_table(table, fx["table"], "mirror against the reference")
    off = dict(fx["s"], override_sampled_pitches_based_on_velocity_info=False)
    roll_off = sw.window_statistics(fx["idx"], fx["vel"], off, device=False, return_velocity=True)[1]
    assert np.array_equal(roll_off.view(np.uint32), fx["velocity_rules_off"].view(np.uint32))


def test_fixture_exercises_the_rules_and_the_medians(fx):
    changed = np.any(fx["velocity_rules_on"] != fx["velocity_rules_off"], axis=1)
    assert changed.mean() >= 0.25
    for column in (0, 9):
        counts = fx["table"][:, column]
        counts = counts[counts > 0]
        assert np.any(counts % 2 == 0) and np.any(counts % 2 == 1)
    K, n = fx["K"], fx["idx"].shape[0]
    silent, quiet, lone, quirk = (slice(n - (4 - i) * K, n - (3 - i) * K) for i in range(4))
    assert np.all(fx["table"][silent][:, [0, 9]] == 0) and np.all(np.isnan(fx["table"][silent][:, 1:7]))
    assert np.all(fx["table"][quiet][:, 9] == 0) and np.all(fx["table"][quiet][:, 0] > 0)
    assert (fx["table"][lone][:, 0] > 0).sum() == 1
    # previous pitch column 0: `previous_pitch > 0` leaves the silent velocity of voice 0, voice 1 (previous pitch 3) inherits
    w = quirk.start
    assert list(fx["idx"][w, [0, 1, 4, 5]]) == [0, 3, 5, 7]
    assert fx["velocity_rules_on"][w, 4] == fx["vel"][w, 4] == 0.125 and fx["velocity_rules_on"][w, 5] == fx["vel"][w, 1] == 0.8125


def test_mirror_without_a_velocity_head(fx):
    """every row has the default velocity, silent rows included, and no rule runs (reference vae_definition.py:1211-1213)"""
    idx = fx["idx"][:20]
    table, roll = sw.window_statistics(idx, None, fx["s"], device=False, return_velocity=True)
    assert np.all(roll == 0.75) and np.all(table[:, 9] == 64)
    assert np.all(table[:, 10:14] == 0.75) and np.all(table[:, 14:16] == 0)
    assert np.all(table[:, 16] == 31.5) and np.all(table[:, 17] == 31.5) and np.all(table[:, 18] == 0) and np.all(table[:, 19] == 63)
    with_head = sw.window_statistics(idx, fx["vel"][:20], fx["s"], device=False)
    assert np.array_equal(table[:, :9], with_head[:, :9], equal_nan=True)          # the pitch columns do not read the velocities


def test_inputs(fx):
    idx, vel = fx["idx"][:9], fx["vel"][:9]
    want = sw.window_statistics(idx, vel, fx["s"], device=False)
    assert np.array_equal(sw.window_statistics(np.eye(61)[idx], vel.astype(np.float64), fx["s"], device=False), want, equal_nan=True)
    with pytest.raises(ValueError):
        sw.window_statistics(idx[:, :63], vel[:, :63], fx["s"], device=False)
    with pytest.raises(ValueError):
        sw.window_statistics(idx, vel[:, :60], fx["s"], device=False)
    other = sw.window_statistics(idx, vel, fx["s"], device=False, counted=(0, 59))
    assert np.array_equal(np.delete(other, [7, 8], 1), np.delete(want, [7, 8], 1), equal_nan=True)
    on = idx.reshape(9, 16, 4)
    assert np.array_equal(other[:, 7], (on == 0).any(2).sum(1)) and np.array_equal(other[:, 8], (on == 59).any(2).sum(1))


# ---- the summaries against the reference ------------------------------------------------------------------------------------------
def _same_number(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def _reference_summaries(fx):
    G = fx["idx"].shape[0] // fx["K"]
    out = [dict() for _ in range(G)]
    for key, g, (strength, probability) in zip(fx["summary_key"].tolist(), fx["summary_group"].tolist(), fx["summary_value"].tolist()):
        out[g][key] = (strength, probability)
    return out


def _table_with_reference_stds(fx):
    """the mirror's table; its stds may differ from np.std by 1e-12 before they enter a strength, so the summaries are compared on
    the reference's stds (the comparison of the stds themselves is assert_table's)"""
    table = sw.window_statistics(fx["idx"], fx["vel"], fx["s"], device=False)
    assert_table(table, fx["table"], "mirror")
    table[:, STD_COLUMNS] = fx["table"][:, STD_COLUMNS]
    return table


def test_summarize_is_the_reference(fx):
    K, table = fx["K"], _table_with_reference_stds(fx)
    programs = sw.programs_of(fx["instr"], fx["s"]["instrument_attach_method"])
    assert np.array_equal(programs, fx["programs"])
    want = _reference_summaries(fx)
    sizes = set()
    for g, ref in enumerate(want):
        got = sw.summarize_sweep(table[g * K:(g + 1) * K][None, None], programs[g * K:(g + 1) * K][None, None])[0][0][0]
        assert set(got) == set(ref), (g, sorted(set(got) ^ set(ref)))
        assert not any("style" in key for key in got)
        for key in ref:
            assert _same_number(got[key][0], ref[key][0]) and _same_number(got[key][1], ref[key][1]), (g, key, got[key], ref[key])
        sizes.add(len(got))
    assert sizes == {2, 11, 24}          # instruments only; no note start; everything
    lone = want[len(want) - 2]
    assert sum(np.isnan(v[0]) for v in lone.values()) >= 12          # one-element lists: strength NaN, probability 0


@pytest.mark.parametrize("K", [1, 2, 5, 9, 17, 40])
def test_summarize_sweep_is_summarize_of_every_pair(K):
    """the batched form against the one-pair form (which test_summarize_is_the_reference pins), bit for bit: tables of random numbers
    with empty windows, pairs without any pitch or note start, ties and exact steps; K = 17 and 40 make NumPy sum pairwise"""
    rng = np.random.default_rng(K)
    n, Z, V = 3, 40, 4
    table = rng.standard_normal((n, Z, K, 22)) * rng.choice([1.0, 1e-3, 1e3], (n, Z, 1, 22))
    table[..., [0, 7, 8, 9]] = rng.integers(0, 4, (n, Z, K, 4))
    table[:, ::7, :, 0] = 0
    table[:, 3::9, :, 9] = 0
    table[:, 1::5, :, 1:7] = np.round(table[:, 1::5, :, 1:7])
    for base in (0, 9):
        empty = table[..., base] == 0
        table[..., base + 1:base + 7][empty] = np.nan
        if base == 9:
            table[..., 16:22][empty] = np.nan
    programs = rng.integers(0, 3, (n, Z, K, V)) * 8
    programs[:, ::4] = programs[:, ::4, :1]
    summaries, infl, peaked, best = sw.summarize_sweep(table, programs)
    assert len(summaries) == n and all(len(row) == Z for row in summaries)
    sizes = set()
    for i in range(n):
        for d in range(Z):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = sw.summarize(table[i, d], programs[i, d])
            got = summaries[i][d]
            assert list(got) == list(want), (i, d)
            for key in want:
                assert _same_number(got[key][0], want[key][0]) and _same_number(got[key][1], want[key][1]), (i, d, key, got[key], want[key])
            sizes.add(len(got))
    assert len(sizes) >= 3
    again = sw.influence(summaries)
    assert set(again[0]) == set(infl) and again[1] == peaked and again[2] == best


def test_strength_probability_direction():
    assert sw.strength_probability_direction([]) == (0.0, 0.0, "ascending")
    one = sw.strength_probability_direction([3.5])
    assert np.isnan(one[0]) and one[1:] == (0, "ascending")
    assert sw.strength_probability_direction([1, 2, 4]) == (1.5, 1.0, "ascending")
    assert sw.strength_probability_direction([4, 2, 1]) == (1.5, 1.0, "descending")
    assert sw.strength_probability_direction([5, 1, 1, 2, 0]) == (1.25, 0.75, "descending")          # read backwards: 0 2 1 1 5
    assert sw.strength_probability_direction([2, 2]) == (0.0, 1.0, "ascending")


def test_influence(fx):
    """the reference's loops (:1189-1213) written out on two samples x ten dimensions of the fixture's groups"""
    ref = _reference_summaries(fx)
    summaries = [ref[:10], ref[10:20]]
    infl, peaked, best = sw.influence(summaries)
    sums, peak = [dict() for _ in range(10)], {}
    for per_dim in summaries:
        for dim, d in enumerate(per_dim):
            for key, (strength, probability) in d.items():
                sums[dim][key] = sums[dim].get(key, 0.0) + strength * probability
        for dim, d in enumerate(per_dim):
            for key, (strength, probability) in d.items():
                if key not in peak or (strength >= peak[key][0] and probability >= peak[key][1]):
                    peak[key] = (strength, probability, dim)
    assert set(infl) == set(peak) == set(peaked) == set(best) and len(peak) > 24
    for key in peak:
        want = np.array([sums[dim].get(key, 0.0) for dim in range(10)])
        assert infl[key].shape == (10,) and np.array_equal(infl[key], want, equal_nan=True), key
        assert peaked[key] == peak[key][2] and best[key] == int(np.argmax(want)), key
    assert any(np.isnan(v).any() for v in infl.values()) and len(set(peaked.values())) > 1
    assert sw.influence([]) == ({}, {}, {})


def test_sweep_values(fx):
    for i in range(2):
        stds, sigma, per_dim, both = fx["sweep_args_%d" % i].tolist()
        got = sw.sweep_values(stds, sigma, int(per_dim), bool(both))
        want = fx["sweep_values_%d" % i]
        assert len(got) == len(want) == (2 * int(per_dim) - 1 if both else int(per_dim)) and got == sorted(got)
        assert np.abs(np.asarray(got) - want).max() <= 1e-12
        assert 0.0 in got
    assert len(sw.sweep_values()) == 9


# ---- the third header ------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_sweep.h")
    assert declared == {"mvae_sweep_abi_version", "mvae_sweep_windows"} == set(hl.SWEEP_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert name not in hl.SIGNATURES and name not in hl.DESC_SIGNATURES
        assert name not in _declared("midivae_hip.h") and name not in _declared("midivae_descriptors.h")
    assert _declared("midivae_descriptors.h") == {"mvae_desc_abi_version", "mvae_desc_windows"} == set(hl.DESC_SIGNATURES)
    assert _declared("midivae_hip.h") == set(hl.SIGNATURES)
    assert lib.mvae_sweep_abi_version() == 1 == hl.SWEEP_ABI_VERSION
    assert lib.mvae_desc_abi_version() == 1 == hl.DESC_ABI_VERSION
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_sweep.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_sweep_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_sweep_args, %s));' % (f, f) for f, _ in hl.SweepArgs._fields_]
    lines += ['printf("MVAE_SWEEP_COLUMNS %d\\n", (int)MVAE_SWEEP_COLUMNS);', 'printf("MVAE_SWEEP_MAX_T %d\\n", (int)MVAE_SWEEP_MAX_T);',
              'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.SweepArgs) and ctypes.sizeof(hl.SweepArgs) % 8 == 0
    for f, _ in hl.SweepArgs._fields_:
        assert int(got[f]) == getattr(hl.SweepArgs, f).offset, f
    assert int(got["MVAE_SWEEP_COLUMNS"]) == sw.N_COLUMNS and int(got["MVAE_SWEEP_MAX_T"]) == sw.MAX_T >= 4096 * 8


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_sweep_stats_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert sc.invoke(lib, sc.baseline(sc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in sc.ACCEPTED:
        assert sc.invoke(lib, mutate(sc.baseline(sc.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("row", sc.ROWS, ids=[r[0] for r in sc.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = sc.invoke(hl.load(), mutate(sc.baseline(sc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_covers_every_documented_limit():
    names = " | ".join(r[0] for r in sc.ROWS)
    for what in ("a NULL", "idx NULL", "both outputs NULL", "n = 0", "T = 0", "n_pitch = 0", "stride_t = 0", "stride_w = -1", "voices = 1",
                 "voices = 9", "T % voices", "ld_out = 21", "silent = 256", "silent = -2", "count_a = 256", "count_a = -1", "count_b = 256",
                 "count_b = -1", "override_rules = 2", "override_rules = -1", "threshold = nan", "threshold = inf", "n_pitch = 193",
                 "T = 65536 + 4"):
        assert what in names, what
    assert len([r for r in sc.ROWS if r[3]]) >= 8
