"""Style-transfer scoring without a device: the NumPy mirror of midi_vae_amd.style against the reference's own ensemble and a
restatement of its per-song counters (tests/golden/style_scores.npz, written by tests/golden/make_style_fixtures.py), the seventh
header's hygiene, the layout of StyleArgs, the refusals of mvae_style_scores as a table (tests/style_contract.py), and the builders
of the switched songs.

Bounds (derived, not measured).  The ensemble is the reference's expression evaluated by the same NumPy on the same float32 tables:
BIT-EQUAL.  Argmaxes are np.argmax on those bits: equal.  Accuracies are one integer count divided once in double on both sides:
bit-equal.  Confusion counts are integers: equal.  Confidences: the installed NumPy (2.x) accumulates the reference's ``+=`` on
float32 scalars in float32, the NumPy of the reference's day widened to double; this project defines double, and the mirror's
math.fsum is the exactly rounded sum.  Sequential float32 summation of n terms in [0, 1] rounds n - 1 times (0.0 + x is exact), each
time by at most 2^-24 of a partial sum, and no partial sum exceeds the total n * mean: the recorded mean is within
(n - 1) * 2^-24 * mean of the exact one before its float32 division adds 2^-24 * mean - together n * 2^-24 * mean, which is inside
(n - 1) * 2^-24 wherever mean <= (n - 1) / n.  The test checks that the fixture's groups are such (a one-window group is exact:
x / 1) and prints the largest difference."""
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
from midi_vae_amd import style as st
from tests import style_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    fx = sc.load_fixture()
    for f in fx.values():
        f["mirror"] = sc.mirror_of(f)
    return fx


# ---- the mirror against the reference ------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises(cases):
    a, b = cases["a"], cases["b"]
    assert a["p_pitch"].shape == (330, 2) and b["p_pitch"].shape == (70, 3) and b["p_instr"].shape == (7, 3)
    assert a["instr_row"] is None and b["instr_row"].dtype == np.int32 and list(np.unique(b["instr_row"])) == [0, 1, 3, 4, 5, 6]
    assert list(np.diff(a["group_off"])) == [300, 0, 1, 12, 9, 8] and list(np.diff(b["group_off"])) == [20, 1, 0, 17, 22, 7, 3]
    assert a["weights"] == (0.999 - 0.5,) * 3 == st.DEFAULT_WEIGHTS and b["weights"] == (0.999 - 0.5, 0.3, 0.2)
    for fx in (a, b):
        assert all(fx[k].dtype == np.float32 for k in ("p_pitch", "p_vel", "p_instr", "ensemble")) and fx["cls"].dtype == np.uint8
        assert (fx["cls"] == 255).any() and (fx["count"] == 0).any() and (fx["count"] == 1).any() and fx["fma_rows"] >= 10 and fx["halfway_rows"] >= 10
    assert a["count"][0] > 256 and b["count"][6] == 0 and b["count"][2] == 0
    assert st.COLUMNS[0] == "count" and st.COLUMNS[7:] == ("ensemble_accuracy", "ensemble_confidence") and st.N_COLUMNS == 9


@pytest.mark.parametrize("case", ["a", "b"])
def test_mirror_is_the_reference(cases, case):
    fx = cases[case]
    got = fx["mirror"]
    assert got["ensemble"].dtype == np.float32 and np.array_equal(got["ensemble"].view(np.uint32), fx["ensemble"].view(np.uint32))
    assert got["pred"].dtype == np.uint8 and np.array_equal(got["pred"], fx["pred"])
    assert np.array_equal(got["table"][:, 0], fx["count"].astype(np.float64))
    assert sc.same_bits(got["table"][:, 1::2], fx["accuracy"])
    assert got["confusion"].dtype == np.int32 and np.array_equal(got["confusion"], fx["confusion"])
    assert got["confusion"].sum() == 4 * fx["count"].sum()
    conf = got["table"][:, 2::2]
    assert np.array_equal(np.isnan(conf), np.isnan(fx["confidence"]))
    worst = 0.0
    for g, n_g in enumerate(fx["count"].tolist()):
        for j in range(4):
            if n_g:
                assert n_g == 1 or conf[g, j] <= (n_g - 1) / n_g          # where the derivation of the bound applies
                diff = abs(conf[g, j] - fx["confidence"][g, j])
                worst = max(worst, diff)
                assert diff <= (n_g - 1) * 2.0 ** -24, (g, j, n_g, conf[g, j], fx["confidence"][g, j])
    print("case %s: largest difference between the fsum mean and the float32-accumulated mean: %.3g" % (case, worst))


def test_a_song_judged_once_reports_its_single_prediction(cases):
    """case b: one instrument row per song.  The reference does not divide its figures (:2151); the mean of n copies of a float32
    is that float32 (n * x is exact in double), and the accuracy is 0 or 1"""
    fx = cases["b"]
    table = fx["mirror"]["table"]
    for g in np.nonzero(fx["count"])[0]:
        k = fx["song_class"][g]
        assert table[g, 6] == float(fx["p_instr"][g, k]) and table[g, 5] == float(np.argmax(fx["p_instr"][g]) == k)


def test_ensemble_prediction_steps():
    """every product, sum and the division is its own float32 rounding - which is not the same as rounding once"""
    w = (0.499, 0.3, 0.2)
    rng = np.random.default_rng(3)
    t = rng.random((3, 50, 4)).astype(np.float32)
    want = ((t[0] * np.float32(w[0]) + t[1] * np.float32(w[1])) + t[2] * np.float32(w[2])) / np.float32(w[0] + w[1] + w[2])
    assert np.array_equal(st.ensemble_prediction(t[0], t[1], t[2], w).view(np.uint32), want.view(np.uint32))
    in_double = ((t[0].astype(np.float64) * w[0] + t[1] * w[1] + t[2] * w[2]) / sum(w)).astype(np.float32)
    assert (in_double != want).any()          # rounding every step in float32 is not rounding once


def test_mirror_edges():
    rng = np.random.default_rng(5)
    n, C = 12, 4
    p = rng.random((3, n, C)).astype(np.float32)
    p[0, 2] = [0.25, 0.5, 0.5, 0.125]                 # the first maximum wins
    p[0, 3] = [0.25, np.nan, 0.9, np.nan]             # the first NaN wins
    cls = (np.arange(n) % C).astype(np.uint8)
    cls[5], cls[6] = 255, C                           # left out: 255, and a class that does not exist
    off = np.array([0, 4, 4, n])
    rows = np.arange(n, dtype=np.int32)
    rows[1], rows[8] = -1, n                          # out of range: never read
    got = st.scores(p[0], p[1], p[2], cls, off, rows, (1.0, 2.0, 3.0), device=False)
    assert got["pred"][2, 0] == 1 and got["pred"][3, 0] == 1
    assert list(got["pred"][1, 2:]) == [255, 255] and list(got["pred"][8, 2:]) == [255, 255] and np.all(np.isnan(got["ensemble"][[1, 8]]))
    assert list(got["table"][:, 0]) == [4, 0, 6] and np.all(np.isnan(got["table"][1, 1:]))
    assert np.all(np.isnan(got["table"][[0, 2]][:, [6, 8]])) and not np.any(np.isnan(got["table"][[0, 2]][:, [1, 3, 5, 7]]))
    assert np.isnan(got["table"][0, 2]) and not np.isnan(got["table"][2, 2])          # window 3 of group 0 is scored on class 3: NaN
    assert got["confusion"][0].sum() == 10 and got["confusion"][2].sum() == 8 == got["confusion"][3].sum()
    alone = st.scores(None, p[1], None, cls, off, device=False)
    assert alone["ensemble"] is None and np.all(alone["pred"][:, [0, 2, 3]] == 255) and np.all(np.isnan(alone["table"][:, [1, 2, 5, 6, 7, 8]]))
    assert np.array_equal(alone["table"][:, [0, 3, 4]], got["table"][:, [0, 3, 4]], equal_nan=True)
    assert alone["confusion"][[0, 2, 3]].sum() == 0 and np.array_equal(alone["confusion"][1], got["confusion"][1])
    for bad in (dict(weights=(1.0, float("nan"), 1.0)), dict(weights=(1.0, -1.0, 0.0)), dict(weights=(1.0, 1.0))):
        with pytest.raises(ValueError):
            st.scores(p[0], p[1], p[2], cls, off, device=False, **bad)
    with pytest.raises(ValueError):
        st.scores(None, None, None, cls, off, device=False)
    with pytest.raises(ValueError):
        st.scores(p[0], p[1][:, :3], p[2], cls, off, device=False)
    with pytest.raises(ValueError):
        st.scores(p[0], p[1], p[2], cls, np.array([0, 5, 4, n]), device=False)
    with pytest.raises(ValueError):
        st.scores(p[0][:, :1], None, None, cls, off, device=False)


# ---- the sweep's summaries with the judges' columns -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 5, 17])
def test_sweep_summaries_with_style_columns(K):
    """summarize / summarize_sweep with ``style``: the three keys of vae_evaluation.py:1035-1039, :1089-1093, :1105-1109 - the pitch
    key only where some window has a pitch, the velocity key only where some has a note start, the instrument key always; a NaN
    column (no such judge) adds nothing; without ``style`` both are what they were"""
    import warnings
    from midi_vae_amd import sweep as sw
    rng = np.random.default_rng(K)
    n, Z, V = 2, 12, 4
    table = rng.standard_normal((n, Z, K, 22))
    table[..., [0, 7, 8, 9]] = rng.integers(0, 4, (n, Z, K, 4))
    table[:, ::5, :, 0] = 0
    table[:, 2::4, :, 9] = 0
    for base in (0, 9):
        empty = table[..., base] == 0
        table[..., base + 1:base + 7][empty] = np.nan
        if base == 9:
            table[..., 16:22][empty] = np.nan
    programs = rng.integers(0, 3, (n, Z, K, V)) * 8
    style = rng.random((n, Z, K, 3)).astype(np.float32)
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a == b
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = sw.summarize_sweep(table, programs)
        for st_in, absent in ((style, ()), (np.where(np.arange(3) == 1, np.nan, style), ("velocitystyle",))):
            summaries, infl, peaked, best = sw.summarize_sweep(table, programs, style=st_in)
            for i in range(n):
                for d in range(Z):
                    got, want = summaries[i][d], sw.summarize(table[i, d], programs[i, d], style=st_in[i, d])
                    assert list(got) == list(want) and all(same(got[k][0], want[k][0]) and same(got[k][1], want[k][1]) for k in want), (i, d)
                    rest = {k: v for k, v in got.items() if "style" not in k}
                    before = sw.summarize(table[i, d], programs[i, d])
                    assert list(rest) == list(before) == list(plain[0][i][d]), (i, d)
                    assert all(same(rest[k][0], before[k][0]) and same(rest[k][1], before[k][1]) for k in before), (i, d)
                    names = {k.split("_")[1] for k in got if "style" in k}
                    expect = {"instrumentstyle"} | ({"pitchstyle"} if (table[i, d, :, 0] > 0).any() else set())
                    expect |= {"velocitystyle"} if (table[i, d, :, 9] > 0).any() else set()
                    assert names == expect - set(absent), (i, d, names)
            assert any("style" in k for k in infl) and set(best) == set(infl)
    # one pair by hand: the list is the K class-0 probabilities themselves (the mean of a one-element list)
    key = [k for k in summaries[0][1] if "instrumentstyle" in k][0]
    want = sw.strength_probability_direction(st_in[0, 1, :, 2].astype(np.float64).tolist())
    assert key == "mean_instrumentstyle_" + want[2] and same(summaries[0][1][key][0], want[0]) and same(summaries[0][1][key][1], want[1])


# ---- the switched songs' builders --------------------------------------------------------------------------------------------------
def test_switched_latents_and_instrument_matrix_follow_the_reference():
    """a restatement of vae_evaluation.py:2451-2452, :2460, :2471-2478, :2550 and :2608-2619 on a 3-class toy"""
    rng = np.random.default_rng(9)
    num_classes, latent_dim = 3, 6
    classes = [2, 0, 1, 0]
    songs = [rng.standard_normal((m, latent_dim)) for m in (3, 1, 4, 2)]
    programs = [[0, 8, 40, 127], [0, 0, 0, 0], [24, 25, 26, 27], [56, 57, 0, 8]]
    pairs = st.switch_pairs(classes, num_classes)
    want_pairs, want_matrix = [], np.zeros((num_classes, num_classes, 16, 16))
    voted = {}
    for song, (encoded_representation, C) in enumerate(zip(songs, classes)):
        for C_switch in range(num_classes):
            if C != C_switch:
                want_pairs.append((song, C, C_switch))
                previous_switched_rep = np.zeros((1, latent_dim))
                reps, hists = [], []
                for i in range(len(encoded_representation)):
                    original_rep = encoded_representation[i]
                    switched_rep = np.copy(original_rep)
                    switched_rep[C] = original_rep[C_switch]
                    switched_rep[C_switch] = original_rep[C]
                    switched_rep = np.asarray([switched_rep])
                    reps.append(switched_rep[0])
                    hists.append(previous_switched_rep[0])
                    previous_switched_rep = switched_rep
                got_z, got_h = st.switched_latents(encoded_representation, C, C_switch)
                assert np.array_equal(got_z, np.asarray(reps)) and np.array_equal(got_h, np.asarray(hists))
                switched_programs_for_whole_song = [int(v) for v in rng.integers(0, 128, 4)] if (song + C_switch) % 2 else list(programs[song])
                voted[(song, C_switch)] = switched_programs_for_whole_song
                for program, switched_program in zip(programs[song], switched_programs_for_whole_song):
                    want_matrix[C, C_switch, program // 8, switched_program // 8] += 1
    assert pairs == want_pairs and len(pairs) == 8
    switched = [voted[(song, t)] for song, _, t in pairs]
    got = st.switch_instruments_matrix(pairs, programs, switched, num_classes)
    assert got.shape == (3, 3, 16, 16) and np.array_equal(got, want_matrix) and got.sum() == 32
    for (song, C, t), sp in zip(pairs, switched):
        flag, used = st.instruments_switched(programs[song], sp)
        assert flag == (sp != programs[song]) and used == (sp if flag else programs[song])
        assert st.instruments_switched(programs[song], sp, meta_instrument=False) == (False, programs[song])
    z = songs[0]
    assert np.array_equal(st.switched_latents(st.switched_latents(z, 2, 0)[0], 0, 2)[0], z)


# ---- the seventh header -----------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_style.h")
    assert declared == {"mvae_style_abi_version", "mvae_style_scores"} == set(hl.STYLE_SIGNATURES)
    others = [sig for _, _, _, sig in hl.HEADERS if sig is not hl.STYLE_SIGNATURES]
    assert len(hl.HEADERS) == 7 and hl.HEADERS[-1][1:] == ("mvae_style_abi_version", 1, hl.STYLE_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert not any(name in sig for sig in others) and name not in _declared("midivae_hip.h")
    assert lib.mvae_style_abi_version() == 1 == hl.STYLE_ABI_VERSION
    # the other versions do not move with this header
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION
    assert [lib.mvae_desc_abi_version(), lib.mvae_sweep_abi_version(), lib.mvae_recon_abi_version(), lib.mvae_events_abi_version(),
            lib.mvae_import_abi_version()] == [1, 1, 1, 1, 1]


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_style.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_style_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_style_args, %s));' % (f, f) for f, _ in hl.StyleArgs._fields_]
    lines += ['printf("%s %%d\\n", (int)%s);' % (c, c) for c in ("MVAE_STYLE_COLUMNS", "MVAE_STYLE_JUDGES", "MVAE_STYLE_MIN_CLASSES",
                                                                  "MVAE_STYLE_MAX_CLASSES", "MVAE_STYLE_LANES")]
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.StyleArgs) and ctypes.sizeof(hl.StyleArgs) % 8 == 0
    for f, _ in hl.StyleArgs._fields_:
        assert int(got[f]) == getattr(hl.StyleArgs, f).offset, f
    assert int(got["MVAE_STYLE_COLUMNS"]) == st.N_COLUMNS and int(got["MVAE_STYLE_JUDGES"]) == len(st.JUDGES)
    assert (int(got["MVAE_STYLE_MIN_CLASSES"]), int(got["MVAE_STYLE_MAX_CLASSES"])) == (st.MIN_CLASSES, st.MAX_CLASSES) == (2, 64)
    assert int(got["MVAE_STYLE_LANES"]) == 256


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_style_scores_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert sc.invoke(lib, sc.baseline(sc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in sc.ACCEPTED:
        assert sc.invoke(lib, mutate(sc.baseline(sc.fake_alloc))) == hl.E_LAUNCH, name
    big = sc.S(C=64, ld_pitch=64, ld_vel=64, ld_instr=64, ld_ens=64)
    assert sc.invoke(lib, big(sc.baseline(sc.fake_alloc))) == hl.E_LAUNCH


@no_device
@pytest.mark.parametrize("row", sc.ROWS, ids=[r[0] for r in sc.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = sc.invoke(hl.load(), mutate(sc.baseline(sc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_covers_every_documented_limit():
    names = " | ".join(r[0] for r in sc.ROWS)
    for what in ("a NULL", "all three tables NULL", "all outputs NULL", "ens_out without p_pitch", "ens_out without p_vel",
                 "ens_out without p_instr", "n = 0", "n = -1", "n_groups = 0", "cls NULL", "group_off NULL", "ld_pitch = C - 1",
                 "ld_vel = C - 1", "ld_instr = 0", "ld_ens = C - 1", "ld_table = 8", "n_instr_rows = 0", "weight 0 = nan", "weight 1 = inf",
                 "weight sum = 0", "weight sum < 0", "C = 1", "C = 65"):
        assert what in names, what
    assert len([r for r in sc.ROWS if r[3]]) >= 20
