"""Long songs without a device: the NumPy mirrors of midi_vae_amd.longsongs against tests/golden/long_songs.npz - the reference's
restated search loop and its own process_decoder_outputs / prepare_encoder_input_list - the Python-side argument checks, the ninth
header's hygiene and, where no device is visible, the refusals of both entry points on addresses nothing maps.

Nothing here has a tolerance: picked indices are integers, the pull is NumPy's own separately rounded steps, the feedback's velocities
are input values and zeros."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import generation as gen
from midi_vae_amd import hiplib as hl
from midi_vae_amd import longsongs as ls
from midi_vae_amd.model import Decoder
from tests import longsong_contract as lc

ROOT = lc.ROOT
WALKS, FEEDBACK = lc.load_fixture()


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases_it_promises():
    assert sorted(WALKS) == sorted(["n1", "runout", "dups", "zero", "z1", "z3", "z256", "z257", "n63", "n64", "n65", "n255", "n256", "n257",
                                    "s7", "s8", "s9", "n3000"])
    assert all(sorted(fx) == sorted(lc.WALK_KEYS) for fx in WALKS.values())
    assert WALKS["n1"]["all_z"].shape[0] == 1 and np.all(WALKS["n1"]["picked"] == 0)
    assert WALKS["runout"]["picked"].tolist() == [[0, 1, 2, 3, 4, 0, 0, 0], [3, 4, 2, 1, 0, 0, 0, 0]]
    assert WALKS["dups"]["picked"][0].tolist() == [0, 1, 6, 8, 3, 7]          # rows 6 and 8 repeat row 1, row 7 repeats row 3
    assert WALKS["zero"]["picked"][0].tolist() == [0, 0, 0, 3, 0]             # index 0: picked before, nearest again
    assert {fx["all_z"].shape[1] for fx in WALKS.values()} >= {1, 3, 256, 257}
    assert {fx["start"].shape[0] for fx in WALKS.values()} >= {1, 2, 7, 8, 9, 17}
    assert {fx["all_z"].shape[0] for fx in WALKS.values()} >= {ls.ROW_CHUNK - 1, ls.ROW_CHUNK, ls.ROW_CHUNK + 1, 3000}
    assert max(fx["picked"].max() for fx in WALKS.values()) == 2999
    for fx in WALKS.values():
        assert fx["all_z"].dtype == np.float32 and fx["start"].dtype == np.float64 and fx["script"].dtype == np.float32
        assert fx["e"].dtype == np.float32 and float(fx["den"]) == float(1 + fx["e"])
    assert len(FEEDBACK) == 63
    assert {(c["voices"], c["T"] // c["voices"]) for c in FEEDBACK} == {(v, k) for v in (2, 4, 8) for k in (1, 3, 16)}
    assert {(c["silent"], c["has_vel"], c["has_held"], c["override"]) for c in FEEDBACK} >= {
        (True, True, False, True), (False, True, True, False), (True, False, True, True), (False, False, False, False),
        (True, True, True, True), (False, True, False, True), (True, True, False, False)}
    assert any(np.all(c["idx"][-1] == c["n_pitch"]) for c in FEEDBACK)                          # a window that is all silent
    assert any(np.any(c["vel"][c["idx"] < c["n_pitch"]] == np.float32(c["threshold"])) for c in FEEDBACK)
    assert any(c["idx"][0, 0] == 0 and c["has_vel"] and c["override"] for c in FEEDBACK)          # the previous_pitch > 0 quirk


@pytest.mark.parametrize("name", sorted(WALKS))
def test_the_walk_mirror_is_the_reference(name):
    """all songs of a case at once, iteration by iteration: picked indices equal, pulled codes bit-equal in both precisions"""
    fx = WALKS[name]
    S, L = fx["picked"].shape
    picked = np.zeros((S, 0), np.int64)
    for it in range(L):
        R = lc.walk_inputs(fx, it)
        got = ls.nearest_walk(fx["all_z"], R, picked, fx["e"], device=False)
        assert got["best"].dtype == np.int32 and np.array_equal(got["best"], fx["picked"][:, it]), (name, it)
        assert got["r"].dtype == R.dtype and lc.same_bits(got["z"], fx["z"][:, it]), (name, it)
        if it == 0:
            assert lc.same_bits(got["r"], fx["r0"])
        else:
            assert lc.same_bits(got["r"], fx["z"][:, it])
        np.testing.assert_allclose(got["distances"], fx["dist"][:, it], rtol=1e-5, atol=0)
        picked = got["picked"]
        # den as the caller formed it is the same call
        again = ls.nearest_walk(fx["all_z"], R, picked[:, :it], float(fx["e"]), device=False, den=float(fx["den"]))
        assert np.array_equal(again["best"], got["best"]) and lc.same_bits(again["r"], got["r"])
    assert np.array_equal(picked, fx["picked"])


@pytest.mark.parametrize("name", ["runout", "dups", "zero", "z257", "n257"])
def test_walk_reference_is_nearest_walk_iteration_by_iteration(name):
    fx = WALKS[name]
    S, L = fx["picked"].shape
    for s in range(S):
        script = fx["script"][s]
        ref = ls.walk_reference(fx["all_z"], fx["start"][s], L, fx["e"], step=lambda it, R, prev: script[it] if it < L - 1 else R)
        picked = np.zeros((1, 0), np.int64)
        for it in range(L):
            got = ls.nearest_walk(fx["all_z"], lc.walk_inputs(fx, it)[s:s + 1], picked, fx["e"], device=False)
            picked = got["picked"]
            assert lc.same_bits(got["r"], ref["rows"][it])
        assert np.array_equal(picked[0], ref["picked"]) and np.array_equal(ref["picked"], fx["picked"][s])
        assert lc.same_bits(ref["z"], fx["z"][s])
    # without a step the pulled code goes on, and the history the step sees is the code pulled one iteration earlier
    seen = []
    free = ls.walk_reference(fx["all_z"], fx["start"][0], 3, fx["e"], step=lambda it, R, prev: (seen.append(prev.copy()), R)[1])
    plain = ls.walk_reference(fx["all_z"], fx["start"][0], 3, fx["e"])
    assert np.array_equal(free["picked"], plain["picked"]) and lc.same_bits(free["z"], plain["z"])
    assert not seen[0].any() and np.array_equal(seen[1], free["rows"][0]) and np.array_equal(seen[2], free["rows"][1])


def test_nan_and_infinite_distances():
    """a NaN distance never wins against another candidate; a NaN at index 0 keeps the walk there, as the reference's loop does"""
    all_z = np.array([[0, 0], [1, 1], [np.nan, 0], [0.5, 0.5]], np.float32)
    R = np.array([[0.9, 0.9]], np.float32)
    got = ls.nearest_walk(all_z, R, np.zeros((1, 0)), 0.5, device=False)
    assert got["best"][0] == 1
    got = ls.nearest_walk(all_z, R, [[1, 3]], 0.5, device=False)
    assert got["best"][0] == 0 and np.isfinite(got["distances"][0])          # row 2 is the only other candidate, and it is NaN
    swapped = all_z[[2, 1, 0, 3]]
    got = ls.nearest_walk(swapped, R, np.zeros((1, 0)), 0.5, device=False)
    ref = ls.walk_reference(swapped, R[0], 1, np.float32(0.5))
    assert got["best"][0] == 0 == ref["picked"][0] and np.isnan(got["distances"][0]) and np.isnan(got["z"]).any()
    far = np.array([[np.inf, 0], [np.inf, -np.inf]], np.float32)
    got = ls.nearest_walk(far, np.zeros((1, 2), np.float32), np.zeros((1, 0)), 0.5, device=False)
    assert got["best"][0] == 0 and np.isinf(got["distances"][0])              # an equal later distance never replaces an earlier one


def test_the_python_side_checks():
    all_z = np.zeros((4, 3), np.float32)
    R = np.zeros((2, 3))
    ok = ls.nearest_walk(all_z, R, np.zeros((2, 0)), 0.5, device=False)
    assert ok["picked"].shape == (2, 1) and ok["z"].dtype == np.float32 and ok["r"].dtype == np.float64
    for bad in (dict(all_z=all_z.astype(np.float64)), dict(all_z=all_z[:0]), dict(all_z=all_z[0]), dict(R=R[:, :2]), dict(R=R[0]),
                dict(R=R[:0]), dict(picked=[[4], [0]]), dict(picked=[[-1], [0]]), dict(e=float("nan")), dict(e=float("inf")), dict(e=-1.0),
                dict(all_z=np.zeros((2, 4097), np.float32), R=np.zeros((1, 4097)))):
        kw = dict(dict(all_z=all_z, R=R, picked=np.zeros((2, 0)), e=0.5), **bad)
        with pytest.raises(ValueError):
            ls.nearest_walk(kw["all_z"], kw["R"], kw["picked"], kw["e"], device=False)
    with pytest.raises(ValueError):
        ls.nearest_walk(all_z, R, np.zeros((2, 0)), 0.5, device=False, den=0.0)
    assert ls.pull_factors(np.float32(0.3)) == (float(np.float32(0.3)), float(1 + np.float32(0.3)))
    assert ls.pull_factors(0.3) == (0.3, 1.3)
    c = FEEDBACK[0]
    s = lc.feedback_settings(c)
    with pytest.raises(ValueError):
        ls.feedback_rows(c["idx"][:, :-1], None, None, None, s, device=False)                    # rows that are not whole ticks
    with pytest.raises(ValueError):
        ls.feedback_rows(c["idx"], c["vel"][:1], None, None, s, device=False)
    with pytest.raises(ValueError):
        ls.feedback_rows(c["idx"], None, None, c["instr"][:, :1], s, device=False)
    with pytest.raises(ValueError):
        ls.feedback_rows(c["idx"], None, None, None, dict(s, velocity_threshold_such_that_it_is_a_played_note=float("nan")), device=False)


# ---- the feedback --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FEEDBACK, ids=[lc.feedback_id(c) + "-%d" % i for i, c in enumerate(FEEDBACK)])
def test_the_feedback_mirror_is_the_reference(c):
    got = ls.feedback_rows(c["idx"], c["vel"] if c["has_vel"] else None, c["held"] if c["has_held"] else None, c["instr"],
                           lc.feedback_settings(c), device=False)
    assert got["x"].dtype == np.uint8 and np.array_equal(got["x"], c["X"])
    assert np.array_equal(got["x_rev"], c["X"][:, ::-1])
    assert got["vel"].dtype == np.float32 and lc.same_bits(got["vel"], c["V"])
    assert got["held"].dtype == np.uint8 and np.array_equal(got["held"], c["D"])
    assert np.array_equal(got["instr"], c["I"])
    none = ls.feedback_rows(c["idx"], None, None, None, lc.feedback_settings(c), device=False)
    assert none["instr"] is None and np.all(none["held"] == 1)
    assert np.all(none["vel"] == np.float32(c["threshold"] + (1.0 - c["threshold"]) * 0.5))


# ---- the siblings' host side -----------------------------------------------------------------------------------------------------------
def test_code_paths_and_class_knob_codes():
    code = np.arange(6, dtype=np.float64) / 4 - 1
    path = gen.code_path(code)
    z, hist = gen.latent_rows(path["anchors"], path, device=False)
    assert z.shape == (1, 6) and lc.same_bits(z, code.astype(np.float32)[None]) and not hist.any()
    knobs = Decoder.class_knob_codes(code, 3)
    want = np.repeat(code[None], 3, 0)
    for C in range(3):          # vae_evaluation.py:1796-1797
        want[C, 0:3] = -1
        want[C, C] = 1
    assert knobs.dtype == np.float64 and np.array_equal(knobs, want) and np.array_equal(code, np.arange(6) / 4 - 1)
    assert Decoder.class_knob_codes(code.astype(np.float32), 1).dtype == np.float32
    for bad in (0, 7):
        with pytest.raises(ValueError):
            Decoder.class_knob_codes(code, bad)


# ---- the ninth header ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_longsong.h")
    assert declared == {"mvae_longsong_abi_version", "mvae_nearest_walk_workspace", "mvae_nearest_walk", "mvae_feedback_rows"} \
        == set(hl.LONGSONG_SIGNATURES)
    assert hl.LONGSONG_HEADERS == (("long song ", "mvae_longsong_abi_version", 1, hl.LONGSONG_SIGNATURES),)
    others = [sig for _, _, _, sig in hl.HEADERS + hl.LATER_HEADERS]
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert not any(name in sig for sig in others) and name not in _declared("midivae_hip.h")
    assert lib.mvae_longsong_abi_version() == 1 == hl.LONGSONG_ABI_VERSION
    # the other versions do not move with this header
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION
    assert [lib.mvae_desc_abi_version(), lib.mvae_sweep_abi_version(), lib.mvae_recon_abi_version(), lib.mvae_events_abi_version(),
            lib.mvae_import_abi_version(), lib.mvae_style_abi_version(), lib.mvae_generate_abi_version()] == [1] * 7
    # the workspace helper is the header's formula
    for N, S, Z in ((1, 1, 1), (256, 3, 8), (257, 3, 8), (65536, 32, 256), (1 << 20, 256, 256)):
        assert lib.mvae_nearest_walk_workspace(N, S, Z) == S * -(-N // ls.ROW_CHUNK) * 16 + S * 8
    assert [lib.mvae_nearest_walk_workspace(*a) for a in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1))] == [0, 0, 0, 0]


def test_ctypes_structs_match_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = (("mvae_walk_args", hl.WalkArgs), ("mvae_feedback_args", hl.FeedbackArgs))
    constants = ("MVAE_WALK_MAX_Z", "MVAE_WALK_ROW_CHUNK", "MVAE_WALK_SONG_GROUP", "MVAE_FEEDBACK_MAX_VOICES", "MVAE_FEEDBACK_MAX_T")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_longsong.h"', 'int main(void) {']
    for cname, cls in structs:
        lines.append('printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    lines += ['printf("%s %%d\\n", (int)%s);' % (c, c) for c in constants]
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    for cname, cls in structs:
        assert int(got[cname + ".sizeof"]) == ctypes.sizeof(cls) and ctypes.sizeof(cls) % 8 == 0, cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert int(got["MVAE_WALK_MAX_Z"]) == ls.MAX_Z == 4096 and int(got["MVAE_FEEDBACK_MAX_T"]) == ls.MAX_T == 65536
    assert (int(got["MVAE_WALK_ROW_CHUNK"]), int(got["MVAE_WALK_SONG_GROUP"])) == (ls.ROW_CHUNK, ls.SONG_GROUP) == (256, 8)
    assert int(got["MVAE_FEEDBACK_MAX_VOICES"]) == 8


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_long_songs_gpu.py runs the safe rows on real buffers)")
ENTRIES = {"walk": ("mvae_nearest_walk", lc.walk_baseline, lc.WALK_ROWS, lc.WALK_ACCEPTED),
           "feedback": ("mvae_feedback_rows", lc.feedback_baseline, lc.FEEDBACK_ROWS, lc.FEEDBACK_ACCEPTED)}
ALL_ROWS = [(which, row) for which, e in ENTRIES.items() for row in e[2]]


@no_device
@pytest.mark.parametrize("which", sorted(ENTRIES))
def test_baseline_and_accepted_forms_pass_validation(which):
    entry, baseline, _, accepted = ENTRIES[which]
    lib = hl.load()
    assert lc.invoke(lib, entry, baseline(lc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in accepted:
        assert lc.invoke(lib, entry, mutate(baseline(lc.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("which,row", ALL_ROWS, ids=["%s: %s" % (w, r[0]) for w, r in ALL_ROWS])
def test_violation_is_refused_before_anything_is_enqueued(which, row):
    entry, baseline = ENTRIES[which][:2]
    name, mutate, code, _ = row
    rc = lc.invoke(hl.load(), entry, mutate(baseline(lc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_tables_cover_every_documented_limit():
    names = " | ".join(r[0] for r in lc.WALK_ROWS)
    for what in ("a NULL", "all_z NULL", "r_in NULL", "picked NULL", "workspace NULL", "best_out NULL", "dist_out NULL", "z_out NULL",
                 "r_out NULL", "N = 0", "S = 0", "Z = 0", "cap = 0", "ld_all = Z - 1", "ld_r = Z - 1", "ld_z = Z - 1", "ld_rout = Z - 1",
                 "ld_hist = Z - 1", "ld_hist_in = Z - 1", "n_picked = -1", "n_picked = cap", "r_f64 = 2", "r_f64 = -1", "hist_f64 = 2",
                 "e = nan", "e = inf", "den = nan", "den = -inf", "den = 0", "Z = 4097"):
        assert what in names, what
    names = " | ".join(r[0] for r in lc.FEEDBACK_ROWS)
    for what in ("a NULL", "idx NULL", "every output NULL", "n = 0", "T = 0", "n_pitch = 0", "stride_t = 0", "stride_w = -1",
                 "instr_stride_v = 0", "voices = 1", "voices = 9", "T % voices != 0", "silent = -2", "silent = 256", "override_rules = 2",
                 "threshold = nan", "threshold = inf", "ld_out = n - 1", "T = 65538"):
        assert what in names, what
    assert len([r for r in lc.WALK_ROWS if r[3]]) >= 15 and len([r for r in lc.FEEDBACK_ROWS if r[3]]) >= 12
