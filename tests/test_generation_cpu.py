"""Interpolation songs, medleys and piano-roll images without a device: the NumPy mirrors of midi_vae_amd.generation and
midi_vae_amd.pianoroll against the reference's own functions and its restated generation loops (tests/golden/generation.npz, written
by tests/golden/make_generation_fixtures.py), medley_samples' clamps, the PNG writer, the eighth header's hygiene, the layout of
PathsArgs and PianorollArgs, and the refusals of the two entry points as tables (tests/generate_contract.py).

Bounds (derived, not measured).  A latent row is two products and a sum evaluated by the same NumPy in the same type on the same
anchors, then one cast: BIT-EQUAL, signed zeros included.  An image cell is one subtraction, one multiplication and at most
max_voices - 1 additions in double in the reference's order: bit-equal.  Nothing here has a tolerance."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import generation as gen
from midi_vae_amd import hiplib as hl
from midi_vae_amd import pianoroll as pr
from midi_vae_amd.reconstruction import first_windows
from tests import generate_contract as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return gc.load_fixture()


def fixture_paths(fx):
    """the four songs of a fixture run, rebuilt from its anchors by the public builders"""
    A = fx["anchors"]
    return [gen.medley_path([A[0:1]], 4), gen.interpolation_path(A[1], A[2:3], 10),
            gen.medley_path([A[3:11], A[11:19], A[19:27]], 4), gen.medley_path([A[27:36], A[36:43], A[43:48]], 5, mode="slerp")]


# ---- the mirrors against the reference ---------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises(cases):
    for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
        fx = cases["paths_" + tag]
        assert fx["anchors"].shape == (48, 32) and fx["anchors"].dtype == dtype and list(fx["lengths"]) == gc.PATH_LENGTHS
        assert fx["z"].shape == fx["hist"].shape == (75, 32) and fx["z"].dtype == fx["hist"].dtype == np.float32
        assert ((fx["anchors"] == 0) & np.signbit(fx["anchors"])).sum() >= 4 and ((fx["z"] == 0) & np.signbit(fx["z"])).sum() >= 3
    assert cases["paths_f32"]["fma_rows"] >= 10
    a, b = cases["image_a"], cases["image_b"]
    assert a["idx"].shape == (49, 16) and list(a["lengths"]) == [1, 3, 40, 5] and (a["voices"], a["n_pitch"], a["held_song"]) == (2, 20, 2)
    assert b["idx"].shape == (9, 12) and list(b["lengths"]) == [2, 1, 6] and (b["voices"], b["n_pitch"]) == (3, 9)
    for fx in (a, b):
        ticks = fx["idx"].size // int(fx["voices"])
        assert fx["vel"].dtype == np.float32 and fx["image"].shape == fx["binary"].shape == (ticks, int(fx["n_pitch"]))
        assert set(np.unique(fx["binary"])) == {0.0, 1.0} and (fx["image"] > 0).any()
        assert ((fx["binary"] > 0) & (fx["image"] == 0)).any() and ((fx["binary"] == 0) & (fx["image"] > 0)).any()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_paths_mirror_is_the_reference(cases, tag):
    fx = cases["paths_" + tag]
    first = first_windows(fx["lengths"], 75)
    z, hist = gen.latent_rows(fx["anchors"], fx, first, device=False)
    assert gc.same_bits(z, fx["z"]) and gc.same_bits(hist, fx["hist"])
    # the builders make the fixture's recipe, and windows in the middle of the run are the same rows
    run = gen.concat_paths(fixture_paths(fx))
    assert run["lengths"] == gc.PATH_LENGTHS and np.array_equal(run["first_window"], first) and run["anchors"].dtype == fx["anchors"].dtype
    assert gc.same_bits(run["anchors"], fx["anchors"])
    for k in ("a0", "a1", "c0", "c1"):
        assert run[k].dtype == fx[k].dtype and np.array_equal(run[k], fx[k]), k
    z2, h2 = gen.latent_rows(run["anchors"], run, run["first_window"], lo=30, count=40, device=False)
    assert gc.same_bits(z2, fx["z"][30:70]) and gc.same_bits(h2, fx["hist"][30:70])
    # every window a song of its own: no history
    z3, h3 = gen.latent_rows(run["anchors"], run, None, device=False)
    assert gc.same_bits(z3, fx["z"]) and not h3.any() and not np.signbit(h3).any()


def test_blend_is_not_a_copy_and_not_fused(cases):
    """t = 0 turns -0.0 into +0.0 where the other anchor is positive; the float32 blend rounds both products before the sum"""
    fx = cases["paths_f32"]
    A = fx["anchors"]
    w = 1                                                    # the interpolation song's first window: a blend at t = 0
    assert (fx["a0"][w], fx["a1"][w], fx["c0"][w], fx["c1"][w]) == (1, 2, 1.0, 0.0)
    z = gen.latent_rows(A, fx, device=False)[0]
    assert np.signbit(A[1, 3]) and A[1, 3] == 0 and A[2, 3] > 0 and z[w, 3] == 0 and not np.signbit(z[w, 3])
    assert np.signbit(A[1, 9]) and A[2, 9] < 0 and np.signbit(z[w, 9])
    assert np.array_equal(z[w][A[1] != 0], A[1][A[1] != 0])
    in_double = (A[fx["a0"]].astype(np.float64) * fx["c0"][:, None] + A[np.maximum(fx["a1"], 0)] * fx["c1"][:, None]).astype(np.float32)
    blended = fx["a1"] >= 0
    assert (in_double[blended] != z[blended]).any()          # rounding every step in float32 is not rounding once
    linear = gen.linear_interpolation(A[1], A[2], 0.3)
    assert linear.dtype == np.float32 and gc.same_bits(linear, A[1] * (1.0 - 0.3) + A[2] * 0.3)
    t = 0.4
    omega = np.arccos(np.dot(A[1] / np.linalg.norm(A[1]), A[2] / np.linalg.norm(A[2])))
    assert gc.same_bits(gen.slerp(A[1], A[2], t), np.sin((1.0 - t) * omega) / np.sin(omega) * A[1] + np.sin(t * omega) / np.sin(omega) * A[2])


def test_paths_edges():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((3, 6)).astype(np.float32)
    t = dict(a0=np.array([0, 3, -1, 1, 2], np.int32), a1=np.array([1, 0, 0, 3, -1], np.int32), c0=np.full(5, 0.5), c1=np.full(5, 0.5))
    first = np.zeros(5, np.int32)
    z, hist = gen.latent_rows(A, t, first, device=False)
    assert np.isnan(z[[1, 2, 3]]).all() and not np.isnan(z[[0, 4]]).any()          # an index out of range is never read: NaN
    assert np.array_equal(z[4], A[2]) and not hist[0].any() and np.array_equal(hist[1], z[0]) and np.isnan(hist[[2, 3, 4]]).all()
    for bad in (dict(lo=-1), dict(lo=3, count=3), dict(count=0)):
        with pytest.raises(ValueError):
            gen.latent_rows(A, t, first, device=False, **bad)
    with pytest.raises(ValueError):
        gen.latent_rows(A, dict(t, c1=t["c1"][:4]), first, device=False)
    with pytest.raises(ValueError):
        gen.latent_rows(A, t, first[:3], device=False)
    with pytest.raises(ValueError):
        gen.latent_rows(np.zeros((2, 4097), np.float32), t, None, device=False)
    with pytest.raises(ValueError):
        gen.interpolation_path(A[0], A[1], 0)
    with pytest.raises(ValueError):
        gen.interpolation_path(A[0], A[1].astype(np.float64), 3)
    with pytest.raises(ValueError):
        gen.interpolation_path(A[0], A[1], 3, mode="cubic")
    with pytest.raises(ValueError):
        gen.medley_path([], 4)
    with pytest.raises(ValueError):
        gen.concat_paths([gen.interpolation_path(A[0], A[1], 3), gen.interpolation_path(A[0].astype(np.float64), A[1].astype(np.float64), 3)])
    # a bridge of length 0 joins the songs directly; integer codes are read as float64
    m = gen.medley_path([A[:2], A[2:]], 0)
    assert list(m["a0"]) == [0, 1, 2] and list(m["a1"]) == [-1, -1, -1]
    assert gen.interpolation_path([1, 2], [3, 4], 2)["anchors"].dtype == np.float64


def test_medley_samples_clamps():
    """vae_evaluation.py:735-764 on designed lengths: songs that are too short are drawn again, the first song's sample is raised to
    ``noninterpolated``, every other sample is lowered to ``length - noninterpolated - 1``"""
    class Script:
        """np.random.RandomState's randint, replaying a script of draws and recording the bounds it was asked for"""

        def __init__(self, draws):
            self.draws, self.asked = list(draws), []

        def randint(self, high):
            self.asked.append(high)
            return self.draws.pop(0)

    lengths = [8, 30, 9, 20]
    rng = Script([0, 1, 3,          # song 0 has 8 windows, not more than 8: drawn again -> song 1, sample 3 < 8 -> 8
                  3, 15,            # song 3, sample 15 >= 20 - 8 -> 11
                  2, 0,             # song 2 (9 windows), sample 0 -> stays below 9 - 8 = 1
                  2, 5])            # song 2, sample 5 >= 1 -> 0
    got = gen.medley_samples(lengths, 4, 8, rng)
    assert rng.asked == [4, 4, 30, 4, 20, 4, 9, 4, 9] and not rng.draws
    assert [(s, k, list(r)) for s, k, r in got] == [(1, 8, list(range(0, 8))), (3, 11, list(range(11, 19))), (2, 0, list(range(0, 8))),
                                                    (2, 0, list(range(0, 8)))]
    # the first song's second clamp (the reference's elif): a sample at the song's end goes to length - k - 1, even below k
    first = gen.medley_samples([9], 1, 8, Script([0, 8]))
    assert [(s, k, list(r)) for s, k, r in first] == [(0, 0, list(range(-8, 0)))]
    # a real RandomState draws in the reference's order
    a = gen.medley_samples(lengths, 3, 8, np.random.RandomState(5))
    r = np.random.RandomState(5)
    song = r.randint(4)
    while lengths[song] <= 8:
        song = r.randint(4)
    assert a[0][0] == song and len(a) == 3 and all(len(x[2]) == 8 for x in a)
    with pytest.raises(ValueError):
        gen.medley_samples([8, 3], 2, 8, np.random.RandomState(0))
    with pytest.raises(ValueError):
        gen.medley_samples([9], 2, 0, np.random.RandomState(0))


@pytest.mark.parametrize("case", ["a", "b"])
def test_image_mirror_is_the_reference(cases, case):
    fx = cases["image_" + case]
    s = gc.image_settings(fx)
    ticks = fx["idx"].shape[1] // int(fx["voices"])
    drawn = pr.images(fx["idx"], fx["vel"], fx["lengths"], s, device=False)
    binary = pr.images(fx["idx"], None, fx["lengths"], s, device=False)
    assert [im.shape for im in drawn] == [(int(fx["n_pitch"]), int(m) * ticks) for m in fx["lengths"]]
    assert gc.same_bits(np.concatenate(drawn, 1).T, fx["image"]) and gc.same_bits(np.concatenate(binary, 1).T, fx["binary"])
    # one-hot rolls are taken too, and the drop-in works on the one-hot rows of one song
    K = int(fx["n_pitch"])
    onehot = np.eye(K + 1)[fx["idx"]]
    assert gc.same_bits(np.concatenate(pr.images(onehot, fx["vel"], fx["lengths"], s, device=False), 1).T, fx["image"])
    lo = int(fx["lengths"][0])
    m = int(fx["lengths"][1])
    Y = onehot[lo:lo + m, :, :K].reshape(-1, K)
    V = fx["vel"][lo:lo + m].reshape(-1).astype(np.float64)
    assert gc.same_bits(pr.prepare_for_drawing(Y, V, s), fx["image"][lo * ticks:(lo + m) * ticks].T)
    assert gc.same_bits(pr.prepare_for_drawing(Y, None, s), fx["binary"][lo * ticks:(lo + m) * ticks].T)
    # a song drawn alone is the same song: nothing leaks across a song's first window
    alone = pr.images(fx["idx"][lo:lo + m], fx["vel"][lo:lo + m], [m], s, device=False)[0]
    assert gc.same_bits(alone, drawn[1])


def test_image_quirks_by_hand():
    """2 voices, 4 pitches, silent index 4, threshold 0.5, MAX_VELOCITY 100: pitch-0 continuation, step == voices, a
    broken chain, a struck row that does not sound"""
    s = dict(max_voices=2, low_crop=0, high_crop=4, include_silent_note=True, velocity_threshold_such_that_it_is_a_played_note=0.5,
             MAX_VELOCITY=100.0)
    #          tick:  0        1        2        3        4        5
    v0 = [(2, 0.75), (2, 0.25), (2, 0.75), (2, 0.25), (3, 0.25), (4, 0.75)]          # struck, step == V: nothing, struck, held, broken, struck but silent
    v1 = [(0, 1.0), (4, 0.25), (4, 0.0), (2, 0.25), (2, 1.0), (2, 0.0)]              # pitch 0 struck, silence continues it twice, broken, struck, held
    idx = np.array([x for pair in zip(v0, v1) for x in (pair[0][0], pair[1][0])], np.uint8).reshape(2, 6)
    vel = np.array([x for pair in zip(v0, v1) for x in (pair[0][1], pair[1][1])], np.float32).reshape(2, 6)
    want = np.zeros((6, 4))
    want[0, 2], want[0, 0] = 25.0, 50.0
    want[1, 0] = 50.0                       # voice 0 at step == 2 does not inherit; the silence of voice 1 continues pitch 0
    want[2, 2], want[2, 0] = 25.0, 50.0
    want[3, 2] = 25.0                       # voice 1 sounds 2 after displaying pitch 0: broken
    want[4, 2] = 50.0                       # voice 0 changes to 3 without a strike: broken; voice 1 strikes 2
    want[5, 2] = 50.0                       # voice 0 strikes the silent index: nothing
    got = pr.images(idx, vel, [2], s, device=False)[0]
    assert np.array_equal(got, want.T)
    # two songs of one window each: the second song's rows start at step 0 again
    two = pr.images(idx, vel, [1, 1], s, device=False)
    assert np.array_equal(two[0], want[:3].T)
    second = np.zeros((3, 4))
    second[1, 2], second[2, 2] = 50.0, 50.0          # voice 1: tick 3 of the run is step 1 of its song, tick 4 strikes, tick 5 (step 5) holds
    assert np.array_equal(two[1], second.T)
    with pytest.raises(ValueError):
        pr.images(idx, vel, [1], s, device=False)
    with pytest.raises(ValueError):
        pr.images(idx[:, :5], vel[:, :5], [2], s, device=False)
    with pytest.raises(ValueError):
        pr.images(idx, vel, [2], dict(s, MAX_VELOCITY=float("inf")), device=False)
    assert np.array_equal(pr.difference_image([[0, 1], [2, 0]], [[0, 3], [0, 1]]), [[0, 3], [1, 2]])


# ---- PNG -----------------------------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    image = np.zeros((5, 7))
    image[0, 0], image[4, 6], image[2, 3], image[1, 1] = 10.0, 5.0, 2.5, 0.02
    path = str(tmp_path / "roll.png")
    pr.write_png(path, image)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
    assert struct.unpack(">IIBBBBB", data[16:29]) == (7, 5, 8, 0, 0, 0, 0)          # width = ticks, height = pitches, 8-bit grey
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29]) & 0xFFFFFFFF
    at, kinds = 8, []
    while at < len(data):          # every chunk's CRC, and the raw scanlines: pitch 0 is the BOTTOM row
        size = struct.unpack(">I", data[at:at + 4])[0]
        kinds.append(data[at + 4:at + 8])
        assert struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(data[at + 4:at + 8 + size]) & 0xFFFFFFFF
        if kinds[-1] == b"IDAT":
            rows = np.frombuffer(zlib.decompress(data[at + 8:at + 8 + size]), np.uint8).reshape(5, 8)
        at += 12 + size
    assert kinds == [b"IHDR", b"IDAT", b"IEND"] and not rows[:, 0].any()
    assert rows[4, 1] == 0 and rows[0, 7] == 127 and rows[4, 2] == 255          # the maximum is black, half of it 127.5 -> 128 steps from white
    got = pr.read_png(path)
    assert got.shape == (5, 7) and got.dtype == np.uint8
    assert got[0, 0] == 0 and got[4, 6] == 127 and got[2, 3] == 191 and got[1, 1] == 254 and got[3, 3] == 255
    assert np.array_equal(got, pr.grey_levels(image))
    pr.write_png(path, image, vmax=20.0)          # a scale of the caller's: 10 of 20 is mid grey, values above clip to black
    assert pr.read_png(path)[0, 0] == 127 and pr.grey_levels(image * 4, vmax=20.0)[0, 0] == 0
    assert np.all(pr.grey_levels(np.zeros((2, 2))) == 255)
    broken = bytearray(data)
    broken[40] ^= 1
    (tmp_path / "broken.png").write_bytes(bytes(broken))
    with pytest.raises(ValueError):
        pr.read_png(str(tmp_path / "broken.png"))
    with pytest.raises(ValueError):
        pr.write_png(path, np.zeros((0, 4)))


# ---- the eighth header -------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_generate.h")
    assert declared == {"mvae_generate_abi_version", "mvae_latent_paths", "mvae_pianoroll"} == set(hl.GENERATE_SIGNATURES)
    assert len(hl.HEADERS) == 7 and hl.HEADERS[-1][1] == "mvae_style_abi_version"
    assert hl.LATER_HEADERS == (("generate ", "mvae_generate_abi_version", 1, hl.GENERATE_SIGNATURES),)
    others = [sig for _, _, _, sig in hl.HEADERS]
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert not any(name in sig for sig in others) and name not in _declared("midivae_hip.h")
    assert lib.mvae_generate_abi_version() == 1 == hl.GENERATE_ABI_VERSION
    # the other versions do not move with this header
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION
    assert [lib.mvae_desc_abi_version(), lib.mvae_sweep_abi_version(), lib.mvae_recon_abi_version(), lib.mvae_events_abi_version(),
            lib.mvae_import_abi_version(), lib.mvae_style_abi_version()] == [1, 1, 1, 1, 1, 1]


def test_ctypes_structs_match_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = (("mvae_paths_args", hl.PathsArgs), ("mvae_pianoroll_args", hl.PianorollArgs))
    constants = ("MVAE_PATHS_MAX_Z", "MVAE_PIANOROLL_MAX_VOICES", "MVAE_PIANOROLL_MAX_PITCH", "MVAE_PIANOROLL_MAX_T")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_generate.h"', 'int main(void) {']
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
    assert int(got["MVAE_PATHS_MAX_Z"]) == gen.MAX_Z == 4096 and int(got["MVAE_PIANOROLL_MAX_T"]) == pr.MAX_T == 65536
    assert (int(got["MVAE_PIANOROLL_MAX_VOICES"]), int(got["MVAE_PIANOROLL_MAX_PITCH"])) == (8, 192)


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_generation_gpu.py runs the safe rows on real buffers)")
ENTRIES = {"paths": ("mvae_latent_paths", gc.paths_baseline, gc.PATHS_ROWS, gc.PATHS_ACCEPTED),
           "pianoroll": ("mvae_pianoroll", gc.pianoroll_baseline, gc.PIANOROLL_ROWS, gc.PIANOROLL_ACCEPTED)}
ALL_ROWS = [(which, row) for which, e in ENTRIES.items() for row in e[2]]


@no_device
@pytest.mark.parametrize("which", sorted(ENTRIES))
def test_baseline_and_accepted_forms_pass_validation(which):
    entry, baseline, _, accepted = ENTRIES[which]
    lib = hl.load()
    assert gc.invoke(lib, entry, baseline(gc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in accepted:
        assert gc.invoke(lib, entry, mutate(baseline(gc.fake_alloc))) == hl.E_LAUNCH, name
    if which == "paths":
        big = gc.S(Z=4096, ld_anchor=4096, ld_z=4096, ld_hist=4096, anchor_f64=1)
    else:
        big = gc.S(n_pitch=192, ld_img=192, silent=192, T=65536, voices=8)
    assert gc.invoke(lib, entry, big(baseline(gc.fake_alloc))) == hl.E_LAUNCH


@no_device
@pytest.mark.parametrize("which,row", ALL_ROWS, ids=["%s: %s" % (w, r[0]) for w, r in ALL_ROWS])
def test_violation_is_refused_before_anything_is_enqueued(which, row):
    entry, baseline = ENTRIES[which][:2]
    name, mutate, code, _ = row
    rc = gc.invoke(hl.load(), entry, mutate(baseline(gc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_tables_cover_every_documented_limit():
    names = " | ".join(r[0] for r in gc.PATHS_ROWS)
    for what in ("a NULL", "anchors NULL", "a0 NULL", "a1 NULL", "c0 NULL", "c1 NULL", "z_out NULL", "n = 0", "count = 0", "Z = 0",
                 "n_anchors = 0", "lo = -1", "lo + count = n + 1", "ld_anchor = Z - 1", "ld_z = Z - 1", "ld_hist = Z - 1", "anchor_f64 = 2",
                 "anchor_f64 = -1", "Z = 4097"):
        assert what in names, what
    names = " | ".join(r[0] for r in gc.PIANOROLL_ROWS)
    for what in ("a NULL", "idx NULL", "img_out NULL", "n = 0", "T = 0", "n_pitch = 0", "stride_t = 0", "stride_w = -1", "voices = 1",
                 "voices = 9", "T % voices != 0", "silent = -2", "silent = 256", "ld_img = n_pitch - 1", "threshold = nan",
                 "threshold = inf", "max_velocity = nan", "max_velocity = -inf", "n_pitch = 193", "T = 65538"):
        assert what in names, what
    assert len([r for r in gc.PATHS_ROWS if r[3]]) >= 10 and len([r for r in gc.PIANOROLL_ROWS if r[3]]) >= 12
