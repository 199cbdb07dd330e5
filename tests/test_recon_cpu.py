"""The song-level decode without a device: the NumPy mirror and the report of midi_vae_amd.reconstruction against the reference's own
outputs (tests/golden/recon.npz, written by tests/golden/make_recon_fixtures.py) and against packers.apply_velocity_rules, the fourth
header's hygiene, the layout of ReconArgs, and the refusals of mvae_recon_songs as a table (tests/recon_contract.py).

Bounds (derived, not measured).  Every velocity after the rules is an input float32 or a zero, every note start a byte, every count an
integer, every metric one integer or one division of two of them: everything here is BIT-EQUAL, no tolerance anywhere."""
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
from midi_vae_amd import packers
from midi_vae_amd import reconstruction as rec
from midi_vae_amd import sweep as sw
from tests import recon_contract as rcn
from tests.recon_contract import load_fixture, random_songs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the mirror against the reference ------------------------------------------------------------------------------------------
def test_fixture_is_the_shipped_shape(fx):
    n = int(fx["lengths"].sum())
    assert fx["idx"].shape == (n, 64) and fx["idx"].dtype == np.uint8 and fx["vel"].dtype == np.float32 and fx["orig"].dtype == np.uint8
    assert fx["s"] == dict(max_voices=4, low_crop=24, high_crop=84, include_silent_note=True,
                           velocity_threshold_such_that_it_is_a_played_note=0.5, override_sampled_pitches_based_on_velocity_info=True,
                           meta_velocity=True, meta_held_notes=False)
    assert rec.params(fx["s"]) == dict(voices=4, n_pitch=60, silent=60, threshold=0.5, override=True)
    assert len(fx["lengths"]) == 28 and fx["lengths"].min() == 1 and fx["lengths"].max() <= 12
    assert np.any(fx["lengths"] % 2 == 0) and np.any(fx["lengths"] % 2 == 1)
    assert tuple(fx["metric_names"]) == rec.METRICS and len(rec.COUNTS) == 8 == rec.N_COUNTS


def test_mirror_is_the_reference(fx):
    got = rec.song_decode(fx["idx"], fx["vel"], fx["lengths"], fx["s"], orig=fx["orig"], device=False)
    assert same_bits(got["velocity"], fx["velocity"])
    assert got["starts"].dtype == np.uint8 and np.array_equal(got["starts"], fx["starts"])
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], fx["counts"])
    held = rec.song_decode(fx["idx"], fx["vel"], fx["lengths"], fx["s"], held=fx["held"], orig=fx["orig"], device=False)
    assert same_bits(held["velocity"], fx["velocity"]) and np.array_equal(held["starts"], fx["held"])
    assert np.array_equal(held["counts"], fx["counts_held"])
    onehot = rec.song_decode(np.eye(61)[fx["idx"]], fx["vel"].astype(np.float64), fx["lengths"], fx["s"], orig=np.eye(61)[fx["orig"]],
                             device=False)
    assert all(np.array_equal(onehot[k], got[k]) for k in got)


def test_fixture_needs_the_state_carried_across_windows(fx):
    """what a kernel that restarts the rule in every window computes is the sweep's mirror: it differs in at least a quarter of the
    multi-window songs, and at the two planted rows"""
    per_window = sw.window_statistics(fx["idx"], fx["vel"], fx["s"], device=False, return_velocity=True)[1]
    first = np.cumsum(fx["lengths"]) - fx["lengths"]
    differs = [bool(np.any(per_window[lo:lo + m] != fx["velocity"][lo:lo + m])) for lo, m in zip(first, fx["lengths"]) if m > 1]
    assert np.mean(differs) >= 0.25
    assert all(np.array_equal(per_window[lo], fx["velocity"][lo]) for lo in first)          # a song's first window starts from nothing
    far, edge = first[-2], first[-1]
    assert fx["lengths"][-2] == 5 and fx["velocity"][far + 4, 0] == 0.875 == fx["vel"][far, 60] and per_window[far + 4, 0] == 0.125
    assert np.all(fx["vel"][far + 1:far + 4, 0::4] == 0.25)                                   # three whole windows under the threshold
    assert list(fx["idx"][edge, 60:62]) == [0, 3] and list(fx["idx"][edge + 1, 0:2]) == [5, 7]
    assert fx["velocity"][edge + 1, 0] == fx["vel"][edge + 1, 0] == 0.125                     # previous pitch column 0: `> 0` leaves it
    assert fx["velocity"][edge + 1, 1] == fx["vel"][edge, 61] == 0.8125                       # previous pitch 3: inherited
    assert np.all(np.delete(fx["counts"].sum(0), 6) > 0) and np.all(fx["counts_held"].sum(0) > 0)
    silent = first[-4]
    assert np.all(fx["counts"][silent:silent + 3] == 0) and np.all(fx["velocity"][silent:silent + 3] == 0)


def test_song_metrics_are_the_reference(fx):
    counts = rec.song_decode(fx["idx"], fx["vel"], fx["lengths"], fx["s"], orig=fx["orig"], device=False)["counts"]
    got = rec.song_metrics(counts, fx["lengths"], 64, fx["s"])
    assert len(got) == len(fx["lengths"])
    for i, d in enumerate(got):
        assert tuple(d) == rec.METRICS
        for k, want in zip(rec.METRICS, fx["metrics"][i].tolist()):
            assert d[k] == want or (np.isnan(d[k]) and np.isnan(want)), (i, k, d[k], want)
    assert np.isnan(got[-4]["pitch_reconstruction_accuracy"]) and sum(np.isnan(d["pitch_reconstruction_accuracy"]) for d in got) == 1
    assert any(d["predicted_note_start_to_original_errors"] > 0 for d in got)
    # the switch of vae_evaluation.py:2213: no held head, and no velocity head or a threshold of 0 - no note-start errors are counted
    for off in (dict(fx["s"], meta_velocity=False), dict(fx["s"], velocity_threshold_such_that_it_is_a_played_note=0.0)):
        quiet = rec.song_metrics(counts, fx["lengths"], 64, off)
        assert all(d["predicted_note_start_to_original_errors"] == 0 == d["predicted_note_start_to_predicted_errors"] for d in quiet)
        assert [d["total_original_notes"] for d in quiet] == [d["total_original_notes"] for d in got]
    held = rec.song_metrics(fx["counts_held"], fx["lengths"], 64, dict(fx["s"], meta_velocity=False, meta_held_notes=True))
    assert any(d["predicted_note_start_to_predicted_errors"] > 0 for d in held)
    mean = rec.mean_metrics(got[:10])
    assert mean["song_name"] == "Mean" and set(mean) == set(rec.METRICS) | {"song_name"}
    for k in rec.METRICS:
        total = 0.0
        for d in got[:10]:
            total += d[k]
        assert mean[k] == total / 10, k
    assert np.isnan(rec.mean_metrics(got)["pitch_reconstruction_accuracy"])


# ---- the mirror against the host rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 4, 8])
@pytest.mark.parametrize("threshold", [0.5, 0.25, 0.0])
def test_mirror_is_apply_velocity_rules_song_by_song(V, threshold):
    rng = np.random.default_rng(int(1000 * threshold) + V)
    s = dict(max_voices=V, low_crop=24, high_crop=84, include_silent_note=True,
             velocity_threshold_such_that_it_is_a_played_note=threshold, override_sampled_pitches_based_on_velocity_info=True)
    T, carried = 8 * V, 0
    for _ in range(25):
        lengths = rng.integers(1, 6, int(rng.integers(1, 5)))
        idx, vel = random_songs(rng, lengths, T, V)
        got = rec.song_decode(idx, vel, lengths, s, device=False)
        alone = rec.song_decode(idx, vel, np.ones(len(idx), np.int64), s, device=False)["velocity"]
        lo = 0
        for m in lengths.tolist():
            Y = packers.notes_from_indices(s, idx[lo:lo + m].astype(np.int64), 61)
            want = packers.apply_velocity_rules(s, Y, vel[lo:lo + m].astype(np.float64).reshape(-1))
            assert np.array_equal(got["velocity"][lo:lo + m].astype(np.float64).reshape(-1), want)
            assert np.array_equal(got["starts"][lo:lo + m].reshape(-1), np.where(want > threshold, 0, 1))
            carried += bool(np.any(alone[lo:lo + m] != got["velocity"][lo:lo + m]))
            lo += m
    assert carried > 0 or threshold == 0.0          # (at threshold 0 no velocity is silent: nothing is ever inherited)


def test_songs_of_one_window_are_the_sweep(fx):
    n = len(fx["idx"])
    for s in (fx["s"], dict(fx["s"], override_sampled_pitches_based_on_velocity_info=False)):
        want = sw.window_statistics(fx["idx"], fx["vel"], s, device=False, return_velocity=True)[1]
        assert same_bits(rec.song_decode(fx["idx"], fx["vel"], np.ones(n, np.int64), s, device=False)["velocity"], want)
    # without a velocity head: the default velocity everywhere, every note start off
    want = sw.window_statistics(fx["idx"], None, fx["s"], device=False, return_velocity=True)[1]
    got = rec.song_decode(fx["idx"], None, fx["lengths"], fx["s"], device=False)
    assert same_bits(got["velocity"], want) and np.all(got["velocity"] == 0.75) and np.all(got["starts"] == 1)
    assert np.all(got["counts"][:, [0, 2, 3, 5, 6, 7]] == 0) and np.array_equal(got["counts"][:, 4], got["counts"][:, 1])


def test_song_decode_refuses_bad_inputs(fx):
    idx, vel, s = fx["idx"][:9], fx["vel"][:9], fx["s"]
    for device in (False, True):          # the checks of the device path come before anything touches a device
        kw = dict(device=device)
        for lengths in ([4, 4], [5, 5], [9, 0], [10, -1], []):
            with pytest.raises(ValueError):
                rec.song_decode(idx, vel, lengths, s, **kw)
        if device:
            continue
        with pytest.raises(ValueError):
            rec.song_decode(idx[:, :63], vel[:, :63], [9], s, **kw)
        with pytest.raises(ValueError):
            rec.song_decode(idx, vel[:, :60], [9], s, **kw)
        with pytest.raises(ValueError):
            rec.song_decode(idx, vel, [9], s, orig=fx["orig"][:8], **kw)
        with pytest.raises(ValueError):
            rec.song_decode(idx, vel, [9], s, held=fx["held"][:9, :32], **kw)
        with pytest.raises(ValueError):
            rec.song_decode(idx, vel, [9], dict(s, velocity_threshold_such_that_it_is_a_played_note=float("nan")), **kw)
    with pytest.raises(ValueError):
        rec.song_metrics(fx["counts"], [3, 4], 64, s)


# ---- the fourth header -----------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_recon.h")
    assert declared == {"mvae_recon_abi_version", "mvae_recon_songs"} == set(hl.RECON_SIGNATURES)
    others = ("midivae_hip.h", "midivae_descriptors.h", "midivae_sweep.h")
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert name not in hl.SIGNATURES and name not in hl.DESC_SIGNATURES and name not in hl.SWEEP_SIGNATURES
        assert all(name not in _declared(h) for h in others)
    assert _declared("midivae_sweep.h") == set(hl.SWEEP_SIGNATURES) and _declared("midivae_descriptors.h") == set(hl.DESC_SIGNATURES)
    assert _declared("midivae_hip.h") == set(hl.SIGNATURES)
    assert lib.mvae_recon_abi_version() == 1 == hl.RECON_ABI_VERSION
    assert lib.mvae_sweep_abi_version() == 1 == hl.SWEEP_ABI_VERSION and lib.mvae_desc_abi_version() == 1 == hl.DESC_ABI_VERSION
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_recon.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_recon_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_recon_args, %s));' % (f, f) for f, _ in hl.ReconArgs._fields_]
    lines += ['printf("MVAE_RECON_COUNTS %d\\n", (int)MVAE_RECON_COUNTS);', 'printf("MVAE_RECON_MAX_T %d\\n", (int)MVAE_RECON_MAX_T);',
              'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.ReconArgs) and ctypes.sizeof(hl.ReconArgs) % 8 == 0
    for f, _ in hl.ReconArgs._fields_:
        assert int(got[f]) == getattr(hl.ReconArgs, f).offset, f
    assert int(got["MVAE_RECON_COUNTS"]) == rec.N_COUNTS and int(got["MVAE_RECON_MAX_T"]) == rec.MAX_T


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_recon_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert rcn.invoke(lib, rcn.baseline(rcn.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in rcn.ACCEPTED:
        assert rcn.invoke(lib, mutate(rcn.baseline(rcn.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("row", rcn.ROWS, ids=[r[0] for r in rcn.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = rcn.invoke(hl.load(), mutate(rcn.baseline(rcn.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_covers_every_documented_limit():
    names = " | ".join(r[0] for r in rcn.ROWS)
    for what in ("a NULL", "idx NULL", "all outputs NULL", "n = 0", "T = 0", "n_pitch = 0", "stride_t = 0", "stride_w = -1",
                 "orig_stride_t = 0", "orig_stride_w = -1", "voices = 1", "voices = 9", "T % voices", "ld_counts = 7", "silent = 256",
                 "silent = -2", "override_rules = 2", "override_rules = -1", "threshold = nan", "threshold = inf", "carry NULL",
                 "n_pitch = 193", "T = 65536 + 4"):
        assert what in names, what
    assert len([r for r in rcn.ROWS if r[3]]) >= 8
