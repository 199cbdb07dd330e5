"""Note events without a device: the NumPy mirror of midi_vae_amd.events against the notes the reference's own rolls_to_midi recorded
(tests/golden/midi_events.npz, written by tests/golden/make_midi_fixtures.py) and against the literal restatement of its tracker loop;
the per-voice program vote; the fifth header and the refusals of mvae_note_events; the root-level drop-in ``midi_functions``.

Bounds: everything is an integer - EQUAL, no tolerance anywhere."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import hiplib as hl
from midi_vae_amd import midifile as mf
from tests import events_contract as evc
from tests.events_contract import PASSES, load_fixture, pass_inputs
from tests.recon_contract import random_songs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def settings(V=4, n_pitch=60, threshold=0.5, smallest_note=16, silent=True):
    return dict(max_voices=V, low_crop=24, high_crop=24 + n_pitch, include_silent_note=silent,
                velocity_threshold_such_that_it_is_a_played_note=threshold, SMALLEST_NOTE=smallest_note)


def assert_same_table(got, want, what):
    assert got[0].dtype == ev.RECORD and np.array_equal(got[1], want[1]), "%s: offsets" % what
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, "%s: %d of %d notes differ, first at %d: %r vs %r" % (what, len(bad), len(want[0]), bad[0], got[0][bad[0]], want[0][bad[0]])


# ---- the reference's notes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PASSES)
@pytest.mark.parametrize("group", "ab")
def test_mirror_is_the_reference(fx, group, name):
    g = fx[group]
    vel, held = pass_inputs(g, name)
    got = ev.event_table(g["idx"], vel, held, g["lengths"], fx["s"], device=False)
    assert_same_table(got, g["notes_" + name], "group %s, pass %s" % (group, name))
    assert len(got[0]) > 100 and got[1][-1] == len(got[0])
    songs = ev.note_events(g["idx"], vel, held, g["lengths"], fx["s"], device=False)
    assert len(songs) == len(g["lengths"]) and np.array_equal(np.concatenate(songs), got[0])
    assert_same_table(ev.tracker_loop(g["idx"], vel, held, g["lengths"], ev.params(fx["s"])), g["notes_" + name], "the literal loop, %s %s" % (group, name))


def test_the_fixture_has_its_hard_cases(fx):
    a, low = fx["a"], fx["s"]["low_crop"]
    rec, off = a["notes_held"]
    hand = off[(len(a["lengths"]) - 2) * 4]          # the first hand-made song
    assert tuple(rec[hand]) == (0, 48, 10 + low, 0, rec[hand]["velocity"]), "the note held across three windows"
    assert off[-1] - off[-5] > 40 and {0, 127} <= set(rec[off[-5]:]["velocity"].tolist())
    for name in PASSES:
        spans = sum(int(np.sum(g["notes_" + name][0]["start"] // (g["idx"].shape[1] // 4) != (g["notes_" + name][0]["end"] - 1) // (g["idx"].shape[1] // 4)))
                    for g in (fx["a"], fx["b"]))
        assert spans > 0, name
    assert len(a["notes_held"][0]) != len(a["notes_tick"][0]) and np.all(a["notes_plain"][0]["velocity"] == 80)
    # closing at the end adds exactly the notes the reference drops: one per voice whose last row sounds
    for g in (fx["a"], fx["b"]):
        last = np.cumsum(g["lengths"]) - 1
        open_notes = int(np.sum(g["idx"][last, -4:] < 60))
        closed = ev.event_table(g["idx"], g["vel"], g["held"], g["lengths"], fx["s"], device=False, close_at_end=True)
        assert open_notes > 0 and len(closed[0]) == len(g["notes_held"][0]) + open_notes
        ends = closed[0]["end"][closed[1][1:][np.diff(closed[1]) > np.diff(g["notes_held"][1])] - 1]
        assert np.array_equal(np.sort(ends), np.sort(np.repeat(g["lengths"] * (g["idx"].shape[1] // 4), np.sum(g["idx"][last, -4:] < 60, 1))))


# ---- the mirror against the tracker loop -------------------------------------------------------------------------------------------
def test_mirror_is_the_tracker_loop_on_random_songs():
    rng = np.random.default_rng(20261022)
    negative = spanning = dropped = 0
    for case in range(200):
        V = int(rng.integers(2, 9))
        T = (V, 24 // V * V if 24 % V else 24, 64 // V * V)[case % 3]
        threshold = (0.5, 0.25)[case // 3 % 2]
        with_held = bool(case // 6 % 2)
        lengths = rng.integers(1, 7, int(rng.integers(1, 5)))
        idx, vel = random_songs(rng, lengths, T, V)
        vel[rng.random(vel.shape) < 0.05] = np.float32(1.5)
        held = (rng.random(idx.shape) < 0.7).astype(np.uint8) if with_held else None
        s = settings(V=V, threshold=threshold)
        want = ev.tracker_loop(idx, vel, held, lengths, ev.params(s))
        got = ev.event_table(idx, vel, held, lengths, s, device=False)
        assert_same_table(got, want, "case %d: V = %d, T = %d, threshold %g, held %s" % (case, V, T, threshold, with_held))
        plain = ev.event_table(idx, None, held, lengths, s, device=False)
        assert np.array_equal(plain[0][["start", "end", "pitch", "voice"]], got[0][["start", "end", "pitch", "voice"]])
        assert np.all(plain[0]["velocity"] == 80)
        negative += int(np.sum(got[0]["velocity"] < 0))
        spanning += int(np.sum(got[0]["start"] // (T // V) != (got[0]["end"] - 1) // (T // V)))
        closed = ev.event_table(idx, vel, held, lengths, s, device=False, close_at_end=True)
        dropped += len(closed[0]) - len(got[0])
    assert negative > 0 and spanning > 0 and dropped > 0          # (threshold 0.25: velocities in [0.25, 0.5) scale below zero)


def test_velocity_scaling():
    p = ev.params(settings())
    x = np.array([0.5, 1.0, 1.5, 0.625, 0.4999, 0.0, 0.75, 100.0, np.nan], np.float32)
    assert ev.note_velocities(x, p).tolist() == [0, 127, 127, 31, 0, 0, 63, 127, 0]
    p = ev.params(settings(threshold=0.25))
    assert ev.note_velocities(np.array([0.25, 0.375, 0.5, 0.2], np.float32), p).tolist() == [-42, -21, 0, 0]


def test_note_events_refuses_bad_inputs(fx):
    g = fx["b"]
    idx, vel = g["idx"][:6], g["vel"][:6]
    for device in (False, True):          # the checks of the device path come before anything touches a device
        for lengths in ([3, 4], [6, 0], [7, -1], []):
            with pytest.raises(ValueError):
                ev.note_events(idx, vel, None, lengths, fx["s"], device=device)
        with pytest.raises(ValueError):
            ev.note_events(idx[:, :22], vel[:, :22], None, [6], fx["s"], device=device)
        with pytest.raises(ValueError):
            ev.note_events(idx, vel, None, [6], dict(fx["s"], SMALLEST_NOTE=0), device=device)
        with pytest.raises(ValueError):
            ev.note_events(idx, vel, None, [6], dict(fx["s"], low_crop=200, high_crop=260), device=device)
    with pytest.raises(ValueError):
        ev.note_events(idx, vel[:, :20], None, [6], fx["s"], device=False)
    with pytest.raises(ValueError):
        ev.note_events(idx, vel, g["held"][:5], [6], fx["s"], device=False)


# ---- the vote ----------------------------------------------------------------------------------------------------------------------
def test_vote_for_programs_ties_go_to_the_program_seen_first():
    s = dict(instrument_attach_method="1hot-category")
    instr = np.array([[3, 1, 0, 5], [2, 1, 0, 5], [2, 4, 0, 6], [3, 4, 7, 6],          # song 0: ties 3-2, 1-4; 0 wins; tie 5-6
                      [9, 9, 9, 9],                                                    # song 1: one window
                      [1, 2, 2, 0], [2, 2, 1, 0], [2, 1, 1, 0]], np.uint8)             # song 2: clear winners that are not seen first
    assert ev.vote_for_programs(instr, [4, 1, 3], s) == [[24, 8, 0, 40], [72, 72, 72, 72], [16, 16, 8, 0]]
    assert ev.vote_for_programs(instr, [4, 1, 3], dict(instrument_attach_method="1hot-instrument"))[0] == [3, 1, 0, 5]
    # the reference's own loop (vae_evaluation.py:598-617), restated on programs
    rng = np.random.default_rng(7)
    instr = rng.integers(0, 3, (40, 4)).astype(np.uint8)
    want, lo = [], 0
    for m in (7, 13, 20):
        song = []
        for voice in range(4):
            votes = dict()
            for program in (instr[lo:lo + m, voice].astype(int) * 8).tolist():
                votes[program] = votes.get(program, 0) + 1
            best_program, highest_value = 0, 0
            for k in votes.keys():
                if votes[k] > highest_value:
                    best_program, highest_value = k, votes[k]
            song.append(best_program)
        want.append(song)
        lo += m
    assert ev.vote_for_programs(instr, [7, 13, 20], s) == want
    with pytest.raises(ValueError):
        ev.vote_for_programs(instr, [7, 13], s)


# ---- the fifth header --------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))


def test_header_hygiene():
    lib = hl.load()
    declared = _declared("midivae_events.h")
    assert declared == {"mvae_events_abi_version", "mvae_note_events"} == set(hl.EVENTS_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert all(name not in sig for sig in (hl.SIGNATURES, hl.DESC_SIGNATURES, hl.SWEEP_SIGNATURES, hl.RECON_SIGNATURES))
        assert all(name not in _declared(h) for h in ("midivae_hip.h", "midivae_descriptors.h", "midivae_sweep.h", "midivae_recon.h"))
    assert lib.mvae_events_abi_version() == 1 == hl.EVENTS_ABI_VERSION
    assert lib.mvae_recon_abi_version() == 1 and lib.mvae_sweep_abi_version() == 1 and lib.mvae_desc_abi_version() == 1
    assert lib.mvae_abi_version() == 9 == hl.ABI_VERSION


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_events.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_events_args));', 'printf("record %zu\\n", sizeof(mvae_note_event));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_events_args, %s));' % (f, f) for f, _ in hl.EventsArgs._fields_]
    lines += ['printf("r_%s %%zu\\n", offsetof(mvae_note_event, %s));' % (f, f) for f in ev.RECORD.names]
    lines += ['printf("MVAE_EVENTS_MAX_T %d\\n", (int)MVAE_EVENTS_MAX_T);',
              'printf("MVAE_EVENTS_DEFAULT_VELOCITY %d\\n", (int)MVAE_EVENTS_DEFAULT_VELOCITY);',
              'printf("workspace_bytes %zu\\n", MVAE_EVENTS_WORKSPACE_BYTES(167, 26, 4));', 'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.EventsArgs) and ctypes.sizeof(hl.EventsArgs) % 8 == 0
    for f, _ in hl.EventsArgs._fields_:
        assert int(got[f]) == getattr(hl.EventsArgs, f).offset, f
    assert int(got["record"]) == ev.RECORD.itemsize == 12
    for f in ev.RECORD.names:
        assert int(got["r_" + f]) == ev.RECORD.fields[f][1], f
    assert int(got["MVAE_EVENTS_MAX_T"]) == ev.MAX_T and int(got["MVAE_EVENTS_DEFAULT_VELOCITY"]) == ev.DEFAULT_VELOCITY
    assert int(got["workspace_bytes"]) == ev.workspace_bytes(167, 26, dict(voices=4))


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_events_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert evc.invoke(lib, evc.baseline(evc.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in evc.ACCEPTED:
        assert evc.invoke(lib, mutate(evc.baseline(evc.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("row", evc.ROWS, ids=[r[0] for r in evc.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = evc.invoke(hl.load(), mutate(evc.baseline(evc.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_covers_every_documented_limit():
    names = " | ".join(r[0] for r in evc.ROWS)
    for what in ("a NULL", "idx NULL", "song NULL", "workspace NULL", "offsets NULL", "total NULL", "records NULL", "n = 0", "T = 0",
                 "n_pitch = 0", "n_songs = 0", "n_songs > n", "stride_t = 0", "stride_w = -1", "voices = 1", "voices = 9", "T % voices",
                 "silent = 256", "silent = -2", "smallest_note = 0", "threshold = nan", "threshold = inf", "pitch_base = -1",
                 "pitch_base + n_pitch = 257", "close_at_end = 2", "close_at_end = -1", "capacity = -1", "T = 65536 + 4", "n * T = 2^31"):
        assert what in names, what
    assert len([r for r in evc.ROWS if r[3]]) >= 8


# ---- the drop-in -------------------------------------------------------------------------------------------------------------------
def test_root_midi_functions_writes_the_fixture_notes(fx, tmp_path):
    sys.path.insert(0, ROOT)
    import midi_functions
    g, V, low = fx["b"], 4, fx["s"]["low_crop"]
    bounds = np.concatenate([[0], np.cumsum(g["lengths"])])
    folder = str(tmp_path) + os.sep + "new" + os.sep
    for i in (1, 2):
        rows = g["idx"][bounds[i]:bounds[i + 1]].reshape(-1)
        Y = np.zeros((rows.size, 60))
        Y[np.nonzero(rows < 60)[0], rows[rows < 60]] = 1
        velocity, held_roll = g["vel"][bounds[i]:bounds[i + 1]].reshape(-1), g["held"][bounds[i]:bounds[i + 1]].reshape(-1)
        for name, kw in (("held", dict(velocity_roll=velocity, held_notes_roll=held_roll)), ("tick", dict(velocity_roll=velocity)),
                         ("plain", {})):
            path = midi_functions.rolls_to_midi(Y, fx["programs"], folder, "song%d_%s" % (i, name), fx["bpm"], **kw)
            assert path == folder + "song%d_%s.mid" % (i, name) and os.path.exists(path)
            got = mf.read_midi(path)
            assert got["division"] == 1000 and got["tempos"] == [(0, int(round(60e6 / fx["tempo"])))]
            rec, off = g["notes_" + name]
            for v in range(V):
                want = rec[off[i * V + v]:off[i * V + v + 1]]
                track = got["tracks"][1 + v]
                assert track["program"] == fx["programs"][v] and track["channel"] == v
                assert track["notes"] == [(int(r["start"]) * 1000, int(r["end"]) * 1000, int(r["pitch"]), min(max(int(r["velocity"]), 0), 127))
                                          for r in want]
            assert sum(len(t["notes"]) for t in got["tracks"]) == off[(i + 1) * V] - off[i * V] > 0
    Y[5, 3] = Y[5, 9] = 1
    with pytest.raises(NotImplementedError, match="polyphonic"):
        midi_functions.rolls_to_midi(Y, fx["programs"], folder, "no", fx["bpm"])
    M = midi_functions.programs_to_instrument_matrix([0, 40, 56, 32], "1hot-category", 4)
    assert M.shape == (4, 16) and M.argmax(1).tolist() == [0, 5, 7, 4]
