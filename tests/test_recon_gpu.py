"""The song-level decode on the device (csrc/recon.hip, mvae_recon_songs) against the NumPy mirror of midi_vae_amd.reconstruction -
which tests/test_recon_cpu.py pins to the reference's own outputs and to packers.apply_velocity_rules - and against those outputs.

Bounds (derived, not measured).  Velocities after the rules are input float32 values or zeros, note starts bytes, counts integers:
BIT-EQUAL throughout, in both layouts, no tolerance anywhere.  Shapes are the smallest at which the kernels can go wrong: a workgroup
holds 256 / voices windows (64 at four voices), so 63 / 65 / 257 windows, songs of 70 and 300 windows and song boundaries at windows
64 and 256 put the look-back and the song across workgroups."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import reconstruction as rec
from midi_vae_amd import sweep as sw
from tests import footprint as fp
from tests import recon_contract as rcn
from tests.gpu_util import DEV
from tests.recon_contract import load_fixture, random_songs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def settings(V=4, n_pitch=60, silent=True, threshold=0.5, override=True):
    return dict(max_voices=V, low_crop=24, high_crop=24 + n_pitch, include_silent_note=silent,
                velocity_threshold_such_that_it_is_a_played_note=threshold, override_sampled_pitches_based_on_velocity_info=override)


def time_major(a, fill, pad_to=16, dtype=torch.uint8):
    """the (n, T) view of a time-major (T, Bp) device buffer whose pad columns hold ``fill``, which nobody may read"""
    if a is None:
        return None
    n, T = a.shape
    Bp = -(-n // pad_to) * pad_to
    t = torch.full((T, Bp), fill, dtype=dtype, device=DEV)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)
    return t.t()[:n]


def assert_same(got, want, what):
    assert got["velocity"].dtype == np.float32 and got["velocity"].shape == want["velocity"].shape, what
    bad = np.argwhere(got["velocity"].view(np.uint32) != want["velocity"].view(np.uint32))
    assert bad.size == 0, "%s: %d velocities differ, first at window %d row %d: %r vs %r" % (
        what, len(bad), bad[0][0], bad[0][1], got["velocity"][tuple(bad[0])], want["velocity"][tuple(bad[0])])
    assert got["starts"].dtype == np.uint8 and np.array_equal(got["starts"], want["starts"]), "%s: note starts" % what
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], want["counts"]), "%s: counts" % what


def both_layouts(idx, vel, lengths, s, what, held=None, orig=None):
    """window-major host arrays and the views of time-major (T, Bp) buffers - NaN velocities, notes, note starts and other notes in the
    pad columns, the originals in a buffer of another pitch - against the mirror; returns the mirror's result"""
    want = rec.song_decode(idx, vel, lengths, s, held=held, orig=orig, device=False)
    assert_same(rec.song_decode(idx, vel, lengths, s, held=held, orig=orig), want, what + ", window-major")
    got = rec.song_decode(time_major(idx, 7), time_major(vel, float("nan"), dtype=torch.float32), lengths, s, held=time_major(held, 0),
                          orig=time_major(orig, 9, pad_to=32))
    assert_same(got, want, what + ", time-major")
    return want


def extras(rng, idx):
    """a held-notes index per row, and originals: the notes with about a third of the rows replaced"""
    held = (rng.random(idx.shape) < 0.6).astype(np.uint8)
    orig = np.where(rng.random(idx.shape) < 1 / 3, rng.integers(0, 61, idx.shape), idx).astype(np.uint8)
    return held, orig


# ---- the reference's songs -------------------------------------------------------------------------------------------------------
def test_fixture_songs(fx):
    want = both_layouts(fx["idx"], fx["vel"], fx["lengths"], fx["s"], "fixture", orig=fx["orig"])
    assert np.array_equal(want["velocity"].view(np.uint32), fx["velocity"].view(np.uint32))
    assert np.array_equal(want["starts"], fx["starts"]) and np.array_equal(want["counts"], fx["counts"])
    want = both_layouts(fx["idx"], fx["vel"], fx["lengths"], fx["s"], "fixture with a held head", held=fx["held"], orig=fx["orig"])
    assert np.array_equal(want["counts"], fx["counts_held"])


# ---- window counts, songs across workgroups ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[1], [63], [40, 25], [257], [70], [300], [64, 192, 44], [3] * 21 + [2]], ids=lambda l: "+".join(map(str, l[:4])))
def test_window_counts_and_song_boundaries(lengths):
    """1, 63, 65 and 257 windows; one song of 70 and one of 300 windows; song boundaries exactly at windows 64 and 256; many short songs"""
    rng = np.random.default_rng(sum(lengths) + len(lengths))
    idx, vel = random_songs(rng, lengths, 64, 4)
    held, orig = extras(rng, idx)
    want = both_layouts(idx, vel, lengths, settings(), "lengths %r" % (lengths[:4],), orig=orig)
    if sum(lengths) > len(lengths):
        alone = rec.song_decode(idx, vel, [1] * len(idx), settings(), device=False)["velocity"]
        assert np.any(alone != want["velocity"]), "nothing is carried in these songs"


@pytest.mark.parametrize("V,T", [(2, 8), (8, 16), (3, 9)], ids=lambda x: str(x))
def test_voices_and_rows(V, T):
    """two voices at T = 8 (128 windows a workgroup), eight at T = 16 (32), three (85 and a lane left over); 200 windows"""
    rng = np.random.default_rng(10 * V + T)
    lengths = [1, 90, 7, 102]
    idx, vel = random_songs(rng, lengths, T, V)
    held, orig = extras(rng, idx)
    both_layouts(idx, vel, lengths, settings(V=V), "V = %d, T = %d" % (V, T), orig=orig)
    both_layouts(idx, vel, lengths, settings(V=V), "V = %d, T = %d, held" % (V, T), held=held, orig=orig)


def test_long_windows():
    """T = 1024 at four voices: 32 staged chunks a window"""
    rng = np.random.default_rng(1024)
    lengths = [3, 1, 66]
    idx, vel = random_songs(rng, lengths, 1024, 4)
    both_layouts(idx, vel, lengths, settings(), "T = 1024", orig=extras(rng, idx)[1])


def test_a_voice_that_is_never_loud():
    """voice 0 of a 130-window song is loud on its first row only, stays on that pitch under the threshold for 128 whole windows and
    changes pitch, quietly, in the last: the look-back walks 129 records through two workgroup edges.  In a second song of 130
    windows it never plays at all: the walk finds nothing and is as long as the song"""
    rng = np.random.default_rng(130)
    lengths = [130, 130]
    idx, vel = random_songs(rng, lengths, 64, 4)
    idx[:, 0::4] = 60
    idx[0, 0], vel[0, 0] = 12, 0.8125
    idx[0, 4:64:4], vel[0, 4:64:4] = 12, 0.25          # the rest of window 0: the same pitch, quiet - the last pitch of the window
    idx[1:129, 0::4] = 12
    vel[1:129, 0::4] = 0.125
    idx[129, 0::4], vel[129, 0::4] = 20, 0.375
    want = both_layouts(idx, vel, lengths, settings(), "a voice that is never loud")
    assert want["velocity"][129, 0] == np.float32(0.8125) and np.all(want["velocity"][130:, 0::4] == 0)


# ---- switches ----------------------------------------------------------------------------------------------------------------------
def test_switches_and_missing_inputs():
    rng = np.random.default_rng(5)
    lengths = [5, 1, 70, 9]
    idx, vel = random_songs(rng, lengths, 64, 4)
    idx[2, ::3], idx[3, ::2], idx[4, 1::2] = 255, 61, 200          # 255, and indices >= n_pitch that are not the silent one
    vel[6] = np.float32(0.5)                                       # exactly the threshold: neither silent nor a start
    held, orig = extras(rng, idx)
    orig[7, ::5] = 255                                             # no target
    for name, s in (("threshold 0.0", settings(threshold=0.0)), ("threshold 0.75", settings(threshold=0.75)),
                    ("rules off", settings(override=False)), ("no silent index", settings(silent=False)),
                    ("48 columns: 48..59 do not sound", settings(n_pitch=48))):
        both_layouts(idx, vel, lengths, s, name, orig=orig)
    s = settings()
    no_vel = both_layouts(idx, None, lengths, s, "vel NULL", held=held, orig=orig)
    assert np.all(no_vel["velocity"] == 0.75) and np.array_equal(no_vel["starts"], held)
    both_layouts(idx, vel, lengths, s, "held NULL", orig=orig)
    no_orig = both_layouts(idx, vel, lengths, s, "orig NULL", held=held)
    assert np.all(no_orig["counts"][:, [0, 2, 3, 7]] == 0) and np.array_equal(no_orig["counts"][:, 4], no_orig["counts"][:, 1])
    neither = both_layouts(idx, None, lengths, s, "vel and held NULL", orig=orig)
    assert np.all(neither["starts"] == 1) and np.all(neither["counts"][:, 5:] == 0)


def test_without_first_window_it_is_the_sweep(fx):
    """first_window = NULL: every window its own song, vel_out bit-equal to mvae_sweep_windows' vel_out on the same buffers"""
    for layout in ("window-major", "time-major"):
        if layout == "window-major":
            idx, vel = torch.from_numpy(fx["idx"]).to(DEV), torch.from_numpy(fx["vel"]).to(DEV)
        else:
            idx, vel = time_major(fx["idx"], 7), time_major(fx["vel"], float("nan"), dtype=torch.float32)
        for s in (fx["s"], dict(fx["s"], override_sampled_pitches_based_on_velocity_info=False)):
            want = sw.window_statistics(idx, vel, s, return_velocity=True)[1]
            got = rec.run_on_device(idx, vel, None, None, None, rec.params(s))[0].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), layout
    want = sw.window_statistics(torch.from_numpy(fx["idx"]).to(DEV), None, fx["s"], return_velocity=True)[1]
    got = rec.run_on_device(torch.from_numpy(fx["idx"]).to(DEV), None, None, None, None, rec.params(fx["s"]))[0].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- which memory the kernels touch ----------------------------------------------------------------------------------------------------
def test_guarded_outputs_and_workspace(fx):
    """the fixture's 167 windows in time-major (T, 176) buffers, the originals window-major, ld_counts = 11: outputs and workspace
    written where they must be and nowhere else, columns 8..10 of the counts and every guard as planted, the inputs unchanged"""
    n, T, V, LD = len(fx["idx"]), 64, 4, 11
    Bp = -(-n // 16) * 16
    p = rec.params(fx["s"])
    rng = np.random.default_rng(3)
    ti = rng.integers(0, 61, (T, Bp)).astype(np.uint8)          # (valid notes in the pad columns)
    ti[:, :n] = fx["idx"].T
    tv = torch.full((T, Bp), float("nan"), dtype=torch.float32)
    tv[:, :n] = torch.from_numpy(np.ascontiguousarray(fx["vel"].T))
    first = rec.first_windows(fx["lengths"], n)
    ar = fp.Arena(DEV)
    b_idx = ar.carve("idx", (T, Bp), torch.uint8, data=ti, guard="zero")
    b_vel = ar.carve("vel", (T, Bp), torch.float32, data=tv)
    b_orig = ar.carve("orig", (n, T), torch.uint8, data=fx["orig"], guard="zero")
    b_first = ar.carve("first_window", (n,), torch.int32, data=torch.from_numpy(first))
    b_carry = ar.carve("carry", (n * V, 2), torch.int32)
    b_roll = ar.carve("vel_out", (n, T), torch.float32)
    b_start = ar.carve("start_out", (n, T), torch.uint8)
    b_counts = ar.carve("counts", (n, LD), torch.int32)
    ar.commit()
    assert rec.carry_bytes(n, p) == b_carry.nbytes
    rec.enqueue(b_idx.t.t()[:n], b_vel.t.t()[:n], None, b_orig.t, b_first.t, p, b_carry.t, b_roll.t, b_start.t, b_counts.t,
                torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(b_roll)
    ar.assert_written(b_carry)
    ar.assert_written(b_counts, np.s_[:, :8])
    ar.assert_untouched(b_counts, np.s_[:, 8:])
    assert np.array_equal(b_idx.bits(), ti) and np.array_equal(b_vel.bits(), tv.numpy().view(np.uint32))
    assert np.array_equal(b_orig.bits(), fx["orig"]) and np.array_equal(b_first.bits().view(np.int32), first)
    assert np.array_equal(b_roll.bits(), fx["velocity"].view(np.uint32))
    assert np.array_equal(b_start.bits(), fx["starts"])          # (0 and 1 everywhere: no byte kept the sentinel 0xFF)
    assert np.array_equal(b_counts.bits()[:, :8].view(np.int32), fx["counts"])


def test_one_output_at_a_time(fx):
    """each output alone gives what the call with all three gives"""
    n, p = len(fx["idx"]), rec.params(fx["s"])
    idx, vel, orig = (torch.from_numpy(fx[k]).to(DEV) for k in ("idx", "vel", "orig"))
    first = torch.from_numpy(rec.first_windows(fx["lengths"], n)).to(DEV)
    carry = torch.empty(rec.carry_bytes(n, p), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    roll = torch.full((n, 64), -7.0, dtype=torch.float32, device=DEV)
    start = torch.full((n, 64), 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((n, 8), -7, dtype=torch.int32, device=DEV)
    rec.enqueue(idx, vel, None, orig, first, p, carry, roll, None, None, stream)
    rec.enqueue(idx, vel, None, orig, first, p, carry, None, start, None, stream)
    rec.enqueue(idx, vel, None, orig, first, p, carry, None, None, counts, stream)
    assert np.array_equal(roll.cpu().numpy().view(np.uint32), fx["velocity"].view(np.uint32))
    assert np.array_equal(start.cpu().numpy(), fx["starts"]) and np.array_equal(counts.cpu().numpy(), fx["counts"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing(fx):
    """the safe rows of tests/recon_contract.py on real buffers: the promised code, and every byte of the arena - the rolls, the
    sentinel-filled outputs and workspace, the guards - as planted; the baseline itself then runs inside its buffers"""
    ar, bufs = fp.Arena(DEV), {}
    N = rcn.N
    first = np.array([0] * 5 + [5] * 12, np.int32)

    def carve(name, shape, kind, out=False):
        if kind == "i32":
            bufs[name] = ar.carve(name, shape, torch.int32, data=None if out else torch.from_numpy(first))
        elif kind == "u8" and not out:
            bufs[name] = ar.carve(name, shape, torch.uint8, data=fx[name][:N], guard="zero")
        elif kind == "u8":
            bufs[name] = ar.carve(name, shape, torch.uint8)
        elif out:
            bufs[name] = ar.carve(name, shape, torch.float32)
        else:
            bufs[name] = ar.carve(name, shape, torch.float32, data=torch.from_numpy(fx["vel"][:N]))
        return 0x1000

    rcn.baseline(carve)
    ar.commit()
    resolve = lambda name, shape, kind, out=False: bufs[name].t.data_ptr()
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in rcn.ROWS if r[3]]
    assert len(safe) >= 8
    for name, mutate, code, _ in safe:
        rc = rcn.invoke(lib, mutate(rcn.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert rcn.invoke(lib, rcn.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    for name in ("carry", "vel_out", "start_out", "counts"):
        ar.assert_written(bufs[name])
    want = rec.song_decode(fx["idx"][:N], fx["vel"][:N], [5, 12], fx["s"], held=fx["held"][:N], orig=fx["orig"][:N], device=False)
    assert np.array_equal(bufs["vel_out"].bits(), want["velocity"].view(np.uint32))
    assert np.array_equal(bufs["start_out"].bits(), want["starts"])
    assert np.array_equal(bufs["counts"].bits().view(np.int32), want["counts"])
