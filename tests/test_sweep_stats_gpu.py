"""The latent sweep's statistics on the device (csrc/sweep.hip, mvae_sweep_windows) against the NumPy mirror of midi_vae_amd.sweep -
which tests/test_sweep_stats_cpu.py pins to the reference's own outputs - and against those outputs themselves.

Bounds (derived, not measured; the split of test_sweep_stats_cpu.py).  Counts, min, max, range, the three medians (selected values
and one exact halving) and the post-rule velocities (input values or zeros): BIT-EQUAL.  Pitch and position means: an exact integer
sum and one double division on both sides: bit-equal.  The velocity mean: device and mirror add the same doubles in the same (row)
order and divide once: bit-equal; against the reference it is bit-equal because at threshold 0.5 the sum of float32 values in
(0.5, 1] is exact in any order.  The stds: pitch and position take sqrt((c * sum(x^2) - sum(x)^2) / c^2) from the same exact integers
on both sides; the velocity std is the two-pass form, where the device may fuse (v - mean)^2 into the running sum: at most T = 4096
terms <= 1, one rounding of 1.1e-16 each - under 1e-12 absolute, the bound, also for positions <= 4095 (std <= 2048, a few roundings
of 1.1e-16 relative: 1e-12 absolute still holds).  Two layouts of the same windows run the same arithmetic per lane: bit-equal."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import sweep as sw
from tests import footprint as fp
from tests import sweep_contract as sc
from tests.gpu_util import DEV
from tests.sweep_contract import assert_table, load_fixture

pytestmark = pytest.mark.gpu
CHUNK_TICKS = 8          # csrc/sweep.hip stages this many ticks at a time


@pytest.fixture(scope="module")
def fx():
    f = load_fixture()
    f["mirror"], f["mirror_roll"] = sw.window_statistics(f["idx"], f["vel"], f["s"], device=False, return_velocity=True)
    return f


def settings(V=4, n_pitch=60, silent=True, threshold=0.5, override=True):
    return dict(max_voices=V, low_crop=24, high_crop=24 + n_pitch, include_silent_note=silent,
                velocity_threshold_such_that_it_is_a_played_note=threshold, override_sampled_pitches_based_on_velocity_info=override)


def time_major(idx, vel, pad_to=16):
    """the (n, T) views of time-major (T, Bp) device buffers; the pad columns hold notes and NaN velocities nobody may read"""
    n, T = idx.shape
    Bp = -(-n // pad_to) * pad_to
    ti = torch.full((T, Bp), 7, dtype=torch.uint8, device=DEV)
    ti[:, :n] = torch.from_numpy(np.ascontiguousarray(idx.T)).to(DEV)
    tv = None
    if vel is not None:
        tv = torch.full((T, Bp), float("nan"), dtype=torch.float32, device=DEV)
        tv[:, :n] = torch.from_numpy(np.ascontiguousarray(vel.T)).to(DEV)
        tv = tv.t()[:n]
    return ti.t()[:n], tv


def both_layouts(idx, vel, s, want_table, want_roll, what):
    """window-major (staged through LDS) and time-major (read directly) against the mirror's table and velocities"""
    for layout in ("window-major", "time-major"):
        a, v = (idx, vel) if layout == "window-major" else time_major(idx, vel)
        table, roll = sw.window_statistics(a, v, s, return_velocity=True)
        assert roll.dtype == np.float32 and np.array_equal(roll.view(np.uint32), want_roll.view(np.uint32)), "%s, %s: velocities" % (what, layout)
        assert_table(table, want_table, "%s, %s" % (what, layout))


def walks(rng, n, T, V, n_pitch, p_silent=0.3, p_hold=0.4, silent=None):
    """voice-wise random walks: steps of -4..4 columns, a rest with p_silent, else the last note again with p_hold"""
    ticks = T // V
    rest, hold = rng.random((n, ticks, V)) < p_silent, rng.random((n, ticks, V)) < p_hold
    step = np.where(hold, 0, rng.integers(-4, 5, (n, ticks, V)))
    step[rest] = 0
    q = np.clip(rng.integers(0, n_pitch, (n, 1, V)) + np.cumsum(step, 1), 0, n_pitch - 1)
    return np.where(rest, n_pitch if silent is None else silent, q).astype(np.uint8).reshape(n, T)


def velocities(rng, shape):
    """float32 in [0, 1], a third of them multiples of 1/8: ties in the selection"""
    v = rng.random(shape)
    return np.where(rng.random(shape) < 1 / 3, np.round(v * 8) / 8, v).astype(np.float32)


# ---- the reference's windows ---------------------------------------------------------------------------------------------------
def test_fixture_windows_window_major(fx):
    table, roll = sw.window_statistics(fx["idx"], fx["vel"], fx["s"], return_velocity=True)
    assert np.array_equal(roll.view(np.uint32), fx["velocity_rules_on"].view(np.uint32))
    assert_table(table, fx["table"], "device against the reference")
    assert_table(table, fx["mirror"], "device against the mirror")
    assert np.array_equal(sw.window_statistics(np.eye(61)[fx["idx"][:40]], fx["vel"][:40], fx["s"]), table[:40], equal_nan=True)


def _f64(buf):
    return np.ascontiguousarray(buf.bits()).view(np.uint64).view(np.float64)


def test_fixture_windows_time_major_padded_guarded(fx):
    """all 180 windows in (T, 192) buffers as the engine keeps them, ld_out = 24: bit-equal to the window-major run; columns 22..23,
    the pad rows of both outputs, every guard and both inputs as planted"""
    B, Bp, T, LD = 180, 192, 64, 24
    p = sw.params(fx["s"])
    rng = np.random.default_rng(7)
    ti = rng.integers(0, 61, (T, Bp)).astype(np.uint8)          # (valid notes in the pad columns)
    ti[:, :B] = fx["idx"].T
    tv = torch.full((T, Bp), float("nan"), dtype=torch.float32)
    tv[:, :B] = torch.from_numpy(np.ascontiguousarray(fx["vel"].T))
    ar = fp.Arena(DEV)
    b_idx = ar.carve("idx", (T, Bp), torch.uint8, data=ti, guard="zero")
    b_vel = ar.carve("vel", (T, Bp), torch.float32, data=tv)
    b_stats = ar.carve("stats", (Bp, 2 * LD), torch.float32)
    b_roll = ar.carve("vel_out", (Bp, T), torch.float32)
    ar.commit()
    stats = b_stats.t.view(torch.float64)
    assert stats.shape == (Bp, LD) and stats.data_ptr() == b_stats.t.data_ptr()
    sw.enqueue(b_idx.t[:, :B].t(), b_vel.t[:, :B].t(), p, stats, b_roll.t, torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(b_roll, np.s_[:B])
    ar.assert_written(b_stats, np.s_[:B, :44])
    ar.assert_untouched(b_roll, np.s_[B:])
    ar.assert_untouched(b_stats, np.s_[B:])
    ar.assert_untouched(b_stats, np.s_[:, 44:])
    assert np.array_equal(b_idx.bits(), ti) and np.array_equal(b_vel.bits(), tv.numpy().view(np.uint32))
    got = _f64(b_stats)[:B, :22]
    want, want_roll = sw.window_statistics(fx["idx"], fx["vel"], fx["s"], return_velocity=True)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "time-major differs from window-major"
    assert np.array_equal(b_roll.bits()[:B], want_roll.view(np.uint32))
    assert_table(np.ascontiguousarray(got), fx["table"], "time-major against the reference")


@pytest.mark.parametrize("n", [1, 65, 130])
def test_window_counts(fx, n):
    """a single window, a second workgroup of one lane, a third of two"""
    both_layouts(fx["idx"][:n], fx["vel"][:n], fx["s"], fx["mirror"][:n], fx["mirror_roll"][:n], "n = %d" % n)


# ---- T edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ticks", [(4, 1), (4, 2 * CHUNK_TICKS + 1), (2, 4 * CHUNK_TICKS + 1), (8, CHUNK_TICKS), (8, 2 * CHUNK_TICKS + 3), (2, 1)],
                         ids=lambda x: str(x))
def test_tick_counts_and_voices(V, ticks):
    """one tick, chunk remainders of the staged path, 2 and 8 voices; 70 windows (a six-lane tail workgroup)"""
    rng = np.random.default_rng(100 * V + ticks)
    T, n = V * ticks, 70
    s = settings(V=V)
    idx, vel = walks(rng, n, T, V, 60), velocities(rng, (n, T))
    want, want_roll = sw.window_statistics(idx, vel, s, device=False, return_velocity=True)
    assert (want[:, 9] > 0).any() and (want[:, 0] > 0).any()
    both_layouts(idx, vel, s, want, want_roll, "V = %d, %d ticks" % (V, ticks))


def test_long_windows_selection_and_counters():
    """T = 4096 at V = 4: velocities from 16 values (every digit of the selection meets ties), from 2 values, all distinct; even and odd
    counts of note starts; a window whose 4096 rows all start a note (the counters' width, the sums of the positions)"""
    rng = np.random.default_rng(4096)
    T, V, n = 4096, 4, 7
    s = settings(V=V, override=False)          # (rules off: the counts below are planted exactly)
    idx = walks(rng, n, T, V, 60, p_silent=0.0)
    vel = np.zeros((n, T), np.float32)
    vel[0] = 0.5 + (1 + rng.integers(0, 16, T)) / 32                      # 16 values, all rows start: count 4096 (even)
    vel[1] = vel[0]
    vel[1, 17] = 0.25                                                    # 4095 (odd)
    half = rng.permutation(T)[:T // 2]
    vel[2] = 0.875
    vel[2, half] = 0.625                                                 # two values, half and half: median (0.625 + 0.875) / 2
    vel[3] = (0.5 + (1 + rng.permutation(T)) / 8192).astype(np.float32)  # all distinct, even count
    vel[4] = vel[3]
    vel[4, 4000] = 0.0                                                   # all distinct, odd count
    vel[5] = velocities(rng, T)                                          # about half of the rows start
    vel[6] = np.float32(1.0)                                             # one value
    want, want_roll = sw.window_statistics(idx, vel, s, device=False, return_velocity=True)
    assert list(want[:5, 9]) == [4096, 4095, 4096, 4096, 4095] and want[2, 11] == 0.75 and want[6, 11] == 1 and want[6, 15] == 0
    assert want[0, 16] == 2047.5 == want[0, 17] and want[3, 11] == 0.5 + 4097 / 16384
    both_layouts(idx, vel, s, want, want_roll, "T = 4096")
    on = settings(V=V)
    want, want_roll = sw.window_statistics(idx[4:6], vel[4:6], on, device=False, return_velocity=True)
    both_layouts(idx[4:6], vel[4:6], on, want, want_roll, "T = 4096, rules on")


# ---- special windows -----------------------------------------------------------------------------------------------------------
def test_special_windows():
    rng = np.random.default_rng(11)
    T, V, n = 64, 4, 66
    idx, vel = walks(rng, n, T, V, 60), velocities(rng, (n, T))
    idx[0] = 60                                                          # all silent
    vel[1] *= np.float32(0.5)                                            # no velocity above the threshold
    idx[2, ::3], idx[3, ::2], idx[4, 1::2] = 255, 61, 200                # 255, and indices >= n_pitch that are not the silent one
    vel[5] = np.float32(0.5)                                             # exactly the threshold: neither silent nor a start
    for name, s, v in (("rules on", settings(), vel), ("rules off", settings(override=False), vel), ("no velocity head", settings(), None),
                       ("no silent index", settings(silent=False), vel), ("threshold 0.75", settings(threshold=0.75), vel),
                       ("48 columns: 48..59 do not sound", settings(n_pitch=48), vel)):
        want, want_roll = sw.window_statistics(idx, v, s, device=False, return_velocity=True)
        if name == "rules on":
            assert want[0, 0] == 0 and want[0, 9] == 0 and np.all(np.isnan(want[0, 1:7])) and np.all(np.isnan(want[0, 10:]))
            assert want[1, 9] == 0 and want[1, 0] > 0 and want[5, 9] == 0
        if name == "no velocity head":
            assert np.all(want_roll == 0.75) and np.all(want[:, 9] == T) and want[0, 0] == 0
        if name == "no silent index":
            assert want[0, 0] == 0          # (60 >= n_pitch does not sound either way)
        both_layouts(idx, v, s, want, want_roll, name)


def test_one_output_at_a_time(fx):
    """stats_out alone and vel_out alone give what the call with both gives"""
    p, n, T = sw.params(fx["s"]), 70, 64
    idx = torch.from_numpy(fx["idx"][:n]).to(DEV)
    vel = torch.from_numpy(fx["vel"][:n]).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    stats = torch.full((n, 22), -7.0, dtype=torch.float64, device=DEV)
    roll = torch.full((n, T), -7.0, dtype=torch.float32, device=DEV)
    sw.enqueue(idx, vel, p, stats, None, stream)
    sw.enqueue(idx, vel, p, None, roll, stream)
    assert_table(stats.cpu().numpy(), fx["mirror"][:n], "stats_out alone")
    assert np.array_equal(roll.cpu().numpy().view(np.uint32), fx["mirror_roll"][:n].view(np.uint32))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing(fx):
    """the safe rows of tests/sweep_contract.py on real buffers: the promised code, and every byte of the arena - the rolls, the
    sentinel-filled outputs, the guards - as planted; the baseline itself then runs inside its buffers"""
    ar, bufs = fp.Arena(DEV), {}

    def carve(name, shape, kind, out=False):
        if kind == "f64":
            bufs[name] = ar.carve(name, (shape[0], 2 * shape[1]), torch.float32)
        elif kind == "u8":
            bufs[name] = ar.carve(name, shape, torch.uint8, data=fx["idx"][:shape[0]], guard="zero")
        elif out:
            bufs[name] = ar.carve(name, shape, torch.float32)
        else:
            bufs[name] = ar.carve(name, shape, torch.float32, data=torch.from_numpy(fx["vel"][:shape[0]]))
        return 0x1000

    sc.baseline(carve)
    ar.commit()
    resolve = lambda name, shape, kind, out=False: bufs[name].t.data_ptr()
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in sc.ROWS if r[3]]
    assert len(safe) >= 8
    for name, mutate, code, _ in safe:
        rc = sc.invoke(lib, mutate(sc.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert sc.invoke(lib, sc.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(bufs["stats"])
    ar.assert_written(bufs["vel_out"])
    assert_table(_f64(bufs["stats"]), fx["table"][:sc.N], "baseline")
    assert np.array_equal(bufs["vel_out"].bits(), fx["velocity_rules_on"][:sc.N].view(np.uint32))
