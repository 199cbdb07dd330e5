"""Note events on the device (csrc/events.hip, mvae_note_events) against the NumPy mirror of midi_vae_amd.events - which
tests/test_events_cpu.py pins to the reference's own notes and to its tracker loop - and against those notes.

Bounds (derived, not measured).  Ticks, pitches, voices and velocities are integers (the velocity one double expression per note, the
reference's operations in its order, truncated): BIT-EQUAL throughout, in both layouts, no tolerance anywhere.  Shapes are the smallest
at which the kernels can go wrong: a workgroup of the walk holds 256 / voices windows (64 at four voices), so 63 / 65 / 257 windows,
songs of 70 and 300 windows and song boundaries at windows 64 and 256 put a note, the previous window's last row and the song across
workgroups; the scan's workgroup takes 1024 / voices windows a pass (256 at four voices, 512 at two), so 257 and 300 windows at four
voices and 600 at two carry ranks from one pass of its loop into the next."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import hiplib as hl
from tests import events_contract as evc
from tests import footprint as fp
from tests.events_contract import PASSES, load_fixture, pass_inputs
from tests.gpu_util import DEV
from tests.recon_contract import random_songs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def settings(V=4, n_pitch=60, threshold=0.5, smallest_note=16, silent=True):
    return dict(max_voices=V, low_crop=24, high_crop=24 + n_pitch, include_silent_note=silent,
                velocity_threshold_such_that_it_is_a_played_note=threshold, SMALLEST_NOTE=smallest_note)


def time_major(a, fill, pad_to=16, dtype=torch.uint8):
    """the (n, T) view of a time-major (T, Bp) device buffer whose pad columns hold ``fill``, which nobody may read"""
    if a is None:
        return None
    n, T = a.shape
    Bp = -(-n // pad_to) * pad_to + pad_to
    t = torch.full((T, Bp), fill, dtype=dtype, device=DEV)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)
    return t.t()[:n]


def assert_same_table(got, want, what):
    assert got[0].dtype == ev.RECORD and got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), "%s: offsets" % what
    assert got[0].shape == want[0].shape, what
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, "%s: %d of %d notes differ, first at %d: %r vs %r" % (what, len(bad), len(want[0]), bad[0], got[0][bad[0]], want[0][bad[0]])


def both_layouts(idx, vel, held, lengths, s, what, close=False):
    """window-major host arrays and the views of time-major (T, Bp) buffers - other notes, NaN velocities and held flags in the pad
    columns - against the mirror; returns the mirror's table"""
    want = ev.event_table(idx, vel, held, lengths, s, device=False, close_at_end=close)
    assert_same_table(ev.event_table(idx, vel, held, lengths, s, close_at_end=close), want, what + ", window-major")
    got = ev.event_table(time_major(idx, 7), time_major(vel, float("nan"), dtype=torch.float32), time_major(held, 1), lengths, s,
                         close_at_end=close)
    assert_same_table(got, want, what + ", time-major")
    return want


# ---- the reference's songs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PASSES)
def test_fixture_songs(fx, name):
    for group in "ab":
        g = fx[group]
        vel, held = pass_inputs(g, name)
        want = both_layouts(g["idx"], vel, held, g["lengths"], fx["s"], "fixture %s, pass %s" % (group, name))
        assert_same_table(want, g["notes_" + name], "the mirror, %s %s" % (group, name))
        both_layouts(g["idx"], vel, held, g["lengths"], fx["s"], "fixture %s, pass %s, closed" % (group, name), close=True)
    songs = ev.note_events(fx["b"]["idx"], *pass_inputs(fx["b"], name), fx["b"]["lengths"], fx["s"])
    assert len(songs) == len(fx["b"]["lengths"]) and np.array_equal(np.concatenate(songs), fx["b"]["notes_" + name][0])


# ---- window counts, songs across workgroups and across the scan's passes ---------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[1], [63], [40, 25], [257], [70], [300], [64, 192, 44], [3] * 21 + [2]], ids=lambda l: "+".join(map(str, l[:4])))
def test_window_counts_and_song_boundaries(lengths):
    """1, 63, 65 and 257 windows; one song of 70 and one of 300 windows; song boundaries exactly at windows 64 and 256; many short songs"""
    rng = np.random.default_rng(sum(lengths) + len(lengths))
    idx, vel = random_songs(rng, lengths, 64, 4)
    held = (rng.random(idx.shape) < 0.8).astype(np.uint8)
    want = both_layouts(idx, vel, held, lengths, settings(), "lengths %r, held" % (lengths[:4],))
    both_layouts(idx, vel, None, lengths, settings(), "lengths %r, the tick rule" % (lengths[:4],), close=True)
    ticks = 16
    if max(lengths) > 1:
        assert np.any(want[0]["start"] // ticks != (want[0]["end"] - 1) // ticks), "no note spans a window boundary"


def test_one_note_through_a_whole_song():
    """voice 1 holds one pitch through all 300 windows of the middle song, every row held: one record with close_at_end - written by
    the lane of the song's first window, four workgroups and a scan pass before the song's end - and none without"""
    rng = np.random.default_rng(300)
    lengths = [3, 300, 2]
    idx, vel = random_songs(rng, lengths, 64, 4)
    held = (rng.random(idx.shape) < 0.5).astype(np.uint8)
    idx[3:303, 1::4], held[3:303, 1::4] = 33, 1
    s = settings()
    dropped = both_layouts(idx, vel, held, lengths, s, "held through the song")
    closed = both_layouts(idx, vel, held, lengths, s, "held through the song, closed", close=True)
    slot = 1 * 4 + 1
    assert dropped[1][slot + 1] - dropped[1][slot] == 0 and closed[1][slot + 1] - closed[1][slot] == 1
    note = closed[0][closed[1][slot]]
    assert (note["start"], note["end"], note["pitch"], note["voice"]) == (0, 300 * 16, 33 + 24, 1)
    assert note["velocity"] == ev.note_velocities(vel[3, 1], ev.params(s))


def test_every_row_starts_a_note_and_the_bound_is_met():
    """pitches alternate on every tick and the last tick is closed: records = rows = the capacity run_on_device allocates; beside it a
    song in which nothing sounds: empty ranges in the offsets"""
    n, T, V = 70, 64, 4
    lengths = [n]
    idx = np.where((np.arange(T) // V) % 2 == 0, 10, 11).astype(np.uint8)[None, :].repeat(n, 0)
    vel = np.random.default_rng(1).random((n, T)).astype(np.float32)
    want = both_layouts(idx, vel, None, lengths, settings(), "every row a note", close=True)
    assert len(want[0]) == n * T and np.all(want[0]["end"] - want[0]["start"] == 1)
    silent = np.concatenate([idx[:5], np.full((66, T), 60, np.uint8), idx[:3]])
    silent[20:30, ::3] = 255
    silent[30:40, ::5] = 200
    want = both_layouts(silent, None, None, [5, 66, 3], settings(), "a silent song between two others", close=True)
    assert np.all(want[1][4:9] == 5 * T) and want[1][-1] == 8 * T


@pytest.mark.parametrize("V,T,sn", [(2, 2, 16), (3, 3, 4), (8, 8, 16), (4, 24, 16), (2, 8, 16), (3, 9, 2), (8, 16, 3)], ids=lambda x: str(x))
def test_voices_rows_and_the_tick_rule(V, T, sn):
    """T = voices (one tick a window); T = 24 at four voices (six ticks a window: i % 16 falls inside windows); two voices (128 windows
    a workgroup, 512 a scan pass: 600 windows), three (85 and a lane left over; 341 a pass), eight (32; 128)"""
    rng = np.random.default_rng(100 * V + T)
    lengths = [1, 90, 7, 502] if V == 2 else [1, 90, 7, 102, 150]
    idx, vel = random_songs(rng, lengths, T, V)
    held = (rng.random(idx.shape) < 0.7).astype(np.uint8)
    s = settings(V=V, smallest_note=sn)
    both_layouts(idx, vel, None, lengths, s, "V = %d, T = %d, the tick rule" % (V, T))
    both_layouts(idx, vel, held, lengths, s, "V = %d, T = %d, held" % (V, T), close=True)
    both_layouts(idx, None, held, lengths, s, "V = %d, T = %d, held, no velocities" % (V, T))


def test_switches():
    rng = np.random.default_rng(5)
    lengths = [5, 1, 70, 9]
    idx, vel = random_songs(rng, lengths, 64, 4)
    idx[2, ::3], idx[3, ::2], idx[4, 1::2] = 255, 61, 200          # 255, and indices >= n_pitch that are not the silent one
    vel[6] = np.float32(0.5)                                       # exactly the threshold
    vel[7, ::2], vel[8, ::3] = np.float32(1.5), np.float32(-3.0)
    held = (rng.random(idx.shape) < 0.7).astype(np.uint8) * rng.integers(1, 256, idx.shape).astype(np.uint8)          # any non-zero byte holds
    for name, s in (("threshold 0.25: negative velocities", settings(threshold=0.25)), ("threshold 0.75", settings(threshold=0.75)),
                    ("threshold 0.0", settings(threshold=0.0)), ("no silent index", settings(silent=False)),
                    ("48 columns: 48..59 do not sound", settings(n_pitch=48)), ("a 12-tick bar", settings(smallest_note=12))):
        both_layouts(idx, vel, held, lengths, s, name + ", held")
        both_layouts(idx, vel, None, lengths, s, name + ", the tick rule", close=True)
    low = both_layouts(idx, vel, held, lengths, settings(threshold=0.25), "negative")
    assert np.any(low[0]["velocity"] < 0) and np.any(low[0]["velocity"] == 127)


# ---- which memory the kernels touch ----------------------------------------------------------------------------------------------------
def arena_call(fx, capacity, close=0):
    """the fixture's group a in time-major (T, Bp) buffers, every output and the workspace carved, guarded and sentinel-filled"""
    g = fx["a"]
    n, T, V = len(g["idx"]), 64, 4
    S = len(g["lengths"])
    Bp = -(-n // 16) * 16
    p = ev.params(fx["s"])
    rng = np.random.default_rng(3)
    ti = rng.integers(0, 61, (T, Bp)).astype(np.uint8)          # (valid notes in the pad columns)
    ti[:, :n] = g["idx"].T
    th = np.ones((T, Bp), np.uint8)
    th[:, :n] = g["held"].T
    tv = torch.full((T, Bp), float("nan"), dtype=torch.float32)
    tv[:, :n] = torch.from_numpy(np.ascontiguousarray(g["vel"].T))
    song = ev.song_ordinals(g["lengths"], n)
    ar = fp.Arena(DEV)
    b = dict(idx=ar.carve("idx", (T, Bp), torch.uint8, data=ti, guard="zero"), vel=ar.carve("vel", (T, Bp), torch.float32, data=tv),
             held=ar.carve("held", (T, Bp), torch.uint8, data=th, guard="zero"),
             song=ar.carve("song", (n,), torch.int32, data=torch.from_numpy(song)),
             workspace=ar.carve("workspace", (ev.workspace_bytes(n, S, p) // 4,), torch.int32),
             records=ar.carve("records", (max(capacity, 1) * 3,), torch.int32), offsets=ar.carve("offsets", (S * V + 1,), torch.int32),
             total=ar.carve("total", (1,), torch.int32))
    ar.commit()
    records = b["records"].t.view(torch.uint8)[:capacity * 12]
    ev.enqueue(b["idx"].t.t()[:n], b["vel"].t.t()[:n], b["held"].t.t()[:n], b["song"].t, S, p, close, b["workspace"].t.view(torch.uint8),
               records if capacity else None, b["offsets"].t, b["total"].t, torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    assert np.array_equal(b["idx"].bits(), ti) and np.array_equal(b["vel"].bits(), tv.numpy().view(np.uint32))
    assert np.array_equal(b["held"].bits(), th) and np.array_equal(b["song"].bits().view(np.int32), song)
    return ar, b


def test_guarded_outputs_and_workspace(fx):
    """records at their bound: outputs and workspace written where they must be and nowhere else, the records past the total and every
    guard as planted, the inputs unchanged"""
    g = fx["a"]
    n = len(g["idx"])
    want, off = g["notes_held"]
    ar, b = arena_call(fx, n * 64)
    ar.assert_written(b["workspace"])
    ar.assert_written(b["offsets"])
    ar.assert_written(b["total"])
    assert b["total"].bits().view(np.int32)[0] == len(want) and np.array_equal(b["offsets"].bits().view(np.int32), off)
    rec = b["records"].bits().reshape(-1, 3)
    ar.assert_written(b["records"], np.s_[:len(want) * 3])
    ar.assert_untouched(b["records"], np.s_[len(want) * 3:])
    assert np.array_equal(np.ascontiguousarray(rec[:len(want)]).view(ev.RECORD).reshape(-1), want)


@pytest.mark.parametrize("capacity", [0, 1, 1000])
def test_capacity_below_the_total(fx, capacity):
    """nothing at or past ``capacity`` changes - with capacity 0 the records pointer is NULL - the records below it are the first of
    the full table, and ``total`` and ``offsets`` still report the full count; closed at the end, so the starts write end fields too"""
    g = fx["a"]
    want, off = ev.event_table(g["idx"], g["vel"], g["held"], g["lengths"], fx["s"], device=False, close_at_end=True)
    assert len(want) > 1000
    ar, b = arena_call(fx, capacity, close=1)
    assert b["total"].bits().view(np.int32)[0] == len(want) and np.array_equal(b["offsets"].bits().view(np.int32), off)
    ar.assert_untouched(b["records"], np.s_[capacity * 3:])
    if capacity:
        ar.assert_written(b["records"], np.s_[:capacity * 3])
        got = np.ascontiguousarray(b["records"].bits().reshape(-1, 3)[:capacity]).view(ev.RECORD).reshape(-1)
        assert np.array_equal(got, want[:capacity])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing(fx):
    """the safe rows of tests/events_contract.py on real buffers: the promised code, and every byte of the arena - the rolls, the
    sentinel-filled outputs and workspace, the guards - as planted; the baseline itself then runs inside its buffers"""
    ar, bufs = fp.Arena(DEV), {}
    N, g = evc.N, fx["a"]
    song = np.array([0] * 5 + [1] * 12, np.int32)

    def carve(name, shape, kind, out=False):
        if kind == "i32":
            bufs[name] = ar.carve(name, shape, torch.int32, data=None if out else torch.from_numpy(song))
        elif kind == "u8":
            bufs[name] = ar.carve(name, shape, torch.uint8, data=g[name][:N], guard="zero")
        else:
            bufs[name] = ar.carve(name, shape, torch.float32, data=torch.from_numpy(g["vel"][:N]))
        return 0x1000

    evc.baseline(carve)
    ar.commit()
    resolve = lambda name, shape, kind, out=False: bufs[name].t.data_ptr()
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in evc.ROWS if r[3]]
    assert len(safe) >= 8
    for name, mutate, code, _ in safe:
        rc = evc.invoke(lib, mutate(evc.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert evc.invoke(lib, evc.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    for name in ("workspace", "offsets", "total"):
        ar.assert_written(bufs[name])
    want, off = ev.event_table(g["idx"][:N], g["vel"][:N], g["held"][:N], [5, 12], fx["s"], device=False)
    assert bufs["total"].bits().view(np.int32)[0] == len(want) > 0 and np.array_equal(bufs["offsets"].bits().view(np.int32), off)
    assert np.array_equal(np.ascontiguousarray(bufs["records"].bits()[:len(want)]).view(ev.RECORD).reshape(-1), want)
    ar.assert_untouched(bufs["records"], np.s_[len(want):])
