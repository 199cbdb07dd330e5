"""Rolls from notes on the device (csrc/import.hip, mvae_rolls_from_notes) against the NumPy mirror of midi_vae_amd.midi_import - which
tests/test_midi_import_cpu.py pins to what the reference's own load_rolls returned and to its tick loops.

Bounds (derived, not measured).  Indices, flags, raw velocities, counts and slots are integers; the float velocity is ONE double
expression per row, product and sum rounded separately as NumPy rounds them, then rounded to float32: BIT-EQUAL throughout, in both
layouts, no tolerance anywhere.  Shapes are the smallest at which the kernels can go wrong: a workgroup is 256 lanes, so a song of 700
ticks (2800 rows at four voices, three passes of the per-track reduction) puts rows, records and a track's ticks across workgroups and
loop passes; 40 songs in one call put records of different songs into one wave and 40 song bounds into the binary searches; T = 8 / 24
at four voices, 6 at two and 8 at eight (one tick a window) move the window bounds against the ticks."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import hiplib as hl
from midi_vae_amd import midi_import as mi
from tests import footprint as fp
from tests import import_contract as ic
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

OUTPUTS = (("idx", torch.uint8), ("held", torch.uint8), ("vel_raw", torch.uint8), ("vel", torch.float32))


@pytest.fixture(scope="module")
def fx():
    return ic.load_fixture()


def assert_same(got, want, what):
    for name in ("idx", "held", "vel_raw", "slots", "slot_voice", "lengths"):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs in %d places" % (what, name, int((a != b).sum()) if a.shape == b.shape else -1)
    assert got["vel"].dtype == np.float32 and np.array_equal(got["vel"].view(np.uint32), want["vel"].view(np.uint32)), "%s: vel" % what
    assert len(got["concurrent"]) == len(want["concurrent"]) and all(np.array_equal(a, b) for a, b in zip(got["concurrent"], want["concurrent"])), what
    assert got["programs"] == want["programs"], what


def arena_call(tables, s, T=None, layout="window", vel=True, raw=True, extra=3):
    """one call on carved, guarded, sentinel-filled buffers: the outputs hold ``extra`` windows (window-major) or 16 .. 31 pad columns
    (time-major) the call does not own.  Checks guards, inputs, that every owned row was written and nothing else; returns what the
    outputs hold in the shape of the mirror's dict (without programs)."""
    p = mi.params(s)
    T = p["T"] if T is None else T
    V, S = p["voices"], len(tables)
    packed = mi.pack_tables(tables, p, T)
    n, n_notes, n_tracks, cells = int(packed["lengths"].sum()), len(packed["notes"]), int(packed["track_off"][-1]), packed["cells"]
    assert n_notes > 0 and n_tracks > 0
    ar = fp.Arena(DEV)
    inputs = dict(notes=packed["notes"].view(np.int32).reshape(-1, 3), note_off=packed["note_off"], track_off=packed["track_off"],
                  ticks=packed["ticks"], win_off=packed["win_off"])
    b = {k: ar.carve(k, a.shape, torch.int32, data=torch.from_numpy(np.ascontiguousarray(a))) for k, a in inputs.items()}
    Bp = -(-n // 16) * 16 + 16
    shape = (n + extra, T) if layout == "window" else (T, Bp)
    for name, dtype in OUTPUTS:
        b[name] = ar.carve(name, shape, dtype)
    b["workspace"] = ar.carve("workspace", (mi.workspace_bytes(cells, S) // 4,), torch.int32)
    b["concurrent"] = ar.carve("concurrent", (n_tracks,), torch.int32)
    b["slots"] = ar.carve("slots", (S * V,), torch.int32)
    b["slot_voice"] = ar.carve("slot_voice", (S * V,), torch.int32)
    ar.commit()
    view = (lambda t: t[:n]) if layout == "window" else (lambda t: t.t()[:n])
    dev = {k: b[k].t for k in ("note_off", "track_off", "ticks", "win_off", "concurrent", "slots", "slot_voice")}
    dev["notes"] = b["notes"].t
    mi.enqueue(dev, p, T, S, n_notes, n_tracks, n, cells, b["workspace"].t, view(b["idx"].t), view(b["held"].t),
               view(b["vel_raw"].t) if raw else None, view(b["vel"].t) if vel else None, torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    for k, a in inputs.items():
        assert np.array_equal(b[k].bits().view(np.int32), a), "input %s changed" % k
    own, rest = (np.s_[:n], np.s_[n:]) if layout == "window" else (np.s_[:, :n], np.s_[:, n:])
    out = {}
    for name, _ in OUTPUTS:
        if (name == "vel" and not vel) or (name == "vel_raw" and not raw):
            ar.assert_untouched(b[name])
            continue
        ar.assert_written(b[name], own)
        ar.assert_untouched(b[name], rest)
        bits = b[name].bits()[own]
        out[name] = np.ascontiguousarray(bits if layout == "window" else bits.T)
    if vel:
        out["vel"] = out["vel"].view(np.float32)
    for name in ("workspace", "concurrent", "slots", "slot_voice"):
        ar.assert_written(b[name])
    conc = b["concurrent"].bits().view(np.int32)
    out["concurrent"] = [conc[packed["track_off"][i]:packed["track_off"][i + 1]] for i in range(S)]
    out["slots"], out["slot_voice"] = b["slots"].bits().view(np.int32).reshape(S, V), b["slot_voice"].bits().view(np.int32).reshape(S, V)
    out["lengths"] = packed["lengths"]
    return out


def everywhere(tables, s, what, T=None):
    """the Python surface and both layouts on guarded buffers against the mirror; returns the mirror's dict"""
    want = mi.rolls_from_notes(tables, s, device=False, T=T)
    assert_same(mi.rolls_from_notes(tables, s, T=T), want, what + ", rolls_from_notes")
    for layout in ("window", "time"):
        got = arena_call(tables, s, T, layout)
        assert_same(dict(got, programs=want["programs"]), want, "%s, %s-major" % (what, layout))
    return want


# ---- the reference's songs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", "abc")
def test_fixture_songs(fx, group):
    """all readable songs of a group in ONE call, the songs without a usable note among them: every output equals the mirror, and
    through load_rolls the device gives the reference's X, Y, I, tempo, V, D bit for bit"""
    g = fx[group]
    tables = ic.fixture_tables(g)
    want = everywhere(tables, g["s"], "fixture %s" % group)
    assert any(not x for x in want["programs"]) and any(len(x) == 4 for x in want["programs"])
    for x in g["songs"][:6]:
        got = mi.rolls_of_song(x["song"], g["s"], device=True)
        for name, a, b in zip("XYItVD", got, x["want"]):
            assert np.array_equal(np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)), "%s %s: %s" % (group, x["name"], name)


# ---- seeded songs at the smallest shapes that can go wrong -----------------------------------------------------------------------
@pytest.mark.parametrize("V,T", [(4, 8), (4, 24), (2, 6), (8, 8)], ids=str)
@pytest.mark.parametrize("M", [1, 2, 3])
def test_random_songs(V, T, M):
    """1..6 tracks, chords up to 5 deep, songs of 1..5 windows, 9 songs a call"""
    rng = np.random.default_rng(1000 * V + 10 * T + M)
    tables = ic.random_tables(rng, 9, V, T)
    want = everywhere(tables, ic.settings(V=V, T=T, M=M), "V = %d, T = %d, M = %d" % (V, T, M))
    assert sorted(set(want["lengths"].tolist())) != [1] and max(int(c.max()) for c in want["concurrent"]) > M
    assert np.any(want["held"] == 1) and np.any(want["vel_raw"] > 0)


def test_a_song_across_workgroups_between_short_ones():
    """700 ticks: 2800 rows and, per track, three passes of the 256-lane reduction - the count's maximum planted on tick 699"""
    rng = np.random.default_rng(700)
    tables = ic.random_tables(rng, 2, 4, 24) + ic.random_tables(rng, 1, 4, 24, ticks=700) + ic.random_tables(rng, 1, 4, 24)
    long = tables[2]
    last = np.array([(699, 700, 50 + k, 100, 0) for k in range(7)], mi.NOTE)
    notes = np.concatenate([long["notes"], last])
    long["notes"] = notes[np.lexsort((notes["pitch"], notes["start"], notes["track"]))]
    for M in (1, 3):
        want = everywhere(tables, ic.settings(T=24, M=M), "700 ticks, M = %d" % M)
        assert want["concurrent"][2][0] >= 7 and want["lengths"][2] == -(-700 * 4 // 24)


def test_forty_songs_in_one_call():
    """short songs, a handful of records each: records of several songs in one wave, empty songs (no track, or no tick) between"""
    rng = np.random.default_rng(40)
    tables = ic.random_tables(rng, 40, 4, 8, max_windows=2, max_tracks=3, depth=2)
    tables[5] = dict(ticks=3, programs=[], tempo=120.0, notes=np.zeros(0, mi.NOTE))
    tables[17] = dict(ticks=0, programs=[7], tempo=120.0, notes=np.zeros(0, mi.NOTE))
    want = everywhere(tables, ic.settings(T=8, M=2), "40 songs")
    assert want["lengths"][17] == 0 and want["lengths"][5] == 2 and np.all(want["idx"][want["lengths"][:5].sum():][:2] == 60)
    assert min(len(t["notes"]) for t in tables) < 64


def test_switches():
    rng = np.random.default_rng(9)
    tables = ic.random_tables(rng, 6, 4, 24)
    for what, s in (("threshold 0", ic.settings(T=24, threshold=0.0)), ("threshold 0.9", ic.settings(T=24, threshold=0.9)),
                    ("the full range", ic.settings(T=24, low=0, high=128, M=2)), ("a narrow crop", ic.settings(T=24, low=60, high=64, M=3)),
                    ("one voice", ic.settings(V=1, T=5, M=2))):
        everywhere(tables, s, what)


@pytest.mark.parametrize("vel,raw", [(False, True), (True, False), (False, False)], ids=["no vel", "no vel_raw", "neither"])
def test_optional_outputs(vel, raw):
    """vel = NULL and vel_raw = NULL: the buffers are not touched, the other outputs are the same"""
    rng = np.random.default_rng(3)
    tables = ic.random_tables(rng, 5, 4, 24)
    s = ic.settings(T=24, M=2)
    want = mi.rolls_from_notes(tables, s, device=False)
    for layout in ("window", "time"):
        got = arena_call(tables, s, layout=layout, vel=vel, raw=raw)
        for name in ("idx", "held") + (("vel_raw",) if raw else ()):
            assert np.array_equal(got[name], want[name]), name
        if vel:
            assert np.array_equal(got["vel"].view(np.uint32), want["vel"].view(np.uint32))


def test_device_tensors_stay_on_the_device(fx):
    g = fx["a"]
    tables = ic.fixture_tables(g)
    r = mi.rolls_from_notes(tables, g["s"], as_device=True)
    want = mi.rolls_from_notes(tables, g["s"], device=False)
    for name, dtype in OUTPUTS:
        assert r[name].is_cuda and r[name].dtype == dtype and np.array_equal(r[name].cpu().numpy(), want[name])


# ---- notes -> rolls -> notes -> rolls -------------------------------------------------------------------------------------------------
def test_device_round_trip(fx):
    """mvae_note_events (closed at the end) on the device's own rolls, the records repacked on the host, mvae_rolls_from_notes again:
    idx and held come back exactly.  The CONDITION is one voice per track and every pitch inside the crop, asserted on the inputs."""
    g = fx["a"]
    s = g["s"]
    V = s["max_voices"]
    tables = [mi.quantise(x["song"], s) for x in g["songs"] if x["name"] in ("mono4", "mono2")]
    r = mi.rolls_from_notes(tables, s, as_device=True)
    for table, conc, slots in zip(tables, r["concurrent"], r["slots"]):
        k = len(table["programs"])
        assert np.all(conc == 1) and slots.tolist() == list(range(k)) + [-1] * (V - k), "one voice per track"
        assert np.all((table["notes"]["pitch"] >= s["low_crop"]) & (table["notes"]["pitch"] < s["high_crop"])), "a cropped pitch"
    p = ev.params(s)
    song = torch.from_numpy(ev.song_ordinals(r["lengths"], len(r["idx"]))).to(r["idx"].device)
    rec, off = ev.read_back(*ev.run_on_device(r["idx"], r["vel"], r["held"], song, len(tables), p, close=True)[:2])
    assert len(rec) == sum(len(t["notes"]) for t in tables)
    back = []
    for i, table in enumerate(tables):
        mine = rec[off[i * V]:off[(i + 1) * V]]
        notes = np.zeros(len(mine), mi.NOTE)
        notes["start"], notes["end"], notes["pitch"], notes["track"] = mine["start"], mine["end"], mine["pitch"], mine["voice"]
        notes["velocity"] = np.clip(mine["velocity"], 0, 127)
        back.append(dict(ticks=table["ticks"], programs=table["programs"], tempo=table["tempo"], notes=notes))
    again = mi.rolls_from_notes(back, s)
    idx, held = r["idx"].cpu().numpy(), r["held"].cpu().numpy()
    assert np.array_equal(again["idx"], idx) and np.array_equal(again["held"], held) and np.array_equal(again["slots"], r["slots"])
    want = np.zeros(idx.shape, np.uint8)
    rows = np.repeat(np.concatenate([[0], np.cumsum(r["lengths"])])[:-1] * idx.shape[1], [off[(i + 1) * V] - off[i * V] for i in range(len(tables))])
    want.reshape(-1)[rows + rec["start"] * V + rec["voice"]] = np.clip(rec["velocity"], 0, 127)
    assert np.array_equal(again["vel_raw"], want)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing():
    """the safe rows of tests/import_contract.py on real buffers: the promised code, and every byte of the arena - the inputs, the
    sentinel-filled outputs and workspace, the guards - as planted; the baseline itself then runs inside its buffers"""
    tables = ic.baseline_tables()
    s = ic.settings(T=ic.T)
    packed = mi.pack_tables(tables, mi.params(s), ic.T)
    assert (int(packed["lengths"].sum()), int(packed["track_off"][-1]), packed["cells"], len(packed["notes"])) == (ic.N_WINDOWS, ic.N_TRACKS, ic.CELLS, ic.N_NOTES)
    inputs = dict(notes=packed["notes"].view(np.int32).reshape(-1, 3), note_off=packed["note_off"], track_off=packed["track_off"],
                  ticks=packed["ticks"], win_off=packed["win_off"])
    ar, bufs = fp.Arena(DEV), {}

    def carve(name, shape, kind, out=False):
        dtype = {"i32": torch.int32, "u8": torch.uint8, "f32": torch.float32}[kind]
        bufs[name] = ar.carve(name, shape, dtype, data=None if out else torch.from_numpy(np.ascontiguousarray(inputs[name])))
        return 0x1000

    ic.baseline(carve)
    ar.commit()
    resolve = lambda name, shape, kind, out=False: bufs[name].t.data_ptr()
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in ic.ROWS if r[3]]
    assert len(safe) >= 8
    for name, mutate, code, _ in safe:
        rc = ic.invoke(lib, mutate(ic.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert ic.invoke(lib, ic.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    want = mi.rolls_from_notes(tables, s, device=False)
    for name, _ in OUTPUTS:
        ar.assert_written(bufs[name])
        assert np.array_equal(bufs[name].bits(), want[name].view(np.uint32) if name == "vel" else want[name]), name
    assert np.array_equal(bufs["slots"].bits().view(np.int32).reshape(ic.S, ic.V), want["slots"])
    assert np.array_equal(bufs["concurrent"].bits().view(np.int32), np.concatenate(want["concurrent"]))
