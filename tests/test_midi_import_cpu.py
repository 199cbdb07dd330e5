"""MIDI import without a device: the NumPy mirror of midi_vae_amd.midi_import against what the reference's own load_rolls returned
(tests/golden/import_rolls.npz) and against its tick loops restated; the file round trip; import_folder; the sixth header and the
refusals of mvae_rolls_from_notes; the root-level drop-in.

Bounds: ticks, pitches, flags and raw velocities are integers, X / Y / D are 0 / 1 and V is one double expression written in the
reference's order - BIT-EQUAL in float64, no tolerance anywhere."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import hiplib as hl
from midi_vae_amd import midi_import as mi
from midi_vae_amd import midifile
from tests import import_contract as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return ic.load_fixture()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                                        b.view(np.uint64) if b.dtype == np.float64 else b)


# ---- the reference's songs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", "abc")
def test_load_rolls_reproduces_the_reference(fx, group):
    """X, Y, I, tempo, V, D of every song of the fixture, the None songs included, bit for bit in float64"""
    g = fx[group]
    nones = 0
    for x in g["songs"]:
        got = (None,) * 6 if x["song"] is None else mi.rolls_of_song(x["song"], g["s"], device=False)
        for name, a, b in zip(("X", "Y", "I", "tempo", "V", "D"), got, x["want"]):
            assert (a is None) == (b is None), "%s %s: %s" % (group, x["name"], name)
            if a is not None:
                assert same_bits(np.float64(a) if name == "tempo" else a, np.float64(b) if name == "tempo" else b), \
                    "%s %s: %s differs from the reference" % (group, x["name"], name)
        nones += got[0] is None
    assert nones == 3


def test_the_fixture_kept_its_point(fx):
    """a few of the generator's assertions again, on what was committed: an override, a cropped row that keeps flag and velocity, the
    X[-0:] quirk"""
    g = fx["a"]
    by_name = {x["name"]: x for x in g["songs"]}
    table = mi.quantise(by_name["override"]["song"], g["s"])
    r = mi.rolls_from_notes([table], g["s"], device=False)
    assert r["slots"][0].tolist() == [0, 0, 0, 1] and r["slot_voice"][0].tolist() == [0, 1, 2, 0] and r["concurrent"][0].tolist() == [3, 2]
    cropped = r["idx"] == 60
    assert np.any(cropped & (r["held"] == 1)) and np.any(cropped & (r["vel_raw"] > 0))
    grid = by_name["grid"]["want"][1]
    assert np.all(grid[..., -1] == 1) and np.any(grid[..., :-1].sum(-1) == 1)
    quiet = mi.rolls_from_notes([mi.quantise(by_name["silent_voice"]["song"], g["s"])], g["s"], device=False)
    assert quiet["slots"][0].tolist() == [0, 0, -1, -1] and np.all(quiet["idx"][:, 1::4] == 60)


# ---- the mirror against the reference's loops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,T,M", [(4, 8, 1), (4, 24, 2), (2, 6, 3), (8, 8, 1), (1, 4, 2)], ids=str)
def test_mirror_equals_the_tick_loops(V, T, M):
    rng = np.random.default_rng(100 * V + T + M)
    s = ic.settings(V=V, T=T, M=M)
    p = mi.params(s)
    tables = ic.random_tables(rng, 12, V, T)
    r = mi.rolls_from_notes(tables, s, device=False)
    lo = 0
    for i, table in enumerate(tables):
        idx, held, raw, conc, slots, voice = mi.tick_loops(table, p)
        rows, m = table["ticks"] * V, int(r["lengths"][i])
        for name, got, want, fill in (("idx", r["idx"], idx, p["silent"]), ("held", r["held"], held, 0), ("vel_raw", r["vel_raw"], raw, 0)):
            flat = got[lo:lo + m].reshape(-1)
            assert np.array_equal(flat[:rows], want) and np.all(flat[rows:] == fill), "song %d: %s" % (i, name)
        assert np.array_equal(r["concurrent"][i], conc) and np.array_equal(r["slots"][i], slots) and np.array_equal(r["slot_voice"][i], voice)
        lo += m
    assert lo == len(r["idx"]) and r["vel"].dtype == np.float32
    assert np.array_equal(r["vel"], np.where(r["vel_raw"] > 0, 0.5 + (r["vel_raw"] / 127.0) * 0.5, 0.0).astype(np.float32))


def test_quantise_rounds_half_to_even_and_keeps_the_end_unshifted():
    s = ic.settings()
    tick = 0.125
    song = dict(instruments=[dict(program=3, notes=np.array([[2.5 * tick, 5 * tick, 60, 80], [3.5 * tick, 6 * tick, 62, 81],
                                                             [10.3 * tick, 10.45 * tick, 64, 82], [12.3 * tick, 14.2 * tick, 65, 83]]))],
                tempo_changes=(np.array([0.0]), np.array([120.0])), end_time=2.0)
    t = mi.quantise(song, s)
    assert t["ticks"] == 16 and t["programs"] == [3] and t["notes"]["start"].tolist() == [2, 4, 12] and t["notes"]["end"].tolist() == [5, 6, 14]
    # the longest steady part is the middle one: 1 s .. 4 s at 120 bpm; the end stays 4 s, so ceil(4 * 8) = 32 ticks, not 24
    song = dict(instruments=[dict(program=0, notes=np.array([[0.0, 0.5, 60, 80], [1.0, 1.5, 61, 80], [3.5, 4.25, 62, 80]]))],
                tempo_changes=(np.array([0.0, 1.0, 4.0]), np.array([90.0, 120.0, 60.0])), end_time=5.0)
    t = mi.quantise(song, s)
    assert t["ticks"] == 32 and t["tempo"] == 120.0 and t["notes"]["pitch"].tolist() == [61] and t["notes"]["start"].tolist() == [0]


def test_refused_settings():
    table = ic.random_tables(np.random.default_rng(0), 1, 4, 8)
    for bad in (dict(T=6), dict(V=9, T=9), dict(low=-1), dict(high=129), dict(M=0), dict(threshold=1.0), dict(threshold=float("nan")),
                dict(include_only_monophonic_instruments=True)):
        with pytest.raises(ValueError):
            mi.rolls_from_notes(table, ic.settings(**bad), device=False)


# ---- through a file and back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mono4", "mono2"])
def test_file_round_trip(fx, name, tmp_path):
    """rolls -> note events (closed at the end) -> write_midi -> read_song -> quantise -> rolls: idx and held come back exactly, vel_raw
    as the velocities the events carry.  The CONDITION is one voice per track, every pitch inside the crop - asserted on the inputs.
    The writer makes one roll tick one beat, so the file is read with SMALLEST_NOTE = 4 (one tick a quarter note)."""
    g = fx["a"]
    s = g["s"]
    V = s["max_voices"]
    song = next(x["song"] for x in g["songs"] if x["name"] == name)
    table = mi.quantise(song, s)
    r = mi.rolls_from_notes([table], s, device=False)
    tracks = len(table["programs"])
    assert np.all(r["concurrent"][0] == 1) and r["slots"][0].tolist() == list(range(tracks)) + [-1] * (V - tracks), "one voice per track"
    assert np.all((table["notes"]["pitch"] >= s["low_crop"]) & (table["notes"]["pitch"] < s["high_crop"])), "a cropped pitch"
    songs = ev.note_events(r["idx"], r["vel"], r["held"], [len(r["idx"])], s, device=False, close_at_end=True)
    rec = songs[0]
    assert len(rec) == len(table["notes"])
    path = str(tmp_path / (name + ".mid"))
    midifile.write_midi(path, [rec[rec["voice"] == v] for v in range(tracks)], r["programs"][0], table["tempo"], s["SMALLEST_NOTE"])
    back = mi.quantise(mi.read_song(path), dict(s, SMALLEST_NOTE=4))
    assert back["programs"] == table["programs"], "the tracks changed places: the round trip's condition does not hold"
    again = mi.rolls_from_notes([back], s, device=False)
    assert np.array_equal(again["idx"], r["idx"]) and np.array_equal(again["held"], r["held"])
    want = np.zeros(r["idx"].size, np.uint8)
    want[rec["start"] * V + rec["voice"]] = np.clip(rec["velocity"], 0, 127)
    assert np.array_equal(again["vel_raw"].reshape(-1), want)
    assert np.all(np.abs(want.astype(int) - r["vel_raw"].reshape(-1)) <= 1)          # (the float32 velocity truncates to v or v - 1)


def test_read_song_tempo_map_and_choices(tmp_path):
    """seconds through two tempi; one instrument per chunk with notes, the conductor chunk none; a cut file raises"""
    import struct
    vlq = midifile.vlq
    conductor = b"\x00\xff\x51\x03" + (500000).to_bytes(3, "big") + vlq(960) + b"\xff\x51\x03" + (250000).to_bytes(3, "big") + b"\x00\xff\x2f\x00"
    track = (b"\x00\xc0\x07" + b"\x00\x90\x3c\x40" + vlq(480) + b"\x80\x3c\x00" + vlq(480) + b"\x90\x3e\x50" + vlq(480) + b"\x80\x3e\x00"
             + b"\x00\xff\x2f\x00")
    data = (b"MThd" + struct.pack(">IHHH", 6, 1, 2, 480) + b"MTrk" + struct.pack(">I", len(conductor)) + conductor
            + b"MTrk" + struct.pack(">I", len(track)) + track)
    path = tmp_path / "two_tempi.mid"
    path.write_bytes(data)
    song = mi.read_song(str(path))
    assert len(song["instruments"]) == 1 and song["instruments"][0]["program"] == 7
    assert song["instruments"][0]["notes"].tolist() == [[0.0, 0.5, 60.0, 64.0], [1.0, 1.25, 62.0, 80.0]]
    assert song["tempo_changes"][0].tolist() == [0.0, 1.0] and song["tempo_changes"][1].tolist() == [120.0, 240.0] and song["end_time"] == 1.25
    for cut in (10, 30, len(data) - 3):
        (tmp_path / "cut.mid").write_bytes(data[:cut])
        with pytest.raises(mi.UNREADABLE):
            mi.read_song(str(tmp_path / "cut.mid"))
        assert mi.load_rolls(str(tmp_path) + "/", "cut.mid", ic.settings()) == (None,) * 6


# ---- a folder of files ------------------------------------------------------------------------------------------------------------------
def test_import_folder(tmp_path):
    rng = np.random.default_rng(5)
    folder = str(tmp_path / "midi") + "/"
    cache = str(tmp_path / "cache") + "/"
    good = None
    for c, sub in ((0, "Style1/a"), (1, "other/style2")):
        os.makedirs(folder + sub)
        for i in range(10):          # (song 0 ends on a window's last tick: it needs no padding)
            notes = [np.array([(4 * k, 4 * k + (4 if i == 0 else int(rng.integers(1, 4))), int(rng.integers(30, 80)), 0, int(rng.integers(1, 128)))
                               for k in range(int(rng.integers(4, 30)))], ev.RECORD) for _ in range(3)]
            good = folder + sub + "/song%d.mid" % i
            midifile.write_midi(good, notes, [0, 10, 20], 120)
    data = open(good, "rb").read()
    with open(folder + "Style1/a/cut.mid", "wb") as f:
        f.write(data[:40])
    with open(folder + "Style1/a/notes.txt", "w") as f:
        f.write("not a song")
    with open(folder + "unknown.mid", "wb") as f:          # no class in its path and include_unknown is off: not imported
        f.write(data)
    s = ic.settings(T=16, SMALLEST_NOTE=4, classes=["style1", "style2"], num_classes=2, include_unknown=False, only_unknown=False, max_songs=1000,
                    test_fraction=0.1, split_equally_to_train_and_test=True, equal_mini_songs=False, smaller_training_set_factor=1.0,
                    save_imported_midi_as_pickle=True, pickle_store_folder=cache)
    import import_midi
    lists = import_midi.import_folder(folder, s, device=False)
    assert len(lists) == 16
    (V_tr, V_te, D_tr, D_te, T_tr, T_te, I_tr, I_te, Y_tr, Y_te, X_tr, X_te, c_tr, c_te, p_tr, p_te) = lists
    assert [len(x) for x in lists] == [18, 2] * 8
    assert sorted(c_te) == [0, 1] and sorted(c_tr) == [0] * 9 + [1] * 9
    assert not any("cut.mid" in p or "unknown.mid" in p or "notes.txt" in p for p in p_tr + p_te)
    for X, Y, V, D, I, tempo in zip(X_tr, Y_tr, V_tr, D_tr, I_tr, T_tr):
        assert X.shape == Y.shape == V.shape + (61,) == D.shape + (61,) and X.shape[1] == 16 and I.shape == (4, 16)
        assert tempo == 480.0          # (write_midi: one roll tick one beat, bpm * SMALLEST_NOTE / 4 beats a minute)
        assert np.all(Y.sum(-1) == 1) or np.all(Y[..., -1] == 1)
    back = import_midi.load_pickle_cache(cache)
    for a, b in zip(lists, back):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    # the classes follow the path below the folder, case-insensitively
    assert all(("Style1" in p) == (c == 0) for p, c in zip(p_tr + p_te, c_tr + c_te))
    with pytest.raises(ValueError, match="X_array"):
        mi.import_folder(folder, dict(s, split_equally_to_train_and_test=False), device=False)
    # equal_mini_songs keeps the classes' window counts level and max_songs stops the walk
    few = mi.import_folder(folder, dict(s, equal_mini_songs=True, save_imported_midi_as_pickle=False), device=False)
    assert len(few[10]) <= 18 and len(few[11]) == 2
    assert sum(map(len, mi.import_folder(folder, dict(s, max_songs=10, save_imported_midi_as_pickle=False), device=False)[10:12])) == 10
    with pytest.raises(NotImplementedError, match="import_folder"):
        import_midi.import_midi_from_folder(folder)
    # what the training scripts take from it: every row one-hot, also in songs that needed no padding
    import vae_training
    quiet = dict(s, save_imported_midi_as_pickle=False, signature_vector_length=8)
    train, test = vae_training.songs_from_midi_dir(folder.rstrip("/"), quiet, device=False)
    assert len(train) == 18 and len(test) == 2 and all(np.all(sg[k].sum(-1) == 1) for sg in train + test for k in ("X", "Y"))
    assert any(np.any(Y.sum(-1) == 2) for Y in Y_tr + Y_te), "no song without padding: the repair above is not exercised"


# ---- the sixth header --------------------------------------------------------------------------------------------------------------
def test_header_hygiene():
    lib = hl.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midivae_import.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text))
    assert declared == {"mvae_import_abi_version", "mvae_rolls_from_notes"} == set(hl.IMPORT_SIGNATURES)
    assert lib.mvae_import_abi_version() == 1 == hl.IMPORT_ABI_VERSION
    assert lib.mvae_events_abi_version() == 1 and lib.mvae_recon_abi_version() == 1 and lib.mvae_sweep_abi_version() == 1
    assert lib.mvae_desc_abi_version() == 1 and lib.mvae_abi_version() == 9 == hl.ABI_VERSION


def test_ctypes_struct_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_import.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(mvae_import_args));', 'printf("record %zu\\n", sizeof(mvae_import_note));']
    lines += ['printf("%s %%zu\\n", offsetof(mvae_import_args, %s));' % (f, f) for f, _ in hl.ImportArgs._fields_]
    lines += ['printf("r_%s %%zu\\n", offsetof(mvae_import_note, %s));' % (f, f) for f in mi.NOTE.names]
    lines += ['printf("MVAE_IMPORT_MAX_TRACKS %d\\n", (int)MVAE_IMPORT_MAX_TRACKS);', 'printf("MVAE_IMPORT_MAX_VOICES %d\\n", (int)MVAE_IMPORT_MAX_VOICES);',
              'printf("workspace_bytes %zu\\n", MVAE_IMPORT_WORKSPACE_BYTES(1234, 26));', 'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(hl.ImportArgs) and ctypes.sizeof(hl.ImportArgs) % 8 == 0
    for f, _ in hl.ImportArgs._fields_:
        assert int(got[f]) == getattr(hl.ImportArgs, f).offset, f
    assert int(got["record"]) == mi.NOTE.itemsize == 12
    for f in mi.NOTE.names:
        assert int(got["r_" + f]) == mi.NOTE.fields[f][1], f
    assert int(got["MVAE_IMPORT_MAX_TRACKS"]) == mi.MAX_TRACKS and int(got["MVAE_IMPORT_MAX_VOICES"]) == 8
    assert int(got["workspace_bytes"]) == mi.workspace_bytes(1234, 26)


# ---- refusals: on addresses nothing maps, so only where no device could run a wrongly accepted call ------------------------------------
def _device_visible():
    import torch
    if torch.cuda.is_available():
        return True
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    n = ctypes.c_int(0)
    return bool(paths) and ctypes.CDLL(sorted(paths)[0]).hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


no_device = pytest.mark.skipif(_device_visible(), reason="a device is visible: fake addresses must never reach a kernel "
                               "(tests/test_midi_import_gpu.py runs the safe rows on real buffers)")


@no_device
def test_baseline_and_accepted_forms_pass_validation():
    lib = hl.load()
    assert ic.invoke(lib, ic.baseline(ic.fake_alloc)) == hl.E_LAUNCH
    for name, mutate in ic.ACCEPTED:
        assert ic.invoke(lib, mutate(ic.baseline(ic.fake_alloc))) == hl.E_LAUNCH, name


@no_device
@pytest.mark.parametrize("row", ic.ROWS, ids=[r[0] for r in ic.ROWS])
def test_violation_is_refused_before_anything_is_enqueued(row):
    name, mutate, code, _ = row
    rc = ic.invoke(hl.load(), mutate(ic.baseline(ic.fake_alloc)))
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == code, "%s: returned %d, promised %d - %s" % (name, rc, code, how)


def test_the_table_and_the_header_cover_every_documented_limit():
    names = " | ".join(r[0] for r in ic.ROWS)
    for what in ("a NULL", "notes NULL", "note_off NULL", "track_off NULL", "ticks NULL", "win_off NULL", "workspace NULL", "idx NULL",
                 "held NULL", "concurrent NULL", "slots NULL", "slot_voice NULL", "n_songs = 0", "n_windows = 0", "T = 0", "stride_t = 0",
                 "stride_w = -1", "voices = 0", "voices = 9", "T % voices", "max_per_track = 0", "pitch_base = -1", "pitch_base + n_pitch = 129",
                 "silent = 256", "silent = -1", "threshold = nan", "threshold = inf", "threshold = 1.0", "threshold = -0.25",
                 "n_tracks = 65536", "n_windows * T = 2^31"):
        assert what in names, what
    assert len([r for r in ic.ROWS if r[3]]) >= 8
    header = open(os.path.join(ROOT, "include", "midivae_import.h")).read()
    for word in ("note_off", "track_off", "win_off", "workspace", "slot_voice", "max_per_track", "1..8", "T % voices", "pitch_base < 0",
                 "> 128", "0..255", "[0, 1)", "65535", "2^31 - 1", "CALLER'S CONTRACT"):
        assert word in header, word
