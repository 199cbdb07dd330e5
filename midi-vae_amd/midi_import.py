"""MIDI files into training windows (reference import_midi.py:13-574): ``read_song`` (file -> notes in seconds), ``quantise`` (notes ->
the tick-quantised note table of a song, :30-129 up to the integers), ``rolls_from_notes`` (tables -> index, velocity and held rolls in
windows: ``mvae_rolls_from_notes`` of include/midivae_import.h, or with ``device=False`` the NumPy mirror below, vectorised per song),
``load_rolls`` (the reference's six values X, Y, I, tempo, V, D) and ``import_folder`` (its sixteen lists).

What is the reference's and what is this module's own:
  - Everything from the tempo changes and the notes in seconds onwards is the reference's arithmetic, every double expression written
    in its order; tests/golden/import_rolls.npz pins ``quantise`` + ``rolls_from_notes`` + ``load_rolls`` to the reference's own
    ``load_rolls``, run on synthetic songs through a feeding pretty_midi stub.
  - ``read_song`` is NOT pretty_midi's parser and no parity with it is claimed.  Its choices: one instrument per MTrk chunk that holds
    at least one note, in file order, all channels of the chunk together; its program is the chunk's last program change (0 if none);
    seconds come from the file's set-tempo events (120 bpm before the first); the END TIME is the latest note end of the file.  Drums,
    pitch bends and controllers are not treated specially.
  - The order of the instruments follows ``np.argsort(cells)[::-1]`` as in the reference, ``cells`` being the non-zero cells of
    ``get_piano_roll(fs=100)``.  pretty_midi is not at hand, so what that function returns is an ASSUMPTION: 128 x int(100 * latest
    end) frames, every note ADDING its velocity to int(start * 100):int(end * 100) of its pitch - so a note of velocity 0 fills no
    cell.  Ties between instruments are whatever argsort makes of them.

``s`` is a settings mapping or module read like packers._g does (None: the root-level ``settings`` module).
"""
from __future__ import annotations

import ctypes as C
import io
import math
import os
import struct

import numpy as np

from . import hiplib as hl
from . import midifile
from .packers import _g, notes_from_indices, programs_to_instrument_matrix

NOTE = np.dtype([("start", "<i4"), ("end", "<i4"), ("pitch", "u1"), ("velocity", "u1"), ("track", "<u2")])          # mvae_import_note
MAX_TRACKS = 65535
UNREADABLE = (ValueError, EOFError, IndexError, OSError, KeyError, ZeroDivisionError, AttributeError, struct.error)


def _settings(s):
    if s is None:
        import importlib
        return vars(importlib.import_module("settings"))
    return s


def params(s):
    """what the import reads from the settings"""
    s = _settings(s)
    low, high = int(_g(s, "low_crop")), int(_g(s, "high_crop"))
    T = int(_g(s, "output_length"))
    return dict(voices=int(_g(s, "max_voices")), pitch_base=low, n_pitch=high - low, silent=high - low,
                threshold=float(_g(s, "velocity_threshold_such_that_it_is_a_played_note")), smallest_note=_g(s, "SMALLEST_NOTE"),
                max_per_track=int(_g(s, "MAXIMAL_NUMBER_OF_VOICES_PER_TRACK")), T=T)


def _check(p, T):
    V = p["voices"]
    if not 1 <= V <= 8 or T <= 0 or T % V:
        raise ValueError("rows per window (%d) must be a positive multiple of max_voices (%d, 1..8)" % (T, V))
    if p["pitch_base"] < 0 or p["n_pitch"] <= 0 or p["pitch_base"] + p["n_pitch"] > 128:
        raise ValueError("pitch columns %d..%d: a MIDI pitch is 0..127" % (p["pitch_base"], p["pitch_base"] + p["n_pitch"]))
    if p["max_per_track"] < 1:
        raise ValueError("MAXIMAL_NUMBER_OF_VOICES_PER_TRACK must be at least 1")
    if not (math.isfinite(p["threshold"]) and 0.0 <= p["threshold"] < 1.0):
        raise ValueError("the velocity threshold must lie in [0, 1)")


# ---- file -> notes in seconds ------------------------------------------------------------------------------------------------------
def read_song(path_or_file):
    """A Standard MIDI File as dict ``instruments`` [dict ``program``, ``notes`` (k, 4) float64: start s, end s, pitch, velocity, in
    file order of their note-ons], ``tempo_changes`` (times s, bpm = 6e7 / microseconds per beat) and ``end_time`` (the latest note
    end, 0.0 without notes).  Built on midifile.read_midi; see the module's docstring for how chunks become instruments.  A file whose
    chunks are cut short raises ValueError."""
    if hasattr(path_or_file, "read"):
        data = path_or_file.read()
    else:
        with open(path_or_file, "rb") as f:
            data = f.read()
    if len(data) < 14 or data[:4] != b"MThd":
        raise ValueError("not a Standard MIDI File")
    at, chunks = 8 + struct.unpack(">I", data[4:8])[0], 0
    while at < len(data):
        if at + 8 > len(data) or at + 8 + struct.unpack(">I", data[at + 4:at + 8])[0] > len(data):
            raise ValueError("a chunk of the file is cut short")
        at += 8 + struct.unpack(">I", data[at + 4:at + 8])[0]
        chunks += 1
    if chunks < struct.unpack(">H", data[10:12])[0]:
        raise ValueError("the file ends before its last track")
    mid = midifile.read_midi(io.BytesIO(data))
    division = float(mid["division"])
    # the tempo map: set-tempo events by tick, the last of a tick winning, 120 bpm from tick 0 where the file sets none there
    tempo_at = {}
    for tick, us in mid["tempos"]:
        tempo_at[tick] = us
    if 0 not in tempo_at:
        tempo_at[0] = 500000
    ticks = np.array(sorted(tempo_at), np.int64)
    us = np.array([tempo_at[t] for t in ticks.tolist()], np.float64)
    seconds_per_tick = us / (division * 1e6)
    starts = np.concatenate([[0.0], np.cumsum(np.diff(ticks) * seconds_per_tick[:-1])])

    def seconds(tick):
        tick = np.asarray(tick, np.int64)
        part = np.searchsorted(ticks, tick, side="right") - 1
        return starts[part] + (tick - ticks[part]) * seconds_per_tick[part]

    instruments, end_time = [], 0.0
    for track in mid["tracks"]:
        if not track["notes"]:
            continue
        raw = np.array(track["notes"], np.int64).reshape(-1, 4)
        notes = np.stack([seconds(raw[:, 0]), seconds(raw[:, 1]), raw[:, 2].astype(np.float64), raw[:, 3].astype(np.float64)], 1)
        instruments.append(dict(program=int(track["program"] or 0), notes=notes))
        end_time = max(end_time, float(notes[:, 1].max()))
    return dict(instruments=instruments, tempo_changes=(seconds(ticks), 6e7 / us), end_time=end_time)


# ---- notes in seconds -> the tick-quantised table -----------------------------------------------------------------------------------
def piano_roll_cells(notes, fs=100):
    """np.count_nonzero of what pretty_midi's Instrument.get_piano_roll(fs) is ASSUMED to return (see the module's docstring)"""
    if len(notes) == 0:
        return 0
    frames = int(fs * notes[:, 1].max())
    loud = notes[notes[:, 3] > 0]
    if frames <= 0 or len(loud) == 0:
        return 0
    a = np.minimum((loud[:, 0] * fs).astype(np.int64), frames)
    b = np.minimum((loud[:, 1] * fs).astype(np.int64), frames)
    pitch = loud[:, 2].astype(np.int64)
    edges = np.zeros((128, frames + 1), np.int64)
    np.add.at(edges, (pitch, a), 1)
    np.add.at(edges, (pitch, np.maximum(a, b)), -1)
    return int(np.count_nonzero(np.cumsum(edges, axis=1)[:, :frames] > 0))


def quantise(song, s=None):
    """reference import_midi.py:30-129 up to the integers.  ``song``: what read_song returns.  dict ``ticks`` (total_ticks),
    ``programs`` (the instruments ordered by their piano-roll cells, descending), ``tempo`` and ``notes``: a NOTE array (start tick,
    end tick, pitch, velocity 0..127, track = the instrument's place in that order) sorted stably by (track, start, pitch, file
    order).  A kept note with end tick == start tick stays in the table: it paints nothing and is a key."""
    s = _settings(s)
    SMALLEST_NOTE = _g(s, "SMALLEST_NOTE")
    tempo_change_times, tempo_change_bpm = song["tempo_changes"]
    song_start = 0
    song_end = song["end_time"]
    if len(tempo_change_times) > 1:
        longest_part = 0
        longest_part_start_time = 0
        longest_part_end_time = song_end
        longest_part_tempo = 0
        for i, tempo_change_time in enumerate(tempo_change_times):
            if i == len(tempo_change_times) - 1:
                end_time = song_end
            else:
                end_time = tempo_change_times[i + 1]
            current_part_length = end_time - tempo_change_time
            if current_part_length > longest_part:
                longest_part = current_part_length
                longest_part_start_time = tempo_change_time
                longest_part_end_time = end_time
                longest_part_tempo = tempo_change_bpm[i]
        song_start = longest_part_start_time
        song_end = longest_part_end_time
        tempo = longest_part_tempo
    else:
        tempo = tempo_change_bpm[0]

    kept = []
    for instrument in song["instruments"]:
        notes = np.asarray(instrument["notes"], np.float64).reshape(-1, 4)
        notes = notes[(notes[:, 0] >= song_start) & (notes[:, 1] <= song_end)].copy()
        notes[:, 0] -= song_start
        notes[:, 1] -= song_start
        kept.append(notes)
    number_of_notes = [piano_roll_cells(notes) for notes in kept]
    permutation = np.argsort(number_of_notes)[::-1]

    quarter_note_length = 1. / (tempo / 60.)
    fs = 1. / (quarter_note_length * 4. / SMALLEST_NOTE)
    total_ticks = math.ceil(song_end * fs)

    tables = []
    for track, i in enumerate(permutation.tolist()):
        notes = kept[i]
        note_tick_start = notes[:, 0] * fs
        note_tick_end = notes[:, 1] * fs
        absolute_start = np.rint(note_tick_start).astype(np.int64)          # (half to even, as Python's round)
        absolute_end = np.rint(note_tick_end).astype(np.int64)
        decimal = note_tick_start - absolute_start
        keep = (decimal < 10e-3) | (absolute_end - absolute_start >= 1)
        rec = np.zeros(int(keep.sum()), NOTE)
        rec["start"], rec["end"] = absolute_start[keep], absolute_end[keep]
        rec["pitch"], rec["velocity"], rec["track"] = notes[keep, 2], notes[keep, 3], track
        tables.append(rec[np.lexsort((rec["pitch"], rec["start"]))])
    notes = np.concatenate(tables) if tables else np.zeros(0, NOTE)
    return dict(ticks=int(total_ticks), programs=[int(song["instruments"][i]["program"]) for i in permutation.tolist()],
                tempo=tempo, notes=notes)


# ---- the NumPy mirror -------------------------------------------------------------------------------------------------------------
def allot_voices(concurrent, V, M):
    """reference :161-231: (slots, slot_voice), V values each - the track of every output voice (-1: none) and its voice in the track"""
    c = [int(x) for x in concurrent]
    cap = [M] * len(c)
    free = V - sum(min(M, x) if x > 0 else 0 for x in c[:V])
    for k in range(min(V, len(c))):
        if free > 0 and c[k] > M:
            add = min(free, c[k] - M)
            cap[k] += add
            free -= add
    slots, voice_of = [], []
    for k, x in enumerate(c):
        if x > 0:
            for voice in range(min(x, cap[k])):
                if len(slots) < V:
                    slots.append(k)
                    voice_of.append(voice)
    pad = V - len(slots)
    return np.array(slots + [-1] * pad, np.int32), np.array(voice_of + [0] * pad, np.int32)


def _mirror_song(table, p, T):
    """one song: (idx, held, vel_raw) of shape (windows, T), concurrent (tracks,), slots and slot_voice (V,)"""
    V, n = p["voices"], int(table["ticks"])
    tracks = len(table["programs"])
    notes = table["notes"]
    notes = notes[(notes["track"] < tracks) & (notes["pitch"] < 128)]
    trk, pitch = notes["track"].astype(np.int64), notes["pitch"].astype(np.int64)
    a = np.clip(notes["start"].astype(np.int64), 0, n)
    b = np.maximum(np.clip(notes["end"].astype(np.int64), 0, n), a)
    edges = np.zeros((tracks, n + 1, 128), np.int32)
    np.add.at(edges, (trk, a, pitch), 1)
    np.add.at(edges, (trk, b, pitch), -1)
    cover = np.cumsum(edges, axis=1)[:, :n]                     # notes of (track, tick, pitch): per note, not per pitch
    painted = cover > 0
    concurrent = cover.sum(2).max(1).astype(np.int32) if n else np.zeros(tracks, np.int32)
    key = np.zeros((tracks, n, 128), bool)
    key_velocity = np.zeros((tracks, n, 128), np.uint8)
    inside = (notes["start"] >= 0) & (notes["start"] < n)
    at = (trk[inside], notes["start"][inside].astype(np.int64), pitch[inside])
    key[at] = True
    key_velocity[at] = notes["velocity"][inside]              # (a repeated index takes the last value: the table's order)
    slots, slot_voice = allot_voices(concurrent, V, p["max_per_track"])

    windows = -(-n * V // T)
    idx = np.full(windows * T, p["silent"], np.uint8)
    held, vel_raw = np.zeros(windows * T, np.uint8), np.zeros(windows * T, np.uint8)
    for j in range(V):
        if slots[j] < 0 or n == 0:
            continue
        mask = painted[slots[j]][:, ::-1]                       # highest pitch first
        chosen = mask & (np.cumsum(mask, axis=1) == slot_voice[j] + 1)
        found = chosen.any(1)
        tick = np.nonzero(found)[0]
        got = 127 - np.argmax(chosen, axis=1)[found]
        rows = tick * V + j
        is_key = key[slots[j], tick, got]
        held[rows] = ~is_key
        vel_raw[rows] = np.where(is_key, key_velocity[slots[j], tick, got], 0)
        kept = (got >= p["pitch_base"]) & (got < p["pitch_base"] + p["n_pitch"])
        idx[rows[kept]] = got[kept] - p["pitch_base"]
    return idx.reshape(windows, T), held.reshape(windows, T), vel_raw.reshape(windows, T), concurrent, slots, slot_voice


def tick_loops(table, p):
    """The reference's own loops (import_midi.py:94-286) over every tick of every track, restated on a note table - dicts, lists and
    ``sorted`` as there: the song's unpadded rows (idx, held, vel_raw) and concurrent, slots, slot_voice as _mirror_song returns them.
    What the CPU tests hold the mirror to beside the fixture, and what the profile times the device against."""
    V, total_ticks, M = p["voices"], int(table["ticks"]), p["max_per_track"]
    piano_rolls, velocity_rolls, held_note_rolls, counts = [], [], [], []
    for track in range(len(table["programs"])):
        piano_roll = np.zeros((total_ticks, 128))
        concurrent_notes_count = np.zeros((total_ticks,))
        note_to_velocity_dict = dict()
        for note in table["notes"][table["notes"]["track"] == track].tolist():
            absolute_start, absolute_end, pitch, velocity = note[:4]
            piano_roll[absolute_start:absolute_end, pitch] = 1
            concurrent_notes_count[absolute_start:absolute_end] += 1
            note_to_velocity_dict[(absolute_start, pitch)] = velocity
        max_concurrent_notes = int(np.max(concurrent_notes_count)) if total_ticks else 0
        velocity_roll = np.zeros((total_ticks, max_concurrent_notes))
        held_note_roll = np.zeros((total_ticks, max_concurrent_notes))
        for step, note_vector in enumerate(piano_roll):
            pitches = list(note_vector.nonzero()[0])
            for voice_number, pitch in enumerate(sorted(pitches)[::-1]):
                if (step, pitch) in note_to_velocity_dict.keys():
                    velocity_roll[step, voice_number] = note_to_velocity_dict[(step, pitch)]
                else:
                    held_note_roll[step, voice_number] = 1
        piano_rolls.append(piano_roll)
        velocity_rolls.append(velocity_roll)
        held_note_rolls.append(held_note_roll)
        counts.append(max_concurrent_notes)
    slots, slot_voice = allot_voices(counts, V, M)
    idx = np.full(total_ticks * V, p["silent"], np.uint8)
    held, vel_raw = np.zeros(total_ticks * V, np.uint8), np.zeros(total_ticks * V, np.uint8)
    for i in range(V):
        if slots[i] < 0:
            continue
        piano_roll, voice = piano_rolls[slots[i]], slot_voice[i]
        for step in range(total_ticks):
            notes = np.nonzero(piano_roll[step, :])[0][::-1]
            if len(notes) > voice:
                if p["pitch_base"] <= notes[voice] < p["pitch_base"] + p["n_pitch"]:
                    idx[i + step * V] = notes[voice] - p["pitch_base"]
            vel_raw[i + step * V] = velocity_rolls[slots[i]][step, voice]
            held[i + step * V] = held_note_rolls[slots[i]][step, voice]
    return idx, held, vel_raw, np.array(counts, np.int32), slots, slot_voice


def velocities_of(vel_raw, threshold, dtype=np.float64):
    """reference :273 in double: threshold + (v / 127.) * (1.0 - threshold) where v > 0, else 0; float32 is that double rounded"""
    v = np.asarray(vel_raw).astype(np.float64)
    return np.where(v > 0, threshold + (v / 127.0) * (1.0 - threshold), 0.0).astype(dtype)


# ---- the device path --------------------------------------------------------------------------------------------------------------
def workspace_bytes(cells, n_songs):
    """MVAE_IMPORT_WORKSPACE_BYTES"""
    return 4 * (9 * cells + n_songs + 1)


def pack_tables(tables, p, T):
    """the host side of a call: the records of all songs and the four offset lists, and the totals the entry point is told"""
    V = p["voices"]
    counts = np.array([len(t["notes"]) for t in tables], np.int64)
    tracks = np.array([len(t["programs"]) for t in tables], np.int64)
    ticks = np.array([t["ticks"] for t in tables], np.int64)
    windows = -(-ticks * V // T)
    if ticks.size and (ticks.min() < 0 or tracks.sum() > MAX_TRACKS or windows.sum() * T > 2 ** 31 - 1 or (tracks * ticks).sum() > 2 ** 31 - 1
                       or counts.sum() > 2 ** 31 - 1):
        raise ValueError("a call takes at most %d tracks, 2^31 - 1 rows, notes and track ticks; import the songs in several calls" % MAX_TRACKS)
    off = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int32)
    notes = np.concatenate([t["notes"] for t in tables]) if len(tables) else np.zeros(0, NOTE)
    return dict(notes=np.ascontiguousarray(notes, NOTE), note_off=off(counts), track_off=off(tracks), ticks=ticks.astype(np.int32),
                win_off=off(windows), cells=int((tracks * ticks).sum()), lengths=windows)


def enqueue(dev, p, T, n_songs, n_notes, n_tracks, n_windows, cells, workspace, idx, held, vel_raw, vel, stream):
    """mvae_rolls_from_notes on device memory the caller owns.  ``dev``: dict of the device tensors notes (bytes), note_off, track_off,
    ticks, win_off, concurrent, slots, slot_voice; ``idx`` / ``held`` (n_windows, T) uint8 tensors of any (equal, positive) strides,
    ``vel_raw`` uint8 / ``vel`` float32 of the same strides or None."""
    a = hl.ImportArgs(notes=hl.ptr(dev["notes"]) if n_notes else None, note_off=dev["note_off"].data_ptr(),
                      track_off=dev["track_off"].data_ptr(), ticks=dev["ticks"].data_ptr(), win_off=dev["win_off"].data_ptr(),
                      n_songs=n_songs, n_notes=n_notes, n_tracks=n_tracks, n_windows=n_windows, T=T, voices=p["voices"],
                      max_per_track=p["max_per_track"], pitch_base=p["pitch_base"], n_pitch=p["n_pitch"], silent=p["silent"],
                      cells=cells, stride_t=idx.stride(1), stride_w=idx.stride(0), threshold=p["threshold"],
                      workspace=workspace.data_ptr(), idx=idx.data_ptr(), held=held.data_ptr(), vel_raw=hl.ptr(vel_raw), vel=hl.ptr(vel),
                      concurrent=dev["concurrent"].data_ptr() if n_tracks else None, slots=dev["slots"].data_ptr(),
                      slot_voice=dev["slot_voice"].data_ptr())
    hl.check(hl.load().mvae_rolls_from_notes(C.byref(a), stream), "mvae_rolls_from_notes")


def upload(packed, p, device="cuda"):
    """the lists of pack_tables and the small outputs as device tensors: ONE host-to-device copy"""
    import torch
    n_songs = len(packed["ticks"])
    parts = [packed["note_off"], packed["track_off"], packed["ticks"], packed["win_off"]]
    blob = np.concatenate([np.concatenate(parts).view(np.uint8), packed["notes"].view(np.uint8).reshape(-1)])
    t = torch.from_numpy(blob).to(device)
    dev, at = {}, 0
    for name, part in zip(("note_off", "track_off", "ticks", "win_off"), parts):
        dev[name] = t[at:at + 4 * len(part)].view(torch.int32)
        at += 4 * len(part)
    dev["notes"] = t[at:]
    n_tracks = int(packed["track_off"][-1])
    small = torch.empty(max(n_tracks, 1) + 2 * n_songs * p["voices"], dtype=torch.int32, device=t.device)
    dev["concurrent"] = small[:n_tracks]
    dev["slots"] = small[max(n_tracks, 1):max(n_tracks, 1) + n_songs * p["voices"]]
    dev["slot_voice"] = small[max(n_tracks, 1) + n_songs * p["voices"]:]
    dev["small"] = small
    return dev


def rolls_from_notes(tables, s=None, device=True, T=None, as_device=False):
    """The rolls of ``len(tables)`` songs (``tables``: what quantise returns) in windows of ``T`` rows (None: output_length): dict
    ``idx`` (n, T) uint8 (the silent index where no note is), ``vel`` float32, ``vel_raw`` uint8, ``held`` uint8 - window-major, the
    windows of the songs one after the other - ``lengths`` (windows per song), ``programs`` (per song max_voices programs, the
    reference's ``chosen_programs``; shorter where voices stay empty), ``concurrent`` (per song an int32 array over its tracks) and
    ``slots`` / ``slot_voice`` (songs, max_voices).  ``device``: all songs go through ONE launch sequence of mvae_rolls_from_notes
    and one read back (``as_device``: idx, vel, vel_raw and held stay device tensors); else the NumPy mirror."""
    s = _settings(s)
    p = params(s)
    T = p["T"] if T is None else int(T)
    _check(p, T)
    if _g(s, "include_only_monophonic_instruments"):
        raise ValueError("include_only_monophonic_instruments: the reference's own branch raises (import_midi.py:201); not supported")
    V, S = p["voices"], len(tables)
    packed = pack_tables(tables, p, T)
    lengths = packed["lengths"]
    n = int(lengths.sum())
    track_off = packed["track_off"]
    if device and n > 0:
        import torch
        dev = upload(packed, p)
        where = dev["small"].device
        rolls = torch.empty(3 * n * T, dtype=torch.uint8, device=where)
        idx, held, vel_raw = (rolls[k * n * T:(k + 1) * n * T].view(n, T) for k in range(3))
        vel = torch.empty((n, T), dtype=torch.float32, device=where)
        workspace = torch.empty(workspace_bytes(packed["cells"], S), dtype=torch.uint8, device=where)
        with torch.cuda.device(where):
            enqueue(dev, p, T, S, len(packed["notes"]), int(track_off[-1]), n, packed["cells"], workspace, idx, held, vel_raw, vel,
                    torch.cuda.current_stream().cuda_stream)
            small = dev["small"].cpu().numpy()
            if not as_device:
                host = rolls.cpu().numpy().reshape(3, n, T)
                idx, held, vel_raw = host[0], host[1], host[2]
                vel = vel.cpu().numpy()
        n_tracks = int(track_off[-1])
        concurrent_all = small[:n_tracks]
        slots = small[max(n_tracks, 1):max(n_tracks, 1) + S * V].reshape(S, V)
        slot_voice = small[max(n_tracks, 1) + S * V:].reshape(S, V)
    else:
        out = [_mirror_song(t, p, T) for t in tables]
        cat = lambda k, dtype, shape: np.concatenate([o[k] for o in out]) if out else np.zeros(shape, dtype)
        idx, held, vel_raw = cat(0, np.uint8, (0, T)), cat(1, np.uint8, (0, T)), cat(2, np.uint8, (0, T))
        vel = velocities_of(vel_raw, p["threshold"], np.float32)
        concurrent_all = cat(3, np.int32, (0,))
        slots = np.stack([o[4] for o in out]) if out else np.zeros((0, V), np.int32)
        slot_voice = np.stack([o[5] for o in out]) if out else np.zeros((0, V), np.int32)
    programs = [[t["programs"][k] for k in row if k >= 0] for t, row in zip(tables, slots.tolist())]
    concurrent = [concurrent_all[track_off[i]:track_off[i + 1]] for i in range(S)]
    return dict(idx=idx, vel=vel, vel_raw=vel_raw, held=held, lengths=lengths, programs=programs, concurrent=concurrent, slots=slots,
                slot_voice=slot_voice)


# ---- the reference's load_rolls ---------------------------------------------------------------------------------------------------
def rolls_of_song(song, s=None, device=False):
    """``load_rolls`` from what read_song returns: X, Y, I, tempo, V, D as the reference returns them, six None without a note"""
    s = _settings(s)
    p = params(s)
    V = p["voices"]
    if len(song["instruments"]) == 0:          # (no roll is chosen: the reference's last branch)
        return (None,) * 6
    table = quantise(song, s)
    r = rolls_from_notes([table], s, device=device, T=V)          # one tick a window: the song's rows, unpadded
    if not r["programs"][0]:
        return (None,) * 6
    idx = np.asarray(r["idx"]).reshape(-1)
    width = p["n_pitch"] + 1
    Y = notes_from_indices(dict(low_crop=p["pitch_base"], high_crop=p["pitch_base"] + p["n_pitch"], include_silent_note=True), idx, width)
    Vr = velocities_of(np.asarray(r["vel_raw"]).reshape(-1), p["threshold"])
    D = np.asarray(r["held"]).reshape(-1).astype(np.float64)
    I = programs_to_instrument_matrix(r["programs"][0], _g(s, "instrument_attach_method"), V)
    import import_midi as drop_in
    if not _g(s, "attach_instruments"):
        X, Yw, Vw, Dw = drop_in.windows_from_unrolled_rolls(Y, Vr, D, s, as_written=True)
        return X, Yw, I, table["tempo"], Vw, Dw
    # :290-292: the instrument rows, tiled over the ticks, become columns of Y BEFORE the split - so the padding's "silent bit" (:314,
    # :328) lands in the last instrument column, as in the reference
    unsplit = dict(s if isinstance(s, dict) else vars(s), input_length=0, output_length=0, song_completion=False)
    _, Y, _, _ = drop_in.windows_from_unrolled_rolls(Y, Vr, D, unsplit)
    Y = np.append(Y, np.transpose(np.tile(np.transpose(I), len(Y) // V)), axis=1)
    X = Y[::V, :] if _g(s, "song_completion") else Y
    silent = bool(_g(s, "include_silent_note"))

    def split(a, length, fill):
        if length <= 0:
            return a
        out = drop_in._split_padded(a, length, fill)
        if fill and a.shape[0] % length == 0:          # (``X[-0:, -1] = 1``: every row)
            out[..., -1] = 1
        return out

    Lin, Lout = _g(s, "input_length"), _g(s, "output_length")
    return split(X, Lin, silent), split(Y, Lout, silent), I, table["tempo"], split(Vr, Lout, False), split(D, Lout, False)


def load_rolls(path, name, s=None, device=False):
    """reference import_midi.py:13-350: the file ``path + name`` as X, Y, I, tempo, V, D (float64 windows; V from the raw velocities
    in float64), or six None for a file that cannot be read or has no track with a note"""
    try:
        song = read_song(path + name)
    except UNREADABLE as e:
        print("Unexpected error in " + name + ":\n", e)
        return (None,) * 6
    return rolls_of_song(song, s, device)


# ---- the reference's import_midi_from_folder --------------------------------------------------------------------------------------
def import_folder(folder, s=None, device=True):
    """reference import_midi.py:375-574: the sixteen lists V_train, V_test, D_train, D_test, T_train, T_test, I_train, I_test, Y_train,
    Y_test, X_train, X_test, c_train, c_test, train_paths, test_paths from the ``.mid`` / ``.midi`` files under ``folder``, a file's
    class being the first of ``classes`` its path below ``folder`` names.  The reference's branch without
    split_equally_to_train_and_test reads an undefined name (:464) and is refused."""
    from sklearn.model_selection import train_test_split
    s = _settings(s)
    g = lambda name: _g(s, name)
    if not g("split_equally_to_train_and_test"):
        raise ValueError("split_equally_to_train_and_test = False: the reference's own branch fails (import_midi.py:464 reads an "
                         "undefined X_array); set it to True")
    classes, max_songs = list(g("classes")), g("max_songs")
    X_list, Y_list, paths, c_classes, I_list, T_list, V_list, D_list = [], [], [], [], [], [], [], []

    def take(_path, _name, c):
        X, Y, I, T, V, D = load_rolls(_path, _name, s, device)
        if X is not None and Y is not None:
            for lst, x in ((X_list, X), (Y_list, Y), (I_list, I), (T_list, T), (V_list, V), (D_list, D), (paths, _path + _name), (c_classes, c)):
                lst.append(x)

    for path, subdirs, files in os.walk(folder):
        for name in files:
            if len(X_list) >= max_songs:
                break
            _path = path.replace('\\', '/') + '/'
            _name = name.replace('\\', '/')
            if _name.endswith('.mid') or _name.endswith('.midi'):
                shortpath = _path[len(folder):]
                found = False
                for i, c in enumerate(classes):
                    if c.lower() in shortpath.lower():
                        found = True
                        if not g("only_unknown"):
                            take(_path, _name, i)
                        break
                if not found and g("include_unknown"):
                    take(_path, _name, g("num_classes") - 1)
        if len(X_list) >= max_songs:
            break

    (V_train, V_test, D_train, D_test, T_train, T_test, I_train, I_test, Y_train, Y_test, X_train, X_test, c_train, c_test, train_paths,
     test_paths) = train_test_split(V_list, D_list, T_list, I_list, Y_list, X_list, c_classes, paths, test_size=g("test_fraction"),
                                    random_state=42, stratify=c_classes)

    if g("equal_mini_songs"):
        per_window = g("output_length") // g("max_voices")
        splits_per_class = np.zeros((g("num_classes"),))
        for i, song in enumerate(X_train):
            splits_per_class[c_train[i]] += math.ceil(len(song) / per_window)
        amount_of_splits = int(min(splits_per_class) * g("smaller_training_set_factor"))
        keep, splits_per_class_new = [], np.zeros((g("num_classes"),))
        for i, song in enumerate(X_train):
            c = c_train[i]
            if splits_per_class_new[c] + math.ceil(len(song) / per_window) <= amount_of_splits:
                keep.append(i)
                splits_per_class_new[c] += math.ceil(len(song) / per_window)
        pick = lambda lst: [lst[i] for i in keep]
        V_train, D_train, T_train, I_train, Y_train, X_train, c_train, train_paths = map(
            pick, (V_train, D_train, T_train, I_train, Y_train, X_train, c_train, train_paths))

    lists = (V_train, V_test, D_train, D_test, T_train, T_test, I_train, I_test, Y_train, Y_test, X_train, X_test, c_train, c_test,
             train_paths, test_paths)
    if g("save_imported_midi_as_pickle"):
        import import_midi as drop_in
        drop_in.save_pickle_cache(g("pickle_store_folder"), lists)
    return lists
