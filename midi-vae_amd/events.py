"""Note events of decoded songs (reference midi_functions.py:57-137, ``rolls_to_midi`` without its file): one note per (start, end,
pitch, velocity, voice) from the index rolls, the velocities and the held-notes roll of whole songs - what midifile.write_midi takes.

``note_events`` runs on the device (``mvae_note_events``, include/midivae_events.h: one lane per window and voice, four launches, no
lane waits for another workgroup) or, with ``device=False``, through the NumPy mirror below - two flag passes, a prefix sum and a
compaction, the yardstick of the device tests.  ``tracker_loop`` is a deliberately literal restatement of the reference's row-by-row
loop, which the CPU tests hold the mirror to; both are pinned to the reference's own function by tests/golden/midi_events.npz.
Everything is an integer: device, mirror, loop and reference are EQUAL.

Tick i of voice v of a song is row i * voices + v of the song's rows.  With a held-notes roll a note continues on a tick whose row
holds (!= 0) the pitch of the tick before; without one it continues while the pitch repeats and the tick is no multiple of
SMALLEST_NOTE.  A note still sounding on a song's last row is dropped, as the reference drops it, or - ``close_at_end`` - closed at the
song's tick count.

``s`` is a settings mapping or module read like packers._g does: max_voices, low_crop, high_crop, include_silent_note,
velocity_threshold_such_that_it_is_a_played_note, SMALLEST_NOTE (and, for ``vote_for_programs``, instrument_attach_method).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hiplib as hl
from .packers import _g
from .reconstruction import first_windows
from .rolls import as_rolls, base_params, check_rows, device_roll, host_roll, sounding, with_strides_of

RECORD = np.dtype([("start", "<i4"), ("end", "<i4"), ("pitch", "u1"), ("voice", "u1"), ("velocity", "<i2")])          # mvae_note_event
MAX_T = 65536
MAX_VELOCITY = 127.0
DEFAULT_VELOCITY = 80


def params(s):
    """what the note events read from the settings"""
    return dict(base_params(s), threshold=float(_g(s, "velocity_threshold_such_that_it_is_a_played_note")),
                smallest_note=int(_g(s, "SMALLEST_NOTE")), pitch_base=int(_g(s, "low_crop")))


def _check(T, p, n=0):
    check_rows(T, p, MAX_T, "note events")
    if p["smallest_note"] <= 0:
        raise ValueError("SMALLEST_NOTE must be positive")
    if p["n_pitch"] <= 0 or p["pitch_base"] < 0 or p["pitch_base"] + p["n_pitch"] > 256:
        raise ValueError("pitch columns %d..%d: a MIDI pitch is one byte" % (p["pitch_base"], p["pitch_base"] + p["n_pitch"]))
    if n * T > 2 ** 31 - 1:
        raise ValueError("%d windows of %d rows: ticks and record counts are int32" % (n, T))


def song_ordinals(lengths, n):
    """(n,) int32: for every window the ordinal of its song, from the songs' window counts"""
    first_windows(lengths, n)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    return np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)


def note_velocities(x, p):
    """the velocity of a note that starts on a row of velocity ``x`` (reference :78-81, :117-118, :134): in double, the reference's
    operations in its order, truncated toward zero, 127 above 127, negative values kept (down to the int16's end), 0 for a NaN"""
    thr = p["threshold"]
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        x = np.where(x < thr, 0.0, x)
        x = np.where(x >= thr, x - 0.5, x)
        y = (x / (1.0 - thr)) * MAX_VELOCITY
        y = np.where(np.isnan(y), 0.0, np.clip(y, -32768.0, MAX_VELOCITY))
    return np.trunc(y).astype(np.int16)


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _mirror(idx, vel, held, lengths, p, close):
    """(records, offsets): the table of all songs sorted by (song, voice, start) and the n_songs * voices + 1 range bounds"""
    n, T = idx.shape
    V, sn = p["voices"], p["smallest_note"]
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    S, ticks = len(lengths), T // V
    L = n * ticks
    # one sequence per voice through all songs: row r of (L, V) is tick r % ticks of window r // ticks
    pitch = np.where(sounding(idx, p), idx.astype(np.int64), -1).reshape(L, V)
    song_of = np.repeat(np.arange(S), lengths * ticks)
    tick = np.arange(L) - np.repeat((np.cumsum(lengths) - lengths) * ticks, lengths * ticks)
    previous = np.full((L, V), -1, np.int64)
    previous[1:] = pitch[:-1]
    previous[tick == 0] = -1
    repeats = (previous >= 0) & (pitch == previous)
    continues = repeats & ((held.reshape(L, V) != 0) if held is not None else (tick % sn != 0)[:, None])
    ends, starts = (previous >= 0) & ~continues, (pitch >= 0) & ~continues

    def ordered(flags):
        """the flagged (row, voice) pairs sorted by (song, voice, row): their slot song * V + voice, row, and rank within the slot"""
        v, r = np.nonzero(flags.T)
        slot = song_of[r] * V + v
        order = np.argsort(slot, kind="stable")
        slot, r, v = slot[order], r[order], v[order]
        count = np.bincount(slot, minlength=S * V)
        return slot, r, v, count, np.arange(len(slot)) - np.repeat(np.cumsum(count) - count, count)

    s_slot, s_row, s_voice, n_starts, s_rank = ordered(starts)
    e_slot, e_row, _, n_ends, e_rank = ordered(ends)
    open_at_end = n_starts - n_ends
    assert np.all((open_at_end == 0) | (open_at_end == 1)), "starts and ends do not alternate"
    notes = n_ends + (open_at_end if close else 0)
    offsets = np.concatenate([[0], np.cumsum(notes)]).astype(np.int32)
    rec = np.zeros(int(offsets[-1]), RECORD)
    keep = s_rank < notes[s_slot]
    at = offsets[s_slot[keep]] + s_rank[keep]
    rec["start"][at] = tick[s_row[keep]]
    rec["pitch"][at] = pitch[s_row[keep], s_voice[keep]] + p["pitch_base"]
    rec["voice"][at] = s_voice[keep]
    rec["velocity"][at] = DEFAULT_VELOCITY if vel is None else note_velocities(vel.reshape(L, V)[s_row[keep], s_voice[keep]], p)
    closed = np.nonzero(notes > n_ends)[0]
    rec["end"][offsets[closed] + n_ends[closed]] = (lengths * ticks)[closed // V]
    rec["end"][offsets[e_slot] + e_rank] = tick[e_row]
    assert np.all(rec["start"] < rec["end"]), "a note ends before it starts"
    return rec, offsets


# ---- the reference's loop, restated ----------------------------------------------------------------------------------------------
def tracker_loop(idx, vel, held, lengths, p):
    """The reference's own loop (midi_functions.py:69-134) on index rolls, row by row with its tracker list and its two dicts - a
    row's ``notes`` list is [pitch] or [] - song by song: (records, offsets) as the mirror returns them, never closed at the end."""
    idx = np.asarray(idx)
    n, T = idx.shape
    V, thr, SMALLEST_NOTE = p["voices"], p["threshold"], p["smallest_note"]
    on = sounding(idx, p)
    rows, counts, lo = [], [], 0
    for m in np.asarray(lengths, np.int64).reshape(-1).tolist():
        song_idx, song_on = idx[lo:lo + m].reshape(-1), on[lo:lo + m].reshape(-1)
        velocity_roll = None if vel is None else np.asarray(vel[lo:lo + m], np.float32).astype(np.float64).reshape(-1)
        held_notes_roll = None if held is None else np.asarray(held[lo:lo + m]).reshape(-1)
        lo += m
        for voice in range(V):
            current_idx, current_on = song_idx[voice::V], song_on[voice::V]
            if velocity_roll is not None:
                current_velocity_roll = np.copy(velocity_roll[voice::V])
                with np.errstate(all="ignore"):
                    current_velocity_roll[np.where(current_velocity_roll < thr)] = 0
                    current_velocity_roll[np.where(current_velocity_roll >= thr)] -= 0.5
                    current_velocity_roll /= (1.0 - thr)
                    current_velocity_roll *= MAX_VELOCITY
            if held_notes_roll is not None:
                current_held_notes_roll = held_notes_roll[voice::V]
            found = []
            tracker = []
            start_times = dict()
            velocities = dict()
            for i in range(len(current_idx)):
                notes = [int(current_idx[i]) + p["pitch_base"]] if current_on[i] else []
                removal_list = []
                for note in tracker:
                    hold_this_note = True
                    if held_notes_roll is not None:
                        hold_this_note = current_held_notes_roll[i] > 0.5
                        if note not in notes:
                            hold_this_note = False
                    else:
                        hold_this_note = note in notes and i % SMALLEST_NOTE != 0
                    if hold_this_note:
                        notes.remove(note)
                    else:
                        if velocity_roll is not None:
                            velocity = velocities[note]
                            if velocity > MAX_VELOCITY:
                                velocity = int(MAX_VELOCITY)
                        else:
                            velocity = DEFAULT_VELOCITY
                        found.append((start_times[note], i, note, voice, velocity))
                        removal_list.append(note)
                for note in removal_list:
                    tracker.remove(note)
                for note in notes:
                    tracker.append(note)
                    start_times[note] = i
                    if velocity_roll is not None:
                        velocities[note] = int(current_velocity_roll[i])
            rows += found
            counts.append(len(found))
    rec = np.array(rows, RECORD) if rows else np.zeros(0, RECORD)
    return rec, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ---- the device path -----------------------------------------------------------------------------------------------------------
def workspace_bytes(n, n_songs, p):
    """MVAE_EVENTS_WORKSPACE_BYTES: the size of the workspace mvae_note_events wants"""
    return 4 * (2 * n * p["voices"] + 2 * n_songs * (p["voices"] + 1))


def enqueue(idx, vel, held, song, n_songs, p, close, workspace, records, offsets, total, stream):
    """mvae_note_events on device memory the caller owns.  ``idx`` (n, T) uint8 tensor of any strides, ``vel`` float32 / ``held`` uint8
    tensors of the same strides or None, ``song`` (n,) int32, ``workspace`` a tensor of workspace_bytes(n, n_songs, p) bytes,
    ``records`` a uint8 tensor of 12 bytes per record (its size sets the capacity) or None to count only, ``offsets``
    (n_songs * voices + 1,) int32, ``total`` (1,) int32."""
    n, T = idx.shape
    a = hl.EventsArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), vel=hl.ptr(vel), held=hl.ptr(held),
                      song=song.data_ptr(), n=n, T=T, voices=p["voices"], silent=p["silent"], n_pitch=p["n_pitch"], n_songs=n_songs,
                      smallest_note=p["smallest_note"], pitch_base=p["pitch_base"], close_at_end=int(bool(close)),
                      capacity=0 if records is None else records.numel() // RECORD.itemsize, threshold=p["threshold"],
                      workspace=workspace.data_ptr(), records=hl.ptr(records), offsets=offsets.data_ptr(), total=total.data_ptr())
    hl.check(hl.load().mvae_note_events(C.byref(a), stream), "mvae_note_events")


def run_on_device(idx, vel, held, song, n_songs, p, close=False):
    """``enqueue`` with outputs and workspace of its own on the current stream of ``idx``'s device, the records allocated at their
    bound of n * T: the tensors (records as bytes, offsets, total).  ``vel`` and ``held`` are brought to the strides of ``idx``."""
    import torch
    n, T = idx.shape
    dev = idx.device
    if idx.stride(0) <= 0 or idx.stride(1) <= 0:          # (a window axis of one element may carry any stride)
        idx = idx.contiguous()
    vel, held = with_strides_of(idx, vel), with_strides_of(idx, held)
    records = torch.empty(n * T * RECORD.itemsize, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n_songs * p["voices"] + 1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    workspace = torch.empty(workspace_bytes(n, n_songs, p), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        enqueue(idx, vel, held, song, n_songs, p, close, workspace, records, offsets, total, torch.cuda.current_stream().cuda_stream)
    return records, offsets, total


def read_back(records, offsets):
    """the tensors of run_on_device on the host: the offsets first, then only the records they count"""
    offsets = offsets.cpu().numpy()
    return records[:int(offsets[-1]) * RECORD.itemsize].cpu().numpy().view(RECORD), offsets


def event_table(idx, vel, held, lengths, s, device=True, close_at_end=False):
    """``note_events`` as one table: (records, offsets) - a RECORD array of all songs sorted by (song, voice, start) and
    len(lengths) * max_voices + 1 int32 bounds; the notes of voice v of song i are records[offsets[i * V + v]:offsets[i * V + v + 1]]"""
    p = params(s)
    if device:
        import torch
        if not hasattr(idx, "data_ptr"):
            idx = as_rolls(idx)
        if len(idx.shape) != 2:
            raise ValueError("notes are (n, T) index rolls, got shape %r" % (tuple(idx.shape),))
        n, T = idx.shape
        _check(T, p, n)
        song = song_ordinals(lengths, n)          # (every refusal comes before anything touches the device)
        t = device_roll(idx, torch.uint8, "notes")
        v = device_roll(vel, torch.float32, "velocities", t.shape, device=t.device)
        h = device_roll(held, torch.uint8, "held notes", t.shape, device=t.device)
        if n == 0:
            return np.zeros(0, RECORD), np.zeros(1, np.int32)
        with torch.cuda.device(t.device):
            records, offsets, _ = run_on_device(t, v, h, torch.from_numpy(song).to(t.device), len(lengths), p, close_at_end)
            return read_back(records, offsets)
    a = host_roll(idx, np.uint8, "notes")
    n, T = a.shape
    _check(T, p, n)
    first_windows(lengths, n)
    return _mirror(a, host_roll(vel, np.float32, "velocities", a.shape), host_roll(held, np.uint8, "held notes", a.shape), lengths, p,
                   bool(close_at_end))


def split_songs(records, offsets, V):
    """one RECORD array per song (views of ``records``) from the table's bounds"""
    return [records[offsets[i]:offsets[i + V]] for i in range(0, len(offsets) - 1, V)]


def note_events(idx, vel, starts_or_held, lengths, s, device=True, close_at_end=False):
    """The notes of ``len(lengths)`` songs (``lengths``: the songs' window counts, in order; their sum is n and each is > 0, else
    ValueError).  ``idx`` (n, T) uint8 index rolls or (n, T, K) one-hot rolls, ``vel`` (n, T) float velocities or None (every note
    gets 80), ``starts_or_held`` (n, T) the note-start roll of a song-level decode or the held-notes index - 0: a note may start, else
    the row holds - or None (the tick rule) - host arrays, or 2-D device tensors of any strides.  One RECORD array per song (fields
    start, end in ticks of the song, pitch as a MIDI pitch, voice, velocity), sorted by (voice, start)."""
    records, offsets = event_table(idx, vel, starts_or_held, lengths, s, device, close_at_end)
    return split_songs(records, offsets, params(s)["voices"])


def vote_for_programs(instr, lengths, s):
    """The reference's per-voice vote (vae_evaluation.py:598-617) over each song's windows: ``instr`` (n, max_voices) instrument
    indices -> one list of max_voices GM programs per song, the program most windows chose; a tie goes to the program seen first (the
    reference's dict keeps insertion order and replaces on a strict ``>``).  Host arithmetic on n * max_voices bytes."""
    from .sweep import programs_of
    instr = np.asarray(instr)
    first_windows(lengths, instr.shape[0])
    programs = programs_of(instr, _g(s, "instrument_attach_method"))
    out, lo = [], 0
    for m in np.asarray(lengths, np.int64).reshape(-1).tolist():
        song = []
        for voice in range(programs.shape[1]):
            seen, first_seen, votes = np.unique(programs[lo:lo + m, voice], return_index=True, return_counts=True)
            song.append(int(seen[np.lexsort((first_seen, -votes))[0]]))
        out.append(song)
        lo += m
    return out
