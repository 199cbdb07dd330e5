"""A Standard MIDI File writer for decoded songs, and the minimal reader its tests need.  Pure Python, no dependency.

``write_midi`` writes what the reference configures pretty_midi to write (midi_functions.py:60-67, :122, :137): format 1, 1000 ticks
per beat, the tempo ``bpm * smallest_note / 4`` beats per minute, 4/4 at tick 0, one roll tick = one beat = 1000 MIDI ticks, one
track per voice with its program.  The notes, ticks, tempo and programs are the reference's; the BYTE ORDER of the file is this
module's own and no byte-for-byte equality with pretty_midi's output is claimed:

    MThd  format 1, 1 + voices tracks, division 1000
    MTrk  the conductor track: set-tempo (round(60e6 / tempo) microseconds per beat), time signature 4/4 (24 clocks a click, 8
          32nd notes a beat), end of track - all at delta 0
    MTrk  per voice v, on channel v: program change at delta 0, then the voice's note events sorted by tick - at equal ticks every
          note-off (0x8v, velocity 0) before every note-on (0x9v), otherwise in the order given - each with its full status byte (no
          running status), deltas as variable-length quantities, end of track at delta 0 after the last event.

Velocities are CLAMPED to 0..127 on writing - a deliberate difference: the reference hands pretty_midi the negative velocities its
scaling produces for a threshold below 0.5, and pretty_midi's writer raises.  A note of velocity 0 is written as a note-on of
velocity 0, which players take for a note-off: it is silent, as in the reference's files.

``read_midi`` is the inverse for files of this kind, not a MIDI importer: format 0 or 1, note on and off, program change, set-tempo,
running status accepted, everything else skipped.  A note-on of velocity 0 closes the earliest open note of its pitch and channel -
and OPENS a note of velocity 0 where none is open, so that what write_midi wrote reads back.
"""
from __future__ import annotations

import io
import struct

TICKS_PER_BEAT = 1000


def vlq(value):
    """a variable-length quantity: 7 bits a byte, most significant first, bit 7 set on all but the last"""
    value = int(value)
    if not 0 <= value <= 0x0FFFFFFF:
        raise ValueError("a variable-length quantity holds 0..0x0FFFFFFF, got %d" % value)
    out = [value & 0x7F]
    value >>= 7
    while value:
        out.append(0x80 | (value & 0x7F))
        value >>= 7
    return bytes(reversed(out))


def _read_vlq(data, at):
    value = 0
    for _ in range(4):
        b = data[at]
        at += 1
        value = (value << 7) | (b & 0x7F)
        if not b & 0x80:
            return value, at
    raise ValueError("a variable-length quantity longer than four bytes")


def _chunk(tag, body):
    return tag + struct.pack(">I", len(body)) + body


def _notes_of(track):
    """(start, end, pitch, velocity) tuples of ints from tuples or from a record array with those fields"""
    names = getattr(getattr(track, "dtype", None), "names", None)
    if names:
        return list(zip(track["start"].tolist(), track["end"].tolist(), track["pitch"].tolist(), track["velocity"].tolist()))
    return [tuple(int(x) for x in note[:4]) for note in track]


def write_midi(path_or_file, tracks, programs, bpm, smallest_note=16):
    """Write SMF format 1.  ``tracks``: per voice its notes, (start, end, pitch, velocity) in ticks of the roll - tuples, or a record
    array with those fields (events.RECORD); ``programs``: per voice its GM program 0..127; ``bpm``: quarter notes per minute, a
    tick of the roll being a 1 / ``smallest_note`` note (the file's tempo is bpm * smallest_note / 4, one beat a tick).  Velocities
    are clamped to 0..127 (see the module's docstring).  ``path_or_file``: a path, or a binary file object."""
    if len(tracks) != len(programs):
        raise ValueError("%d tracks, %d programs" % (len(tracks), len(programs)))
    if len(tracks) > 16:
        raise ValueError("one channel per voice: at most 16 voices")
    tempo = float(bpm) * (smallest_note / 4)
    if not tempo > 0:
        raise ValueError("the tempo must be positive, got bpm %r" % (bpm,))
    us_per_beat = int(round(60e6 / tempo))
    if not 1 <= us_per_beat <= 0xFFFFFF:
        raise ValueError("a tempo of %r beats per minute does not fit the set-tempo event" % (tempo,))
    conductor = (b"\x00\xff\x51\x03" + struct.pack(">I", us_per_beat)[1:] + b"\x00\xff\x58\x04\x04\x02\x18\x08" + b"\x00\xff\x2f\x00")
    chunks = [_chunk(b"MThd", struct.pack(">HHH", 1, 1 + len(tracks), TICKS_PER_BEAT)), _chunk(b"MTrk", conductor)]
    for voice, (track, program) in enumerate(zip(tracks, programs)):
        program = int(program)
        if not 0 <= program <= 127:
            raise ValueError("program %d of voice %d is no GM program" % (program, voice))
        events = []          # (MIDI tick, 0 for off / 1 for on, order, bytes)
        for order, (start, end, pitch, velocity) in enumerate(_notes_of(track)):
            if not 0 <= start <= end or not 0 <= pitch <= 127:
                raise ValueError("voice %d: note (start %d, end %d, pitch %d) cannot be written" % (voice, start, end, pitch))
            events.append((start * TICKS_PER_BEAT, 1, order, bytes((0x90 | voice, pitch, min(max(velocity, 0), 127)))))
            events.append((end * TICKS_PER_BEAT, 0, order, bytes((0x80 | voice, pitch, 0))))
        events.sort(key=lambda e: e[:3])
        body, now = bytearray(b"\x00" + bytes((0xC0 | voice, program))), 0
        for tick, _, _, message in events:
            body += vlq(tick - now) + message
            now = tick
        body += b"\x00\xff\x2f\x00"
        chunks.append(_chunk(b"MTrk", bytes(body)))
    data = b"".join(chunks)
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as f:
            f.write(data)


def read_midi(path_or_file):
    """dict ``format``, ``division`` (ticks per beat), ``tempos`` [(tick, microseconds per beat)] and ``tracks``: per MTrk chunk a dict
    ``program`` (the last program change, or None), ``channel`` (of its first channel event, or None) and ``notes``
    [(start, end, pitch, velocity)] in MIDI ticks, sorted by start.  See the module's docstring for what is read."""
    if hasattr(path_or_file, "read"):
        data = path_or_file.read()
    else:
        with open(path_or_file, "rb") as f:
            data = f.read()
    if data[:4] != b"MThd" or struct.unpack(">I", data[4:8])[0] < 6:
        raise ValueError("not a Standard MIDI File")
    fmt, ntracks, division = struct.unpack(">HHH", data[8:14])
    if fmt not in (0, 1) or division & 0x8000:
        raise ValueError("format %d / division 0x%04x: only formats 0 and 1 with ticks per beat are read" % (fmt, division))
    at = 8 + struct.unpack(">I", data[4:8])[0]
    tempos, tracks = [], []
    while at + 8 <= len(data) and len(tracks) < ntracks:
        tag, size = data[at:at + 4], struct.unpack(">I", data[at + 4:at + 8])[0]
        body, at = data[at + 8:at + 8 + size], at + 8 + size
        if tag != b"MTrk":
            continue
        track = dict(program=None, channel=None, notes=[])
        pending = {}          # (channel, pitch) -> [(start, velocity, order)], the earliest first
        i, now, status, order = 0, 0, None, 0
        while i < len(body):
            delta, i = _read_vlq(body, i)
            now += delta
            if body[i] & 0x80:
                status = body[i]
                i += 1
            elif status is None:
                raise ValueError("a data byte without a status")
            if status == 0xFF:
                kind = body[i]
                size, i = _read_vlq(body, i + 1)
                if kind == 0x51 and size == 3:
                    tempos.append((now, int.from_bytes(body[i:i + 3], "big")))
                i += size
                status = None
                if kind == 0x2F:
                    break
                continue
            if status in (0xF0, 0xF7):
                size, i = _read_vlq(body, i)
                i += size
                status = None
                continue
            high, channel = status & 0xF0, status & 0x0F
            if track["channel"] is None:
                track["channel"] = channel
            if high in (0xC0, 0xD0):
                if high == 0xC0:
                    track["program"] = body[i]
                i += 1
                continue
            pitch, value = body[i], body[i + 1]
            i += 2
            open_notes = pending.setdefault((channel, pitch), [])
            if high == 0x90 and (value > 0 or not open_notes):
                open_notes.append((now, value, order))
                order += 1
            elif high in (0x80, 0x90) and open_notes:
                start, velocity, first = open_notes.pop(0)
                track["notes"].append((start, first, now, pitch, velocity))
        track["notes"] = [(start, end, pitch, velocity) for start, _, end, pitch, velocity in sorted(track["notes"])]
        tracks.append(track)
    tempos.sort()
    return dict(format=fmt, division=division, tempos=tempos, tracks=tracks)


def to_bytes(tracks, programs, bpm, smallest_note=16):
    """what write_midi writes, as bytes"""
    f = io.BytesIO()
    write_midi(f, tracks, programs, bpm, smallest_note)
    return f.getvalue()
