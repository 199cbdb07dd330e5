"""midi_vae_amd.midifile: the bytes write_midi produces - derived by hand from the Standard MIDI File layout the module's docstring
states, not taken from its output - the variable-length quantities, and read_midi(write_midi(x)) == x on the songs of
tests/golden/midi_events.npz."""
import io

import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import midifile as mf
from tests.events_contract import PASSES, load_fixture


def h(text):
    return bytes.fromhex(text.replace(" ", ""))


def test_two_voices_three_notes_byte_for_byte(tmp_path):
    # 120 quarter notes a minute, a tick a 16th: 480 beats a minute, 60e6 / 480 = 125000 = 0x01E848 microseconds a beat
    tracks = [[(0, 2, 60, 100), (2, 3, 62, 200)],          # the second starts on the tick the first ends on; velocity 200 is clamped
              [(1, 131, 48, -5)]]                          # 130 ticks = 130000 MIDI ticks: a three-byte delta; velocity -5 is clamped to 0
    want = b"".join([
        h("4D546864 00000006 0001 0003 03E8"),             # MThd, 6 bytes: format 1, three tracks, 1000 ticks a beat
        h("4D54726B 00000013"),                            # MTrk, 19 bytes: the conductor track
        h("00 FF5103 01E848"),                             #   set tempo
        h("00 FF5804 04021808"),                           #   4/4, 24 clocks a click, 8 32nds a beat
        h("00 FF2F00"),                                    #   end of track
        h("4D54726B 00000019"),                            # MTrk, 25 bytes: voice 0
        h("00 C000"),                                      #   program 0 on channel 0
        h("00 903C64"),                                    #   tick 0: note on 60, velocity 100
        h("8F50 803C00"),                                  #   + 2000 = 15 * 128 + 80: note off 60 - before the note on of that tick
        h("00 903E7F"),                                    #   note on 62, velocity 127
        h("8768 803E00"),                                  #   + 1000 = 7 * 128 + 104: note off 62
        h("00 FF2F00"),
        h("4D54726B 00000012"),                            # MTrk, 18 bytes: voice 1
        h("00 C128"),                                      #   program 40 on channel 1
        h("8768 913000"),                                  #   + 1000: note on 48, velocity 0
        h("87F750 813000"),                                #   + 130000 = 7 * 16384 + 119 * 128 + 80: note off 48
        h("00 FF2F00"),
    ])
    assert mf.to_bytes(tracks, [0, 40], 120) == want
    path = tmp_path / "song.mid"
    mf.write_midi(str(path), tracks, [0, 40], 120)
    assert path.read_bytes() == want
    got = mf.read_midi(str(path))
    assert (got["format"], got["division"], got["tempos"]) == (1, 1000, [(0, 125000)])
    assert [(t["program"], t["channel"]) for t in got["tracks"]] == [(None, None), (0, 0), (40, 1)]
    assert got["tracks"][1]["notes"] == [(0, 2000, 60, 100), (2000, 3000, 62, 127)] and got["tracks"][2]["notes"] == [(1000, 131000, 48, 0)]
    # another tempo: 100 bpm at 8th-note ticks = 200 beats a minute = 300000 = 0x0493E0 microseconds
    assert mf.to_bytes([[]], [5], 100, smallest_note=8)[22:41] == h("00 FF5103 0493E0 00 FF5804 04021808 00 FF2F00")


@pytest.mark.parametrize("value,text", [(0, "00"), (127, "7F"), (128, "8100"), (16383, "FF7F"), (16384, "818000"),
                                        (2097151, "FFFF7F"), (2097152, "81808000"), (0x0FFFFFFF, "FFFFFF7F")])
def test_variable_length_quantities(value, text):
    assert mf.vlq(value) == h(text)
    assert mf._read_vlq(h(text) + b"\x00", 0) == (value, len(h(text)))
    # as a delta in a file: a note that long, on roll ticks of one MIDI tick each is not expressible - so through the bytes of a track
    body = b"\x00\xc0\x00" + mf.vlq(value) + h("903C40") + mf.vlq(value) + h("803C00") + h("00FF2F00")
    data = h("4D546864 00000006 0000 0001 03E8") + b"MTrk" + len(body).to_bytes(4, "big") + body
    assert mf.read_midi(io.BytesIO(data))["tracks"][0]["notes"] == [(value, 2 * value, 60, 64)]


def test_vlq_refuses_what_does_not_fit():
    for value in (-1, 0x10000000):
        with pytest.raises(ValueError):
            mf.vlq(value)
    with pytest.raises(ValueError):
        mf._read_vlq(h("8080808000"), 0)


def test_reader_takes_running_status_and_format_0():
    body = (h("00 C105") + h("00 913C40") + h("60 3E50")          # running status: a second note on
            + h("60 3C00") + h("00 FF0103 616263")                # note on of velocity 0 closes the open 60; a text event is skipped
            + h("60 813E00") + h("00 FF2F00"))
    data = h("4D546864 00000006 0000 0001 01E0") + b"MTrk" + len(body).to_bytes(4, "big") + body
    got = mf.read_midi(io.BytesIO(data))
    assert (got["format"], got["division"], got["tempos"]) == (0, 480, [])
    assert got["tracks"] == [dict(program=5, channel=1, notes=[(0, 192, 60, 64), (96, 288, 62, 80)])]
    with pytest.raises(ValueError):
        mf.read_midi(io.BytesIO(b"RIFF" + data[4:]))
    with pytest.raises(ValueError):
        mf.read_midi(io.BytesIO(h("4D546864 00000006 0002 0001 01E0")))


def test_writer_refuses_what_it_cannot_write():
    for tracks, programs, bpm in (([[]], [0, 1], 120), ([[]], [128], 120), ([[(0, 1, 128, 64)]], [0], 120), ([[(2, 1, 60, 64)]], [0], 120),
                                  ([[(-1, 1, 60, 64)]], [0], 120), ([[]], [0], 0), ([[]] * 17, [0] * 17, 120)):
        with pytest.raises(ValueError):
            mf.to_bytes(tracks, programs, bpm)


def test_round_trip_on_the_fixture_songs():
    fx = load_fixture()
    V, songs, notes = 4, 0, 0
    for g in (fx["a"], fx["b"]):
        for name in PASSES:
            rec, off = g["notes_" + name]
            for i in range(len(g["lengths"])):
                tracks = [rec[off[i * V + v]:off[i * V + v + 1]] for v in range(V)]
                got = mf.read_midi(io.BytesIO(mf.to_bytes(tracks, fx["programs"], fx["bpm"], fx["s"]["SMALLEST_NOTE"])))
                assert got["tempos"] == [(0, int(round(60e6 / fx["tempo"])))] and len(got["tracks"]) == 1 + V
                for v in range(V):
                    t = got["tracks"][1 + v]
                    assert (t["program"], t["channel"]) == (fx["programs"][v], v) or (len(tracks[v]) == 0 and t["channel"] == v)
                    want = [(int(r["start"]) * 1000, int(r["end"]) * 1000, int(r["pitch"]), min(max(int(r["velocity"]), 0), 127))
                            for r in tracks[v]]
                    assert t["notes"] == want
                    notes += len(want)
                songs += 1
    assert songs == 3 * (len(fx["a"]["lengths"]) + len(fx["b"]["lengths"])) and notes > 10000
