#!/usr/bin/env python3
"""Time the rolls-from-notes import on the MI355X (profiles/r19_midi_import.txt holds the figures).

    python tools/midi_import_bench.py [--songs 64] [--windows 65536] [--song-length 128] [--repeats 7] [--skip-loops]

The shipped shape: T = 64 rows a window, 4 voices, MAXIMAL_NUMBER_OF_VOICES_PER_TRACK 1, pitches 24..84.  Songs are seeded note tables as
midi_import.quantise returns them: 4 to 6 tracks, a note group every second tick per track, a third of them chords of 2 or 3.
(a) mvae_rolls_from_notes alone on --songs songs of 32 to 197 windows, tables and outputs resident, device events;
(b) the same on --windows windows in songs of --song-length, and (c) as ONE song of --windows windows;
(d) midi_import.rolls_from_notes(device=True) - pack, one upload, the launches, one read back - against device=False (the NumPy
    mirror) on the tables of (a), host clock;
(e) midi_import.tick_loops - the reference's loops over every tick of every track, restated - on the same tables, once.
Every timed shape is warmed up first; medians over --repeats, with the range."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(ms):
    return "%10.3f ms (range %.3f .. %.3f, %d runs)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def table_of(rng, ticks, mi):
    tracks = int(rng.integers(4, 7))
    parts = []
    for k in range(tracks):
        m = max(ticks // 2, 1)
        start = rng.integers(0, ticks, m)
        pitch = rng.integers(30, 90, m)
        depth = np.where(rng.random(m) < 1 / 3, rng.integers(2, 4, m), 1)
        start, pitch, j = np.repeat(start, depth), np.repeat(pitch, depth), np.concatenate([np.arange(d) for d in depth.tolist()])
        rec = np.zeros(len(start), mi.NOTE)
        rec["start"], rec["pitch"], rec["track"] = start, pitch + 4 * j, k
        rec["end"] = start + rng.integers(0, 6, len(start))
        rec["velocity"] = rng.integers(0, 128, len(start))
        parts.append(rec)
    notes = np.concatenate(parts)
    return dict(ticks=int(ticks), programs=[8 * k for k in range(tracks)], tempo=120.0,
                notes=notes[np.lexsort((notes["pitch"], notes["start"], notes["track"]))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--song-length", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-loops", action="store_true")
    args = ap.parse_args()
    import midi_vae_amd  # noqa: F401
    from midi_vae_amd import midi_import as mi
    from midi_vae_amd.config import build_settings
    s = build_settings()
    p = mi.params(s)
    T, V = p["T"], p["voices"]
    ticks_per_window = T // V
    print("T = %d, %d voices, max %d voices a track, pitches %d..%d" % (T, V, p["max_per_track"], p["pitch_base"], p["pitch_base"] + p["n_pitch"]))
    rng = np.random.default_rng(19)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def kernel_ms(tables):
        packed = mi.pack_tables(tables, p, T)
        d = mi.upload(packed, p, dev)
        n, S = int(packed["lengths"].sum()), len(tables)
        idx, held, raw = (torch.empty((n, T), dtype=torch.uint8, device=dev) for _ in range(3))
        vel = torch.empty((n, T), dtype=torch.float32, device=dev)
        work = torch.empty(mi.workspace_bytes(packed["cells"], S), dtype=torch.uint8, device=dev)
        ms = []
        for r in range(args.repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mi.enqueue(d, p, T, S, len(packed["notes"]), int(packed["track_off"][-1]), n, packed["cells"], work, idx, held, raw, vel, stream)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms, n, len(packed["notes"]), packed["cells"]

    lengths = rng.integers(32, 198, args.songs).tolist()
    tables = [table_of(rng, k * ticks_per_window, mi) for k in lengths]
    ms, n, notes, cells = kernel_ms(tables)
    print("(a) %d songs of %d .. %d windows = %d windows, %d notes, %d track ticks" % (len(lengths), min(lengths), max(lengths), n, notes, cells))
    print("    mvae_rolls_from_notes alone              %s" % stat(ms))

    t_d, t_m = [], []
    got = mi.rolls_from_notes(tables, s)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        got = mi.rolls_from_notes(tables, s)
        t1 = time.perf_counter()
        want = mi.rolls_from_notes(tables, s, device=False)
        t2 = time.perf_counter()
        t_d.append(1e3 * (t1 - t0))
        t_m.append(1e3 * (t2 - t1))
    print("(d) rolls_from_notes(device=True), same tables %s" % stat(t_d))
    print("    rolls_from_notes(device=False), the mirror %s" % stat(t_m))
    same = all(np.array_equal(got[k], want[k]) for k in ("idx", "held", "vel_raw", "slots", "slot_voice")) and \
        np.array_equal(got["vel"].view(np.uint32), want["vel"].view(np.uint32))
    print("    device equal to the mirror: %s" % same)
    if not args.skip_loops:
        t0 = time.perf_counter()
        loops = [mi.tick_loops(t, p) for t in tables]
        t_e = 1e3 * (time.perf_counter() - t0)
        lo, ok = 0, True
        for t, k, out in zip(tables, lengths, loops):
            ok = ok and np.array_equal(want["idx"][lo:lo + k].reshape(-1), out[0]) and np.array_equal(want["held"][lo:lo + k].reshape(-1), out[1])
            lo += k
        print("(e) the reference's tick loops, same tables   %10.3f ms (1 run); equal to the mirror: %s" % (t_e, ok))
        print("    loops / device = %.0f, loops / mirror = %.1f" % (t_e / float(np.median(t_d)), t_e / float(np.median(t_m))))

    N, L = args.windows, args.song_length
    many = [table_of(rng, L * ticks_per_window, mi) for _ in range(N // L)]
    ms, n, notes, cells = kernel_ms(many)
    print("(b) %d windows in songs of %d: %d notes, %d track ticks %s" % (n, L, notes, cells, stat(ms)))
    del many
    one = [table_of(rng, N * ticks_per_window, mi)]
    ms, n, notes, cells = kernel_ms(one)
    print("(c) ONE song of %d windows: %d notes, %d track ticks    %s" % (n, notes, cells, stat(ms)))


if __name__ == "__main__":
    main()
