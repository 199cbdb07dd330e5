#!/usr/bin/env python3
"""Time the note events on the MI355X (profiles/r18_note_events.txt holds the figures).

    python tools/note_events_bench.py [--songs 64] [--windows 65536] [--song-length 128] [--repeats 7] [--host-repeats 1]
                                      [--root DIR] [--plain-only]

The default model (GRU, T = 64, Z = 256, H = 256, bf16), --songs songs of 31 to 197 windows (the shape of tools/song_decode_bench.py).
(a) decoder.predict_songs without and (b) with note_events=True on the same decoder inputs, alternating, host clock around calls
    that end in a host read;
(c) the host route to the events of (b): events.tracker_loop - the reference's row-by-row loop - on the rolls (b) returned, once per
    --host-repeats; and the NumPy mirror on the same rolls;
(d) mvae_note_events alone on --windows random windows in songs of --song-length with resident rolls, held roll and tick rule,
    window-major and time-major, device events;
(e) the same as ONE song of --windows windows.
--plain-only stops after (a); with --root DIR the package is imported from another checkout (its library built there): (a) of two
trees on one machine, run in turns, is how "predict_songs without note events costs what it cost" is checked.
Every timed shape is warmed up first; medians over --repeats, with the range."""
import argparse
import os
import sys
import time

import numpy as np
import torch


def stat(ms):
    return "%10.3f ms (range %.3f .. %.3f, %d runs)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--song-length", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import midi_vae_amd  # noqa: F401
    from midi_vae_amd import packers as pk
    from midi_vae_amd.config import build_settings, create_kwargs
    from midi_vae_amd.model import VAE
    s = build_settings()
    m = VAE().create(seed=0, **create_kwargs(s))
    dec = m.decoder
    dec.sample_settings = s
    sp = m.spec
    T, V, n_pitch = sp.T, sp.V, s["high_crop"] - s["low_crop"]
    print("tree: %s" % os.path.abspath(args.root))
    print("model: %s, T = %d, Z = %d, H = %d, %d voices, %s" % (sp.cell, T, sp.Z, sp.H, V, "bf16"))
    rng = np.random.default_rng(17)
    lengths = rng.integers(31, 198, args.songs).tolist()
    n = sum(lengths)
    xs = [pk.prepare_decoder_input(s, rng.standard_normal((k, sp.Z)), 0, np.zeros((k, s["signature_vector_length"])), None) for k in lengths]
    print("%d songs of %d .. %d windows = %d windows" % (len(lengths), min(lengths), max(lengths), n))

    for _ in range(3):
        dec.predict_songs(xs, 32)
    if args.plain_only:
        t_a = []
        for _ in range(2 * args.repeats):
            t0 = time.perf_counter()
            dec.predict_songs(xs, 32)
            t_a.append(1e3 * (time.perf_counter() - t0))
        print("(a) predict_songs, no note events            %s" % stat(t_a))
        print("    runs: %s" % " ".join("%.3f" % t for t in t_a))
        return
    from midi_vae_amd import events as ev
    for _ in range(3):
        dec.predict_songs(xs, 32, note_events=True)
    t_a, t_b = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        dec.predict_songs(xs, 32)
        t1 = time.perf_counter()
        got = dec.predict_songs(xs, 32, note_events=True)
        t2 = time.perf_counter()
        t_a.append(1e3 * (t1 - t0))
        t_b.append(1e3 * (t2 - t1))
    print("(a) predict_songs, no note events            %s" % stat(t_a))
    print("(b) predict_songs(note_events=True)          %s" % stat(t_b))
    print("    %d notes in %d songs" % (sum(len(d["events"]) for d in got), len(got)))
    p = ev.params(s)
    rolls = [np.concatenate([d[k] for d in got], 0) for k in ("notes", "velocity", "starts")]
    t_c, t_m = [], []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        want = ev.tracker_loop(rolls[0], rolls[1], rolls[2], lengths, p)
        t_c.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        mirror = ev.event_table(rolls[0], rolls[1], rolls[2], lengths, s, device=False)
        t_m.append(1e3 * (time.perf_counter() - t0))
    print("(c) the tracker loop on the host, same rolls %s" % stat(t_c))
    print("    the NumPy mirror, same rolls             %s" % stat(t_m))
    table = np.concatenate([d["events"] for d in got])
    print("    events of (b) equal to the loop's: %s, to the mirror's: %s; loop / ((b) - (a)) = %.0f"
          % (np.array_equal(table, want[0]), np.array_equal(table, mirror[0]),
             float(np.median(t_c)) / max(float(np.median(t_b)) - float(np.median(t_a)), 1e-3)))

    # ---- the entry point alone ----
    N, L = args.windows, args.song_length
    idx = rng.integers(0, n_pitch + 1, (N, T)).astype(np.uint8)
    idx[rng.random((N, T)) < 0.3] = n_pitch
    flat = idx.reshape(N * T // V, V)
    hold = rng.random(flat.shape) < 0.5          # the voice's previous row again: notes of a few ticks
    for i in range(1, 8):
        flat[i::8] = np.where(hold[i::8], flat[i - 1::8][:len(flat[i::8])], flat[i::8])
    vel = rng.random((N, T)).astype(np.float32)
    held = (rng.random((N, T)) < 0.7).astype(np.uint8)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def kernel_ms(di, dv, dh, song, n_songs):
        work = torch.empty(ev.workspace_bytes(N, n_songs, p), dtype=torch.uint8, device=dev)
        records = torch.empty(N * T * ev.RECORD.itemsize, dtype=torch.uint8, device=dev)
        offsets = torch.empty(n_songs * V + 1, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        ms = []
        for r in range(args.repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev.enqueue(di, dv, dh, song, n_songs, p, False, work, records, offsets, total, stream)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms, int(total.item()), ev.read_back(records, offsets)[0]

    many = ev.song_ordinals([L] * (N // L) + ([N % L] if N % L else []), N)
    for what, song, n_songs in (("(d) %d windows in songs of %d" % (N, L), many, int(many[-1]) + 1),
                                ("(e) ONE song of %d windows" % N, np.zeros(N, np.int32), 1)):
        song = torch.from_numpy(song).to(dev)
        for rule, h in (("held roll", held), ("tick rule", None)):
            tables = []
            for name in ("window-major", "time-major"):
                tr = (lambda a: None if a is None else torch.from_numpy(a).to(dev)) if name == "window-major" else \
                     (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t())
                ms, total, table = kernel_ms(tr(idx), tr(vel), tr(h), song, n_songs)
                tables.append(table)
                print("%s, %s, %-12s %s  %d notes" % (what, rule, name, stat(ms), total))
            print("    the two layouts agree: %s" % np.array_equal(*tables))


if __name__ == "__main__":
    main()
