#!/usr/bin/env python3
"""Time the generated songs on the MI355X (profiles/r21_generation.txt holds the figures).

    python tools/generation_bench.py [--songs 42] [--windows 65536] [--song-length 128] [--repeats 7] [--root DIR] [--plain-only]

The default model (GRU, T = 64, Z = 256, H = 256, bf16).
(a) decoder.decode_paths(note_events=True, pianoroll=True) on --songs medleys (3 songs of 8 windows, bridges of 4) plus --songs
    interpolation songs of length 10 - the reference's defaults - host clock around calls that end in a host read; the same without
    events and images;
(b) the host route to the same songs, once: the reference's window-by-window loop - a blend on the host, prepare_decoder_input,
    decoder.predict_indices and packers.process_decoder_indices for ONE window per call - then the NumPy mirrors of the note events and
    of the image on the collected rolls;
(c) mvae_latent_paths alone: --windows windows of Z = 256 in songs of --song-length (every window a blend, z and history written),
    float32 and float64 anchors, and as ONE song; device events;
(d) mvae_pianoroll alone on --windows random windows with resident rolls, in songs of --song-length and as ONE song, window-major and
    time-major.
--plain-only times decoder.predict_songs WITHOUT the new flag and stops; with --root DIR the package is imported from another
checkout (its library built there): two trees on one machine, run in turns, is how "predict_songs costs what it cost" is checked.
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
    ap.add_argument("--songs", type=int, default=42)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--song-length", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
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
    T, V, Z, n_pitch = sp.T, sp.V, sp.Z, s["high_crop"] - s["low_crop"]
    print("tree: %s" % os.path.abspath(args.root))
    print("model: %s, T = %d, Z = %d, H = %d, %d voices, %s" % (sp.cell, T, Z, sp.H, V, "bf16"))
    rng = np.random.default_rng(17)

    if args.plain_only:
        lengths = rng.integers(31, 198, 64).tolist()
        xs = [pk.prepare_decoder_input(s, rng.standard_normal((k, Z)), 0, np.zeros((k, s["signature_vector_length"])), None) for k in lengths]
        print("%d songs of %d .. %d windows = %d windows" % (len(lengths), min(lengths), max(lengths), sum(lengths)))
        for _ in range(3):
            dec.predict_songs(xs, 32)
        t_a = []
        for _ in range(2 * args.repeats):
            t0 = time.perf_counter()
            dec.predict_songs(xs, 32)
            t_a.append(1e3 * (time.perf_counter() - t0))
        print("predict_songs, no new flag                   %s" % stat(t_a))
        print("    runs: %s" % " ".join("%.3f" % t for t in t_a))
        return

    from midi_vae_amd import events as ev
    from midi_vae_amd import generation as gen
    from midi_vae_amd import pianoroll as pr
    code = lambda rows: rng.standard_normal((rows, Z)).astype(np.float32)
    paths = [gen.medley_path([code(8), code(8), code(8)], 4) for _ in range(args.songs)]
    paths += [gen.interpolation_path(code(1), code(1), 10) for _ in range(args.songs)]
    n = sum(len(p["a0"]) for p in paths)
    print("%d medleys and %d interpolation songs = %d windows" % (args.songs, args.songs, n))
    for _ in range(3):
        dec.decode_paths(paths, 32, note_events=True, pianoroll=True)
        dec.decode_paths(paths, 32)
    t_a, t_p = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        got = dec.decode_paths(paths, 32, note_events=True, pianoroll=True)
        t1 = time.perf_counter()
        dec.decode_paths(paths, 32)
        t2 = time.perf_counter()
        t_a.append(1e3 * (t1 - t0))
        t_p.append(1e3 * (t2 - t1))
    print("(a) decode_paths with note events and images  %s" % stat(t_a))
    print("    decode_paths without either               %s" % stat(t_p))
    print("    %d notes, %d image cells" % (sum(len(d["events"]) for d in got), sum(d["pianoroll"].size for d in got)))

    t0 = time.perf_counter()
    host, SD = [], s["signature_vector_length"]
    for p in paths:          # the reference's loop: one window per decode call
        A, previous, rows = p["anchors"], np.zeros((1, Z)), []
        for w in range(len(p["a0"])):
            if p["a1"][w] < 0:
                z = A[p["a0"][w]][None]
            else:
                z = (A[p["a0"][w]] * float(p["c0"][w]) + A[p["a1"][w]] * float(p["c1"][w]))[None]          # (Python floats, as the reference's t)
            indices = dec.predict_indices(pk.prepare_decoder_input(s, z, 0, np.zeros((1, SD)), previous), 32)
            Y, I, Vp, D, _ = pk.process_decoder_indices(s, indices)
            rows.append((indices["notes"], Vp.reshape(1, -1), D.reshape(1, -1)))
            previous = z
        notes, vel, starts = (np.concatenate([r[k] for r in rows], 0) for k in range(3))
        m_w = len(rows)
        events = ev.event_table(notes, vel.astype(np.float32), starts.astype(np.uint8), [m_w], s, device=False)
        image = pr.images(notes, vel, [m_w], s, device=False)[0]
        host.append((notes, events, image))
    t_b = 1e3 * (time.perf_counter() - t0)
    print("(b) the host route, window by window          %10.3f ms (1 run)" % t_b)
    same = all(np.array_equal(h[0], d["notes"]) for h, d in zip(host, got))
    print("    notes of the two routes equal: %s (the host route applies the velocity rules per window, as the reference's loop does);"
          " host / device = %.0f" % (same, t_b / float(np.median(t_a))))

    # ---- the entry points alone ----
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    N, L = args.windows, args.song_length

    def timed(call):
        ms = []
        for r in range(args.repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    from midi_vae_amd.reconstruction import first_windows
    songs = [L] * (N // L) + ([N % L] if N % L else [])
    anchors = rng.standard_normal((4096, Z))
    table = dict(a0=rng.integers(0, 4096, N).astype(np.int32), a1=rng.integers(0, 4096, N).astype(np.int32), c0=rng.random(N), c1=rng.random(N))
    z_out = torch.empty((N, Z), dtype=torch.float32, device=dev)
    h_out = torch.empty((N, Z), dtype=torch.float32, device=dev)
    for what, first in (("songs of %d" % L, first_windows(songs, N)), ("ONE song", np.zeros(N, np.int32))):
        for kind in (np.float32, np.float64):
            run = gen.upload(dict(table, anchors=anchors.astype(kind), first_window=first), dev)
            ms = timed(lambda: gen.enqueue(run, 0, N, z_out, h_out, stream))
            print("(c) mvae_latent_paths, %d windows, %s, %s anchors  %s" % (N, what, np.dtype(kind).name, stat(ms)))

    p = pr.params(s)
    idx = rng.integers(0, n_pitch + 1, (N, T)).astype(np.uint8)
    idx[rng.random((N, T)) < 0.3] = n_pitch
    flat = idx.reshape(N * T // V, V)
    hold = rng.random(flat.shape) < 0.5          # the voice's previous row again: notes of a few ticks
    for i in range(1, 8):
        flat[i::8] = np.where(hold[i::8], flat[i - 1::8][:len(flat[i::8])], flat[i::8])
    vel = rng.random((N, T)).astype(np.float32)
    img = torch.empty((N * T // V, n_pitch), dtype=torch.float64, device=dev)
    for what, first in (("songs of %d" % L, first_windows(songs, N)), ("ONE song", np.zeros(N, np.int32))):
        first_d = torch.from_numpy(first).to(dev)
        results = []
        for name in ("window-major", "time-major"):
            tr = (lambda a: torch.from_numpy(a).to(dev)) if name == "window-major" else \
                 (lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t())
            di, dv = tr(idx), tr(vel)
            ms = timed(lambda: pr.enqueue(di, dv, first_d, p, img, stream))
            results.append(img.cpu().numpy())
            print("(d) mvae_pianoroll, %d windows, %s, %-12s %s" % (N, what, name, stat(ms)))
        print("    the two layouts agree: %s; cells drawn: %d" % (np.array_equal(*results), int(np.count_nonzero(results[0]))))


if __name__ == "__main__":
    main()
