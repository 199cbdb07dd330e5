#!/usr/bin/env python3
"""Time the song-level decode on the MI355X (profiles/r17_song_decode.txt holds the figures).

    python tools/song_decode_bench.py [--songs 64] [--windows 65536] [--song-length 128] [--repeats 5] [--host-repeats 1]

The default model (GRU, T = 64, Z = 256, H = 256, bf16), --songs songs of 31 to 197 windows.
(a) decoder.predict_indices alone on all windows and (b) decoder.predict_songs with originals on the same decoder inputs,
    alternating, host clock around calls that end in a host read;
(c) the host route to the result of (b): predict_indices, packers.process_decoder_indices song by song (the velocity rules in a
    Python loop over rows), the reference's count arithmetic in NumPy on one-hot rolls - once per --host-repeats;
(d) mvae_recon_songs alone on --windows random windows in songs of --song-length with resident rolls, originals included,
    window-major and time-major, device events;
(e) the same as ONE song of --windows windows whose voice 0 never plays: the worst case of the look-back.
Every timed shape is warmed up first; medians over --repeats, with the range."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa: E402,F401
from midi_vae_amd import packers as pk  # noqa: E402
from midi_vae_amd import reconstruction as rec  # noqa: E402
from midi_vae_amd.config import build_settings, create_kwargs  # noqa: E402


def stat(ms):
    return "%10.3f ms (range %.3f .. %.3f, %d runs)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def host_route(dec, x_all, s, lengths, orig, T):
    """what the project offered before the kernel: every roll to the host, the rules song by song, the counts on one-hot matrices"""
    ind = dec.predict_indices(x_all, 32)
    n_pitch = s["high_crop"] - s["low_crop"]
    out, lo = [], 0
    for m in lengths:
        Y, _, V, D, _ = pk.process_decoder_indices(s, {k: v[lo:lo + m] for k, v in ind.items()})
        Yo = np.eye(n_pitch + 1)[orig[lo:lo + m].reshape(-1)]
        song = Yo[:, :n_pitch]
        unique, counts = np.unique(song * 2 + Y, return_counts=True)
        diff = dict(zip(unique.tolist(), counts.tolist()))
        original, start = int(np.count_nonzero(song)), D == 0
        out.append((V, D, dict(total_original_notes=original, total_predicted_notes=int(np.count_nonzero(Y)),
                               pitch_reconstruction_accuracy=diff.get(3, 0) / original if original else float("nan"),
                               not_predicted_notes=diff.get(2, 0), new_predicted_notes=diff.get(1, 0),
                               predicted_note_start_to_original_errors=int(np.sum(start & (Yo[:, -1] == 1))) / (m * T),
                               predicted_note_start_to_predicted_errors=int(np.sum(start & (Y.sum(1) == 0))) / (m * T))))
        lo += m
    return out


def kernel_ms(idx, vel, orig, first, p, repeats):
    n, T = idx.shape
    carry = torch.empty(rec.carry_bytes(n, p), dtype=torch.uint8, device=idx.device)
    roll = torch.empty((n, T), dtype=torch.float32, device=idx.device)
    start = torch.empty((n, T), dtype=torch.uint8, device=idx.device)
    counts = torch.empty((n, 8), dtype=torch.int32, device=idx.device)
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for r in range(repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rec.enqueue(idx, vel, None, orig, first, p, carry, roll, start, counts, stream)
        e1.record()
        e1.synchronize()
        if r >= 2:
            ms.append(e0.elapsed_time(e1))
    return ms, roll, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--song-length", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    args = ap.parse_args()
    from midi_vae_amd.model import VAE
    s = build_settings()
    m = VAE().create(seed=0, **create_kwargs(s))
    dec = m.decoder
    dec.sample_settings = s
    sp = m.spec
    T, V, n_pitch = sp.T, sp.V, s["high_crop"] - s["low_crop"]
    print("model: %s, T = %d, Z = %d, H = %d, %d voices, %s" % (sp.cell, T, sp.Z, sp.H, V, "bf16"))
    rng = np.random.default_rng(17)
    lengths = rng.integers(31, 198, args.songs).tolist()
    n = sum(lengths)
    xs = [pk.prepare_decoder_input(s, rng.standard_normal((k, sp.Z)), 0, np.zeros((k, s["signature_vector_length"])), None) for k in lengths]
    x_all = [np.concatenate([x[k] for x in xs], 0) for k in range(len(xs[0]))]
    notes = dec.predict_note_indices(x_all, 32)
    orig = np.where(rng.random(notes.shape) < 1 / 3, rng.integers(0, n_pitch + 1, notes.shape), notes).astype(np.uint8)
    first = np.cumsum(lengths) - lengths
    originals = [orig[lo:lo + k] for lo, k in zip(first, lengths)]
    print("%d songs of %d .. %d windows = %d windows" % (len(lengths), min(lengths), max(lengths), n))

    for _ in range(3):
        dec.predict_indices(x_all, 32)
        dec.predict_songs(xs, 32, originals=originals)
    t_a, t_b = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        dec.predict_indices(x_all, 32)
        t1 = time.perf_counter()
        got = dec.predict_songs(xs, 32, originals=originals)
        t2 = time.perf_counter()
        t_a.append(1e3 * (t1 - t0))
        t_b.append(1e3 * (t2 - t1))
    print("(a) predict_indices alone                   %s" % stat(t_a))
    print("(b) predict_songs with originals            %s" % stat(t_b))
    t_c = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        want = host_route(dec, x_all, s, lengths, orig, T)
        t_c.append(1e3 * (time.perf_counter() - t0))
    print("(c) host route to the same result           %s" % stat(t_c))
    same = all(np.array_equal(d["velocity"].astype(np.float64).reshape(-1), Vh) and np.array_equal(d["starts"].reshape(-1), Dh) and
               all(d["metrics"][k] == mh[k] or (np.isnan(d["metrics"][k]) and np.isnan(mh[k])) for k in mh)
               for d, (Vh, Dh, mh) in zip(got, want))
    print("    velocities, note starts and metrics of (b) equal to (c): %s; host route / device route = %.1f"
          % (same, float(np.median(t_c)) / float(np.median(t_b))))

    # ---- the entry point alone ----
    p = rec.params(s)
    N, L = args.windows, args.song_length
    idx = rng.integers(0, n_pitch + 1, (N, T)).astype(np.uint8)
    idx[rng.random((N, T)) < 0.3] = n_pitch
    vel = rng.random((N, T)).astype(np.float32)
    org = np.where(rng.random((N, T)) < 1 / 3, rng.integers(0, n_pitch + 1, (N, T)), idx).astype(np.uint8)
    dev = torch.device("cuda:0")
    layouts = {}
    for name in ("window-major", "time-major"):
        if name == "window-major":
            layouts[name] = tuple(torch.from_numpy(a).to(dev) for a in (idx, vel, org))
        else:
            layouts[name] = tuple(torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t() for a in (idx, vel, org))
    songs = torch.from_numpy(rec.first_windows([L] * (N // L) + ([N % L] if N % L else []), N)).to(dev)
    results = {}
    for name, (di, dv, do) in layouts.items():
        ms, roll, counts = kernel_ms(di, dv, do, songs, p, args.repeats)
        results[name] = (roll.cpu().numpy(), counts.cpu().numpy())
        print("(d) mvae_recon_songs alone, %d windows in songs of %d, %-12s %s" % (N, L, name, stat(ms)))
    print("    the two layouts agree: %s" % all(np.array_equal(a, b) for a, b in zip(*results.values())))
    idx[:, 0::V] = n_pitch          # voice 0 never plays: every look-back of that voice runs to the start of the song
    one = torch.zeros(N, dtype=torch.int32, device=dev)
    for name in layouts:
        di = torch.from_numpy(idx if name == "window-major" else np.ascontiguousarray(idx.T)).to(dev)
        di = di if name == "window-major" else di.t()
        ms, roll, counts = kernel_ms(di, layouts[name][1], layouts[name][2], one, p, args.repeats)
        print("(e) ONE song of %d windows, voice 0 never plays,        %-12s %s" % (N, name, stat(ms)))
    print("    decode of the same %d windows at the rate of (a): %.1f ms" % (N, float(np.median(t_a)) * N / n))


if __name__ == "__main__":
    main()
