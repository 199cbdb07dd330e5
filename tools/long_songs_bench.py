#!/usr/bin/env python3
"""Time the long songs on the MI355X (profiles/r22_long_songs.txt holds the figures).

    python tools/long_songs_bench.py [--songs 32] [--length 20] [--repeats 5] [--root DIR] [--plain-only] [--skip-loop] [--skip-kernels]

The default model (GRU, T = 64, Z = 256, H = 256, bf16); all_z: as many random codes as the 64-song benchmark set has windows.
(a) decoder.long_songs for --songs songs of --length windows, host clock around calls that end in a host read; the same lockstep
    loop through the host (longsongs.nearest_walk(device=False), predict_indices, process_decoder_indices, prepare_encoder_input_list,
    encoder.predict at batch S), once; decoder.predict_indices of the same songs * length windows as the floor; and the split of one
    iteration - walk, decode, feedback, encode - from device events around each stage of the same loop on the engine;
(b) mvae_nearest_walk alone at N = 65 536 and 1 M codes of Z = 256 for S = 1, 32 and 256 songs, device events, beside a device copy of
    all_z (read + write) as the measured HBM rate;
(c) mvae_feedback_rows alone on 65 536 random windows, window-major and time-major, beside mvae_recon_songs on the same rolls.
--plain-only times decoder.predict_songs and decoder.decode_paths - the paths this feature leaves alone - and stops; with --root DIR the
package is imported from another checkout (its library built there): two trees on one machine, run in turns.
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
    ap.add_argument("--songs", type=int, default=32)
    ap.add_argument("--length", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import midi_vae_amd  # noqa: F401
    from midi_vae_amd import generation as gen
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
    lengths = rng.integers(31, 198, 64).tolist()

    if args.plain_only:
        xs = [pk.prepare_decoder_input(s, rng.standard_normal((k, Z)), 0, np.zeros((k, s["signature_vector_length"])), None) for k in lengths]
        code = lambda rows: rng.standard_normal((rows, Z)).astype(np.float32)
        paths = [gen.medley_path([code(8), code(8), code(8)], 4) for _ in range(42)] + [gen.interpolation_path(code(1), code(1), 10) for _ in range(42)]
        print("%d songs of %d .. %d windows = %d windows; %d paths" % (len(lengths), min(lengths), max(lengths), sum(lengths), len(paths)))
        for _ in range(3):
            dec.predict_songs(xs, 32)
            dec.decode_paths(paths, 32)
        t_a, t_b = [], []
        for _ in range(2 * args.repeats):
            t0 = time.perf_counter()
            dec.predict_songs(xs, 32)
            t1 = time.perf_counter()
            dec.decode_paths(paths, 32)
            t2 = time.perf_counter()
            t_a.append(1e3 * (t1 - t0))
            t_b.append(1e3 * (t2 - t1))
        print("predict_songs, no new call                   %s" % stat(t_a))
        print("decode_paths, no new call                    %s" % stat(t_b))
        return

    from midi_vae_amd import longsongs as ls
    from midi_vae_amd import reconstruction as rec
    S, L, N = args.songs, args.length, int(sum(lengths))
    all_z = rng.standard_normal((N, Z)).astype(np.float32)
    codes = rng.normal(0.0, float(np.std(all_z)), (S, Z))
    e = np.std(all_z)
    SD = s["signature_vector_length"]
    dev = torch.device("cuda:0")

    if not args.skip_loop:
        print("(a) %d songs of %d windows, all_z (%d, %d)" % (S, L, N, Z))
        for _ in range(2):
            got = dec.long_songs(all_z, codes, length=L, batch_size=S)
        t_a = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            got = dec.long_songs(all_z, codes, length=L, batch_size=S)
            t_a.append(1e3 * (time.perf_counter() - t0))
        print("    decoder.long_songs                        %s" % stat(t_a))

        def host_route():
            R, previous, picked = codes, np.zeros((S, Z)), np.zeros((S, 0), np.int64)
            notes = []
            for it in range(L):
                w = ls.nearest_walk(all_z, R, picked, e, device=False)
                picked, pulled = w["picked"], w["r"]
                ind = dec.predict_indices(pk.prepare_decoder_input(s, pulled, 0, np.zeros((S, SD)), previous), batch_size=S)
                lists = []
                for k in range(S):
                    Y, I, Vp, Dp, _ = pk.process_decoder_indices(s, {h: a[k:k + 1] for h, a in ind.items()})
                    X = np.append(Y, np.zeros((Y.shape[0], 1)), axis=1)
                    X[np.sum(X, axis=1) == 0, -1] = 1
                    lists.append(pk.prepare_encoder_input_list(s, np.asarray([X]), I[0], np.expand_dims(Vp, 0), np.expand_dims(Dp, 0)))
                notes.append(ind["notes"])
                previous = pulled
                if it + 1 < L:
                    R = m.encoder.predict([np.concatenate([l[j] for l in lists], 0) for j in range(len(lists[0]))], batch_size=S)
            return picked, np.stack(notes, 1)

        m._shared.rng = np.random.default_rng(5)
        got = dec.long_songs(all_z, codes, length=L, batch_size=S)
        m._shared.rng = np.random.default_rng(5)
        t0 = time.perf_counter()
        picked_h, notes_h = host_route()
        t_h = 1e3 * (time.perf_counter() - t0)
        same = all(np.array_equal(d["picked"], picked_h[k]) and np.array_equal(d["notes"], notes_h[k]) for k, d in enumerate(got))
        print("    the same loop through the host            %10.3f ms (1 run); picked and notes of the two routes equal: %s; host / device = %.1f"
              % (t_h, same, t_h / float(np.median(t_a))))
        x = pk.prepare_decoder_input(s, rng.standard_normal((S * L, Z)), 0, np.zeros((S * L, SD)), None)
        for _ in range(2):
            dec.predict_indices(x, batch_size=S)
        t_f = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            dec.predict_indices(x, batch_size=S)
            t_f.append(1e3 * (time.perf_counter() - t0))
        print("    predict_indices of %d windows (the floor) %s; long_songs / floor = %.1f" % (S * L, stat(t_f), float(np.median(t_a)) / float(np.median(t_f))))

        # the split of an iteration: the same stages on the engine, device events around each
        eng = m._shared.get_infer(S)
        p = ls.params(s)
        e_d, den = ls.pull_factors(e)
        A, start = torch.from_numpy(all_z).to(dev), torch.from_numpy(codes).to(dev)
        eps = torch.zeros((S, Z), dtype=torch.float32, device=dev)
        picked = torch.zeros((S, L), dtype=torch.int32, device=dev)
        best, dist = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.float64, device=dev)
        work = torch.empty(ls.workspace_bytes(N, S, Z), dtype=torch.uint8, device=dev)
        pulled = [torch.empty((S, Z), dtype=torch.float32, device=dev) for _ in range(2)]
        first_out = torch.empty_like(start)
        split = {k: [] for k in ("walk", "decode", "feedback", "encode")}
        for rep in range(args.repeats + 1):
            previous = None
            for it in range(L):
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                marks[0].record()
                r_out = first_out if it == 0 else pulled[it & 1]
                eng.stage_decoder_walk(S, dict(all_z=A, r_in=start if it == 0 else None, hist_in=previous, picked=picked, n_picked=it, e=e_d,
                                               den=den, workspace=work, best_out=best, dist_out=dist, r_out=r_out))
                marks[1].record()
                eng.decode(S, want_probs=False, want_velocity=sp.meta_velocity)
                marks[2].record()
                eng.stage_encoder_feedback(S, eng.decoded(S, False), eps, p)
                marks[3].record()
                eng.encode(S)
                marks[4].record()
                marks[4].synchronize()
                previous = r_out
                if rep:
                    for k, name in enumerate(("walk", "decode", "feedback", "encode")):
                        split[name].append(marks[k].elapsed_time(marks[k + 1]))
        print("    one iteration, device events (the stage's staging included): " +
              ", ".join("%s %.3f ms" % (k, float(np.median(v))) for k, v in split.items()) +
              "; sum %.3f ms" % sum(float(np.median(v)) for v in split.values()))

    if args.skip_kernels:
        return
    stream = torch.cuda.current_stream().cuda_stream

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

    for Nw in (65536, 1 << 20):
        A = torch.randn((Nw, Z), dtype=torch.float32, device=dev)
        B2 = torch.empty_like(A)
        ms = timed(lambda: B2.copy_(A))
        rate = 2 * A.numel() * 4 / (float(np.median(ms)) * 1e-3) / 1e12
        print("(b) device copy of all_z (%d, %d): %s = %.2f TB/s read + write" % (Nw, Z, stat(ms), rate))
        del B2
        for Sw in (1, 32, 256):
            R = torch.randn((Sw, Z), dtype=torch.float32, device=dev)
            pk_d = torch.zeros((Sw, 20), dtype=torch.int32, device=dev)
            pk_d[:, :10] = torch.randint(0, Nw, (Sw, 10), dtype=torch.int32, device=dev)
            ws = torch.empty(ls.workspace_bytes(Nw, Sw, Z), dtype=torch.uint8, device=dev)
            b, d = torch.empty(Sw, dtype=torch.int32, device=dev), torch.empty(Sw, dtype=torch.float64, device=dev)
            z, r, h = (torch.empty((Sw, Z), dtype=torch.float32, device=dev) for _ in range(3))
            ms = timed(lambda: ls.enqueue_walk(A, R, None, pk_d, 10, 0.8, 1.8, ws, b, d, z, r, h, stream))
            t = float(np.median(ms)) * 1e-3
            print("    mvae_nearest_walk N = %7d, S = %3d  %s: all_z bytes / time = %.2f TB/s, %.1f G (row, song, column) terms/s"
                  % (Nw, Sw, stat(ms), A.numel() * 4 / t / 1e12, Nw * Sw * Z / t / 1e9))
        del A

    Nw = 65536
    p = ls.params(s)
    idx = rng.integers(0, n_pitch + 1, (Nw, T)).astype(np.uint8)
    vel = rng.random((Nw, T)).astype(np.float32)
    instr = rng.integers(0, 16, (Nw, V)).astype(np.uint8)
    outs = [torch.empty((T, Nw), dtype=torch.uint8, device=dev) for _ in range(3)]
    vo = torch.empty((T, Nw), dtype=torch.float32, device=dev)
    io = torch.empty((V, Nw), dtype=torch.uint8, device=dev)
    for name in ("window-major", "time-major"):
        tr = (lambda a: torch.from_numpy(a).to(dev)) if name == "window-major" else (lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t())
        di, dv, dn = tr(idx), tr(vel), tr(instr)
        ms = timed(lambda: ls.enqueue_feedback(di, dv, None, dn, p, Nw, outs[0], outs[1], vo, outs[2], io, stream))
        print("(c) mvae_feedback_rows, %d windows, %-12s %s" % (Nw, name, stat(ms)))
        ms = timed(lambda: rec.run_on_device(di, dv, None, None, None, p))
        print("    mvae_recon_songs on the same rolls (every window its own song, its outputs allocated in the call) %s" % stat(ms))


if __name__ == "__main__":
    main()
