#!/usr/bin/env python3
"""Time the window descriptors on the MI355X against their NumPy mirror (profiles/r15_window_descriptors.txt holds the figures).

    python tools/descriptor_bench.py [--windows 65536] [--sweep 2304] [--repeats 7] [--mirror-windows 4096]

1. 65 536 windows at the shipped shape (T = 64, 4 voices, 61 columns), random walks as in tests/golden/make_descriptor_fixtures.py.
   Per descriptor: the kernel alone (device events around the launch, rolls resident, window-major and time-major), the whole call
   (host rolls in, host results out, ends in the device-to-host copy) and the mirror on the host.  The signature mirror is a Python
   loop per window and is timed on the first --mirror-windows windows; its figure is per window.
2. The 2 304-window batch of one latent sweep through the default model: decoder.predict_descriptors against
   decoder.predict_note_indices followed by the two mirrors, alternating, host clock around calls that end in a host read.
Every timed shape is warmed up first; medians over --repeats, with the range."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa: E402,F401
from midi_vae_amd import descriptors as de  # noqa: E402
from midi_vae_amd import packers as pk  # noqa: E402
from midi_vae_amd.config import build_settings, create_kwargs  # noqa: E402


def walks(rng, n, T, V, n_pitch, p_silent, p_hold):
    ticks = T // V
    rest, hold = rng.random((n, ticks, V)) < p_silent, rng.random((n, ticks, V)) < p_hold
    step = np.where(hold, 0, rng.integers(-4, 5, (n, ticks, V)))
    step[rest] = 0
    q = np.clip(rng.integers(0, n_pitch, (n, 1, V)) + np.cumsum(step, 1), 0, n_pitch - 1)
    return np.where(rest, n_pitch, q).astype(np.uint8).reshape(n, T)


def stat(ms):
    return "%9.3f ms (range %.3f .. %.3f)" % (float(np.median(ms)), min(ms), max(ms))


def host_time(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--sweep", type=int, default=2304)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mirror-windows", type=int, default=4096)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("descriptor_bench.py measures the MI355X: no device is visible")
    s = build_settings()
    p = de.params(s)
    T, V, n = s["output_length"], p["voices"], args.windows
    rng = np.random.default_rng(15)
    gens = ((0.35, 0.0), (0.3, 0.6), (0.2, 0.8), (0.9, 0.5))
    idx = np.concatenate([walks(rng, n // 4, T, V, p["n_pitch"], ps, ph) for ps, ph in gens], 0)
    n = idx.shape[0]
    print("%d windows, T = %d, %d voices, %d pitch columns, resolution %d" % (n, T, V, p["n_pitch"], p["resolution"]))

    wm = torch.from_numpy(idx).cuda()
    tm = torch.from_numpy(np.ascontiguousarray(idx.T)).cuda().t()
    sig = torch.empty((n, 15), dtype=torch.float64, device="cuda")
    harm = torch.empty((n, V * V), dtype=torch.float64, device="cuda")
    tonal = de._tonal_on(wm.device)
    stream = torch.cuda.current_stream().cuda_stream

    def kernel_ms(t, so, ho):
        run = lambda: de.enqueue(t, p, so, ho, tonal if ho is not None else None, stream)
        run()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    for name, so, ho in (("signature", sig, None), ("harmonicity", None, harm)):
        for layout, t in (("window-major", wm), ("time-major", tm)):
            print("%-12s kernel, %-12s %s" % (name, layout, stat(kernel_ms(t, so, ho))))
    for name, fn in (("signature", de.signature_vectors), ("harmonicity", de.harmonicity)):
        print("%-12s whole call (host rolls -> host result)  %s" % (name, stat(host_time(lambda: fn(idx, s), args.repeats))))
    m = min(args.mirror_windows, n)
    sub = idx[:: n // m][:m]
    ms = host_time(lambda: de.signature_vectors(sub, s, device=False), 3)
    print("signature    mirror, %d windows %s = %.1f us per window" % (m, stat(ms), 1e3 * np.median(ms) / m))
    ms = host_time(lambda: de.harmonicity(idx, s, device=False), 3)
    print("harmonicity  mirror, %d windows %s = %.2f us per window" % (n, stat(ms), 1e3 * np.median(ms) / n))
    got_s, got_h = de.signature_vectors(sub, s), de.harmonicity(sub, s)
    want_s, want_h = de.signature_vectors(sub, s, device=False), de.harmonicity(sub, s, device=False)
    print("device against mirror on %d windows: signature max |diff| %.3g, harmonicity max |diff| %.3g, NaN places equal: %s"
          % (m, np.abs(got_s - want_s).max(), np.nanmax(np.abs(got_h - want_h)), np.array_equal(np.isnan(got_h), np.isnan(want_h))))

    # ---- one latent sweep through the decoder --------------------------------------------------------------------------------
    from midi_vae_amd.model import VAE
    model = VAE().create(**create_kwargs(s))
    model.decoder.sample_settings = s
    k = args.sweep
    z = np.random.default_rng(16).standard_normal((k, s["latent_dim"]))
    dec_in = pk.prepare_decoder_input(s, z, 0, np.zeros((k, s["signature_vector_length"])), None)

    def fused():
        return model.decoder.predict_descriptors(dec_in, batch_size=k)

    def decode_only():
        return model.decoder.predict_note_indices(dec_in, batch_size=k)

    def split():
        notes = model.decoder.predict_note_indices(dec_in, batch_size=k)
        return notes, de.signature_vectors(notes, s, device=False), de.harmonicity(notes, s, device=False)

    for fn in (fused, decode_only, split, fused, decode_only):
        fn()
    times = {"fused": [], "decode": [], "split": []}
    for _ in range(args.repeats):
        for name, fn in (("fused", fused), ("decode", decode_only), ("split", split)):
            t0 = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t0))
    print("%d-window sweep: predict_descriptors                      %s" % (k, stat(times["fused"])))
    print("%d-window sweep: predict_note_indices alone               %s" % (k, stat(times["decode"])))
    print("%d-window sweep: predict_note_indices + the two mirrors   %s" % (k, stat(times["split"])))


if __name__ == "__main__":
    main()
