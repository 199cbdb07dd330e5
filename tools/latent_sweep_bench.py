#!/usr/bin/env python3
"""Time the latent sweep on the MI355X (profiles/r16_latent_sweep.txt holds the figures).

    python tools/latent_sweep_bench.py [--samples 4] [--evaluations 5] [--windows 65536] [--repeats 5] [--host-repeats 1]

The default model (GRU, T = 64, Z = 256, H = 256, bf16), --samples latent vectors, K = 2 * --evaluations - 1 values: 9 216 windows.
(a) decoder.predict_indices alone and (b) decoder.latent_sweep on the same decoder inputs, alternating, host clock around calls that
    end in a host read;
(c) the statistics kernel alone on --windows random-walk windows with resident rolls, window-major and time-major, device events;
(d) the host route to the result of (b) without the kernel: predict_indices, packers.process_decoder_indices window by window (the
    velocity rules), the NumPy mirror of the statistics and the host summaries - once per --host-repeats, it takes seconds.
Every timed shape is warmed up first; medians over --repeats, with the range."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa: E402,F401
from midi_vae_amd import packers as pk  # noqa: E402
from midi_vae_amd import rolls  # noqa: E402
from midi_vae_amd import sweep as sw  # noqa: E402
from midi_vae_amd.config import build_settings, create_kwargs  # noqa: E402


def walks(rng, n, T, V, n_pitch, p_silent, p_hold):
    ticks = T // V
    rest, hold = rng.random((n, ticks, V)) < p_silent, rng.random((n, ticks, V)) < p_hold
    step = np.where(hold, 0, rng.integers(-4, 5, (n, ticks, V)))
    step[rest] = 0
    q = np.clip(rng.integers(0, n_pitch, (n, 1, V)) + np.cumsum(step, 1), 0, n_pitch - 1)
    return np.where(rest, n_pitch, q).astype(np.uint8).reshape(n, T)


def stat(ms):
    return "%10.3f ms (range %.3f .. %.3f, %d runs)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def host_route(dec, dec_in, s, shape):
    """what the project offered before the kernel: every roll to the host, the rules window by window, statistics in NumPy"""
    n, Z, K = shape
    ind = dec.predict_indices(dec_in, 32)
    T = ind["notes"].shape[1]
    vel = np.empty(ind["notes"].shape, np.float32)
    for w in range(ind["notes"].shape[0]):          # one window per call: the rules' state does not cross a window in a sweep
        one = {k: v[w:w + 1] for k, v in ind.items()}
        vel[w] = pk.process_decoder_indices(s, one)[2]
    p = sw.params(s)
    table = np.full((vel.shape[0], sw.N_COLUMNS), np.nan)
    on = rolls.sounding(ind["notes"], p)
    for w in range(vel.shape[0]):                   # the mirror's statistics on the post-rule velocities
        xs, os_, out = ind["notes"][w].tolist(), on[w].tolist(), vel[w].astype(np.float64).tolist()
        pitches = []
        for k in range(0, T, p["voices"]):
            pitches.extend(sorted({x for x, o in zip(xs[k:k + p["voices"]], os_[k:k + p["voices"]]) if o}))
        starts = [t for t in range(T) if out[t] > p["threshold"]]
        table[w] = ([float(len(pitches))] + sw._integer_stats(pitches) + [float(pitches.count(35)), float(pitches.count(39)),
                    float(len(starts))] + sw._velocity_stats([out[t] for t in starts]) + sw._integer_stats(starts))
    programs = sw.programs_of(ind["instr"], s["instrument_attach_method"])
    return (table.reshape(n, Z, K, -1),) + sw.summarize_sweep(table.reshape(n, Z, K, -1), programs.reshape(n, Z, K, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--evaluations", type=int, default=5)
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("latent_sweep_bench.py measures the MI355X: no device is visible")
    from midi_vae_amd.model import VAE
    s = build_settings()
    m = VAE().create(compute_dtype="bf16", seed=16, **create_kwargs(s))
    dec = m.decoder
    dec.sample_settings = s
    sp = m.spec
    print("model: %s, T = %d, Z = %d, H = %d, %d voices, bf16" % (sp.cell, sp.T, sp.Z, sp.H, sp.V))
    z = np.random.default_rng(16).standard_normal((args.samples, sp.Z))
    values = sw.sweep_values(1.0, 1.0, args.evaluations, True)
    dec_in = dec.sweep_inputs(z, values, s)
    shape = (args.samples, sp.Z, len(values))
    print("%d samples x %d dimensions x %d values = %d windows" % (shape + (int(np.prod(shape)),)))

    def run_a():
        return dec.predict_indices(dec_in, 32)

    def run_b():
        return dec.latent_sweep(z, evaluations_per_dimension=args.evaluations)

    for _ in range(3):
        run_a(), run_b()
    ta, tb = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        run_a()
        t1 = time.perf_counter()
        res = run_b()
        t2 = time.perf_counter()
        ta.append(1e3 * (t1 - t0))
        tb.append(1e3 * (t2 - t1))
    print("(a) predict_indices alone                 " + stat(ta))
    print("(b) latent_sweep                          " + stat(tb))
    t0 = time.perf_counter()
    sw.summarize_sweep(res["table"], res["programs"])
    print("    of which the host summaries           %10.3f ms" % (1e3 * (time.perf_counter() - t0)))

    # (c) the kernel alone
    p = sw.params(s)
    rng = np.random.default_rng(17)
    T, V, n = sp.T, p["voices"], args.windows
    idx = np.concatenate([walks(rng, n // 4, T, V, p["n_pitch"], ps, ph) for ps, ph in ((0.35, 0.0), (0.3, 0.6), (0.2, 0.8), (0.9, 0.5))], 0)
    n = idx.shape[0]
    vel = rng.random((n, T)).astype(np.float32)
    stats = torch.empty((n, sw.N_COLUMNS), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    layouts = {"window-major (staged)": (torch.from_numpy(idx).cuda(), torch.from_numpy(vel).cuda()),
               "time-major (direct)  ": (torch.from_numpy(np.ascontiguousarray(idx.T)).cuda().t(), torch.from_numpy(np.ascontiguousarray(vel.T)).cuda().t())}
    for name, (ti, tv) in layouts.items():
        ms = []
        for r in range(args.repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sw.enqueue(ti, tv, p, stats, None, stream)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        print("(c) kernel alone, %d windows, %s " % (n, name) + stat(ms))

    # (d) the host route
    td = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        host = host_route(dec, dec_in, s, shape)
        td.append(1e3 * (time.perf_counter() - t0))
    print("(d) host route to the same result         " + stat(td))
    exact = [c for c in range(22) if c not in (6, 15, 21)]
    same = np.array_equal(host[0][..., exact], res["table"][..., exact], equal_nan=True)
    print("    tables agree outside the std columns: %s; largest std difference %.3g; most_peaked equal: %s" % (
        same, np.nanmax(np.abs(host[0][..., [6, 15, 21]] - res["table"][..., [6, 15, 21]])), host[3] == res["most_peaked"]))


if __name__ == "__main__":
    main()
