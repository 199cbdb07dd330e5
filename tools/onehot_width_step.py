#!/usr/bin/env python3
"""Train step ms at BASELINE configs[1]'s shape (T=512, 256 windows, Z=64, H=256, bf16), GRU and LSTM cells, against the width of
the one-hot rows: input_dim = output_dim = 61 (the default crop), 129 (the full MIDI range + silent), 145 (+ 16 instrument
categories) and 192 (the ceiling).  Every figure is the median of --reps timings of 10 steps, the spread (min .. max) beside it.
   python tools/onehot_width_step.py [--widths 61,129,145,192] [--cells GRU,LSTM] [--reps 5]
An A/B of two trees is this script run from each in turn, several times (--widths 61): one line per run, medians by the caller."""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa
from midi_vae_amd.engine import Engine
from midi_vae_amd.layout import ModelSpec
from midi_vae_amd.synth import make_windows

ap = argparse.ArgumentParser()
ap.add_argument("--widths", default="61,129,145,192")
ap.add_argument("--cells", default="GRU,LSTM")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tag", default="")
a = ap.parse_args()
B, T, Z = 256, 512, 64
for cell in a.cells.split(","):
    for D in map(int, a.widths.split(",")):
        spec = ModelSpec(cell=cell, H=256, Z=Z, Din=D, Dout=D, T=T, V=4, ID=16, C=2, Le=2, Ld=2)
        w = make_windows(B, T, D, 4, 16, 2, Z, seed=1, epsilon_std=spec.epsilon_std)
        eng = Engine(spec, max_batch=B, dtype="bf16", device="cuda:0", seed=1)
        eng.stage_encoder_inputs(w["x_idx"], w["i_idx"], w["vel"], w["eps"])
        eng.stage_decoder_inputs(B, hist=w["hist"])
        eng.stage_targets(B, w["x_idx"], w["c_idx"])
        for _ in range(3):
            eng.train_step(B)
        torch.cuda.synchronize()
        ms = []
        for rep in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(10):
                eng.train_step(B)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 100)
        eng.check_pipeline()
        print("%strain step %s Din=Dout=%d (head NP %d) T=%d B=%d H=256 bf16: %.3f ms (median of %d x 10 steps, %.3f .. %.3f); loss %.4f" % (
            a.tag and a.tag + " ", cell, D, eng.head["notes"].NP, T, B, statistics.median(ms), a.reps, min(ms), max(ms),
            eng.metrics(B)["loss"]), flush=True)
        del eng
        torch.cuda.empty_cache()
