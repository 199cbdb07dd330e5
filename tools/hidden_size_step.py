#!/usr/bin/env python3
"""Train step ms at the reference's shipped shape (T=64, Z=256, B=256, bf16), GRU and LSTM cells, lstm_size 256 and 512.
   python tools/hidden_size_step.py"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa
from midi_vae_amd.engine import Engine
from midi_vae_amd.layout import ModelSpec
from midi_vae_amd.synth import make_windows

B, T, Z = 256, 64, 256
for cell in ("GRU", "LSTM"):
    for H in (256, 512):
        spec = ModelSpec(cell=cell, H=H, Z=Z, Din=61, Dout=61, T=T, V=4, ID=16, C=2, Le=2, Ld=2)
        w = make_windows(B, T, 61, 4, 16, 2, Z, seed=1, epsilon_std=spec.epsilon_std)
        eng = Engine(spec, max_batch=B, dtype="bf16", device="cuda:0", seed=1)
        eng.stage_encoder_inputs(w["x_idx"], w["i_idx"], w["vel"], w["eps"])
        eng.stage_decoder_inputs(B, hist=w["hist"])
        eng.stage_targets(B, w["x_idx"], w["c_idx"])
        for _ in range(3):
            eng.train_step(B)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            for _ in range(10):
                eng.train_step(B)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 100)
        print("train step %s H=%d T=%d Z=%d B=%d bf16: %.3f ms (best of 3 x 10 steps); loss %.4f" % (
            cell, H, T, Z, B, best, eng.metrics(B)["loss"]), flush=True)
        del eng
        torch.cuda.empty_cache()
