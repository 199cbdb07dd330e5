"""The engine's schedule knobs: name -> default value, in one place.

``Engine.__init__`` applies the dict with setattr and keeps it; the names of that same dict are what ``engine_plan._plan_state``
iterates, so a knob cannot exist without keying the step plans (a live change of one then selects other plans instead of
replaying the launch list recorded under the old value).  A caller - a test, an A/B script under tools/ - changes a
knob by plain assignment on the live engine.  No torch, no GPU: the defaults that depend on the model or the batch are computed
here from the spec and the padded batch."""
from __future__ import annotations

import os


def schedule_knobs(spec, max_batch_padded, env=os.environ):
    """``spec``: ModelSpec / ClassifierSpec (cell, T, GH are read); ``max_batch_padded``: Engine.maxB; ``env``: where the
    MVAE_* overrides are looked up"""
    k = {}
    k["use_plans"] = env.get("MVAE_PLANS", "1") == "1"       # step plans (engine_plan.py): record three calls of a kind, then replay
    # Stacked layers are pipelined over TIME CHUNKS: layer l runs chunk k (on its own stream) as soon as layer l-1
    # has produced it, instead of waiting for the whole sequence.  The f32 state is carried across launches.
    k["time_chunks"] = 4
    # ... and where the slot-interleaved LSTM / GRU kernels apply AND the stack's kernels fit on the chip together
    # (_pipelined), as ONE launch per layer with device-side hand-over every pipe_chunk time steps (no relaunch, no weight
    # reload, layers pipe_chunk steps apart instead of T/4).
    # time steps per hand-over: a hand-over costs every workgroup a drained vmcnt and a counter, the persistent GEMM a wait - the
    # bigger the batch, the more rows a chunk should carry (A/B r02: 256 windows 8 / 16 / 32 / 64 -> 8.18 / 8.08 / 8.13 / 8.31 ms;
    # 512 windows, T=2048: 35.7 / 34.5 / 35.4 at 16 / 32 / 64; decode of 1024 windows: 57.0 / 58.9 / 60.1 / 59.9 k at 16 / 32 / 64 / 128)
    pipe_chunk = 16 if max_batch_padded <= 256 else 32 if max_batch_padded <= 512 else 64
    while pipe_chunk > 16 and spec.T % pipe_chunk:
        pipe_chunk //= 2
    k["pipe_chunk"] = pipe_chunk
    # the HOST is held at these points of a train step until the device has reached them (_pace: bit 2 in front of the backward
    # pass, 4 in front of the encoder BPTT; 1 in front of the decoder forward): a device whose queues already hold the packets of
    # the later phases - value waits on a dozen queues - runs the current phase slower.  T = 64: 1.71 -> 1.45 ms per step with
    # 6, configs[1] 6.65 -> 6.57 (profiles/r05_c_steps_in_flight.txt); a replayed step is split into call ranges there
    k["pace_mask"] = 6
    # ... of a step enqueued in TWO calls (train_step_begin / train_step_finish: model.Autoencoder.fit, whose host converts the
    # next minibatch - or the caller's next song - between two steps): only the pause in front of the backward pass.  A host that
    # is held until the encoder BPTT starts comes back too late for that work: `python vae_training.py` at default settings
    # 58 k -> 71 k windows/s end to end (no pause at all: 75 k, but configs[1] GRU fit 5.8 -> 7.6 ms per step); fit at configs[1]
    # LSTM 7.9-8.1 -> 7.2-7.7 ms per 256-window step, GRU 5.64 -> 5.80 (profiles/r05_t_pace_mask_by_caller.txt)
    k["pace_mask_split"] = 2
    k["_pace_mask_now"] = k["pace_mask"]       # (state derived from the two: the mask of the running call, set by train_step / train_step_finish)
    k["pipe_gemm_blocks"] = 64       # persistent grid of the dX GEMM between two pipelined layers (backward)
    # ... and of the forward projection x*W + b: the weights-stationary kernel (csrc/gemm.hip proj_ws_k) wants a multiple of
    # 8 XCDs x (G*H / 128) column tiles - one workgroup per (XCD, column tile) keeps its weight panel in LDS for the whole launch:
    # 64 for LSTM, 48 for GRU.  (Round 1's kernel reloaded the panel per tile; decoder inference at 1024 windows was bound by it:
    # 8.2 us per decoder step at 64 workgroups, 6.2 at 128 - 4.1 now at 64)
    k["pipe_proj_blocks"] = 8 * max(spec.GH // 128, 1)
    k["fused_latent"] = True         # Dense chain around the latent as one launch each way (csrc/latent.hip)
    # Encoder stack (the LAST recurrence phase of a step): its weight-gradient GEMMs FOLLOW the running BPTT kernels chunk by chunk
    # (mvae_gemm k_wait: one resident workgroup per (output tile, K partition) accumulates in registers over all chunks) - what
    # is left when the recurrence ends is one chunk's share instead of four whole GEMMs (0.55 ms of the 0.77 ms tail).  All of
    # them are ONE launch (mvae_gemm_kstream_multi) on the second gradient queue - a queue each cost more than the tail saved -
    # and the other gradient work of that phase (velocity / instrument encoders) goes to the first one.
    # kstream_wgs workgroups per GEMM: they wait beside the recurrences, one per CU (_kstream_ok: residency).
    # SHORT sequences (the reference's shipped T = 64, settings.py:108-109): every weight-gradient GEMM is a 20-120 us launch
    # that is mostly fill and drain, a dozen of them beside and behind the recurrences were two thirds of what followed the last
    # BPTT, and their workgroups kept the recurrent launches (one workgroup per EMPTY CU) waiting for a place.  Up to
    # defer_grads_rows rows (T x padded batch) per sequence they are collected during the backward pass and leave as ONE launch
    # (mvae_gemm_multi) on the critical queue behind the last recurrence (_wgemm / _flush_deferred_gemms); above that the
    # GEMMs are long enough to be worth running beside the recurrences.  (profiles/r05_c_*; 0 = never)
    # Measured on T = 64 with the host paced (steps_in_flight / pace_mask): 256 windows GRU 2.07 -> 1.47 ms per step, LSTM
    # 1.72 -> 1.69; 64 windows GRU 1.46 -> 1.18
    k["defer_grads_rows"] = int(env.get("MVAE_DEFER_GRADS_ROWS", "32768"))
    # ... the decoder side's (and the latent block's) BESIDE the encoder BPTT launch, on the gradient queue, released by that
    # launch's first published chunk (_flush_deferred_gemms(early=...)): reference shape GRU 1.46 -> 1.39 ms, LSTM 1.705 -> 1.70;
    # from defer_early_rows rows per sequence (192 windows x 64 steps: 1.525 -> 1.46; 128 windows 1.324 -> 1.327; 64: 1.17 -> 1.18)
    k["defer_early"], k["defer_early_rows"] = True, 12288
    # ... with K split further until a launch has about this many workgroups (_flush_deferred_gemms): at T*B = 16384 rows the
    # usual split (2) makes ~150 workgroups of 128 k tiles each.  0 / 256 / 384 / 512 / 1024: GRU 1.405 / 1.39 / 1.40 / 1.338 / 1.383
    # ms per step at the reference's shape, LSTM 1.70-1.71 throughout
    k["defer_split_wgs"] = 512
    k["kstream_grads"] = env.get("MVAE_KSTREAM_GRADS", "1") == "1"
    # (GRU: 3 GEMMs per layer -> 8 problems in the encoder launch.  Round 5, 256 windows T=512: 24 workgroups each = 192 resident
    #  beside the 64 of the recurrences left the decoder side's held-back GEMMs no CU - 5.66 ms per step; 20 / 16 / 14 / 12:
    #  5.42 / 5.43 / 5.36 / 5.34-5.39 (12-15 = one workgroup per output tile: under a tracer they fall 0.26 ms behind the BPTT);
    #  <= 10: a workgroup owns two tiles and streams the second one after the BPTT: 6.13.  LSTM: 16 / 24 / 32 all 6.53, <= 12: 7.27)
    k["kstream_wgs"] = 16 if spec.cell == "GRU" else 32
    k["kstream_max_B"] = 256
    k["flush_before_join"] = True    # (engine.backward: the encoder's collected GEMMs in front of the gradient queues' joins)
    # k rows per workgroup and chunk of a K-streaming GEMM (0: the round-2 rule, kstream_wgs workgroups per GEMM whatever its tile
    # count).  Round 6, same box: GRU 4.84 -> 4.69 ms per step, LSTM 6.29 -> 6.28; 1024 rows: GRU 4.94 (profiles/r06_k_kstream_rows.txt)
    k["kstream_rows"] = 2048
    # the recurrences of a phase as ONE launch on the critical queue instead of one launch per queue (engine_phases.py) is
    # Engine.phase_multi (state: a replay restores it)
    # ... up to this many (padded) windows per call: measured (profiles/r03_j_*) 256 windows -6 % (LSTM) / -9 % (GRU) per train
    # step, but 512 windows at T=2048 +6.5 % and decoding 1024 windows +4 % - there the recurrences themselves fill the chip
    # and the per-queue launches (producers dispatched first) place them better than one launch's index order
    k["phase_max_B"] = 256
    # (_index_as_dense; measured r03_r: GRU step -0.07 ms, LSTM +0.09 ms - there the bottom layer does not set the pace)
    #  Round 4: the indexed kernels gather tile PAIRS from a paired-column table (8 x 16 bytes per row and step instead of 16 x 8:
    #  LSTM 2.66 -> 2.17, GRU 2.06 -> 1.70 us per step alone - faster than a dense input) and the written-out rows lose on both
    #  cells (GRU 5.71 vs 5.63 ms per step, LSTM 7.11 vs 6.91: profiles/r04_l_index_dense_ab.txt): off by default
    k["index_dense"] = False         # (Engine.__init__ takes the class attribute Engine.INDEX_DENSE: the buffers it needs are allocated there)
    k["index_dense_blocks"] = 16
    k["xpand_blocks"] = 16
    # (_head_forward: inference on per-queue pipelined stacks.  profiles/r03_zz_decode_head_slices.txt: decode configs[4] LSTM
    #  -3..5 % with 2 slices, -1..3 % with 4; GRU -3 % / -6..7 %: the slices take memory bandwidth from the recurrences they follow)
    k["head_slices"] = 2 if spec.cell == "LSTM" else 4
    k["_diag_no_param_grads"] = env.get("MVAE_DIAG_NO_PARAM_GRADS", "0") == "1"
    # (_grad_portions) -1: by the rows of the sequence (4 portions from 2^20 rows, none below 2^19), 0: off, N: N portions
    k["grad_portions"] = -1
    return k
