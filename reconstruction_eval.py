#!/usr/bin/env python3
"""Reconstruction report - the central block of the reference's evaluation script (vae_evaluation.py:2180-2244 and :2380-2415):
encode a song, decode it again with every window's history, apply the velocity rules over the WHOLE song, derive the note starts and
count how many of the original notes came back.  Every stage runs on the MI355X engine and all songs go through the decoder as one
pass: decoder.predict_songs finishes the decode on the device (midi_vae_amd.reconstruction, mvae_recon_songs) and only the rolls and
eight integers per window come back.  With --midi-dir the notes of every decoded song are extracted on the device as well
(midi_vae_amd.events, mvae_note_events) and written as ``<song>_autoencoded.mid`` (midi_vae_amd.midifile), the reference's
rolls_to_midi call at vae_evaluation.py:2204.

Synthetic songs (the reference reads MIDI folders); the VAE is trained here for a few epochs first, so the printed numbers only show
the pipeline working - not the paper's results.

    python reconstruction_eval.py [--epochs 3] [--songs 8] [--sample-method argmax|choice] [--seed 0] [--midi-dir DIR]
"""
import argparse
import os
import time

import numpy as np

import settings
import vae_definition
from midi_vae_amd import midifile, reconstruction
from midi_vae_amd.config import create_kwargs
from vae_definition import VAE
from vae_training import synthetic_songs

BPM = 100          # (vae_evaluation.py:128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--sample-method", choices=("argmax", "choice"), default="argmax",
                    help="'choice': the reference's default decode (settings.temperature, :1048-1067), drawn on the device")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--midi-dir", default=None, help="write <song>_autoencoded.mid per song into this folder")
    args = ap.parse_args()
    s = vars(settings)
    bs = s["batch_size"]
    songs = synthetic_songs(args.songs, s, 5 + args.seed)
    model = VAE().create(seed=args.seed, **create_kwargs(s))
    model.decoder.sample_settings = s
    for e in range(args.epochs):
        hs = []
        for sg in songs:
            H = np.zeros((sg["X"].shape[0], s["latent_dim"]))
            x, y, w = vae_definition.prepare_autoencoder_input_and_output_list(sg["X"], sg["Y"], sg["C"], sg["I"], sg["V"], sg["D"],
                                                                               sg["S"], H, return_sample_weight=True)
            hs.append(model.autoencoder.fit(x, y, epochs=1, batch_size=bs, shuffle=False, sample_weight=w, verbose=False))
        print("epoch %d: VAE loss %.4f" % (e, np.mean([h.history["loss"][0] for h in hs])))
    t0 = time.time()
    dec_in = []
    for sg in songs:
        z = model.encoder.predict(vae_definition.prepare_encoder_input_list(sg["X"], sg["I"], sg["V"], sg["D"]), batch_size=bs)   # :2180-2181
        dec_in.append(vae_definition.prepare_decoder_input(z, sg["C"], sg["S"], None))      # history = the previous window's z
    kw = dict(seed=args.seed) if args.sample_method == "choice" else {}
    res = model.decoder.predict_songs(dec_in, batch_size=bs, sample_method=args.sample_method, originals=[sg["Y"] for sg in songs],
                                      note_events=args.midi_dir is not None, **kw)
    dt = time.time() - t0
    if args.midi_dir is not None:
        os.makedirs(args.midi_dir, exist_ok=True)
        for i, d in enumerate(res):
            tracks = [d["events"][d["events"]["voice"] == v] for v in range(s["max_voices"])]
            path = os.path.join(args.midi_dir, "song%d_autoencoded.mid" % i)
            midifile.write_midi(path, tracks, d.get("programs", [0] * s["max_voices"]), BPM, s["SMALLEST_NOTE"])
        print("wrote %d files to %s (%d notes)" % (len(res), args.midi_dir, sum(len(d["events"]) for d in res)))
    short = ("original", "predicted", "accuracy", "not pred.", "new", "start/orig", "start/pred")
    print("%-8s %7s " % ("song", "windows") + " ".join("%10s" % k for k in short))
    rows = [dict(d["metrics"], song_name="song %d" % i) for i, d in enumerate(res)]
    for name, windows, d in [(r["song_name"], len(x["notes"]), r) for r, x in zip(rows, res)] + \
            [("Mean", sum(len(x["notes"]) for x in res) / len(res), reconstruction.mean_metrics(rows))]:
        print("%-8s %7.4g " % (name, windows) + " ".join(("%10d" if isinstance(d[k], int) else "%10.4f") % d[k] for k in reconstruction.METRICS))
    n_win = sum(len(x["notes"]) for x in res)
    print("%d windows of %d songs: encode + one decode pass + song-level rules and counts on the device: %.0f windows/s"
          % (n_win, len(res), n_win / dt))


if __name__ == "__main__":
    main()
