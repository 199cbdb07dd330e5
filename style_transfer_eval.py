#!/usr/bin/env python3
"""Style transfer by latent swap, scored by the three style judges and their ensemble - the reference's evaluation script
(vae_evaluation.py) from the encode (:2180-2181) to the switched songs (:2448-2625), with every stage on the MI355X engine:

  original      the songs' own windows through the pitch, velocity and instrument classifiers, the instruments once per song
                (:2075-2172; midi_vae_amd.style.score_originals);
  autoencoded   encode, decode every song with its own history, velocity rules carried through the song (:2248-2340;
                decoder.predict_songs(judges=...));
  switched      for every song and every other class the style coordinates of z trade places; all (song, target) pairs decode as ONE
                pass, velocities window by window, signatures, harmonicity, the instrument vote (:2448-2625; decoder.switch_styles).

Per block the accuracy and confidence of each judge against the song's OWN class, as the reference prints them; the rolls, the
probabilities and the scores (mvae_style_scores) stay on the device between the decode and the table.  With ``--out-dir`` every
switched song is written as ``<song>_fullswitch_[SI_]<C>to<C'>.mid`` (:2625).

Synthetic songs, or ``--midi-dir``: the MIDI files of a folder with class-named subfolders.  The VAE and the three classifiers are
trained here for a few epochs first, so the printed numbers only show the pipeline working - not the paper's results.

    python style_transfer_eval.py [--epochs 3] [--songs 8] [--sample-method argmax|choice] [--midi-dir DIR] [--out-dir DIR]
"""
import argparse
import os
import time

import numpy as np

import settings
import vae_definition
import data_class
from midi_vae_amd import descriptors, midifile, style
from midi_vae_amd import sweep as sweep_mod
from midi_vae_amd.classifier import StyleClassifier
from midi_vae_amd.config import create_kwargs
from style_classifier_training import sample, songs_from_midi_dir, synthetic_songs
from vae_definition import VAE

BPM = 100          # (vae_evaluation.py:128)
KINDS = ("pitch", "velocity", "instrument")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--sample-method", choices=("argmax", "choice"), default="argmax",
                    help="'choice': the reference's default decode (settings.temperature, :1048-1067), drawn on the device")
    ap.add_argument("--midi-dir", default=None, help="read the songs from this folder (one subfolder per class) instead of making them")
    ap.add_argument("--out-dir", default=None, help="write <song>_fullswitch_[SI_]<C>to<C'>.mid per switched song into this folder")
    args = ap.parse_args()
    s = vars(settings)
    nc, bs, V = s["num_classes"], s["batch_size"], s["max_voices"]
    if args.midi_dir is not None:
        train, test = songs_from_midi_dir(args.midi_dir, s)
        songs = train + test
    else:
        songs = synthetic_songs(args.songs, s, 5, "pitch")
    for sg in songs:
        n = sg["X"].shape[0]
        sg.setdefault("Y", sg["X"])
        sg.setdefault("D", np.zeros(np.asarray(sg["V"]).shape))
        sg.setdefault("S", np.zeros((n, s["signature_vector_length"])))
    model = VAE().create(**create_kwargs(s))
    model.decoder.sample_settings = s
    dims = dict(pitch=s["input_dim"], velocity=1, instrument=s["meta_instrument_dim"])
    clfs = {k: StyleClassifier(k, input_dim=dims[k], num_classes=nc, learning_rate=2e-4) for k in KINDS}
    for e in range(args.epochs):
        hs = []
        for sg in songs:
            H = np.zeros((sg["X"].shape[0], s["latent_dim"]))
            x, y, w = vae_definition.prepare_autoencoder_input_and_output_list(sg["X"], sg["Y"], sg["C"], sg["I"], sg["V"], sg["D"],
                                                                               sg["S"], H, return_sample_weight=True)
            hs.append(model.autoencoder.fit(x, y, epochs=1, batch_size=bs, shuffle=False, sample_weight=w, verbose=False))
            for k in KINDS:
                clfs[k].fit(*sample(sg, k, nc), epochs=1, batch_size=bs, shuffle=False)
        print("epoch %d: VAE loss %.4f" % (e, np.mean([h.history["loss"][0] for h in hs])))
    judges = style.Judges(clfs["pitch"], clfs["velocity"], clfs["instrument"])
    # the training signatures of every class: what a switched decode is measured against (vae_evaluation.py:1542-1628, :2836-2862)
    class_stats = {}
    for c in sorted({sg["C"] for sg in songs}):
        sigs = np.concatenate([descriptors.signature_vectors(sg["X"], s) for sg in songs if sg["C"] == c], 0)
        class_stats[c] = data_class.get_mean_and_cov_from_vector_list(sigs)

    t0 = time.time()
    classes = [sg["C"] for sg in songs]
    onehot_index = lambda a: np.argmax(np.asarray(a), axis=-1).astype(np.uint8)
    instr_idx = [onehot_index(sg["I"]).reshape(-1)[:V] for sg in songs]
    programs = [[int(p) for p in sweep_mod.programs_of(i, s["instrument_attach_method"])] for i in instr_idx]
    original = style.score_originals([onehot_index(sg["X"]) for sg in songs], [np.asarray(sg["V"]).reshape(sg["X"].shape[0], -1) for sg in songs],
                                     instr_idx, classes, judges, batch_size=bs)
    zs = [model.encoder.predict(vae_definition.prepare_encoder_input_list(sg["X"], sg["I"], sg["V"], sg["D"]), batch_size=bs)
          for sg in songs]                                                                                       # :2180-2181
    dec_in = [vae_definition.prepare_decoder_input(z, sg["C"], sg["S"], None) for z, sg in zip(zs, songs)]
    kw = dict(seed=0) if args.sample_method == "choice" else {}
    autoencoded = model.decoder.predict_songs(dec_in, batch_size=bs, sample_method=args.sample_method, judges=judges, classes=classes, **kw)
    switched = model.decoder.switch_styles(zs, classes, S=[sg["S"] for sg in songs], judges=judges, note_events=args.out_dir is not None,
                                           batch_size=bs, programs=programs, sample_method=args.sample_method, **kw)
    dt = time.time() - t0

    def mean_of(styles, judge, what):
        values = [d[judge][what] for d in styles if d["windows"]]
        return float(np.mean(values)) if values else float("nan")

    blocks = (("original", [d["style"] for d in original]), ("autoencoded", [d["style"] for d in autoencoded]),
              ("switched", [d["style"] for d in switched["pairs"]]), ("switched, vs target", [d["style_target"] for d in switched["pairs"]]))
    print("%-20s " % "mean over songs" + " ".join("%21s" % j for j in style.JUDGES))
    print("%-20s " % "" + " ".join("%10s %10s" % ("accuracy", "confidence") for _ in style.JUDGES))
    for name, styles in blocks:
        print("%-20s " % name + " ".join("%10.4f %10.4f" % (mean_of(styles, j, "accuracy"), mean_of(styles, j, "confidence"))
                                         for j in style.JUDGES))
    pairs = switched["pairs"]
    n_win = sum(z.shape[0] for z in zs)
    print("%d windows of %d songs, %d switched songs (%d with other instruments): three blocks in %.2f s"
          % (n_win, len(songs), len(pairs), sum(d["instruments_switched"] for d in pairs), dt))
    with np.printoptions(precision=3, suppress=True):
        harm = np.concatenate([d["harmonicity"] for d in pairs], 0)
        print("mean harmonicity between the voices of the switched decodes (NaN: the two voices never sound in the same segment):\n%s"
              % descriptors.nanmean_windows(harm))
    distances = [data_class.mahalanobis_distance(v, *class_stats[d["C_switch"]]) for d in pairs if d["C_switch"] in class_stats
                 for v in d["signature"]]
    if distances:
        print("mean Mahalanobis distance of the switched decodes' signatures to the target style's training signatures: %.3f"
              % float(np.mean(distances)))
    if args.out_dir is not None:
        os.makedirs(args.out_dir, exist_ok=True)
        for d in pairs:
            tracks = [d["events"][d["events"]["voice"] == v] for v in range(V)]
            name = "song%d_fullswitch_%s%dto%d.mid" % (d["song"], "SI_" if d["instruments_switched"] else "", d["C"], d["C_switch"])
            midifile.write_midi(os.path.join(args.out_dir, name), tracks, d["programs"], BPM, s["SMALLEST_NOTE"])
        print("wrote %d files to %s" % (len(pairs), args.out_dir))


if __name__ == "__main__":
    main()
