#!/usr/bin/env python3
"""Style transfer by latent swap, scored by a style classifier - the inference pipeline of the reference's evaluation script
(vae_evaluation.py:2180-2181 encode, :2471-2478 swap the style dimensions of z, :2481-2483 decode window by window + argmax,
:78-91 / :2585-2625 classify the result) with every stage on the MI355X engine and batched: the windows of a song are independent
given (z', history), so the decoder runs them as ONE batch (BASELINE configs[4]) and nothing but one byte per row leaves the chip.

Synthetic songs (the reference reads MIDI folders); the VAE and the pitch classifier are trained here for a few epochs first, so
the printed numbers only show the pipeline working - not the paper's results.

    python style_transfer_eval.py [--epochs 3] [--songs 8] [--sample-method argmax|choice]
"""
import argparse
import time

import numpy as np

import settings
import vae_definition
import data_class
from midi_vae_amd import descriptors
from midi_vae_amd.classifier import StyleClassifier
from midi_vae_amd.config import create_kwargs
from style_classifier_training import synthetic_songs
from vae_definition import VAE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--sample-method", choices=("argmax", "choice"), default="argmax",
                    help="'choice': the reference's default decode (settings.temperature, :1048-1067), drawn on the device")
    args = ap.parse_args()
    s = vars(settings)
    nc, bs = s["num_classes"], s["batch_size"]
    songs = synthetic_songs(args.songs, s, 5, "pitch")
    for sg in songs:
        n = sg["X"].shape[0]
        sg.update(Y=sg["X"], D=np.zeros(sg["V"].shape), S=np.zeros((n, s["signature_vector_length"])))
    model = VAE().create(**create_kwargs(s))
    model.decoder.sample_settings = s
    clf = StyleClassifier("pitch", input_dim=s["input_dim"], num_classes=nc, learning_rate=2e-4)
    for e in range(args.epochs):
        hs = []
        for sg in songs:
            H = np.zeros((sg["X"].shape[0], s["latent_dim"]))
            x, y, w = vae_definition.prepare_autoencoder_input_and_output_list(sg["X"], sg["Y"], sg["C"], sg["I"], sg["V"], sg["D"],
                                                                               sg["S"], H, return_sample_weight=True)
            hs.append(model.autoencoder.fit(x, y, epochs=1, batch_size=bs, shuffle=False, sample_weight=w, verbose=False))
            clf.fit(sg["X"], np.tile(np.eye(nc)[sg["C"]][None], (sg["X"].shape[0], 1)), epochs=1, batch_size=bs, shuffle=False)
        print("epoch %d: VAE loss %.4f" % (e, np.mean([h.history["loss"][0] for h in hs])))
    # the training signatures of every class: what a switched decode is measured against (vae_evaluation.py:1542-1628, :2836-2862)
    class_stats = {}
    for c in sorted({sg["C"] for sg in songs}):
        sigs = np.concatenate([descriptors.signature_vectors(sg["X"], s) for sg in songs if sg["C"] == c], 0)
        class_stats[c] = data_class.get_mean_and_cov_from_vector_list(sigs)
    t0 = time.time()
    n_win = kept = switched = 0
    harm, distances = {"kept": [], "switched": []}, []
    for sg in songs:
        X, I, V, D, C = sg["X"], sg["I"], sg["V"], sg["D"], sg["C"]
        n = X.shape[0]
        z = model.encoder.predict(vae_definition.prepare_encoder_input_list(X, I, V, D), batch_size=bs)      # :2180-2181
        target = (C + 1) % nc
        z2 = z.copy()
        z2[:, C], z2[:, target] = z[:, target], z[:, C]                                                     # :2471-2478
        for name, zz in (("kept", z), ("switched", z2)):
            dec_in = vae_definition.prepare_decoder_input(zz, C, sg["S"], None)    # history = previous window's (switched) z, :2481
            dec = model.decoder.predict_descriptors(dec_in, batch_size=max(bs, n), sample_method=args.sample_method)    # :2482-2483, fused
            idx = dec["notes"]
            harm[name].append(dec["harmonicity"])                                                       # :2314-2317, :2537-2543
            if name == "switched" and target in class_stats:
                distances += [data_class.mahalanobis_distance(v, *class_stats[target]) for v in dec["signature"]]
            pred = np.argmax(clf.predict(idx, batch_size=bs), axis=1)
            if name == "kept":
                kept += int(np.sum(pred == C))
            else:
                switched += int(np.sum(pred == target))
        n_win += n
    dt = time.time() - t0
    print("%d windows: classified as their own style after autoencoding %.1f %%, as the TARGET style after the latent swap %.1f %% "
          "(encode + 2 x decode with descriptors + 2 x classify: %.0f windows/s)" % (n_win, 100.0 * kept / n_win, 100.0 * switched / n_win, n_win / dt))
    with np.printoptions(precision=3, suppress=True):
        for name in ("kept", "switched"):
            print("mean harmonicity between the voices, %s decodes (NaN: the two voices never sound in the same segment):\n%s"
                  % (name, descriptors.nanmean_windows(np.concatenate(harm[name], 0))))
    if distances:
        print("mean Mahalanobis distance of the switched decodes' signatures to the target style's training signatures: %.3f"
              % float(np.mean(distances)))


if __name__ == "__main__":
    main()
