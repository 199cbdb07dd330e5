#!/usr/bin/env python3
"""Latent sweep: which latent dimension moves which musical statistic - the reference's latent_sweep_over_all_dimensions
(vae_evaluation.py:1123-1213) without its plots.  For every sample z and every latent dimension the decoder runs the windows in which
that one coordinate takes 2 * k - 1 values around 0; pitch, velocity, note-start and instrument statistics of those windows are
taken on the device behind the decode (decoder.latent_sweep), and every statistic is printed with the dimension of largest summed
influence ("overall best"), the dimension whose single summary peaked ("most peaked") and the influence per dimension.

    python latent_sweep_eval.py [--weights model.npz] [--seed 0] [--samples 4] [--z drawn|encoded] [--evaluations 5]
                                [--range-end 1.0] [--sigma 1.0] [--one-sided] [--sample-method argmax|choice] [--top 8]

Without --weights the model is a seeded random one, so the printed numbers only show the pipeline working.  --z encoded takes z
from the encoder on synthetic windows (the reference reads MIDI folders); --z drawn samples it from N(0, 1).
"""
import argparse

import numpy as np

import settings
import vae_definition
from midi_vae_amd.config import create_kwargs
from vae_definition import VAE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None, help=".npz weights written by save_weights; default: a seeded random model")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--z", choices=("drawn", "encoded"), default="drawn")
    ap.add_argument("--evaluations", type=int, default=5, help="values per side and dimension (k): 2 * k - 1 windows")
    ap.add_argument("--range-end", type=float, default=1.0, help="range_end_in_stds")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--one-sided", action="store_true")
    ap.add_argument("--sample-method", choices=("argmax", "choice"), default="argmax")
    ap.add_argument("--top", type=int, default=8, help="dimensions listed per statistic, by influence")
    args = ap.parse_args()
    s = vars(settings)
    model = VAE().create(seed=args.seed, **create_kwargs(s))
    if args.weights:
        model.autoencoder.load_weights(args.weights)
    model.decoder.sample_settings = s
    if args.z == "encoded":
        from vae_training import synthetic_songs
        sg = synthetic_songs(1, dict(s, batch_size=max(4 * args.samples, 8)), args.seed)[0]
        z = model.encoder.predict(vae_definition.prepare_encoder_input_list(sg["X"], sg["I"], sg["V"], sg["D"]),
                                  batch_size=s["batch_size"])[:args.samples]
    else:
        z = np.random.default_rng(args.seed).standard_normal((args.samples, s["latent_dim"]))
    kw = dict(seed=args.seed) if args.sample_method == "choice" else {}
    res = model.decoder.latent_sweep(z, range_end_in_stds=args.range_end, sigma=args.sigma, evaluations_per_dimension=args.evaluations,
                                     positive_and_negative=not args.one_sided, sample_method=args.sample_method, **kw)
    n, Z, K = res["table"].shape[:3]
    print("%d samples x %d dimensions x %d values (%s) = %d windows" % (n, Z, K, ", ".join("%.3f" % v for v in res["values"]), n * Z * K))
    for key in sorted(res["influence"]):
        infl = res["influence"][key]
        order = np.argsort(-np.nan_to_num(infl, nan=-np.inf), kind="stable")[:args.top]
        print("%-44s overall best dim %3d, most peaked dim %3d | %s" % (
            key, res["overall_best"][key], res["most_peaked"][key], "  ".join("%d: %.4g" % (d, infl[d]) for d in order)))


if __name__ == "__main__":
    main()
