#!/usr/bin/env python3
"""Medleys and random interpolation songs - the two generation blocks of the reference's evaluation script (vae_evaluation.py:705-837
and :841-887), with every stage on the MI355X engine:

  medleys          a few songs are drawn from the set, a few consecutive windows of each are encoded, and the songs are joined by
                   bridges that walk through latent space from the last window of one song to the first window of the next;
  interpolations   two random codes drawn with the training latents' standard deviation, and the windows between them.

All medleys and all interpolation songs decode as ONE pass (decoder.decode_paths): the decoder's latent rows are written on the device
from the anchors (mvae_latent_paths), the velocity rules run over the whole song, the notes are extracted (mvae_note_events) and the
piano-roll image is drawn (mvae_pianoroll) on the same device rolls.  Per song ``<name>.mid`` (the instruments voted over the song's
windows, vae_evaluation.py:876-885), ``<name>.png`` (prepare_for_drawing's array as an 8-bit greyscale image) and, for a medley,
``<name>_info.txt``.  The reference also writes every medley through restructure_song_to_fit_more_instruments; as written there it
puts all notes on the first max_voices tracks, so the medley's file here is the voted-programs form.

Synthetic songs, or ``--midi-dir``: the MIDI files of a folder with class-named subfolders.  The VAE is trained here for a few epochs
first, so the songs only show the pipeline working - not the paper's results: after a few epochs on random synthetic songs the
argmax of most rows is the silent column and the files are nearly empty; ``--sample-method choice`` draws notes.

    python generate_songs.py [--epochs 3] [--songs 8] [--medleys 2] [--interpolations 2] [--sample-method argmax|choice]
                             [--random N] [--long N [--long-length 20]] [--midi-dir DIR] [--out-dir generated]

``--random N`` adds the reference's random songs (:1771-1814): N one-window songs from random codes (``random_<i>.mid``) and, per code,
one window per class with the class knob turned (``random_<i>_<C>.mid``).  ``--long N`` adds its long songs (:1821-1896): N songs of
``--long-length`` windows that walk from a random code through the training codes, every window decoded, fed back and encoded on the
device (decoder.long_songs); ``random_long_<i>.mid`` with the programs voted over the song's windows.
"""
import argparse
import os
import time

import numpy as np

import settings
import vae_definition
from midi_vae_amd import generation, midifile, pianoroll
from midi_vae_amd import sweep as sweep_mod
from midi_vae_amd.config import create_kwargs
from style_classifier_training import songs_from_midi_dir, synthetic_songs
from vae_definition import VAE

BPM = 100          # (vae_evaluation.py:128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--medleys", type=int, default=2, help="max_new_chosen_interpolation_songs")
    ap.add_argument("--interpolations", type=int, default=2, help="max_new_sampled_interpolation_songs")
    ap.add_argument("--songs-per-medley", type=int, default=3, help="how_many_songs_in_one_medley")
    ap.add_argument("--own-windows", type=int, default=8, help="noninterpolated_samples_between_interpolation")
    ap.add_argument("--bridge", type=int, default=4, help="interpolation_length")
    ap.add_argument("--length", type=int, default=10, help="interpolation_song_length")
    ap.add_argument("--mode", choices=("lerp", "slerp"), default="lerp")
    ap.add_argument("--sample-method", choices=("argmax", "choice"), default="argmax",
                    help="'argmax' is what the reference generates with (:709, :845); 'choice' draws from the tempered softmax on the device")
    ap.add_argument("--random", type=int, default=0, help="max_new_sampled_songs")
    ap.add_argument("--long", type=int, default=0, help="max_new_sampled_long_songs")
    ap.add_argument("--long-length", type=int, default=20, help="long_song_length")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--midi-dir", default=None, help="read the songs from this folder (one subfolder per class) instead of making them")
    ap.add_argument("--out-dir", default="generated")
    args = ap.parse_args()
    s = vars(settings)
    bs, V = s["batch_size"], s["max_voices"]
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
    encode = lambda sg, rows: model.encoder.predict(vae_definition.prepare_encoder_input_list(
        sg["X"][rows], sg["I"], np.asarray(sg["V"])[rows], np.asarray(sg["D"])[rows]), batch_size=bs)
    all_z = np.concatenate([encode(sg, np.arange(sg["X"].shape[0])) for sg in songs], 0)                     # :673-699
    z_std_train = float(np.std(all_z))
    print("z mean train: %.4f   z std train: %.4f" % (float(np.mean(all_z)), z_std_train))

    rng = np.random.RandomState(args.seed)
    lengths = [sg["X"].shape[0] for sg in songs]
    paths, names, infos = [], [], []
    for _ in range(args.medleys):
        picks = generation.medley_samples(lengths, args.songs_per_medley, args.own_windows, rng)
        name = "medley_songs_%d_original_%d_bridge_%d_" % (args.songs_per_medley, args.own_windows, args.bridge)
        info, Rs = [], []
        for k, (song, sample, rows) in enumerate(picks):
            name += "_%d-%d" % (song, sample)
            programs = sweep_mod.programs_of(np.argmax(np.asarray(songs[song]["I"]), -1).reshape(-1)[:V], s["instrument_attach_method"])
            info += [("song_name_%d" % k, "song%d" % song), ("sample_num_%d" % k, sample), ("programs_%d" % k, [int(p) for p in programs])]
            Rs.append(encode(songs[song], np.asarray(list(rows))))                                          # :778-790
        paths.append(generation.medley_path(Rs, args.bridge, args.mode))
        names.append(name)
        infos.append(info)
    for i in range(args.interpolations):
        random_code_1 = rng.normal(loc=0.0, scale=z_std_train, size=(1, s["latent_dim"]))                    # :851-852
        random_code_2 = rng.normal(loc=0.0, scale=z_std_train, size=(1, s["latent_dim"]))
        # (one run holds anchors of one type: the random codes join the encoder's float32 latents)
        as_type = (lambda c: c.astype(np.float32)) if args.medleys else (lambda c: c)
        paths.append(generation.interpolation_path(as_type(random_code_1), as_type(random_code_2), args.length, args.mode))
        names.append("random_interpolation_%d_length_%d" % (i, args.length))
        infos.append(None)
    if not paths and not args.random and not args.long:
        raise SystemExit("nothing to generate")
    kw = dict(seed=args.seed) if args.sample_method == "choice" else {}
    decode = dict(batch_size=bs, sample_method=args.sample_method, note_events=True, pianoroll=True, **kw)
    res = model.decoder.decode_paths(paths, **decode) if paths else []
    if args.random:                                                                                             # :1771-1814
        codes = rng.normal(loc=0.0, scale=z_std_train, size=(args.random, s["latent_dim"]))
        res += model.decoder.random_songs(codes, **decode)
        names += ["random_%d" % i for i in range(args.random)]
        for i in range(args.random):
            random_code = rng.normal(loc=0.0, scale=z_std_train, size=(s["latent_dim"],))
            res += model.decoder.class_knob_songs(random_code, s["num_classes"], **decode)
            names += ["random_%d_%d" % (i, C) for C in range(s["num_classes"])]
        infos += [None] * (args.random * (1 + s["num_classes"]))
    if args.long:                                                                                               # :1821-1896
        codes = rng.normal(loc=0.0, scale=z_std_train, size=(args.long, s["latent_dim"]))
        res += model.decoder.long_songs(all_z, codes, length=args.long_length, **decode)
        names += ["random_long_%d" % i for i in range(args.long)]
        infos += [None] * args.long
    dt = time.time() - t0

    os.makedirs(args.out_dir, exist_ok=True)
    for d, name, info in zip(res, names, infos):
        tracks = [d["events"][d["events"]["voice"] == v] for v in range(V)]
        midifile.write_midi(os.path.join(args.out_dir, name + ".mid"), tracks, d.get("programs", [0] * V), BPM, s["SMALLEST_NOTE"])
        pianoroll.write_png(os.path.join(args.out_dir, name + ".png"), d["pianoroll"])
        if info is not None:
            with open(os.path.join(args.out_dir, name + "_info.txt"), "w", encoding="utf-8") as f:
                for k, v in info:
                    f.write(k + ": %s" % v + "\n")
        print("%-60s %4d windows %5d notes, image %s, programs %s" % (name, len(d["notes"]), len(d["events"]), d["pianoroll"].shape,
                                                                      list(d.get("programs", []))))
    n_win = sum(len(d["notes"]) for d in res)
    print("%d windows of %d songs: encode, decode passes, rules, note events and images on the device: %.2f s; files in %s"
          % (n_win, len(res), dt, args.out_dir))


if __name__ == "__main__":
    main()
