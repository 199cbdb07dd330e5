"""The song-level decodes of ``model.Decoder``: the latent sweep, whole songs, generated songs, long songs and the style switch.
Every public name here is the body of the Decoder method of that name - ``dec`` is the decoder, the other arguments are the method's,
and the method's docstring is the documentation of record.  All of them decode through ``dec._run`` into a sink of decode_sinks; the
ones that return songs share ONE tail on the run's device rolls, ``finish_rolls``, and one cut into per-song dicts, ``song_dicts``.
"""
from __future__ import annotations

import numpy as np

from . import decode_sinks as sinks
from . import descriptors as desc
from . import events as ev
from . import generation as gen
from . import longsongs as ls
from . import packers
from . import pianoroll as pr
from . import reconstruction as rec
from . import style as style_mod
from . import sweep as sweep_mod
from .rolls import as_rolls

PER_WINDOW = ("notes", "velocity", "starts", "counts", "instr", "signature", "harmonicity", "z", "picked",
              "distances")                                                                           # run arrays song_dicts slices
PER_SONG = ("metrics", "events", "programs", "pianoroll")                                              # run lists it hands out


# ---- the latent sweep ------------------------------------------------------------------------------------------------------------
def sweep_inputs(dec, z, values, s):
    sp = dec._s.spec
    z = np.asarray(z, np.float64)
    if z.ndim != 2 or z.shape[1] != sp.Z:
        raise ValueError("z must be (n, %d), got %r" % (sp.Z, z.shape))
    n, Z, K = z.shape[0], sp.Z, len(values)
    zs = np.repeat(z[:, None, None, :], Z, axis=1).repeat(K, axis=2)
    zs[:, np.arange(Z), :, np.arange(Z)] = np.asarray(values, np.float64)
    zs = zs.reshape(n * Z * K, Z)
    return packers.prepare_decoder_input(s, zs, 0, np.zeros((n * Z * K, int(packers._g(s, "signature_vector_length")))),
                                         np.zeros(zs.shape))


def latent_sweep(dec, z, range_end_in_stds, sigma, evaluations_per_dimension, positive_and_negative, batch_size, sample_method,
                 temperature, seed, return_rolls, judges):
    (s, p), sp = dec._analysis(sweep_mod), dec._s.spec
    values = np.asarray(sweep_mod.sweep_values(range_end_in_stds, sigma, evaluations_per_dimension, positive_and_negative))
    z = np.asarray(z, np.float64)
    x = sweep_inputs(dec, z, values, s)
    n, Z, K = z.shape[0], sp.Z, len(values)
    if n == 0:
        raise ValueError("z holds no sample")
    if judges is None:
        sink = sinks.SweepStatistics(p=p, T=sp.T, return_rolls=return_rolls)
    else:
        sink = sinks.JudgedSweepStatistics(p=p, T=sp.T, return_rolls=return_rolls, judges=judges, batch_size=batch_size, style=[])
    got = dec._sampled_run(x, batch_size, sink, sample_method, temperature, seed, None)
    table = got["table"].reshape(n, Z, K, sweep_mod.N_COLUMNS)
    if got["instr"] is not None:
        programs = sweep_mod.programs_of(got["instr"], packers._g(s, "instrument_attach_method")).reshape(n, Z, K, sp.V)
    else:          # the reference's default I: all piano
        programs = np.zeros((n, Z, K, sp.V), np.int64)
    style = got["style"].reshape(n, Z, K, 3) if judges is not None else None
    summaries, infl, peaked, best = sweep_mod.summarize_sweep(table, programs, style=style)
    res = dict(table=table, programs=programs, values=values, summaries=summaries, influence=infl, most_peaked=peaked,
               overall_best=best)
    if style is not None:
        res["style"] = style
    if return_rolls:
        res["notes"] = got["notes"].reshape(n, Z, K, sp.T)
        res["velocity"] = got["velocity"].reshape(n, Z, K, sp.T)
    return res


# ---- the tail of every decode of whole songs -------------------------------------------------------------------------------------
def check_song_extras(dec, note_events, pianoroll):
    """the refusals of what finish_rolls runs behind mvae_recon_songs as asked, before anything is decoded"""
    if note_events:
        dec._analysis(ev)
    if pianoroll:
        dec._analysis(pr)


def finish_rolls(dec, rolls, lengths, carried=True, orig=None, descriptors=False, note_events=False, close_at_end=False, vote=False,
                 judges=None, class_lists=(), batch_size=32, pianoroll=False, counts=True, filled_velocity=True):
    """What follows the decode of whole songs, on the run's device rolls (decode_sinks.SongRolls / LockstepRolls) of songs of
    ``lengths`` windows laid end to end.  Enqueued in this order: mvae_recon_songs - ``carried`` False: the velocity rules start afresh
    in every window, as where the reference post-processes one window a call; ``orig`` (n, T) uint8: the targets of the counts - then as
    asked mvae_desc_windows (``descriptors``), mvae_note_events (``note_events``, ``close_at_end``), the ``judges``, scored against
    every list of ``class_lists`` (one class per song each), and mvae_pianoroll (``pianoroll``).  For a model WITHOUT the velocity
    head the velocity judge gets no roll; ``filled_velocity`` says what else stands in for the missing head: True - the default-filled
    roll mvae_recon_songs writes is what mvae_note_events reads and what ``velocity`` reads back; False - mvae_note_events gets no
    velocities (every note has velocity 80) and ``velocity`` is filled on the host, without a read.  Run-level host arrays, one
    device-to-host read each: ``notes``, ``velocity``, with ``counts`` ``starts`` and ``counts``, with the head ``instr``, with
    ``descriptors`` ``signature`` and ``harmonicity``; lists with an item per song: ``events`` (two reads), ``pianoroll`` (one), with
    ``orig`` ``metrics`` and, with ``vote`` and the instrument head, ``programs`` (events.vote_for_programs), both host arithmetic;
    ``style``: per class list the pair (table, ensemble or None), one read each."""
    import torch
    (s, p), sp = dec._analysis(rec), dec._s.spec
    n, notes_d, dev = int(sum(lengths)), rolls["notes"], rolls["notes"].device
    run = {}
    with torch.cuda.device(dev):
        first = torch.from_numpy(rec.first_windows(lengths, n)).to(dev)
        vel_d, starts_d, counts_d = rec.run_on_device(notes_d, rolls.get("velocity"), rolls.get("held"),
                                                      None if orig is None else torch.from_numpy(orig).to(dev), first if carried else None, p)
        headed = "velocity" in rolls
        filled = headed or filled_velocity
        if descriptors:
            _, dp = dec._analysis(desc, True)
            sig_d = torch.empty((n, desc.SIGNATURE_LENGTH), dtype=torch.float64, device=dev)
            harm_d = torch.empty((n, sp.V * sp.V), dtype=torch.float64, device=dev)
            desc.enqueue(notes_d, dp, sig_d, harm_d, desc._tonal_on(dev), torch.cuda.current_stream().cuda_stream)
        if note_events:
            _, ep = dec._analysis(ev)
            ev._check(sp.T, ep, n)
            song = torch.from_numpy(ev.song_ordinals(lengths, n)).to(dev)
            table = ev.run_on_device(notes_d, vel_d if filled else None, starts_d, song, len(lengths), ep, close_at_end)
        if judges is not None:
            tables = judges.probabilities(notes_d, vel_d if headed else None, rolls.get("instr"), batch_size)
            run["style"] = [judges.score_groups(tables, classes, lengths) for classes in class_lists]
        if pianoroll:
            _, pp = dec._analysis(pr)
            run["pianoroll"] = pr.split_songs(pr.run_on_device(notes_d, vel_d, first, pp).cpu().numpy(), lengths, sp.T // sp.V)
        run["velocity"] = vel_d.cpu().numpy() if filled else np.full((n, sp.T), rec.default_velocity(p), np.float32)
        if counts:
            run.update(starts=starts_d.cpu().numpy(), counts=counts_d.cpu().numpy())
        run["notes"] = notes_d.cpu().numpy()
        if "instr" in rolls:
            run["instr"] = rolls["instr"].cpu().numpy()
        if descriptors:
            run.update(signature=sig_d.cpu().numpy(), harmonicity=harm_d.cpu().numpy().reshape(n, sp.V, sp.V))
        if note_events:
            run["events"] = ev.split_songs(*ev.read_back(table[0], table[1]), sp.V)
    if vote and "instr" in run:
        run["programs"] = ev.vote_for_programs(run["instr"], lengths, s)
    if orig is not None:
        run["metrics"] = rec.song_metrics(run["counts"], lengths, sp.T, s)
    return run


def song_dicts(run, lengths):
    """one dict per song from what finish_rolls returns: the song's rows of every run-level array, its item of every per-song list,
    and ``style`` from the FIRST class list's table and ensemble"""
    res, lo = [], 0
    for i, m in enumerate(lengths):
        d = {k: run[k][lo:lo + m] for k in PER_WINDOW if k in run}
        d.update({k: run[k][i] for k in PER_SONG if k in run})
        if "style" in run:
            table, ensemble = run["style"][0]
            d["style"] = dict(style_mod.style_of(table[i]), ensemble_prediction=None if ensemble is None else ensemble[lo:lo + m])
        res.append(d)
        lo += m
    return res


# ---- whole songs -----------------------------------------------------------------------------------------------------------------
def predict_songs(dec, xs, batch_size, sample_method, temperature, seed, uniforms, originals, note_events, close_at_end, judges, classes,
                  pianoroll):
    from .model import _as_list
    (s, p), sp = dec._analysis(rec), dec._s.spec
    packers.refuse_meta_without_instrument(s)
    check_song_extras(dec, note_events, pianoroll)
    xs = [_as_list(x) for x in xs]
    if not xs:
        return []
    if len({len(x) for x in xs}) != 1:
        raise ValueError("predict_songs: every song must pass the same inputs, in the same order")
    lengths = [np.asarray(x[1]).shape[0] for x in xs]
    for i, m in enumerate(lengths):
        if m <= 0:
            raise ValueError("predict_songs: song %d has no windows - leave empty songs out of the list" % i)
    if judges is not None and (classes is None or len(classes) != len(xs)):
        raise ValueError("predict_songs: judges score every song against its class - pass one class per song")
    orig = None
    if originals is not None:
        originals = [np.asarray(as_rolls(o)) for o in originals]
        if len(originals) != len(xs):
            raise ValueError("predict_songs: %d originals for %d songs" % (len(originals), len(xs)))
        for i, (o, m) in enumerate(zip(originals, lengths)):
            if o.shape != (m, sp.T):
                raise ValueError("predict_songs: the original of song %d has shape %r, expected %r" % (i, o.shape, (m, sp.T)))
        orig = np.concatenate(originals, 0)
    x = [np.concatenate([np.asarray(xi[k]) for xi in xs], 0) for k in range(len(xs[0]))]
    rolls = dec._sampled_run(x, batch_size, sinks.SongRolls(int(sum(lengths))), sample_method, temperature, seed, uniforms)
    return song_dicts(finish_rolls(dec, rolls, lengths, orig=orig, note_events=note_events, close_at_end=close_at_end, vote=note_events,
                                   judges=judges, class_lists=(classes,), batch_size=batch_size, pianoroll=pianoroll), lengths)


# ---- generated songs ---------------------------------------------------------------------------------------------------------------
def decode_paths(dec, paths, batch_size, sample_method, temperature, seed, note_events, close_at_end, pianoroll):
    import torch
    (s, _), sp = dec._analysis(rec), dec._s.spec
    packers.refuse_meta_without_instrument(s)
    check_song_extras(dec, note_events, pianoroll)
    paths = list(paths)
    if not paths:
        return []
    run = gen.concat_paths(paths)
    if int(run["anchors"].shape[1]) != sp.Z:
        raise ValueError("decode_paths: the anchors have %d columns, the model's latent has %d" % (run["anchors"].shape[1], sp.Z))
    lengths, n = run["lengths"], len(run["a0"])
    sample = dec._sample_spec(n, sample_method, temperature, seed, None, dec._softmax_heads())
    state = {}

    def fill(eng, lo, hi):
        if "run" not in state:          # (once per run: the engine, and with it the device, exists from here on)
            state["run"] = gen.upload(run, eng.device)
        eng.stage_decoder_paths(hi - lo, lo, state["run"])

    rolls = dec._run(None, batch_size, sinks.SongRolls(n), sample, stage=(n, fill))
    dev = rolls["notes"].device
    with torch.cuda.device(dev):
        z_dev = torch.empty((n, sp.Z), dtype=torch.float32, device=dev)
        gen.enqueue(state["run"], 0, n, z_dev, None, torch.cuda.current_stream().cuda_stream)
        z = z_dev.cpu().numpy()
    host = finish_rolls(dec, rolls, lengths, note_events=note_events, close_at_end=close_at_end, vote=note_events, batch_size=batch_size,
                        pianoroll=pianoroll)
    host["z"] = z
    return song_dicts(host, lengths)


def interpolation_songs(dec, code_pairs, length, mode, **kw):
    return dec.decode_paths([gen.interpolation_path(a, b, length, mode) for a, b in code_pairs], **kw)


def medleys(dec, list_of_Rs, interpolation_length, mode, **kw):
    return dec.decode_paths([gen.medley_path(Rs, interpolation_length, mode) for Rs in list_of_Rs], **kw)


def random_songs(dec, codes, **kw):
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.shape[0] <= 0:
        raise ValueError("random_songs: codes are (n > 0, Z), got %r" % (codes.shape,))
    return dec.decode_paths([gen.code_path(c) for c in codes], **kw)


def class_knob_codes(code, num_classes):
    code = np.asarray(code).reshape(-1)
    if code.dtype not in (np.float32, np.float64):
        code = code.astype(np.float64)
    num_classes = int(num_classes)
    if not 1 <= num_classes <= code.shape[0]:
        raise ValueError("class_knob_songs: %d classes for a code of %d columns" % (num_classes, code.shape[0]))
    out = np.repeat(code[None, :], num_classes, 0)
    out[:, :num_classes] = -1
    out[np.arange(num_classes), np.arange(num_classes)] = 1
    return out


def class_knob_songs(dec, code, num_classes, **kw):
    return dec.random_songs(dec.class_knob_codes(code, num_classes), **kw)


# ---- long songs ------------------------------------------------------------------------------------------------------------------
def long_songs(dec, all_z, codes, length, e, sample_method, temperature, seed, note_events, pianoroll, close_at_end, batch_size):
    import torch
    (s, _), sp = dec._analysis(rec), dec._s.spec
    p = ls.params(s)
    packers.refuse_meta_without_instrument(s)
    check_song_extras(dec, note_events, pianoroll)
    if sp.attach or packers._g(s, "attach_instruments"):
        raise NotImplementedError("long_songs with attach_instruments: a decoded row does not carry the attached instrument")
    if packers._g(s, "combine_velocity_and_held_notes"):
        raise NotImplementedError("long_songs with combine_velocity_and_held_notes: a fed-back decode can break the reference's "
                                  "own assertion that a held step has no velocity")
    all_z = np.asarray(all_z)
    if all_z.dtype != np.float32:
        raise ValueError("long_songs: all_z is float32, as encoder.predict returns it, got %s" % all_z.dtype)
    codes = ls._host_codes(codes, "long_songs: the start codes")
    ls._check_walk(all_z, codes, ())
    if all_z.shape[1] != sp.Z:
        raise ValueError("long_songs: all_z has %d columns, the model's latent has %d" % (all_z.shape[1], sp.Z))
    length = int(length)
    if length <= 0:
        raise ValueError("long_songs: length must be positive")
    e_d, den = ls.pull_factors(np.std(all_z) if e is None else e)
    S, Z, N = codes.shape[0], sp.Z, all_z.shape[0]
    sample = dec._sample_spec(S * length, sample_method, temperature, seed, None, dec._softmax_heads())
    eps = dec._s.epsilon(S * length).reshape(length, S, Z)
    eng = dec._s.get_infer(S)
    dev = eng.device
    sink = sinks.LockstepRolls(S, length)
    with torch.cuda.device(dev):
        A = torch.from_numpy(np.ascontiguousarray(all_z)).to(dev)
        start = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
        eps_d = torch.from_numpy(np.ascontiguousarray(eps)).to(dev)
        picked = torch.zeros((S, length), dtype=torch.int32, device=dev)
        best = torch.empty((length, S), dtype=torch.int32, device=dev)
        dist = torch.empty((length, S), dtype=torch.float64, device=dev)
        z_run = torch.empty((length, S, Z), dtype=torch.float32, device=dev)
        for g0 in range(0, S, eng.maxB):
            B = min(S, g0 + eng.maxB) - g0
            work = torch.empty(ls.workspace_bytes(N, B, Z), dtype=torch.uint8, device=dev)
            # the pulled codes of two iterations: what is written now, and the history of the next one
            pulled = [torch.empty((B, Z), dtype=torch.float32, device=dev) for _ in range(2)]
            previous = None
            for it in range(length):
                r_in = start[g0:g0 + B] if it == 0 else None
                r_out = torch.empty_like(r_in) if it == 0 else pulled[it & 1]
                eng.stage_decoder_walk(B, dict(all_z=A, r_in=r_in, hist_in=previous, picked=picked[g0:g0 + B], n_picked=it, e=e_d,
                                               den=den, workspace=work, best_out=best[it, g0:g0 + B], dist_out=dist[it, g0:g0 + B],
                                               r_out=r_out))
                z_run[it, g0:g0 + B].copy_(eng._v("zh", eng.pad16(B), sp.zin)[:B, :Z])
                spec = None if sample is None else dict(sample, first_window=it * S + g0, uniforms={})
                eng.decode(B, want_probs=False, sample=spec, want_velocity=sp.meta_velocity)
                views = eng.decoded(B, sample is not None)
                sink.batch_at(eng, it, g0, B, views)
                if it + 1 < length:
                    eng.stage_encoder_feedback(B, views, eps_d[it, g0:g0 + B], p)
                    eng.encode(B)
                previous = r_out
        eng.check_pipeline()
        # song-major like the rolls: row s * length + it
        walked = dict(picked=picked.cpu().numpy().astype(np.int64).reshape(-1),
                      distances=np.ascontiguousarray(dist.cpu().numpy().T).reshape(-1),
                      z=np.ascontiguousarray(z_run.cpu().numpy().transpose(1, 0, 2)).reshape(S * length, Z))
    host = finish_rolls(dec, sink.result(), [length] * S, carried=False, note_events=note_events, close_at_end=close_at_end, vote=True,
                        batch_size=batch_size, pianoroll=pianoroll)
    return song_dicts(dict(host, **walked), [length] * S)


# ---- the style switch ------------------------------------------------------------------------------------------------------------
def switch_styles(dec, zs, classes, S, judges, note_events, batch_size, programs, close_at_end, sample_method, temperature, seed):
    (s, _), sp = dec._analysis(rec), dec._s.spec
    dec._analysis(desc, True)
    packers.refuse_meta_without_instrument(s)
    check_song_extras(dec, note_events, False)
    zs = [np.asarray(z, np.float64) for z in zs]
    if len(classes) != len(zs) or (S is not None and len(S) != len(zs)) or (programs is not None and len(programs) != len(zs)):
        raise ValueError("switch_styles: one class (and one signature array, one program list) per song")
    for i, z in enumerate(zs):
        if z.ndim != 2 or z.shape[0] <= 0 or z.shape[1] != sp.Z:
            raise ValueError("switch_styles: the latents of song %d have shape %r, expected (m > 0, %d)" % (i, z.shape, sp.Z))
        if not 0 <= int(classes[i]) < sp.C:
            raise ValueError("switch_styles: song %d has class %r, the model has %d" % (i, classes[i], sp.C))
    pairs = style_mod.switch_pairs(classes, sp.C)
    if not pairs:
        return dict(pairs=[], switch_instruments_matrix=None)
    SD = int(packers._g(s, "signature_vector_length"))
    xs = []
    for song, C, C_switch in pairs:
        switched, history = style_mod.switched_latents(zs[song], C, C_switch)
        sig = np.zeros((switched.shape[0], SD)) if S is None else np.asarray(S[song])
        xs.append(packers.prepare_decoder_input(s, switched, C_switch, sig, history))           # :2481
    x = [np.concatenate([np.asarray(xi[k]) for xi in xs], 0) for k in range(len(xs[0]))]
    lengths = [zs[song].shape[0] for song, _, _ in pairs]
    rolls = dec._sampled_run(x, batch_size, sinks.SongRolls(int(sum(lengths))), sample_method, temperature, seed, None)
    # the rules restart in every window; without the velocity head every note gets velocity 80; scored against own and target class
    host = finish_rolls(dec, rolls, lengths, carried=False, descriptors=True, note_events=note_events, close_at_end=close_at_end,
                        judges=judges, class_lists=([C for _, C, _ in pairs], [t for _, _, t in pairs]), batch_size=batch_size,
                        counts=False, filled_velocity=False)
    headed = "instr" in host
    # (without the instrument head the reference decodes its default I, all piano, and votes on that)
    voted = ev.vote_for_programs(host["instr"], lengths, s) if headed else [[0] * sp.V for _ in pairs]
    out = song_dicts(host, lengths)
    for k, (d, (song, C, C_switch)) in enumerate(zip(out, pairs)):
        d.update(song=song, C=C, C_switch=C_switch)
        if headed:
            d["voted_programs"] = voted[k]
        if programs is not None:
            flag, used = style_mod.instruments_switched([int(v) for v in programs[song]], voted[k], headed)
            d.update(instruments_switched=flag, programs=used)
        if judges is not None:
            d["style_target"] = style_mod.style_of(host["style"][1][0][k])
    matrix = None
    if programs is not None:
        matrix = style_mod.switch_instruments_matrix(pairs, [[int(v) for v in pr] for pr in programs], voted, sp.C)
    return dict(pairs=out, switch_instruments_matrix=matrix)
