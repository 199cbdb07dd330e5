"""Song-level decode and the reconstruction report (reference vae_definition.py:1156-1190 run over a whole song, and
vae_evaluation.py:2211-2236, :2380-2415): the velocity post-rules with the per-voice state carried from one window of a song into the
next, the note starts (the reference's D) and, per window, the eight counts the report's numbers are sums of.

``song_decode`` runs on the device (``mvae_recon_songs``, include/midivae_recon.h: one lane per window and voice, three launches, no
lane waits for another workgroup) or, with ``device=False``, through the NumPy mirror below - the closed form of the rule, vectorised,
the yardstick of the device tests.  Both are pinned to the reference's own functions by tests/golden/recon.npz.  ``song_metrics`` and
``mean_metrics`` are host arithmetic on eight integers per window.

The rule is applied in its closed form (rolls.carried_velocity_rule states it).  Every output is an input value or a zero and every
count an integer: device, mirror and reference are BIT-EQUAL.

``s`` is a settings mapping or module read like packers._g does: max_voices, low_crop, high_crop, include_silent_note,
velocity_threshold_such_that_it_is_a_played_note, override_sampled_pitches_based_on_velocity_info (and, for ``song_metrics``,
meta_held_notes and meta_velocity).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hiplib as hl
from .packers import _g
from .rolls import as_rolls, base_params, carried_velocity_rule, check_rows, device_roll, host_roll, sounding, with_strides_of

COUNTS = ("original_notes", "predicted_notes", "correct_notes", "not_predicted_notes", "new_predicted_notes", "note_starts",
          "note_starts_on_silent_prediction", "note_starts_on_silent_original")
N_COUNTS = len(COUNTS)
MAX_T = 65536
NO_TARGET = 255
METRICS = ("total_original_notes", "total_predicted_notes", "pitch_reconstruction_accuracy", "not_predicted_notes",
           "new_predicted_notes", "predicted_note_start_to_original_errors", "predicted_note_start_to_predicted_errors")


def params(s):
    """what the song-level decode reads from the settings"""
    return dict(base_params(s), threshold=float(_g(s, "velocity_threshold_such_that_it_is_a_played_note")),
                override=bool(_g(s, "override_sampled_pitches_based_on_velocity_info")))


def _check(T, p):
    check_rows(T, p, MAX_T, "song-level decode")
    if not 1 <= p["n_pitch"] <= 192:
        raise ValueError("%d pitch columns: the song-level decode takes 1..192" % p["n_pitch"])


def first_windows(lengths, n):
    """(n,) int32: for every window the index of the first window of its song, from the songs' window counts"""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size and lengths.min() <= 0:
        raise ValueError("every song needs at least one window, got lengths %r" % (lengths.tolist(),))
    if int(lengths.sum()) != n:
        raise ValueError("the songs' lengths sum to %d, the rolls hold %d windows" % (int(lengths.sum()), n))
    return np.repeat(np.cumsum(lengths) - lengths, lengths).astype(np.int32)


def default_velocity(p):
    """every row's velocity for a model without the velocity head (reference vae_definition.py:1211-1213), as the float32 kept"""
    return np.float32(p["threshold"] + (1.0 - p["threshold"]) * 0.5)


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _mirror(idx, vel, held, orig, first, p):
    n, T = idx.shape
    thr = p["threshold"]
    on = sounding(idx, p)
    if vel is None:
        velocity = np.full((n, T), default_velocity(p), np.float32)
    else:
        velocity = np.where(on, vel, np.float32(0)).astype(np.float32)
        if p["override"]:
            velocity = carried_velocity_rule(idx, on, velocity, first, p)
    if held is not None:
        starts = held.astype(np.uint8)
    elif vel is not None:
        starts = np.where(velocity.astype(np.float64) > thr, 0, 1).astype(np.uint8)
    else:
        starts = np.ones((n, T), np.uint8)
    counts = np.zeros((n, N_COUNTS), np.int32)
    is_start = starts == 0
    counts[:, 1] = on.sum(1)
    counts[:, 5] = is_start.sum(1)
    counts[:, 6] = (is_start & ~on).sum(1)
    if orig is not None:
        orig_on = sounding(orig, p)
        counts[:, 0] = orig_on.sum(1)
        counts[:, 2] = (orig_on & on & (orig == idx)).sum(1)
        counts[:, 7] = (is_start & ~orig_on).sum(1)
    counts[:, 3] = counts[:, 0] - counts[:, 2]
    counts[:, 4] = counts[:, 1] - counts[:, 2]
    return velocity, starts, counts


# ---- the device path -----------------------------------------------------------------------------------------------------------
def carry_bytes(n, p):
    """the size of the workspace mvae_recon_songs wants for ``n`` windows"""
    return n * p["voices"] * 8


def enqueue(idx, vel, held, orig, first, p, carry, vel_out, start_out, counts_out, stream):
    """mvae_recon_songs on device memory the caller owns.  ``idx`` (n, T) uint8 tensor of any strides, ``vel`` float32 / ``held`` uint8
    tensors of the same strides or None, ``orig`` (n, T) uint8 of any strides or None, ``first`` (n,) int32 or None (every window its
    own song), ``carry`` a tensor of carry_bytes(n, p) bytes or None, the outputs contiguous (n, T) float32 / (n, T) uint8 /
    (n, >= 8) int32 tensors or None."""
    n, T = idx.shape
    a = hl.ReconArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), vel=hl.ptr(vel), held=hl.ptr(held),
                     orig=hl.ptr(orig), orig_stride_t=0 if orig is None else orig.stride(1),
                     orig_stride_w=0 if orig is None else orig.stride(0), first_window=hl.ptr(first), n=n, T=T, voices=p["voices"],
                     silent=p["silent"], n_pitch=p["n_pitch"], override_rules=int(p["override"]), threshold=p["threshold"],
                     carry=hl.ptr(carry), vel_out=hl.ptr(vel_out), start_out=hl.ptr(start_out), counts_out=hl.ptr(counts_out),
                     ld_counts=0 if counts_out is None else counts_out.stride(0))
    hl.check(hl.load().mvae_recon_songs(C.byref(a), stream), "mvae_recon_songs")


def run_on_device(idx, vel, held, orig, first, p):
    """``enqueue`` with outputs and workspace of its own on the current stream of ``idx``'s device: the three output tensors.  A window
    axis of one element may carry any stride; the entry point wants them positive."""
    import torch
    n, T = idx.shape
    dev = idx.device
    fix = lambda t: t if t is None or (t.stride(0) > 0 and t.stride(1) > 0) else t.contiguous()
    idx, orig = fix(idx), fix(orig)
    vel, held = with_strides_of(idx, vel), with_strides_of(idx, held)
    vel_out = torch.empty((n, T), dtype=torch.float32, device=dev)
    start_out = torch.empty((n, T), dtype=torch.uint8, device=dev)
    counts = torch.empty((n, N_COUNTS), dtype=torch.int32, device=dev)
    carried = vel is not None and p["override"] and first is not None
    carry = torch.empty(carry_bytes(n, p), dtype=torch.uint8, device=dev) if carried else None
    with torch.cuda.device(dev):
        enqueue(idx, vel, held, orig, first, p, carry, vel_out, start_out, counts, torch.cuda.current_stream().cuda_stream)
    return vel_out, start_out, counts


def song_decode(idx, vel, lengths, s, held=None, orig=None, device=True):
    """The song-level decode of ``n`` windows that form ``len(lengths)`` songs (``lengths``: the songs' window counts, in order; their
    sum is n and each is > 0, else ValueError).  ``idx`` (n, T) uint8 index rolls or (n, T, K) one-hot rolls, ``vel`` (n, T) float
    velocities or None for a model without the velocity head, ``held`` (n, T) held-notes indices or None, ``orig`` the original
    target index per row (255 = no target; one-hot rolls are taken too) or None - host arrays, or 2-D device tensors of any strides
    (``vel`` and ``held`` are brought to the strides of ``idx``).  dict ``velocity`` (n, T) float32 after the song-carried rules,
    ``starts`` (n, T) uint8 (0 = a note starts) and ``counts`` (n, 8) int32 (columns: ``COUNTS``)."""
    p = params(s)
    if device:
        import torch
        if not hasattr(idx, "data_ptr"):
            idx = as_rolls(idx)
        if len(idx.shape) != 2:
            raise ValueError("notes are (n, T) index rolls, got shape %r" % (tuple(idx.shape),))
        n, T = idx.shape
        _check(T, p)
        first = first_windows(lengths, n)          # (every refusal comes before anything touches the device)
        t = device_roll(idx, torch.uint8, "notes")
        v = device_roll(vel, torch.float32, "velocities", t.shape, device=t.device)
        h = device_roll(held, torch.uint8, "held notes", t.shape, device=t.device)
        o = device_roll(orig, torch.uint8, "originals", t.shape, device=t.device)
        if n == 0:
            return dict(velocity=np.zeros((0, T), np.float32), starts=np.zeros((0, T), np.uint8), counts=np.zeros((0, N_COUNTS), np.int32))
        with torch.cuda.device(t.device):
            outs = run_on_device(t, v, h, o, torch.from_numpy(first).to(t.device), p)
        velocity, starts, counts = (x.cpu().numpy() for x in outs)
    else:
        a = host_roll(idx, np.uint8, "notes")
        n, T = a.shape
        _check(T, p)
        first = first_windows(lengths, n)
        velocity, starts, counts = _mirror(a, host_roll(vel, np.float32, "velocities", a.shape), host_roll(held, np.uint8, "held notes", a.shape),
                                           host_roll(orig, np.uint8, "originals", a.shape), first, p)
    return dict(velocity=velocity, starts=starts, counts=counts)


# ---- the report ------------------------------------------------------------------------------------------------------------------
def song_metrics(counts, lengths, T, s):
    """one dict per song with the reference's keys (``METRICS``) from the (n, 8) per-window counts: the sums over the song's windows,
    pitch_reconstruction_accuracy = correct / original notes (NaN for a song without original notes), the two note-start error
    counts divided by windows * T - and 0 unless ``meta_held_notes or (meta_velocity and threshold > 0)`` (vae_evaluation.py:2213)"""
    counts = np.asarray(counts)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    first_windows(lengths, counts.shape[0])
    starts_count = bool(_g(s, "meta_held_notes") or (_g(s, "meta_velocity") and
                                                     float(_g(s, "velocity_threshold_such_that_it_is_a_played_note")) > 0))
    out = []
    for lo, n in zip((np.cumsum(lengths) - lengths).tolist(), lengths.tolist()):
        c = [int(x) for x in counts[lo:lo + n].astype(np.int64).sum(0)]
        rows = n * int(T)
        out.append(dict(total_original_notes=c[0], total_predicted_notes=c[1],
                        pitch_reconstruction_accuracy=c[2] / c[0] if c[0] else float("nan"),
                        not_predicted_notes=c[3], new_predicted_notes=c[4],
                        predicted_note_start_to_original_errors=c[7] / rows if starts_count else 0.0,
                        predicted_note_start_to_predicted_errors=c[6] / rows if starts_count else 0.0))
    return out


def mean_metrics(list_of_dicts):
    """the reference's "Mean" row (vae_evaluation.py:1987, :2888-2891): every key summed over the songs in order, from 0.0, and divided by
    the number of songs (a NaN accuracy makes the mean NaN, as there)"""
    mean = dict(song_name="Mean")
    songs = list(list_of_dicts)
    for d in songs:
        for k, v in d.items():
            if k not in ("song_name", "class"):
                mean[k] = mean.get(k, 0.0) + v
    for k in mean:
        if k != "song_name":
            mean[k] /= len(songs)
    return mean
