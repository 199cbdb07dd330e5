"""Window descriptors: the 15-entry signature vector and the voice-by-voice harmonicity of piano-roll windows (reference
data_class.py:96-215 and :25-88), from the one-byte index per row the engine stages and decodes.

``signature_vectors`` / ``harmonicity`` run on the device (``mvae_desc_windows``, include/midivae_descriptors.h: one lane per window)
or, with ``device=False``, through the NumPy mirror below - the same semantics written out in Python, the yardstick of the device
tests and the host path of ``vae_training.py --signatures host``.  Both are pinned to the reference's own functions by
tests/golden/descriptors.npz.

Semantics.  Row t of a window is voice t % V of tick t // V.  An index is a note unless it is the silent index, 255, or >= n_pitch;
its pitch is index + low_crop.  The signature walks the ticks with the reference's bookkeeping, quirks included: the note set of
a tick is the distinct pitches, ascending; held notes are dropped by deleting from the list being iterated, so the note after a
deleted one is skipped and stays held; a silent tick ends every held note, notes held at the window's end are not counted; the
interval list pairs the sorted note sets of consecutive non-silent ticks, and for sets of unequal size keeps of the longer set the
notes nearest to the shorter one (stable order on ties).  Harmonicity: per segment of ``SMALLEST_NOTE // 4`` ticks each voice's
chroma (bin = index // (n_pitch / 12)) is normalised and mapped by the 6 x 12 tonal matrix; an entry is the mean distance of two
voices' centroids over the segments in which both sound, NaN if there is none, 0 on the diagonal.

``s`` is a settings mapping or module read like packers._g does: max_voices, low_crop, high_crop, include_silent_note, SMALLEST_NOTE.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import hiplib as hl
from .packers import _g
from .rolls import HostPack, as_rolls, base_params, check_rows, device_roll, host_roll, sounding

SIGNATURE_LENGTH = 15


def params(s):
    """what the descriptors read from the settings"""
    return dict(base_params(s), low_crop=int(_g(s, "low_crop")), resolution=int(_g(s, "SMALLEST_NOTE")) // 4)


def tonal_matrix(r1=1.0, r2=1.0, r3=0.5):
    """the 6 x 12 tonal matrix (Harte et al., "Detecting harmonic change in musical audio", 2006) as float32: circle of fifths, of
    minor thirds and of major thirds, evaluated in float64 and rounded once"""
    k = np.arange(12)
    tm = np.empty((6, 12), dtype=np.float32)
    for row, (r, step) in enumerate(((r1, 7. / 6.), (r2, 3. / 2.), (r3, 2. / 3.))):
        tm[2 * row] = r * np.sin(k * step * np.pi)
        tm[2 * row + 1] = r * np.cos(k * step * np.pi)
    return tm


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _stats(values, scale, np_std):
    if not values:
        return [0.0, 0.0, 0.0, 0.0]
    if np_std:
        return [np.max(values) / scale, np.min(values) / scale, np.mean(values) / scale, np.std(values) / scale]
    c, sm, sq = len(values), sum(values), sum(v * v for v in values)
    return [max(values) / scale, min(values) / scale, (sm / c) / scale, float(np.sqrt((c * sq - sm * sm) / (c * c))) / scale]


def signature_from_note_sets(song, _tidy=False, _np_std=False):
    """the signature of one window given as a sequence of ascending pitch tuples, one per tick.  ``_tidy`` drops ended notes from
    a COPY of the held list (what the reference's loop looks like it does); it exists to show that the fixtures exercise the
    difference.  ``_np_std``: max / min / mean / std through NumPy as the reference takes them, else from exact integer sums like
    the device."""
    held, age, durations, pitches, intervals = [], [], [], [], []
    previous, polyphonic = (), 0
    for notes in song:
        if _tidy:
            for note in list(held):
                if note not in notes:
                    i = held.index(note)
                    durations.append(age[i])
                    del held[i], age[i]
        else:
            i = 0
            while i < len(held):          # deleting shifts the tail down and the position still moves on: the next note is skipped
                if held[i] not in notes:
                    durations.append(age[i])
                    del held[i], age[i]
                i += 1
        for note in notes:
            pitches.append(note)
            if note in held:
                age[held.index(note)] += 1
            else:
                held.append(note)
                age.append(1)
        if len(notes) != len(previous) and notes and previous:
            shorter, longer = (notes, previous) if len(notes) < len(previous) else (previous, notes)
            nearest = [min(abs(p - q) for q in shorter) for p in longer]
            keep = sorted(np.argsort(nearest, kind="stable")[:len(shorter)].tolist())
            pairs = zip(shorter, [longer[i] for i in keep])
        else:
            pairs = zip(notes, previous)
        intervals.extend(abs(p - q) for p, q in pairs)
        polyphonic += len(notes) > 1
        if notes:
            previous = notes
        else:
            durations.extend(age)
            held, age = [], []
    ticks = len(song)
    return ([len(durations) / ticks, len(pitches) / ticks, polyphonic / ticks] + _stats(pitches, 127, _np_std) +
            _stats(intervals, 127, _np_std) + _stats(durations, 1.0, _np_std))


def _mirror_signatures(idx, p, _tidy=False, _np_std=False):
    n, T = idx.shape
    V = p["voices"]
    on = sounding(idx, p)
    pitch = idx.astype(np.int64) + p["low_crop"]
    out = np.zeros((n, SIGNATURE_LENGTH))
    for w in range(n):
        pw, ow = pitch[w].reshape(T // V, V).tolist(), on[w].reshape(T // V, V).tolist()
        song = [tuple(sorted({x for x, o in zip(pr, orow) if o})) for pr, orow in zip(pw, ow)]
        out[w] = signature_from_note_sets(song, _tidy, _np_std)
    return out


def _mirror_harmonicity(idx, p):
    n, T = idx.shape
    V, res = p["voices"], p["resolution"]
    ticks = T // V
    segs = ticks // res
    out = np.full((n, V, V), np.nan)
    out[:, np.arange(V), np.arange(V)] = 0.0
    if segs == 0 or n == 0:
        return out
    if p["n_pitch"] % 12:
        raise ValueError("harmonicity needs a pitch range that is a multiple of 12 columns, got %d" % p["n_pitch"])
    use = idx[:, :segs * res * V].reshape(n, segs, res, V)
    on = sounding(use, p)
    bins = np.where(on, use // (p["n_pitch"] // 12), 12)
    chroma = (bins[..., None] == np.arange(12)).sum(2).astype(np.float64)          # (n, segs, V, 12)
    total = chroma.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cent = (chroma / total[..., None]) @ tonal_matrix().astype(np.float64).T   # (n, segs, V, 6); NaN rows for empty voices
    d = cent[:, :, :, None, :] - cent[:, :, None, :, :]
    dist = np.sqrt((d * d).sum(-1))                                                # (n, segs, V, V)
    ok = ~np.isnan(dist)
    cnt = ok.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ok, dist, 0.0).sum(1) / cnt
    off = ~np.eye(V, dtype=bool)
    out[:, off] = np.where(cnt > 0, mean, np.nan)[:, off]
    return out


# ---- the device path -----------------------------------------------------------------------------------------------------------
_tonal_dev = {}


def _tonal_on(device):
    import torch
    key = str(device)
    if key not in _tonal_dev:
        _tonal_dev[key] = torch.from_numpy(tonal_matrix()).to(device).contiguous()
    return _tonal_dev[key]


def enqueue(idx, p, sig_out, harm_out, tonal, stream):
    """mvae_desc_windows on device memory the caller owns: ``idx`` (n, T) uint8 tensor view of any strides (a decode's time-major
    buffer: ``rows[:, :B].t()``), ``sig_out`` (n, >= 15) / ``harm_out`` (n, V * V) float64 tensors or None"""
    n, T = idx.shape
    a = hl.DescArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), n=n, T=T, voices=p["voices"], silent=p["silent"],
                    n_pitch=p["n_pitch"], low_crop=p["low_crop"], resolution=p["resolution"],
                    ld_sig=0 if sig_out is None else sig_out.stride(0), tonal=hl.ptr(tonal), sig_out=hl.ptr(sig_out),
                    harm_out=hl.ptr(harm_out))
    hl.check(hl.load().mvae_desc_windows(C.byref(a), stream), "mvae_desc_windows")


def _check(T, p, harm):
    check_rows(T, p)
    if harm and p["n_pitch"] % 12:
        raise ValueError("harmonicity needs a pitch range that is a multiple of 12 columns, got %d" % p["n_pitch"])


def _device_run(idx, p, want_sig, want_harm, device=None):
    import torch
    t = device_roll(idx, torch.uint8, "notes", device=device)
    n, T = t.shape
    V = p["voices"]
    _check(T, p, want_harm)
    sig = torch.empty((n, SIGNATURE_LENGTH), dtype=torch.float64, device=t.device) if want_sig else None
    harm = torch.empty((n, V * V), dtype=torch.float64, device=t.device) if want_harm else None
    if n:
        with torch.cuda.device(t.device):
            enqueue(t, p, sig, harm, _tonal_on(t.device) if want_harm else None, torch.cuda.current_stream().cuda_stream)
    return (None if sig is None else sig.cpu().numpy(), None if harm is None else harm.cpu().numpy().reshape(n, V, V))


def decoded_batch(rows, B, p):
    """the first ``B`` windows of a time-major (T, Bp) uint8 device buffer - what a decode leaves behind - and their descriptors:
    dict ``notes`` (B, T) uint8, ``signature`` (B, 15), ``harmonicity`` (B, V, V).  Enqueued on the current stream of the buffer's
    device; the three results travel to the host in ONE copy."""
    import torch
    T, V = rows.shape[0], p["voices"]
    pack = HostPack(rows.device, [("signature", torch.float64, (B, SIGNATURE_LENGTH)), ("harmonicity", torch.float64, (B, V * V)),
                                  ("notes", torch.uint8, (B, T))])
    with torch.cuda.device(rows.device):
        enqueue(rows[:, :B].t(), p, pack.views["signature"], pack.views["harmonicity"], _tonal_on(rows.device),
                torch.cuda.current_stream().cuda_stream)
        pack.views["notes"].copy_(rows[:, :B].t())
        res = pack.to_host()
    res["harmonicity"] = res["harmonicity"].reshape(B, V, V)
    return res


def signature_vectors(idx, s, device=True, _tidy=False, _np_std=False):
    """(n, 15) float64 signature vectors of (n, T) uint8 index rolls, (n, T, K) one-hot rolls or a 2-D uint8 device tensor"""
    p, idx = params(s), as_rolls(idx)
    if device:
        return _device_run(idx, p, True, False)[0]
    idx = host_roll(idx, np.uint8, "notes")
    _check(idx.shape[1], p, False)
    return _mirror_signatures(idx, p, _tidy, _np_std)


def harmonicity(idx, s, device=True):
    """(n, V, V) float64 tonal distance between the voices of every window; NaN where two voices never sound in the same segment"""
    p, idx = params(s), as_rolls(idx)
    if device:
        return _device_run(idx, p, False, True)[1]
    idx = host_roll(idx, np.uint8, "notes")
    _check(idx.shape[1], p, True)
    return _mirror_harmonicity(idx, p)


def nanmean_windows(h):
    """mean over the windows that have a value, NaN where none has (reference data_class.py:67-73)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(h, axis=0)


def song_harmonicity(idx, s, device=True):
    """(V, V): the windows' harmonicity, averaged over the windows where it is defined"""
    return nanmean_windows(harmonicity(idx, s, device))
