"""What the analyses of decoded windows share (descriptors, sweep, reconstruction): index rolls and which rows sound, the common
settings and refusals, the host-or-device intake of a roll, the one-copy read-back of a batch's results, the closed form of the velocity
post-rule.  Row t of a window is voice t % V of tick t // V; an index is a note unless it is the silent index, 255, or >= n_pitch.
``s`` is a settings mapping or module read like packers._g does; ``p`` a module's ``params(s)``.
"""
from __future__ import annotations

import math

import numpy as np

from .packers import _g


def as_rolls(idx):
    """(n, T) uint8 index rolls from index rolls or (n, T, K) one-hot rolls; device tensors pass through"""
    if hasattr(idx, "data_ptr"):
        return idx
    idx = np.asarray(idx)
    if idx.ndim == 3:
        from .staging import host_onehot_to_index
        return host_onehot_to_index(idx, "piano roll")
    if idx.ndim != 2:
        raise ValueError("expected (n, T) index rolls or (n, T, K) one-hot rolls, got %s" % (idx.shape,))
    if idx.dtype != np.uint8:
        if idx.size and (idx.min() < 0 or idx.max() > 255):
            raise ValueError("indices must fit one byte")
        idx = idx.astype(np.uint8)
    return idx


def sounding(idx, p):
    idx = np.asarray(idx)
    return (idx != p["silent"]) & (idx != 255) & (idx < p["n_pitch"])


def base_params(s):
    """what every analysis reads from the settings: the voices, the pitch columns and the silent index (-1: none)"""
    n_pitch = int(_g(s, "high_crop")) - int(_g(s, "low_crop"))
    return dict(voices=int(_g(s, "max_voices")), n_pitch=n_pitch, silent=n_pitch if _g(s, "include_silent_note") else -1)


def check_rows(T, p, max_T=None, what="statistics"):
    """what every analysis refuses: rows that are not whole ticks of 2..8 voices, more than ``max_T``, a threshold that is not finite"""
    V = p["voices"]
    if not 2 <= V <= 8 or T % V:
        raise ValueError("rows per window (%d) must be a multiple of max_voices (%d, 2..8)" % (T, V))
    if max_T is not None and T > max_T:
        raise ValueError("rows per window (%d) above the limit of the %s (%d)" % (T, what, max_T))
    if not math.isfinite(p.get("threshold", 0.0)):
        raise ValueError("the velocity threshold must be finite")


def device_roll(a, dtype, what, shape=None, strides_of=None, device=None):
    """a 2-D device tensor of ``dtype``: ``a`` itself if it is one (any strides), else the host array - for uint8 whatever as_rolls
    takes - uploaded.  ``shape``: the shape it must have.  ``strides_of``: a tensor whose device and strides a device tensor must
    have and an upload is given."""
    import torch
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        if a.dtype != dtype or a.dim() != 2 or not a.is_cuda:
            raise ValueError("device %s are a 2-D %s tensor (n, T), any strides" % (what, str(dtype).replace("torch.", "")))
        if strides_of is not None and (a.stride() != strides_of.stride() or a.device != strides_of.device):
            raise ValueError("device %s are a tensor with the shape and strides of the notes" % what)
        t = a
    else:
        shape = None if shape is None else tuple(shape)
        t = torch.from_numpy(np.ascontiguousarray(host_roll(a, np.uint8 if dtype == torch.uint8 else np.float32, what, shape)))
        if strides_of is None:
            t = t.to(device or "cuda")
        else:
            t = torch.empty_strided(t.shape, strides_of.stride(), dtype=dtype, device=strides_of.device).copy_(t)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s have shape %r, the notes %r" % (what, tuple(t.shape), tuple(shape)))
    return t


def with_strides_of(idx, roll):
    """the optional device roll ``roll`` (None passes through) at the strides of ``idx``: itself, or a copy laid out like ``idx``"""
    import torch
    if roll is None or roll.stride() == idx.stride():
        return roll
    return torch.empty_strided(idx.shape, idx.stride(), dtype=roll.dtype, device=idx.device).copy_(roll)


def host_roll(a, dtype, what, shape=None):
    """the host counterpart: (n, T) uint8 index rolls (whatever as_rolls takes) or float32 values, from a host array or a device
    tensor; None passes through, as in device_roll"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        a = a.cpu().numpy()
    a = as_rolls(a) if dtype == np.uint8 else np.asarray(a).astype(np.float32)
    if shape is not None and a.shape != shape:
        raise ValueError("%s have shape %r, the notes %r" % (what, a.shape, shape))
    return a


class HostPack(object):
    """Typed 2-D blocks ``(name, torch dtype, (rows, columns))`` in ONE byte tensor on ``device``: ``views[name]`` is written by kernels
    and device copies, ``to_host()`` copies the pack once and returns name -> NumPy array (copies).  The blocks lie in descending
    element size, so every view is aligned to its element."""

    def __init__(self, device, blocks):
        import torch
        kind = {dtype: torch.empty(0, dtype=dtype) for _, dtype, _ in blocks}
        self._blocks, total = [], 0
        for name, dtype, shape in sorted(blocks, key=lambda b: -kind[b[1]].element_size()):          # (stable: ties keep their order)
            nbytes = int(shape[0]) * int(shape[1]) * kind[dtype].element_size()
            self._blocks.append((name, dtype, kind[dtype].numpy().dtype, (int(shape[0]), int(shape[1])), total, total + nbytes))
            total += nbytes
        self.pack = torch.empty(total, dtype=torch.uint8, device=device)
        self.views = {name: self.pack[lo:hi].view(dtype).view(shape) for name, dtype, _, shape, lo, hi in self._blocks}

    def to_host(self):
        host = self.pack.cpu().numpy()
        return {name: host[lo:hi].view(np_dtype).reshape(shape).copy() for name, _, np_dtype, shape, lo, hi in self._blocks}


def carried_velocity_rule(idx, on, v0, first, p):
    """The velocity post-rule (reference vae_definition.py:1156-1190, packers.apply_velocity_rules) in closed form, the per-voice state
    carried through the windows of a song.  ``idx`` (n, T) indices, ``on`` their sounding flags, ``v0`` (n, T) float32 velocities, 0
    where a row does not sound, ``first`` (n,) the first window of every window's song (arange(n): every window its own song).  Per
    voice over the rows of a song: previous_pitch is the index of the previous row (-1 if it does not sound, or at the song's first
    tick), previous_velocity is v0 of the nearest earlier row for which ``v0 < threshold`` is false, 0.0 if there is none.  A row
    becomes previous_velocity if v0 < threshold, it sounds, previous_pitch > 0 (not >= 0: the reference's own test) and previous_pitch
    != its index; 0 if v0 < threshold is false and it does not sound; else it stays v0.  (n, T) float32: input values and zeros."""
    n, T = idx.shape
    V, thr = p["voices"], p["threshold"]
    if n == 0:
        return v0
    ticks = T // V
    # one sequence per voice through all songs: row i of (L, V) is tick i % ticks of window i // ticks
    L = n * ticks
    seq = v0.reshape(L, V)
    snd = on.reshape(L, V)
    pitch = np.where(snd, idx.reshape(L, V).astype(np.int64), -1)
    song_row0 = np.repeat(np.asarray(first).astype(np.int64) * ticks, ticks)          # the first row of the row's song
    at = np.arange(L)
    previous_pitch = np.full((L, V), -1, np.int64)
    previous_pitch[1:] = pitch[:-1]
    previous_pitch[at == song_row0] = -1
    loud = ~(seq.astype(np.float64) < thr)                                # "velocity is silent" is false
    last = np.maximum.accumulate(np.where(loud, at[:, None], -1), axis=0)
    before = np.full((L, V), -1, np.int64)                                # the nearest earlier loud row
    before[1:] = last[:-1]
    inside = before >= song_row0[:, None]
    previous_velocity = np.where(inside, np.take_along_axis(seq, np.maximum(before, 0), axis=0), np.float32(0))
    inherit = ~loud & snd & (previous_pitch > 0) & (previous_pitch != pitch)
    return np.where(inherit, previous_velocity, np.where(loud & ~snd, np.float32(0), seq)).astype(np.float32).reshape(n, T)
