"""Piano-roll images of decoded songs (reference vae_evaluation.py:619-642, ``prepare_for_drawing``, followed by
data_class.monophonic_to_khot_pianoroll): per tick and pitch the grey level of the notes the voices display - a struck row gets a
level from its velocity, a held row inherits the level of the row one tick earlier.

``images`` runs on the device (``mvae_pianoroll``, include/midivae_generate.h: one lane per window and voice, one launch, no lane
waits for another workgroup) or, with ``device=False``, through the NumPy mirror below, the closed form of the reference's row-by-row
recursion.  Every level is one subtraction and one multiplication in double and a cell the sum of at most max_voices of them in voice
order: device, mirror and reference are BIT-EQUAL (tests/golden/generation.npz).  ``write_png`` / ``read_png`` store an image as an
8-bit greyscale PNG with nothing but zlib and struct; no parity with matplotlib's rendering is claimed - only the array is the
reference's.

``s`` is a settings mapping or module read like packers._g does: max_voices, low_crop, high_crop, include_silent_note,
velocity_threshold_such_that_it_is_a_played_note, MAX_VELOCITY.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib

import numpy as np

from . import hiplib as hl
from .packers import _g
from .reconstruction import first_windows
from .rolls import as_rolls, base_params, check_rows, device_roll, host_roll, sounding, with_strides_of

MAX_T = 65536


def params(s):
    """what the image reads from the settings"""
    return dict(base_params(s), threshold=float(_g(s, "velocity_threshold_such_that_it_is_a_played_note")),
                max_velocity=float(_g(s, "MAX_VELOCITY")))


def _check(T, p):
    check_rows(T, p, MAX_T, "piano-roll image")
    if not 1 <= p["n_pitch"] <= 192:
        raise ValueError("%d pitch columns: the piano-roll image takes 1..192" % p["n_pitch"])
    if not math.isfinite(p["max_velocity"]):
        raise ValueError("MAX_VELOCITY must be finite")


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _mirror(idx, vel, first, p):
    """(n * T / voices, n_pitch) float64, tick-major"""
    n, T = idx.shape
    V, K = p["voices"], p["n_pitch"]
    ticks = T // V
    L = n * ticks
    on = sounding(idx, p).reshape(L, V)
    pitch = np.where(on, idx.reshape(L, V).astype(np.int64), -1)
    img = np.zeros((L, K))
    at = np.arange(L)
    if vel is None:
        for v in range(V):
            sel = on[:, v]
            img[at[sel], pitch[sel, v]] = 1.0
        return img
    velocity = vel.astype(np.float32).astype(np.float64).reshape(L, V)
    struck = velocity > p["threshold"]
    cur = np.where(on, pitch, 0)
    song_row0 = np.repeat(np.asarray(first).astype(np.int64) * ticks, ticks)
    # step = (row - song_row0) * V + v: a row that is not struck may inherit if step > V
    step = (at - song_row0)[:, None] * V + np.arange(V)[None, :]
    # a row LINKS to the row one tick earlier if it is not struck, step > V and both share cur; the chain a row sits on reaches
    # back to the nearest row that does not link: what that row displays, the whole chain displays
    links = np.zeros((L, V), bool)
    links[1:] = ~struck[1:] & (step[1:] > V) & (cur[1:] == cur[:-1])
    head = np.maximum.accumulate(np.where(links, -1, at[:, None]), axis=0)          # the chain's first row
    shows = np.take_along_axis(struck & on, head, axis=0)                            # a head displays iff it is struck and sounds
    with np.errstate(all="ignore"):
        level = np.take_along_axis((velocity - p["threshold"]) * p["max_velocity"], head, axis=0)
    for v in range(V):                                                                # ascending voice order, from 0.0
        sel = shows[:, v]
        np.add.at(img, (at[sel], cur[sel, v]), level[sel, v])
    return img


# ---- the device path -----------------------------------------------------------------------------------------------------------
def enqueue(idx, vel, first, p, img_out, stream):
    """mvae_pianoroll on device memory the caller owns: ``idx`` (n, T) uint8 tensor of any positive strides, ``vel`` a float32 tensor
    of the same strides or None, ``first`` (n,) int32 or None, ``img_out`` (n * T / voices, >= n_pitch) float64 with unit column
    stride"""
    n, T = idx.shape
    a = hl.PianorollArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), vel=hl.ptr(vel), first_window=hl.ptr(first),
                         n=n, T=T, voices=p["voices"], silent=p["silent"], n_pitch=p["n_pitch"], ld_img=img_out.stride(0),
                         threshold=p["threshold"], max_velocity=p["max_velocity"], img_out=img_out.data_ptr())
    hl.check(hl.load().mvae_pianoroll(C.byref(a), stream), "mvae_pianoroll")


def run_on_device(idx, vel, first, p):
    """``enqueue`` with an output of its own on the current stream of ``idx``'s device: the (n * T / voices, n_pitch) float64 tensor"""
    import torch
    n, T = idx.shape
    dev = idx.device
    if idx.stride(0) <= 0 or idx.stride(1) <= 0:
        idx = idx.contiguous()
    vel = with_strides_of(idx, vel)
    img = torch.empty((n * (T // p["voices"]), p["n_pitch"]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        enqueue(idx, vel, first, p, img, torch.cuda.current_stream().cuda_stream)
    return img


def split_songs(img, lengths, ticks):
    """the tick-major image of a run -> per song the reference's (n_pitch, ticks of the song) array"""
    out, lo = [], 0
    for m in lengths:
        out.append(np.ascontiguousarray(img[lo * ticks:(lo + m) * ticks].T))
        lo += m
    return out


def images(idx, vel, lengths, s, device=True):
    """The piano-roll images of ``n`` windows that form ``len(lengths)`` songs (``lengths``: the songs' window counts, in order).
    ``idx`` (n, T) uint8 index rolls or (n, T, K) one-hot rolls, ``vel`` (n, T) float velocities (read as float32) or None for the
    reference's ``V=None`` - host arrays, or 2-D device tensors of any strides.  One (n_pitch, song ticks) float64 array per song,
    pitch index 0 in row 0: what ``prepare_for_drawing`` returns for the song."""
    p = params(s)
    if device:
        import torch
        if not hasattr(idx, "data_ptr"):
            idx = as_rolls(idx)
        if len(idx.shape) != 2:
            raise ValueError("notes are (n, T) index rolls, got shape %r" % (tuple(idx.shape),))
        n, T = idx.shape
        _check(T, p)
        first = first_windows(lengths, n)
        t = device_roll(idx, torch.uint8, "notes")
        v = device_roll(vel, torch.float32, "velocities", t.shape, device=t.device)
        if n == 0:
            return []
        with torch.cuda.device(t.device):
            img = run_on_device(t, v, torch.from_numpy(first).to(t.device), p).cpu().numpy()
    else:
        a = host_roll(idx, np.uint8, "notes")
        n, T = a.shape
        _check(T, p)
        first = first_windows(lengths, n)
        img = _mirror(a, host_roll(vel, np.float32, "velocities", a.shape), first, p)
    return split_songs(img, [int(m) for m in np.asarray(lengths).reshape(-1)], T // p["voices"])


def prepare_for_drawing(Y, V=None, s=None):
    """the reference's function on the mirror: ``Y`` (rows, n_pitch) one-hot rows of ONE song (an all-zero row does not sound), ``V``
    (rows,) velocities or None; (n_pitch, rows / max_voices) float64.  ``s``: the settings (None: config.build_settings())."""
    if s is None:
        from .config import build_settings
        s = build_settings()
    Y = np.asarray(Y)
    p = params(s)
    if Y.ndim != 2 or Y.shape[1] != p["n_pitch"] or Y.shape[0] % p["voices"]:
        raise ValueError("Y is (rows, %d) with whole ticks of %d voices, got %r" % (p["n_pitch"], p["voices"], Y.shape))
    idx = np.where(Y.any(1), Y.argmax(1), 255).astype(np.uint8).reshape(1, -1)
    vel = None if V is None else np.asarray(V).reshape(1, -1)
    if idx.shape[1] == 0:
        return np.zeros((p["n_pitch"], 0))
    return _mirror(idx, None if vel is None else vel.astype(np.float32), np.zeros(1, np.int32), p).T.copy()


def difference_image(a, b):
    """``a + 2 * b`` on binary images: 1 only in a, 2 only in b, 3 in both"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError("shape mismatch: %r and %r" % (a.shape, b.shape))
    return (a != 0).astype(np.float64) + 2.0 * (b != 0)


# ---- PNG ---------------------------------------------------------------------------------------------------------------------------
_PNG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def grey_levels(image, vmax=None):
    """(pitches, ticks) uint8: 255 (white) for 0, 0 (black) for ``vmax`` and above (default: the image's maximum, as draw_pianoroll
    scales), linear between and rounded half up; NaN and negative cells are white"""
    image = np.asarray(image, np.float64)
    if image.ndim != 2:
        raise ValueError("an image is (pitches, ticks)")
    top = float(image.max()) if vmax is None and image.size else vmax
    if top is None or not top > 0:
        top = 1.0
    x = np.clip(np.nan_to_num(image, nan=0.0) / top, 0.0, 1.0)
    return (255 - np.floor(x * 255.0 + 0.5)).astype(np.uint8)


def write_png(path, image, vmax=None):
    """``image`` (pitches, ticks) as an 8-bit greyscale PNG, pitch 0 on the bottom row"""
    g = grey_levels(image, vmax)[::-1]
    h, w = g.shape
    if h == 0 or w == 0:
        raise ValueError("an empty image cannot be written")
    raw = b"".join(b"\x00" + g[r].tobytes() for r in range(h))
    with open(path, "wb") as f:
        f.write(_PNG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw, 9)) +
                _chunk(b"IEND", b""))


def read_png(path):
    """the (pitches, ticks) uint8 grey levels of a file ``write_png`` wrote, pitch 0 in row 0; every chunk's CRC is checked"""
    data = open(path, "rb").read()
    if data[:8] != _PNG:
        raise ValueError("not a PNG file")
    at, head, body = 8, None, b""
    while at < len(data):
        (size,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        chunk = data[at + 8:at + 8 + size]
        if struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] != zlib.crc32(kind + chunk) & 0xFFFFFFFF:
            raise ValueError("chunk %r fails its CRC" % kind)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", chunk)
        elif kind == b"IDAT":
            body += chunk
        at += 12 + size
    if head is None or head[2:] != (8, 0, 0, 0, 0):
        raise ValueError("not an 8-bit greyscale PNG without interlace")
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(body), np.uint8).reshape(h, w + 1)
    if raw[:, 0].any():
        raise ValueError("a filtered scanline: not written by write_png")
    return raw[::-1, 1:].copy()
