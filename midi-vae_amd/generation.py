"""Interpolation songs and medleys (reference vae_evaluation.py:578-584, :705-887): a generated song is a few anchor codes plus a
recipe.  Window w is ``A[a0[w]] * c0[w] + A[a1[w]] * c1[w]`` (or, with ``a1[w] < 0``, a copy of ``A[a0[w]]``) and its history is the
window before it, zeros at a song's first window.

A PATH is a dict ``anchors`` (m, Z) float32 or float64 - a host array or a device tensor - and the table ``a0``, ``a1`` (int32),
``c0``, ``c1`` (float64), one entry per window.  ``interpolation_path`` and ``medley_path`` build one song, ``concat_paths`` joins
songs into a RUN (the same keys plus ``first_window`` and ``lengths``).  ``latent_rows`` turns windows of a run into the float32 rows
the decoder reads, on the device (``mvae_latent_paths``, include/midivae_generate.h: one lane per element, written in place with any
row pitch) or, with ``device=False``, through the NumPy mirror - both BIT-EQUAL to what NumPy makes of the reference's
``p0 * (1.0 - t) + p1 * t`` with a Python float t (float32 arithmetic on the float32 codes encoder.predict returns, float64 on
np.random.normal codes) followed by the float32 cast of the decoder's input; tests/golden/generation.npz pins them to the
reference's own functions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hiplib as hl

MAX_Z = 4096


# ---- the reference's two helpers (vae_evaluation.py:578-584) --------------------------------------------------------------------
def slerp(p0, p1, t):
    omega = np.arccos(np.dot(p0 / np.linalg.norm(p0), p1 / np.linalg.norm(p1)))
    so = np.sin(omega)
    return np.sin((1.0 - t) * omega) / so * p0 + np.sin(t * omega) / so * p1


def linear_interpolation(p0, p1, t):
    return p0 * (1.0 - t) + p1 * t


# ---- paths -----------------------------------------------------------------------------------------------------------------------
def _is_device(a):
    return hasattr(a, "data_ptr")


def _coefficients(mode, p0, p1, t):
    """the two factors the reference's expression multiplies p0 and p1 with at ``t``, as Python floats"""
    if mode == "lerp":
        return 1.0 - t, t
    if mode != "slerp":
        raise ValueError("unknown mode %r: 'lerp' or 'slerp'" % (mode,))
    if p0 is None:
        raise ValueError("mode='slerp' computes its coefficients on the host: pass host anchors")
    # the reference's expression under the installed NumPy: with float32 codes omega and both factors are float32 scalars
    omega = np.arccos(np.dot(p0 / np.linalg.norm(p0), p1 / np.linalg.norm(p1)))
    so = np.sin(omega)
    return float(np.sin((1.0 - t) * omega) / so), float(np.sin(t * omega) / so)


def _table(rows):
    a0, a1, c0, c1 = zip(*rows) if rows else ((), (), (), ())
    return dict(a0=np.asarray(a0, np.int32), a1=np.asarray(a1, np.int32), c0=np.asarray(c0, np.float64), c1=np.asarray(c1, np.float64))


def _host_code(a):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return a


def interpolation_path(code_a, code_b, length, mode="lerp"):
    """the ``length + 1`` windows of a random interpolation song (:864-874): window i is the blend of the two codes ((Z,) or (1, Z))
    at t = i / float(length)"""
    length = int(length)
    if length <= 0:
        raise ValueError("interpolation length must be positive")
    a, b = _host_code(code_a).reshape(-1), _host_code(code_b).reshape(-1)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("the two codes differ in shape or type: %r %s, %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    rows = [(0, 1) + _coefficients(mode, a, b, i / float(length)) for i in range(length + 1)]
    return dict(_table(rows), anchors=np.stack([a, b]))


def code_path(code):
    """a song of ONE window that is the code itself ((Z,) or (1, Z); reference vae_evaluation.py:1776-1779): a copy row, no blend"""
    return dict(_table([(0, -1, 1.0, 0.0)]), anchors=_host_code(code).reshape(1, -1))


def medley_path(Rs, interpolation_length, mode="lerp"):
    """a medley (:731-822): the rows of ``Rs[0]``, then for every later song ``interpolation_length`` bridge windows from the previous
    song's LAST row to this song's FIRST row at t = i / float(interpolation_length), i = 0.., then its own rows.  ``Rs``: (m_i, Z)
    host arrays, or device tensors of one type (``mode='lerp'`` only)"""
    L = int(interpolation_length)
    if L < 0 or not len(Rs):
        raise ValueError("a medley needs songs and a bridge length >= 0")
    on_device = _is_device(Rs[0])
    if on_device:
        import torch
        if any(not _is_device(R) or R.dim() != 2 or R.shape[0] <= 0 or R.dtype != Rs[0].dtype for R in Rs):
            raise ValueError("device latents are 2-D tensors (m > 0, Z) of one type")
        anchors = torch.cat(list(Rs), 0)
        host = None
    else:
        Rs = [_host_code(R) for R in Rs]
        if any(R.ndim != 2 or R.shape[0] <= 0 or R.shape[1] != Rs[0].shape[1] or R.dtype != Rs[0].dtype for R in Rs):
            raise ValueError("latents are (m > 0, Z) arrays of one type")
        anchors = host = np.concatenate(Rs, 0)
    rows, off = [], 0
    for k, R in enumerate(Rs):
        m = int(R.shape[0])
        if k:
            p0, p1 = (None, None) if host is None else (host[off - 1], host[off])
            rows += [(off - 1, off) + _coefficients(mode, p0, p1, i / float(L)) for i in range(L)]
        rows += [(off + r, -1, 1.0, 0.0) for r in range(m)]
        off += m
    return dict(_table(rows), anchors=anchors)


def concat_paths(paths):
    """many songs as one run: the anchors stacked, the tables joined, ``first_window`` (n,) int32 and ``lengths``"""
    paths = list(paths)
    if not paths:
        raise ValueError("no path")
    on_device = _is_device(paths[0]["anchors"])
    if any(_is_device(p["anchors"]) != on_device or p["anchors"].dtype != paths[0]["anchors"].dtype for p in paths):
        raise ValueError("the anchors of a run are all host arrays or all device tensors, of one type")
    if on_device:
        import torch
        anchors = torch.cat([p["anchors"] for p in paths], 0)
    else:
        anchors = np.concatenate([p["anchors"] for p in paths], 0)
    lengths = [len(p["a0"]) for p in paths]
    if min(lengths) <= 0:
        raise ValueError("every song needs at least one window")
    offs = np.cumsum([0] + [int(p["anchors"].shape[0]) for p in paths[:-1]])
    starts = np.cumsum(lengths) - lengths
    return dict(anchors=anchors,
                a0=np.concatenate([p["a0"] + o for p, o in zip(paths, offs)]).astype(np.int32),
                a1=np.concatenate([np.where(p["a1"] >= 0, p["a1"] + o, -1) for p, o in zip(paths, offs)]).astype(np.int32),
                c0=np.concatenate([p["c0"] for p in paths]), c1=np.concatenate([p["c1"] for p in paths]),
                first_window=np.repeat(starts, lengths).astype(np.int32), lengths=lengths)


def medley_samples(lengths, songs_per_medley, noninterpolated, rng):
    """the song and sample choice of one medley (:735-764) from the window counts of the set's songs, drawing from ``rng`` (a
    np.random.RandomState) in the reference's order: a song of more than ``noninterpolated`` windows, then a sample, clamped to
    ``noninterpolated`` from below for the first song of the medley, else to ``length - noninterpolated - 1`` from above.  List of
    (song, sample, range of the windows taken) - the windows BEFORE the sample for the first song, from the sample on for the
    others.  (For the first song the second clamp can leave a range that starts below zero; NumPy then indexes from the end, as
    it does in the reference.)"""
    lengths = [int(m) for m in lengths]
    k = int(noninterpolated)
    if k <= 0:
        raise ValueError("noninterpolated_samples_between_interpolation must be positive")          # (:711)
    if not any(m > k for m in lengths):
        raise ValueError("no song has more than %d windows" % k)
    out = []
    for medley_song_num in range(int(songs_per_medley)):
        song_num = rng.randint(len(lengths))
        while lengths[song_num] <= k:
            song_num = rng.randint(len(lengths))
        sample_num = rng.randint(lengths[song_num])
        if sample_num < k and medley_song_num == 0:
            sample_num = k
        elif sample_num >= lengths[song_num] - k:
            sample_num = lengths[song_num] - k - 1
        sample_list = range(sample_num - k, sample_num) if medley_song_num == 0 else range(sample_num, sample_num + k)
        out.append((int(song_num), int(sample_num), sample_list))
    return out


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def _check_run(anchors, table, first_window, lo, count):
    n = len(table["a0"])
    if any(len(table[k]) != n for k in ("a1", "c0", "c1")) or (first_window is not None and len(first_window) != n):
        raise ValueError("a0, a1, c0, c1 and first_window hold one entry per window")
    if len(anchors.shape) != 2 or anchors.shape[0] <= 0 or not 1 <= anchors.shape[1] <= MAX_Z:
        raise ValueError("anchors are (m > 0, Z) with Z in 1..%d, got %r" % (MAX_Z, tuple(anchors.shape)))
    if n <= 0 or count <= 0 or lo < 0 or lo + count > n:
        raise ValueError("windows %d..%d of a run of %d" % (lo, lo + count, n))
    return n


def _mirror_values(A, t, ws):
    a0, a1 = t["a0"][ws].astype(np.int64), t["a1"][ws].astype(np.int64)
    ok = (a0 >= 0) & (a0 < A.shape[0]) & (a1 < A.shape[0])
    out = np.full((len(ws), A.shape[1]), np.nan, np.float32)
    copy, blend = ok & (a1 < 0), ok & (a1 >= 0)
    out[copy] = A[a0[copy]].astype(np.float32)
    k0, k1 = t["c0"][ws][blend].astype(A.dtype)[:, None], t["c1"][ws][blend].astype(A.dtype)[:, None]
    with np.errstate(all="ignore"):
        out[blend] = (A[a0[blend]] * k0 + A[a1[blend]] * k1).astype(np.float32)
    return out


def _mirror(A, t, first_window, lo, count):
    ws = np.arange(lo, lo + count)
    z = _mirror_values(A, t, ws)
    hist = np.zeros_like(z)
    if first_window is not None:
        carried = (ws > 0) & (np.asarray(first_window)[ws] < ws)
        hist[carried] = _mirror_values(A, t, ws[carried] - 1)
    return z, hist


def upload(run, device):
    """a run's anchors and table as device tensors (the anchors stay where they are if they are on the device already): what
    ``enqueue`` takes, uploaded once per run"""
    import torch
    A = run["anchors"]
    if _is_device(A):
        if A.dtype not in (torch.float32, torch.float64) or A.dim() != 2 or A.stride(1) != 1:
            raise ValueError("device anchors are a 2-D float32 or float64 tensor with unit column stride")
        device = A.device
    else:
        A = torch.from_numpy(np.ascontiguousarray(_host_code(A))).to(device)
    first = run.get("first_window")
    d = dict(anchors=A, n=len(run["a0"]))
    for k, dt in (("a0", np.int32), ("a1", np.int32), ("c0", np.float64), ("c1", np.float64)):
        d[k] = torch.from_numpy(np.ascontiguousarray(run[k], dt)).to(device)
    d["first_window"] = None if first is None else torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(device)
    return d


def enqueue(dev_run, lo, count, z_out, hist_out, stream):
    """mvae_latent_paths on device memory the caller owns: ``dev_run`` from ``upload``; ``z_out`` / ``hist_out`` 2-D float32 views of
    ``count`` rows with unit column stride and any row pitch (``hist_out`` may be None)"""
    import torch
    A = dev_run["anchors"]
    Z = int(A.shape[1])
    for o in (z_out, hist_out):
        if o is not None and (o.dtype != torch.float32 or o.dim() != 2 or o.shape[0] < count or o.shape[1] < Z or o.stride(1) != 1):
            raise ValueError("an output is a float32 view of at least (%d, %d) with unit column stride" % (count, Z))
    a = hl.PathsArgs(anchors=A.data_ptr(), a0=dev_run["a0"].data_ptr(), a1=dev_run["a1"].data_ptr(), c0=dev_run["c0"].data_ptr(),
                     c1=dev_run["c1"].data_ptr(), first_window=hl.ptr(dev_run["first_window"]), n=dev_run["n"], lo=lo, count=count, Z=Z,
                     n_anchors=int(A.shape[0]), ld_anchor=int(A.stride(0)) if A.shape[0] > 1 else Z, anchor_f64=int(A.dtype == torch.float64),
                     ld_z=int(z_out.stride(0)) if count > 1 else max(int(z_out.stride(0)), Z),
                     ld_hist=0 if hist_out is None else (int(hist_out.stride(0)) if count > 1 else max(int(hist_out.stride(0)), Z)),
                     z_out=z_out.data_ptr(), hist_out=hl.ptr(hist_out))
    hl.check(hl.load().mvae_latent_paths(C.byref(a), stream), "mvae_latent_paths")


def latent_rows(anchors, table, first_window=None, lo=0, count=None, device=True):
    """(z, history), two (count, Z) float32 host arrays: the decoder's rows of the windows ``lo .. lo + count - 1`` (default: to the
    end) of a run.  ``anchors`` (m, Z) float32 / float64 host array or device tensor, ``table`` a mapping with a0, a1, c0, c1 (a path
    or a run), ``first_window`` (n,) or None: every window is a song of its own, its history zeros."""
    n_all = len(table["a0"])
    count = n_all - lo if count is None else int(count)
    _check_run(anchors, table, first_window, int(lo), count)
    if not device:
        A = anchors.cpu().numpy() if _is_device(anchors) else _host_code(anchors)
        t = {k: np.asarray(table[k]) for k in ("a0", "a1", "c0", "c1")}
        return _mirror(A, t, first_window, int(lo), count)
    import torch
    run = upload(dict(anchors=anchors, first_window=first_window, **{k: table[k] for k in ("a0", "a1", "c0", "c1")}), "cuda")
    dev = run["anchors"].device
    Z = int(run["anchors"].shape[1])
    with torch.cuda.device(dev):
        z = torch.empty((count, Z), dtype=torch.float32, device=dev)
        hist = torch.empty((count, Z), dtype=torch.float32, device=dev)
        enqueue(run, int(lo), count, z, hist, torch.cuda.current_stream().cuda_stream)
        return z.cpu().numpy(), hist.cpu().numpy()
