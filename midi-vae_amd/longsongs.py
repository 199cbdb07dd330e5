"""Long songs (reference vae_evaluation.py:1821-1896): from a random code R every iteration searches the training codes ``all_z`` for
the nearest one not picked before, pulls R towards it, decodes one window from R with the previous R as history, turns the decoded window
back into encoder input and encodes it - the next R.

``nearest_walk`` is one iteration's search and pull for S songs at once, ``feedback_rows`` a decoded batch as the encoder's next input;
both run on the device (``mvae_nearest_walk`` / ``mvae_feedback_rows``, include/midivae_longsong.h) or, with ``device=False``, through
the NumPy mirrors below, which state the kernels' arithmetic: the squared distance is a double sum in ascending column order (the
reference's np.linalg.norm is a float32 BLAS sum whose order is its own - tests/golden/long_songs.npz holds only searches whose winner
is decisive against that), the pull is NumPy's own separately rounded steps in the type of R.  ``walk_reference`` restates the
reference's loop (:1844-1862) as it stands, for one song, with a callable in place of decode and encode.

``den`` is ``1 + e`` as the HOST's NumPy forms it for the ``e`` it is given: an np.float32 (the reference's z_std_train = np.std(all_z))
gives a float32 or a float64 sum depending on NumPy's promotion rules, so the kernel takes the value and never forms it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import hiplib as hl
from . import reconstruction as rec
from .rolls import check_rows, device_roll, host_roll

MAX_Z = 4096
MAX_T = 65536
ROW_CHUNK = 256          # rows of all_z a workgroup of the search takes
SONG_GROUP = 8           # songs whose codes it holds


# ---- the reference's loop, as it stands --------------------------------------------------------------------------------------------
def walk_reference(all_z, code, length, e, step=None):
    """:1844-1862 for ONE song: ``code`` (Z,) or (1, Z) the start code, ``step(it, R, previous)`` -> the next R (what decode and encode
    make of the pulled R and the history; None: the pulled R goes on).  dict ``picked`` (length,), ``distances`` (length,), ``z``
    (length, Z): the pulled codes, in the type NumPy gives them, as a list of (1, Z) arrays under ``rows``."""
    R = np.asarray(code).reshape(1, -1)
    previous_latent_rep = np.zeros(R.shape)
    already_picked_z_indices, distances, rows = [], [], []
    for it in range(int(length)):
        lowest_distance = np.linalg.norm(all_z[0] - R)
        best_z_index = 0
        for i, z in enumerate(all_z):
            distance = np.linalg.norm(z - R)
            if distance < lowest_distance and i not in already_picked_z_indices:
                lowest_distance = distance
                best_z_index = i
        already_picked_z_indices.append(best_z_index)
        closest_z = all_z[best_z_index]
        R = (R + closest_z * e) / (1 + e)
        distances.append(float(lowest_distance))
        rows.append(R)
        nxt = R if step is None else np.asarray(step(it, R, previous_latent_rep)).reshape(1, -1)
        previous_latent_rep = R
        R = nxt
    return dict(picked=np.asarray(already_picked_z_indices, np.int64), distances=np.asarray(distances, np.float64), rows=rows,
                z=np.concatenate([r.astype(np.float32) for r in rows], 0) if rows else np.zeros((0, R.shape[1]), np.float32))


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def pull_factors(e):
    """(e, den) as the two doubles the kernel takes: ``den`` is ``1 + e`` formed by NumPy in e's own type"""
    e_d, den = float(e), float(1 + e)
    if not math.isfinite(e_d) or not math.isfinite(den) or den == 0.0:
        raise ValueError("the pull needs a finite e and a finite, non-zero 1 + e, got e = %r" % (e,))
    return e_d, den


def _host_codes(R, what):
    R = np.asarray(R)
    if R.dtype not in (np.float32, np.float64):
        R = R.astype(np.float64)
    if R.ndim != 2 or R.shape[0] <= 0:
        raise ValueError("%s are (S > 0, Z), got %r" % (what, R.shape))
    return R


def _check_walk(all_z, R, picked):
    if all_z.ndim != 2 or all_z.shape[0] <= 0 or not 1 <= all_z.shape[1] <= MAX_Z:
        raise ValueError("all_z is (N > 0, Z) with Z in 1..%d, got %r" % (MAX_Z, all_z.shape))
    if R.shape[1] != all_z.shape[1]:
        raise ValueError("the codes have %d columns, all_z %d" % (R.shape[1], all_z.shape[1]))
    picked = np.asarray(picked, np.int64).reshape(R.shape[0], -1) if np.size(picked) else np.zeros((R.shape[0], 0), np.int64)
    if picked.size and (picked.min() < 0 or picked.max() >= all_z.shape[0]):
        raise ValueError("picked holds an index outside all_z")
    return picked


# ---- the NumPy mirrors -------------------------------------------------------------------------------------------------------------
def _mirror_search(A64, r, mine):
    """(winner, d2) of one song: A64 all_z as doubles, r (Z,), mine the indices picked so far"""
    diff = A64 - r.astype(np.float64)[None, :]
    with np.errstate(all="ignore"):
        d2 = np.cumsum(diff * diff, axis=1)[:, -1]          # (cumsum: one addition after the other, in column order)
    if np.isnan(d2[0]):
        return 0, d2[0]
    candidate = np.ones(len(d2), bool)
    candidate[np.asarray(mine, np.int64)] = False
    candidate[0] = True
    idx = np.nonzero(candidate & ~np.isnan(d2))[0]
    w = int(idx[np.argmin(d2[idx])])          # (the first minimum: the smallest index)
    return w, d2[w]


def _mirror_pull(all_z, R, winners, e, den):
    prod = all_z[winners] * np.float32(e)
    with np.errstate(all="ignore"):
        if R.dtype == np.float32:
            return (R + prod) / np.float32(den)
        return (R + prod.astype(np.float64)) / np.float64(den)


def _mirror_walk(all_z, R, picked, e, den):
    A64 = all_z.astype(np.float64)
    found = [_mirror_search(A64, R[s], picked[s]) for s in range(R.shape[0])]
    best = np.asarray([w for w, _ in found], np.int32)
    with np.errstate(all="ignore"):
        dist = np.sqrt(np.asarray([d for _, d in found], np.float64))
    r = _mirror_pull(all_z, R, best, e, den)
    return best, dist, r


def workspace_bytes(N, S, Z):
    return int(hl.load().mvae_nearest_walk_workspace(int(N), int(S), int(Z)))


def enqueue_walk(all_z, r_in, hist_in, picked, n_picked, e, den, workspace, best_out, dist_out, z_out, r_out, hist_out, stream):
    """mvae_nearest_walk on device memory the caller owns: ``all_z`` (N, Z) float32, ``r_in`` (S, Z) float32 or float64, ``hist_in`` the
    same or None, ``picked`` (S, cap) int32 contiguous, ``z_out`` / ``hist_out`` float32 and ``r_out`` of r_in's type - 2-D views with
    unit column stride and any row pitch - ``best_out`` (S,) int32, ``dist_out`` (S,) float64, ``workspace`` a byte tensor"""
    import torch
    N, Z = int(all_z.shape[0]), int(all_z.shape[1])
    S = int(r_in.shape[0])
    for t in (all_z, r_in, hist_in, z_out, r_out, hist_out):
        if t is not None and (t.dim() != 2 or t.shape[1] < Z or t.stride(1) != 1):
            raise ValueError("codes are 2-D views of at least %d columns with unit column stride" % Z)
    if all_z.dtype != torch.float32 or r_out.dtype != r_in.dtype or z_out.dtype != torch.float32 or picked.dtype != torch.int32:
        raise ValueError("all_z and z_out are float32, r_out has r_in's type, picked is int32")
    ld = lambda t: 0 if t is None else (int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), Z))
    a = hl.WalkArgs(all_z=all_z.data_ptr(), r_in=r_in.data_ptr(), hist_in=hl.ptr(hist_in), picked=picked.data_ptr(),
                    workspace=workspace.data_ptr(), N=N, S=S, Z=Z, ld_all=ld(all_z), ld_r=ld(r_in), r_f64=int(r_in.dtype == torch.float64),
                    ld_hist_in=ld(hist_in), hist_f64=int(hist_in is not None and hist_in.dtype == torch.float64),
                    cap=int(picked.shape[1]), n_picked=int(n_picked), ld_z=ld(z_out), ld_rout=ld(r_out), ld_hist=ld(hist_out), e=e, den=den,
                    best_out=best_out.data_ptr(), dist_out=dist_out.data_ptr(), z_out=z_out.data_ptr(), r_out=r_out.data_ptr(),
                    hist_out=hl.ptr(hist_out))
    hl.check(hl.load().mvae_nearest_walk(C.byref(a), stream), "mvae_nearest_walk")


def nearest_walk(all_z, R, picked, e, device=True, den=None):
    """One iteration's search and pull for S songs.  ``all_z`` (N, Z) float32, ``R`` (S, Z) float32 or float64 the songs' codes,
    ``picked`` (S, k) the indices every song has picked so far (k the same for all: they run in lockstep; k = 0: an empty list),
    ``e`` the pull's weight (the reference's z_std_train, np.std(all_z)); ``den``: 1 + e if the caller has formed it.  dict ``best``
    (S,) int32, ``distances`` (S,) float64, ``z`` (S, Z) float32 what the decoder reads, ``r`` (S, Z) in R's type the pulled code
    unrounded, ``picked`` (S, k + 1)."""
    all_z = np.asarray(all_z)
    if all_z.dtype != np.float32:
        raise ValueError("all_z is float32 (what encoder.predict returns), got %s" % all_z.dtype)
    R = _host_codes(R, "the codes")
    picked = _check_walk(all_z, R, picked)
    e_d, den_d = pull_factors(e) if den is None else (float(e), float(den))
    if not math.isfinite(e_d) or not math.isfinite(den_d) or den_d == 0.0:
        raise ValueError("the pull needs a finite e and a finite, non-zero den")
    S, Z = R.shape
    k = picked.shape[1]
    if not device:
        best, dist, r = _mirror_walk(all_z, R, picked, e_d, den_d)
    else:
        import torch
        dev = torch.device("cuda")
        with torch.cuda.device(dev):
            A = torch.from_numpy(np.ascontiguousarray(all_z)).to(dev)
            r_in = torch.from_numpy(np.ascontiguousarray(R)).to(dev)
            pk = torch.zeros((S, k + 1), dtype=torch.int32, device=dev)
            pk[:, :k].copy_(torch.from_numpy(picked.astype(np.int32)))
            ws = torch.empty(workspace_bytes(all_z.shape[0], S, Z), dtype=torch.uint8, device=dev)
            best_d = torch.empty(S, dtype=torch.int32, device=dev)
            dist_d = torch.empty(S, dtype=torch.float64, device=dev)
            z_d = torch.empty((S, Z), dtype=torch.float32, device=dev)
            r_d = torch.empty_like(r_in)
            enqueue_walk(A, r_in, None, pk, k, e_d, den_d, ws, best_d, dist_d, z_d, r_d, None, torch.cuda.current_stream().cuda_stream)
            best, dist, r = best_d.cpu().numpy(), dist_d.cpu().numpy(), r_d.cpu().numpy()
    return dict(best=best, distances=dist, z=r.astype(np.float32), r=r, picked=np.concatenate([picked, best[:, None].astype(np.int64)], 1))


# ---- feedback ----------------------------------------------------------------------------------------------------------------------
def params(s):
    """what the feedback reads from the settings: reconstruction.params"""
    return rec.params(s)


def _check(T, p):
    check_rows(T, p, MAX_T, "feedback")


def _mirror_feedback(idx, vel, held, instr, p):
    n = idx.shape[0]
    velocity, starts, _ = rec._mirror(idx, vel, held, None, np.arange(n), p)          # (every window a song of its own)
    return dict(x=idx.copy(), x_rev=idx[:, ::-1].copy(), vel=velocity, held=starts, instr=None if instr is None else instr.copy())


def enqueue_feedback(idx, vel, held, instr, p, ld_out, x_out, x_rev_out, vel_out, held_out, instr_out, stream):
    """mvae_feedback_rows on device memory the caller owns.  ``idx`` (n, T) uint8 tensor of any strides (a time-major buffer: the
    transposed view), ``vel`` float32 / ``held`` uint8 of the same strides or None, ``instr`` (n, voices) uint8 of any strides or None;
    the outputs time-major (T, ld_out) / (voices, ld_out) contiguous tensors or None"""
    n, T = idx.shape
    a = hl.FeedbackArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), vel=hl.ptr(vel), held_idx=hl.ptr(held),
                        instr=hl.ptr(instr), instr_stride_v=0 if instr is None else instr.stride(1),
                        instr_stride_w=0 if instr is None else instr.stride(0), n=n, T=T, voices=p["voices"], silent=p["silent"],
                        n_pitch=p["n_pitch"], override_rules=int(p["override"]), threshold=p["threshold"], ld_out=int(ld_out),
                        x_out=hl.ptr(x_out), x_rev_out=hl.ptr(x_rev_out), vel_out=hl.ptr(vel_out), held_out=hl.ptr(held_out),
                        instr_out=hl.ptr(instr_out))
    hl.check(hl.load().mvae_feedback_rows(C.byref(a), stream), "mvae_feedback_rows")


def feedback_rows(notes, velocity, held, instr, s, device=True):
    """A decoded batch as the encoder receives it next: ``notes`` (n, T) uint8 indices, ``velocity`` (n, T) float32 or None, ``held``
    (n, T) held-notes indices or None, ``instr`` (n, max_voices) instrument indices or None - host arrays, or 2-D device tensors of any
    strides (velocity and held with the strides of notes).  dict, window-major host arrays: ``x`` (n, T) uint8, ``x_rev`` the rows
    reversed, ``vel`` (n, T) float32 after the rule restarted in every window, ``held`` (n, T) uint8 (1 = held), ``instr`` (or None)."""
    p = params(s)
    if not device:
        a = host_roll(notes, np.uint8, "notes")
        _check(a.shape[1], p)
        i = None if instr is None else host_roll(instr, np.uint8, "instruments", (a.shape[0], p["voices"]))
        return _mirror_feedback(a, host_roll(velocity, np.float32, "velocities", a.shape), host_roll(held, np.uint8, "held notes", a.shape), i, p)
    import torch
    t = device_roll(notes, torch.uint8, "notes")
    n, T = t.shape
    _check(T, p)
    fix = lambda x: x if x is None or (x.stride(0) > 0 and x.stride(1) > 0) else x.contiguous()
    t = fix(t)
    v = device_roll(velocity, torch.float32, "velocities", t.shape, device=t.device)
    h = device_roll(held, torch.uint8, "held notes", t.shape, device=t.device)
    if v is not None and v.stride() != t.stride():
        v = torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device).copy_(v)
    if h is not None and h.stride() != t.stride():
        h = torch.empty_strided(t.shape, t.stride(), dtype=torch.uint8, device=t.device).copy_(h)
    i = fix(device_roll(instr, torch.uint8, "instruments", (n, p["voices"]), device=t.device))
    dev = t.device
    with torch.cuda.device(dev):
        x = torch.empty((T, n), dtype=torch.uint8, device=dev)
        xr, hd = torch.empty_like(x), torch.empty_like(x)
        vo = torch.empty((T, n), dtype=torch.float32, device=dev)
        io = None if i is None else torch.empty((p["voices"], n), dtype=torch.uint8, device=dev)
        enqueue_feedback(t, v, h, i, p, n, x, xr, vo, hd, io, torch.cuda.current_stream().cuda_stream)
        back = lambda o: None if o is None else o.t().contiguous().cpu().numpy()
        return dict(x=back(x), x_rev=back(xr), vel=back(vo), held=back(hd), instr=back(io))
