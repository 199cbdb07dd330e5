"""Style-transfer scoring (reference vae_evaluation.py:110-117, :2075-2172, :2248-2340, :2448-2625): every window is judged by the
pitch, velocity and instrument style classifiers and by their weighted ensemble; per group of windows - a song, or a (song, target
class) pair - the accuracy and the confidence of each judge, and the confusion counts the classifier scripts print.

``scores`` runs on the device (``mvae_style_scores``, include/midivae_style.h: one workgroup per group) or, with ``device=False``,
through the NumPy mirror below - the same semantics written out in Python, the yardstick of the device tests.  Both are pinned to
the reference's own ``ensemble_prediction`` and to a restatement of its per-song counters by tests/golden/style_scores.npz.

Semantics.  Window w is judged by row w of ``p_pitch`` and ``p_vel`` and by row ``instr_row[w]`` of ``p_instr`` (row w without
``instr_row``: the reference judges a decoded window's instruments per window, an original song's once per song).  A table that is
None is an absent judge: NaN in the table, 255 in ``pred``.  The ensemble exists when all three are given and follows the
reference's float32 arithmetic operation by operation (``ensemble_prediction``).  Argmax is np.argmax.  A window whose ``cls`` is 255
(or no class at all) is judged but left out of its group's figures.  ``table`` columns are ``COLUMNS``; accuracy is an integer
count divided once, confidence the float32 probabilities of ``cls`` summed as doubles and divided once - the mirror sums with
math.fsum, so its mean is the exactly rounded one.  (The reference's ``+=`` on float32 scalars accumulates in float32 under NumPy 2
and widened to double under the NumPy of its day; double is what this module defines.)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import hiplib as hl

JUDGES = ("pitch", "velocity", "instrument", "ensemble")
COLUMNS = ("count",) + tuple("%s_%s" % (j, k) for j in JUDGES for k in ("accuracy", "confidence"))
N_COLUMNS = len(COLUMNS)
MIN_CLASSES, MAX_CLASSES = 2, 64
NONE = 255
REFERENCE_WEIGHT = 0.999 - 0.5          # vae_evaluation.py:81-91: "subtract 0.5 since you would want to weight a random model with 0"
DEFAULT_WEIGHTS = (REFERENCE_WEIGHT,) * 3


def ensemble_prediction(p_pitch, p_instr, p_vel, weights=DEFAULT_WEIGHTS):
    """the reference's expression (:116) on float32 tables with Python-float ``weights`` (pitch, instrument, velocity): every
    product, every sum and the division is one float32 operation, the denominator the weights' double sum rounded once"""
    w = [float(x) for x in weights]
    wp, wi, wv = (np.float32(x) for x in w)
    den = np.float32(w[0] + w[1] + w[2])
    p, i, v = (np.asarray(t, np.float32) for t in (p_pitch, p_instr, p_vel))
    with np.errstate(all="ignore"):
        return ((p * wp + i * wi) + v * wv) / den


def _check(n, C, tables, cls, group_off, weights):
    if all(t is None for t in tables):
        raise ValueError("no judge: all three probability tables are None")
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        raise ValueError("%d classes: style classes are %d..%d" % (C, MIN_CLASSES, MAX_CLASSES))
    if n <= 0 or len(group_off) < 2:
        raise ValueError("no windows or no groups")
    if len(cls) != n:
        raise ValueError("%d classes for %d windows" % (len(cls), n))
    return _weights(weights)


def _weights(weights):
    w = [float(x) for x in weights]
    if len(w) != 3 or not all(math.isfinite(x) for x in w) or not w[0] + w[1] + w[2] > 0:
        raise ValueError("weights must be three finite numbers with a sum > 0, got %r" % (weights,))
    return w


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _mirror(p_pitch, p_vel, p_instr, cls, group_off, instr_row, weights):
    n, C, G = len(cls), next(t.shape[1] for t in (p_pitch, p_vel, p_instr) if t is not None), len(group_off) - 1
    nan_rows = np.full((n, C), np.nan, np.float32)
    valid_i = np.zeros(n, bool)
    judged_i = None
    if p_instr is not None:
        rows = np.arange(n) if instr_row is None else np.asarray(instr_row, np.int64)
        valid_i = (rows >= 0) & (rows < p_instr.shape[0])
        judged_i = nan_rows.copy()
        judged_i[valid_i] = p_instr[rows[valid_i]]
    have_e = p_pitch is not None and p_vel is not None and p_instr is not None
    ens = ensemble_prediction(p_pitch, judged_i, p_vel, weights) if have_e else None
    per_judge = [(p_pitch, np.ones(n, bool)), (p_vel, np.ones(n, bool)), (judged_i, valid_i), (ens, valid_i)]
    pred = np.full((n, 4), NONE, np.uint8)
    for j, (p, valid) in enumerate(per_judge):
        if p is not None:
            pred[valid, j] = np.argmax(p[valid], axis=1) if valid.any() else 0
    table = np.full((G, N_COLUMNS), np.nan)
    confusion = np.zeros((4, C, C), np.int32)
    counted = cls < C
    for g in range(G):
        lo, hi = (min(max(int(x), 0), n) for x in group_off[g:g + 2])
        ws = [w for w in range(lo, hi) if counted[w]]
        table[g, 0] = len(ws)
        if not ws:
            continue
        k = cls[ws].astype(np.int64)
        for j, (p, valid) in enumerate(per_judge):
            if p is None:
                continue
            table[g, 1 + 2 * j] = float(int((pred[ws, j] == k).sum())) / float(len(ws))
            terms = [float(x) for x in p[ws, k]]
            table[g, 2 + 2 * j] = math.fsum(terms) / float(len(ws)) if not any(math.isnan(x) for x in terms) else np.nan
            seen = pred[ws, j] != NONE
            np.add.at(confusion[j], (k[seen], pred[ws, j][seen].astype(np.int64)), 1)
    return dict(ensemble=ens, pred=pred, table=table, confusion=confusion)


# ---- the device path -----------------------------------------------------------------------------------------------------------
def enqueue(p_pitch, p_vel, p_instr, cls, group_off, instr_row, weights, ens_out, pred_out, table_out, confusion_out, stream):
    """mvae_style_scores on device tensors the caller owns: float32 tables (rows strided, columns contiguous) or None, ``cls`` (n,)
    uint8, ``group_off`` (G + 1,) int32, ``instr_row`` (n,) int32 or None; outputs ``ens_out`` (n, >= C) float32, ``pred_out`` (n, 4)
    uint8, ``table_out`` (G, >= 9) float64, ``confusion_out`` (4, C, C) int32 zeroed by the caller, each or None"""
    given = [t for t in (p_pitch, p_vel, p_instr) if t is not None]
    for t in given + ([ens_out] if ens_out is not None else []):
        assert t.dim() == 2 and t.stride(1) == 1, "a probability table's columns must be contiguous"
    a = hl.StyleArgs(p_pitch=hl.ptr(p_pitch), p_vel=hl.ptr(p_vel), p_instr=hl.ptr(p_instr), instr_row=hl.ptr(instr_row),
                     cls=hl.ptr(cls), group_off=hl.ptr(group_off), n=cls.shape[0], C=given[0].shape[1] if given else 0,
                     n_groups=group_off.shape[0] - 1, n_instr_rows=0 if p_instr is None else p_instr.shape[0],
                     ld_pitch=0 if p_pitch is None else p_pitch.stride(0), ld_vel=0 if p_vel is None else p_vel.stride(0),
                     ld_instr=0 if p_instr is None else p_instr.stride(0), ld_ens=0 if ens_out is None else ens_out.stride(0),
                     ld_table=0 if table_out is None else table_out.stride(0), weights=(C.c_double * 3)(*[float(w) for w in weights]),
                     ens_out=hl.ptr(ens_out), pred_out=hl.ptr(pred_out), table_out=hl.ptr(table_out), confusion_out=hl.ptr(confusion_out))
    hl.check(hl.load().mvae_style_scores(C.byref(a), stream), "mvae_style_scores")


def device_scores(p_pitch, p_vel, p_instr, cls, group_off, instr_row=None, weights=DEFAULT_WEIGHTS):
    """``enqueue`` into fresh device tensors, on the current stream of the tables' device: dict of ``ensemble`` (n, C) float32 or
    None, ``pred`` (n, 4) uint8, ``table`` (G, 9) float64 and ``confusion`` (4, C, C) int32 - device tensors, nothing is read back"""
    import torch
    given = [t for t in (p_pitch, p_vel, p_instr) if t is not None]
    dev, Cn, n, G = given[0].device, given[0].shape[1], cls.shape[0], group_off.shape[0] - 1
    ens = torch.empty((n, Cn), dtype=torch.float32, device=dev) if len(given) == 3 else None
    pred = torch.empty((n, 4), dtype=torch.uint8, device=dev)
    table = torch.empty((G, N_COLUMNS), dtype=torch.float64, device=dev)
    confusion = torch.zeros((4, Cn, Cn), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        enqueue(p_pitch, p_vel, p_instr, cls, group_off, instr_row, weights, ens, pred, table, confusion,
                torch.cuda.current_stream().cuda_stream)
    return dict(ensemble=ens, pred=pred, table=table, confusion=confusion)


def _on_device(x, dtype, device):
    import torch
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)
    return t if t.dim() < 2 or t.stride(-1) == 1 else t.contiguous()


def _on_host(x, dtype):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype)


def scores(p_pitch, p_vel, p_instr, cls, group_off, instr_row=None, weights=DEFAULT_WEIGHTS, device=True):
    """the judges' figures of ``n`` windows in ``G`` groups.  ``p_pitch`` / ``p_vel`` (n, C) and ``p_instr`` (rows, C): float32
    probabilities as host arrays or device tensors, or None for an absent judge; ``cls`` (n,) the class a window is scored against
    (255: not counted); ``group_off`` (G + 1,) ascending from 0 to n; ``instr_row`` (n,) the row of ``p_instr`` per window (None: row
    w); ``weights`` of the ensemble in the order pitch, instrument, velocity.  Returns host arrays: ``ensemble`` (n, C) float32 (None
    unless all three judges are given), ``pred`` (n, 4) uint8 argmaxes in the order of ``JUDGES`` (255: none), ``table`` (G, 9)
    float64 with the columns ``COLUMNS``, ``confusion`` (4, C, C) int32 [judge][class][argmax]."""
    tables = (p_pitch, p_vel, p_instr)
    shapes = {tuple(t.shape)[1] for t in tables if t is not None and len(t.shape) == 2}
    if any(t is not None and len(t.shape) != 2 for t in tables) or len(shapes) > 1:
        raise ValueError("probability tables must be (rows, C) with one C")
    n = len(cls)
    Cn = shapes.pop() if shapes else 0
    group_off_h = _on_host(group_off, np.int64)
    w = _check(n, Cn, tables, cls, group_off_h, weights)
    for t in (p_pitch, p_vel):
        if t is not None and t.shape[0] != n:
            raise ValueError("a pitch or velocity table has %d rows for %d windows" % (t.shape[0], n))
    if group_off_h[0] != 0 or group_off_h[-1] != n or np.any(np.diff(group_off_h) < 0):
        raise ValueError("group_off must ascend from 0 to n")
    if not device:
        pp, pv, pi = (_on_host(t, np.float32) for t in tables)
        return _mirror(pp, pv, pi, _on_host(cls, np.uint8), group_off_h, _on_host(instr_row, np.int64), w)
    import torch
    dev = next((t.device for t in tables if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda:0"))
    pp, pv, pi = (_on_device(t, torch.float32, dev) for t in tables)
    res = device_scores(pp, pv, pi, _on_device(cls, torch.uint8, dev), _on_device(group_off_h, torch.int32, dev),
                        _on_device(instr_row, torch.int32, dev), w)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


def song_groups(lengths):
    """group_off of songs of ``lengths`` windows laid end to end"""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int32)


# ---- the switched songs (reference vae_evaluation.py:2448-2625): builders that need no device ---------------------------------------
def switch_pairs(classes, num_classes):
    """the (song, C, C_switch) triples of :2451-2452 in the reference's order: every song with every class but its own"""
    return [(i, int(C), t) for i, C in enumerate(classes) for t in range(int(num_classes)) if t != int(C)]


def switched_latents(z, C, C_switch):
    """(switched z, history) of one song's (m, Z) latents: coordinates ``C`` and ``C_switch`` of every window trade places
    (:2474-2477); a window's history is the previous window's SWITCHED z, zero for the first (:2460, :2481, :2550)"""
    z = np.asarray(z, np.float64)
    if z.ndim != 2 or not (0 <= C < z.shape[1] and 0 <= C_switch < z.shape[1]):
        raise ValueError("z must be (m, Z) with classes %d and %d inside Z, got %r" % (C, C_switch, z.shape))
    switched = z.copy()
    switched[:, C] = z[:, C_switch]
    switched[:, C_switch] = z[:, C]
    history = np.zeros_like(switched)
    history[1:] = switched[:-1]
    return switched, history


def switch_instruments_matrix(pairs, programs, switched_programs, num_classes):
    """(num_classes, num_classes, 16, 16) counts [C][C_switch][program // 8][switched program // 8] over the voices of every pair
    (:2608-2612; its ``or 'khot-category'`` is always true, so the categories are counted whatever the attach method, :1921-1922).
    ``programs[song]`` the original song's programs, ``switched_programs[k]`` the voted programs of pair k BEFORE :2619 resets them."""
    m = np.zeros((int(num_classes), int(num_classes), 16, 16))
    for (song, C, C_switch), switched in zip(pairs, switched_programs):
        for program, switched_program in zip(programs[song], switched):
            m[C, C_switch, program // 8, switched_program // 8] += 1
    return m


def instruments_switched(programs, switched_programs, meta_instrument=True):
    """the ``SI_`` flag of :2614-2619 and the programs the switched song is written with: (True, the voted programs) when the model
    has the instrument head and the vote differs from the original's programs, else (False, the original's)"""
    if meta_instrument and list(switched_programs) != list(programs):
        return True, list(switched_programs)
    return False, list(programs)


# ---- the three judges on device rolls ------------------------------------------------------------------------------------------------
def style_of(row):
    """one row of the table as the dict a song reports: judge -> {'accuracy', 'confidence'}, plus 'windows' (the counted ones)"""
    d = {j: dict(accuracy=float(row[1 + 2 * i]), confidence=float(row[2 + 2 * i])) for i, j in enumerate(JUDGES)}
    d["windows"] = int(row[0])
    return d


class Judges(object):
    """the pitch, velocity and instrument StyleClassifiers (any of them None: that judge is absent) and the ensemble's ``weights`` in
    the order pitch, instrument, velocity - by default the reference's ``0.999 - 0.5`` for each (vae_evaluation.py:81-91)"""

    def __init__(self, pitch, velocity, instrument, weights=DEFAULT_WEIGHTS):
        for kind, clf in (("pitch", pitch), ("velocity", velocity), ("instrument", instrument)):
            if clf is not None and getattr(clf, "kind", None) != kind:
                raise ValueError("the %s judge must be a StyleClassifier(%r), got %r" % (kind, kind, getattr(clf, "kind", clf)))
        classes = {clf.cfg["C"] for clf in (pitch, velocity, instrument) if clf is not None}
        if len(classes) != 1:
            raise ValueError("the judges must share one number of classes (and one must be given), got %r" % sorted(classes))
        self.pitch, self.velocity, self.instrument = pitch, velocity, instrument
        self.num_classes = classes.pop()
        if not MIN_CLASSES <= self.num_classes <= MAX_CLASSES:
            raise ValueError("%d classes: style classes are %d..%d" % (self.num_classes, MIN_CLASSES, MAX_CLASSES))
        self.weights = tuple(_weights(weights))

    def probabilities(self, notes=None, velocity=None, instr=None, batch_size=32):
        """(p_pitch, p_vel, p_instr): the judges' (rows, C) float32 probabilities as DEVICE tensors - ``notes`` (n, T) uint8 note
        indices, ``velocity`` (n, T) float32 velocities after the post-rules, ``instr`` (rows, max_voices) uint8 instrument
        bytes, as device tensors (copied on the device) or host arrays; None where the roll or the judge is missing"""
        out = []
        for clf, roll in ((self.pitch, notes), (self.velocity, velocity), (self.instrument, instr)):
            if clf is None or roll is None:
                out.append(None)
            else:
                if not hasattr(roll, "data_ptr"):
                    roll = np.asarray(roll, np.float32)[..., None] if clf.kind == "velocity" else np.asarray(roll, np.uint8)
                out.append(clf.predict(roll, batch_size=batch_size, as_device=True))
        return tuple(out)

    def score(self, tables, cls, group_off, instr_row=None, outputs=None):
        """mvae_style_scores on ``tables`` = probabilities(...) with these judges' weights: ``device_scores``' dict of device
        tensors, or - ``outputs``: dict of caller-owned ``ensemble`` / ``pred`` / ``table`` / ``confusion`` tensors - ``enqueue``"""
        import torch
        dev = next(t.device for t in tables if t is not None)
        cls, group_off = _on_device(cls, torch.uint8, dev), _on_device(group_off, torch.int32, dev)
        instr_row = _on_device(instr_row, torch.int32, dev)
        if outputs is None:
            return device_scores(tables[0], tables[1], tables[2], cls, group_off, instr_row, self.weights)
        with torch.cuda.device(dev):
            enqueue(tables[0], tables[1], tables[2], cls, group_off, instr_row, self.weights, outputs.get("ensemble"), outputs.get("pred"),
                    outputs.get("table"), outputs.get("confusion"), torch.cuda.current_stream().cuda_stream)
        return outputs

    def score_groups(self, tables, classes, lengths, instr_row=None):
        """``score`` of groups of ``lengths`` windows laid end to end, every window of group g scored against ``classes[g]``; the
        table and - with all three judges - the ensemble come to the host in ONE copy: (table (G, 9), ensemble (n, C) or None)"""
        import torch
        from .rolls import HostPack
        lengths = np.asarray(lengths, np.int64)
        n, G = int(lengths.sum()), len(lengths)
        dev = next(t.device for t in tables if t is not None)
        blocks = [("table", torch.float64, (G, N_COLUMNS))]
        if all(t is not None for t in tables):
            blocks.append(("ensemble", torch.float32, (n, self.num_classes)))
        pack = HostPack(dev, blocks)
        cls = np.repeat(np.asarray(classes, np.int64), lengths).astype(np.uint8)
        self.score(tables, cls, song_groups(lengths), instr_row, outputs=pack.views)
        with torch.cuda.device(dev):
            res = pack.to_host()
        return res["table"], res.get("ensemble")


def score_originals(X_idx, V, I_idx, classes, judges, batch_size=32):
    """The reference's original-songs block (vae_evaluation.py:2075-2172): per song ``X_idx[i]`` (m_i, T) uint8 note indices (silent
    column included), ``V[i]`` (m_i, T) velocities, ``I_idx[i]`` (max_voices,) instrument indices of the song and its class.  The
    instrument judge sees every song ONCE (:2087-2094): its figure is that single prediction, not a mean over windows (:2151) - the
    table's mean of m_i copies of one float32 is that float32.  One dict per song: ``style``: judge -> accuracy and confidence,
    ``windows`` and ``ensemble_prediction`` (m_i, C) float32 or None, as decoder.predict_songs reports it."""
    lengths = [np.asarray(x).shape[0] for x in X_idx]
    if not lengths or min(lengths) <= 0:
        raise ValueError("score_originals: no songs, or a song without windows")
    notes = np.concatenate([np.asarray(x, np.uint8) for x in X_idx], 0)
    vel = None if V is None else np.concatenate([np.asarray(v, np.float32).reshape(m, -1) for v, m in zip(V, lengths)], 0)
    instr = None if I_idx is None else np.stack([np.asarray(i, np.uint8).reshape(-1) for i in I_idx], 0)
    tables = judges.probabilities(notes, vel, instr, batch_size)
    table, ens = judges.score_groups(tables, classes, lengths, instr_row=np.repeat(np.arange(len(lengths)), lengths))
    out, lo = [], 0
    for g, m in enumerate(lengths):
        out.append(dict(style=dict(style_of(table[g]), ensemble_prediction=None if ens is None else ens[lo:lo + m])))
        lo += m
    return out
