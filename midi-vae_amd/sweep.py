"""The latent sweep's statistics (reference vae_evaluation.py:898-1213): per-window pitch, velocity and note-start statistics of
decoded windows, and the summaries that rank latent dimensions by how monotonically those statistics move along a dimension.

``window_statistics`` runs on the device (``mvae_sweep_windows``, include/midivae_sweep.h: one lane per window) or, with
``device=False``, through the NumPy mirror below - the same semantics written out in Python, the yardstick of the device tests.
Both are pinned to the reference's own functions by tests/golden/sweep_stats.npz.  Everything after the table - ``summarize``,
``influence`` - is host arithmetic on a few numbers per window.

Semantics.  Row t of a window is voice t % V of tick t // V.  An index is a note unless it is the silent index, 255, or >= n_pitch.
The velocity of a row is the velocity head's float32 value, 0 on a row without a note, then - with
``override_sampled_pitches_based_on_velocity_info`` - the reference's per-voice rule (vae_definition.py:1153-1190, what
packers.apply_velocity_rules does), every window starting from previous_pitch = -1, previous_velocity = 0 as the sweep decodes one
window per process_decoder_outputs call.  Without a velocity head every row has the default velocity.  A note start is a row whose
velocity is > the threshold.  The table's 22 columns are ``COLUMNS``: count, mean, median, min, max, range, std of the pitch list (the
distinct sounding columns of every tick; low_crop is not added), the ticks in which the two counted columns sound, and the same
seven of the note starts' velocities and (sharing the count) six of their row positions.  An empty list: count 0, NaN statistics.

``s`` is a settings mapping or module read like packers._g does: max_voices, low_crop, high_crop, include_silent_note,
velocity_threshold_such_that_it_is_a_played_note, override_sampled_pitches_based_on_velocity_info.
"""
from __future__ import annotations

import ctypes as C
import math
import statistics
import warnings

import numpy as np

from . import hiplib as hl
from .packers import _g
from .rolls import HostPack, as_rolls, base_params, carried_velocity_rule, check_rows, device_roll, host_roll, sounding

_SIX = ("mean", "median", "min", "max", "range", "std")
COUNTED = (35, 39)          # the reference's two "specific pitch" columns
COLUMNS = (("pitch_count",) + tuple("pitch_" + k for k in _SIX) + ("pitch_count_a", "pitch_count_b", "note_starts_count") +
           tuple("velocity_" + k for k in _SIX) + tuple("note_starts_" + k for k in _SIX))
N_COLUMNS = len(COLUMNS)
MAX_T = 65536


def params(s, counted=COUNTED):
    """what the statistics read from the settings"""
    thr = float(_g(s, "velocity_threshold_such_that_it_is_a_played_note"))
    return dict(base_params(s), threshold=thr, default_velocity=thr + (1. - thr) * 0.5,
                override=bool(_g(s, "override_sampled_pitches_based_on_velocity_info")), count_a=int(counted[0]), count_b=int(counted[1]))


def _check(T, p):
    check_rows(T, p, MAX_T, "statistics")


# ---- the NumPy mirror ----------------------------------------------------------------------------------------------------------
def _median(values):
    v = sorted(values)
    c = len(v)
    return float(v[c // 2]) if c % 2 else (v[c // 2 - 1] + v[c // 2]) / 2


def _integer_stats(values):
    """mean, median, min, max, range, std of a list of non-negative integers, from exact sums like the device"""
    if not values:
        return [np.nan] * 6
    c, sm, sq, lo, hi = len(values), sum(values), sum(v * v for v in values), min(values), max(values)
    return [float(sm) / float(c), _median(values), float(lo), float(hi), float(hi - lo),
            math.sqrt(float(c * sq - sm * sm) / float(c * c))]


def _velocity_stats(values):
    """the same of a list of doubles: the sum in list order, the std in the two-pass form"""
    if not values:
        return [np.nan] * 6
    total = 0.0
    for v in values:
        total += v
    mean = total / float(len(values))
    dev = 0.0
    for v in values:
        dev += (v - mean) * (v - mean)
    return [mean, _median(values), min(values), max(values), max(values) - min(values), math.sqrt(dev / float(len(values)))]


def _mirror(idx, vel, p):
    n, T = idx.shape
    V = p["voices"]
    on = sounding(idx, p)
    if vel is None:          # no velocity head: the default velocity everywhere (a double), nothing zeroed, no rule
        after = [[p["default_velocity"]] * T] * n
    else:
        v0 = np.where(on, vel, np.float32(0)).astype(np.float32)
        if p["override"]:          # every window its own song
            v0 = carried_velocity_rule(idx, on, v0, np.arange(n), p)
        after = v0.astype(np.float64).tolist()          # Python floats from here on: `> threshold` must compare doubles
    table = np.full((n, N_COLUMNS), np.nan)
    roll = np.zeros((n, T), np.float32)
    for w in range(n):
        xs, os_, out = idx[w].tolist(), on[w].tolist(), after[w]
        pitches, in_a, in_b = [], 0, 0
        for k in range(0, T, V):
            notes = sorted({x for x, o in zip(xs[k:k + V], os_[k:k + V]) if o})
            pitches.extend(notes)
            in_a += p["count_a"] in notes
            in_b += p["count_b"] in notes
        roll[w] = out
        starts = [t for t in range(T) if out[t] > p["threshold"]]
        table[w] = ([float(len(pitches))] + _integer_stats(pitches) + [float(in_a), float(in_b), float(len(starts))] +
                    _velocity_stats([out[t] for t in starts]) + _integer_stats(starts))
    return table, roll


# ---- the device path -----------------------------------------------------------------------------------------------------------
def enqueue(idx, vel, p, stats_out, vel_out, stream):
    """mvae_sweep_windows on device memory the caller owns.  ``idx`` (n, T) uint8 tensor view of any strides (a decode's time-major
    buffer: ``rows[:, :B].t()``), ``vel`` a float32 tensor of the same strides or None for a model without the velocity head,
    ``stats_out`` (n, >= 22) float64 / ``vel_out`` (n, T) float32 contiguous tensors or None."""
    n, T = idx.shape
    a = hl.SweepArgs(idx=idx.data_ptr(), stride_t=idx.stride(1), stride_w=idx.stride(0), vel=hl.ptr(vel), n=n, T=T, voices=p["voices"],
                     silent=p["silent"], n_pitch=p["n_pitch"], count_a=p["count_a"], count_b=p["count_b"],
                     override_rules=int(p["override"]), threshold=p["threshold"], default_velocity=p["default_velocity"],
                     ld_out=0 if stats_out is None else stats_out.stride(0), stats_out=hl.ptr(stats_out), vel_out=hl.ptr(vel_out))
    hl.check(hl.load().mvae_sweep_windows(C.byref(a), stream), "mvae_sweep_windows")


def _device_run(idx, vel, p, want_velocity, device=None):
    import torch
    t = device_roll(idx, torch.uint8, "notes", device=device)
    n, T = t.shape
    _check(T, p)
    v = device_roll(vel, torch.float32, "velocities", t.shape, strides_of=t)
    stats = torch.empty((n, N_COLUMNS), dtype=torch.float64, device=t.device)
    roll = torch.empty((n, T), dtype=torch.float32, device=t.device) if want_velocity else None
    if n:
        with torch.cuda.device(t.device):
            enqueue(t, v, p, stats, roll, torch.cuda.current_stream().cuda_stream)
    return stats.cpu().numpy(), (None if roll is None else roll.cpu().numpy())


def decoded_batch(rows, vel, instr, B, p, return_rolls=False):
    """the statistics of the first ``B`` windows of a decode's time-major buffers: ``rows`` (T, Bp) uint8 note indices, ``vel``
    (T, Bp) float32 velocity head or None, ``instr`` (V, Bp) uint8 instrument indices or None.  Enqueued on the current stream of
    the buffers' device; the table and the instrument bytes travel to the host in ONE copy (with ``return_rolls`` the notes and the
    post-rule velocities ride along).  dict ``table`` (B, 22) float64, ``instr`` (B, V) uint8 or None, and with ``return_rolls``
    ``notes`` (B, T) uint8 and ``velocity`` (B, T) float32."""
    import torch
    T, V = rows.shape[0], p["voices"]
    blocks = [("table", torch.float64, (B, N_COLUMNS))]
    if instr is not None:
        blocks.append(("instr", torch.uint8, (B, V)))
    if return_rolls:
        blocks += [("velocity", torch.float32, (B, T)), ("notes", torch.uint8, (B, T))]
    pack = HostPack(rows.device, blocks)
    with torch.cuda.device(rows.device):
        enqueue(rows[:, :B].t(), None if vel is None else vel[:, :B].t(), p, pack.views["table"], pack.views.get("velocity"),
                torch.cuda.current_stream().cuda_stream)
        if instr is not None:
            pack.views["instr"].copy_(instr[:, :B].t())
        if return_rolls:
            pack.views["notes"].copy_(rows[:, :B].t())
        res = pack.to_host()
    res.setdefault("instr", None)
    return res


def window_statistics(notes, velocity, s, device=True, return_velocity=False, counted=COUNTED):
    """(n, 22) float64 table (columns: ``COLUMNS``) of (n, T) uint8 index rolls, (n, T, K) one-hot rolls or a 2-D uint8 device tensor
    and their (n, T) velocities - a float array, a float32 device tensor with the strides of ``notes``, or None for a model
    without the velocity head.  ``return_velocity``: (table, (n, T) float32 velocities after the rules)."""
    p, idx = params(s, counted), as_rolls(notes)
    if device:
        table, roll = _device_run(idx, velocity, p, return_velocity)
    else:
        idx = host_roll(idx, np.uint8, "notes")
        velocity = host_roll(velocity, np.float32, "velocities", idx.shape)
        _check(idx.shape[1], p)
        table, roll = _mirror(idx, velocity, p)
    return (table, roll) if return_velocity else table


# ---- the sweep's values and summaries --------------------------------------------------------------------------------------------
def sweep_values(range_end_in_stds=1.0, sigma=1.0, evaluations_per_dimension=5, positive_and_negative=True):
    """the values a coordinate of z is set to: the quantiles of N(0, sigma) at ``evaluations_per_dimension`` equally spaced
    probabilities from 0.5 to cdf(range_end_in_stds * sigma), mirrored to the negative side on request, ascending
    (reference vae_evaluation.py:898-911 and :1166)"""
    normal = statistics.NormalDist(0.0, float(sigma))
    range_end = normal.cdf(range_end_in_stds * sigma) - 0.5
    values = []
    for cdf in np.linspace(0.5, 0.5 + range_end, evaluations_per_dimension):
        x = normal.inv_cdf(float(cdf))
        if x != 0 and positive_and_negative:
            values.append(-x)
        values.append(x)
    return sorted(values)


def strength_probability_direction(values):
    """(strength, probability, direction) of a list of numbers (reference :917-951).  The direction is 'descending' when the mean of
    the first half exceeds the mean of the rest, and the list is then read backwards; strength = the mean step between
    neighbours, probability = the share of steps that do not go down.  An empty list gives (0, 0, 'ascending'); a one-element list
    has no steps and an empty first half: (nan, 0, 'ascending')."""
    n = len(values)
    if n == 0:
        return 0.0, 0.0, "ascending"
    a = np.asarray(values, dtype=np.float64)
    first = np.mean(a[:n // 2]) if n // 2 else np.nan
    direction = "descending" if first > np.mean(a[n // 2:]) else "ascending"
    if direction == "descending":
        a = np.ascontiguousarray(a[::-1])
    steps = a[1:] - a[:-1]
    if n == 1:
        return np.nan, 0, direction
    return np.mean(steps), int(np.sum(a[1:] >= a[:-1])) / (n - 1), direction


def programs_of(instr, instrument_attach_method):
    """instrument indices -> GM programs (reference data_class.py:352-373, the one-hot methods)"""
    instr = np.asarray(instr).astype(np.int64)
    if instrument_attach_method == "1hot-category":
        return instr * 8
    if instrument_attach_method == "1hot-instrument":
        return instr
    raise NotImplementedError("instrument_attach_method %r: the sweep maps one-hot instrument heads only" % (instrument_attach_method,))


STYLE_KEYS = ("pitchstyle", "velocitystyle", "instrumentstyle")          # the columns of ``style``: one judge each


def summarize(table, programs, counted=COUNTED, style=None):
    """the reference's summary dict ``name -> (strength, probability)`` of the K windows of one (sample, dimension) pair from their
    ``table`` (K, 22) and ``programs`` (K, V): the keys of evaluate_pitchroll, evaluate_velocityroll and evaluate_instrumentlist
    (:1018-1114); the three '*style' keys only with ``style`` (K, 3): the class-0 probability the pitch, velocity and instrument
    style judges give every window (:1035-1039, :1089-1093, :1105-1109; a NaN column: that judge is absent).  The pitch keys exist
    only if some window has a pitch, the velocity and note-start keys only if some window has a note start; a window with an empty
    list is left out of the statistic lists and counted (as 0) in the count lists."""
    table = np.asarray(table, np.float64)
    style = None if style is None else np.asarray(style, np.float64)
    d = {}

    def judged(column):
        if style is not None and not np.isnan(style[:, column]).all():
            strength, probability, direction = strength_probability_direction(style[:, column].tolist())
            d["mean_" + STYLE_KEYS[column] + "_" + direction] = (strength, probability)

    def statistic(name, stat, column, nonempty):
        strength, probability, direction = strength_probability_direction(table[nonempty, column].tolist())
        d[stat + "_" + name + "_" + direction] = (strength, probability)

    def count(name, counts):
        strength, probability, direction = strength_probability_direction([int(c) for c in counts])
        d["total_count_of_" + name + "_" + direction] = (strength, probability)

    has_pitch = table[:, 0] > 0
    if has_pitch.any():
        for i, stat in enumerate(_SIX):
            statistic("pitch", stat, 1 + i, has_pitch)
        count("pitch", table[:, 0])
        count("specificpitch%d" % counted[0], table[:, 7])
        count("specificpitch%d" % counted[1], table[:, 8])
        judged(0)
    has_start = table[:, 9] > 0
    if has_start.any():
        judged(1)
        for i, stat in enumerate(_SIX):
            statistic("velocity", stat, 10 + i, has_start)
        for i, stat in enumerate(_SIX):
            statistic("note_starts", stat, 16 + i, has_start)
        count("note_starts", table[:, 9])
    programs = np.asarray(programs)
    judged(2)
    steps = programs[1:] != programs[:-1]
    d["total_change_of_instruments"] = (float(steps.sum()) / float(steps.size) if steps.size else 0.0, 1.0)
    count("pianos", (programs == 0).sum(axis=1))
    return d


def influence(summaries):
    """``summaries[sample][dim]`` -> (influence, most_peaked, overall_best): ``influence[key]`` is the length-Z array of strength *
    probability summed over the samples (a key a summary lacks adds nothing); ``most_peaked[key]`` the dimension whose single
    summary was not beaten in strength and probability by a later one (:1189-1202, the dict is a value of this call);
    ``overall_best[key]`` the argmax of the influence (:1205-1213)."""
    Z = len(summaries[0]) if summaries else 0
    sums = [dict() for _ in range(Z)]
    best = {}
    for per_dim in summaries:
        for dim, summary in enumerate(per_dim):
            for key, (strength, probability) in summary.items():
                sums[dim][key] = sums[dim].get(key, 0.0) + strength * probability
        for dim, summary in enumerate(per_dim):
            for key, (strength, probability) in summary.items():
                if key not in best:
                    best[key] = (strength, probability, dim)
                elif strength >= best[key][0] and probability >= best[key][1]:
                    best[key] = (strength, probability, dim)
    infl = {key: np.array([sums[dim].get(key, 0.0) for dim in range(Z)], np.float64) for key in best}
    return infl, {key: b[2] for key, b in best.items()}, {key: int(np.argmax(v)) for key, v in infl.items()}


def _direction_rows(A):
    """strength_probability_direction of every row of ``A`` (M, L), L >= 2: arrays (strength, probability, descending).  The same
    NumPy reductions over the same contiguous runs of L // 2, L - L // 2 and L - 1 numbers as the one-list form, so the same bits
    (tests/test_sweep_stats_cpu.py holds the two against each other)."""
    L = A.shape[1]
    first = np.ascontiguousarray(A[:, :L // 2]).mean(axis=1)
    descending = first > np.ascontiguousarray(A[:, L // 2:]).mean(axis=1)
    A = np.ascontiguousarray(np.where(descending[:, None], A[:, ::-1], A))
    steps = np.ascontiguousarray(A[:, 1:] - A[:, :-1])
    return steps.mean(axis=1), (A[:, 1:] >= A[:, :-1]).sum(axis=1) / (L - 1), descending


def summarize_sweep(table, programs, counted=COUNTED, style=None):
    """``table`` (n, Z, K, 22), ``programs`` (n, Z, K, V), ``style`` (n, Z, K, 3) or None -> (summaries[sample][dim], influence,
    most_peaked, overall_best): ``summarize`` of every (sample, dimension) pair - taken for all pairs with lists of one length at
    once, a sweep has thousands of pairs of a few numbers each - and ``influence`` of the result"""
    table, programs = np.asarray(table, np.float64), np.asarray(programs)
    n, Z, K = table.shape[:3]
    t, pr = table.reshape(n * Z, K, N_COLUMNS), programs.reshape(n * Z, K, -1)
    st = None if style is None else np.asarray(style, np.float64).reshape(n * Z, K, len(STYLE_KEYS))
    out = [dict() for _ in range(n * Z)]

    def put(rows, name, A):
        """``A`` (len(rows), L): one list per pair in ``rows``"""
        L = A.shape[1]
        if L < 2:
            for r in rows.tolist():
                out[r][name + "_ascending"] = (np.nan, 0) if L else (0.0, 0.0)
            return
        strength, probability, descending = (v.tolist() for v in _direction_rows(A))
        for r, pair, down in zip(rows.tolist(), zip(strength, probability), descending):
            out[r][name + ("_descending" if down else "_ascending")] = pair

    def judged(rows, column):
        if st is not None and len(rows) and not np.isnan(st[:, :, column]).all():
            put(rows, "mean_" + STYLE_KEYS[column], st[rows][:, :, column])

    def group(count_column, statistics, counts, judge, judge_first):
        nonempty = t[:, :, count_column] > 0
        lengths = nonempty.sum(axis=1)
        if judge_first:
            judged(np.nonzero(lengths > 0)[0], judge)
        for L in np.unique(lengths[lengths > 0]):
            rows = np.nonzero(lengths == L)[0]
            sub, keep = t[rows], nonempty[rows]
            for name, column in statistics:
                put(rows, name, sub[:, :, column][keep].reshape(len(rows), L))
        rows = np.nonzero(lengths > 0)[0]
        sub = t[rows]
        for name, column in counts:
            put(rows, "total_count_of_" + name, sub[:, :, column])
        if not judge_first:
            judged(rows, judge)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        group(0, [(stat + "_pitch", 1 + i) for i, stat in enumerate(_SIX)],
              [("pitch", 0), ("specificpitch%d" % counted[0], 7), ("specificpitch%d" % counted[1], 8)], 0, False)
        group(9, [(stat + "_velocity", 10 + i) for i, stat in enumerate(_SIX)] + [(stat + "_note_starts", 16 + i) for i, stat in enumerate(_SIX)],
              [("note_starts", 9)], 1, True)
        judged(np.arange(n * Z), 2)
        steps = (pr[:, 1:] != pr[:, :-1]).reshape(n * Z, -1)
        for r in range(n * Z):
            out[r]["total_change_of_instruments"] = (float(steps[r].sum()) / float(steps.shape[1]) if steps.shape[1] else 0.0, 1.0)
        put(np.arange(n * Z), "total_count_of_pianos", (pr == 0).sum(axis=2).astype(np.float64))
    summaries = [out[i * Z:(i + 1) * Z] for i in range(n)]
    return (summaries,) + influence(summaries)
