#!/usr/bin/env python3
"""Generate tests/golden/style_scores.npz: style-transfer scores from the reference's own ``ensemble_prediction`` and a restatement
of its per-song counters.

Runs ONLY where the reference is present (make_fixtures.REF).  The reference's vae_evaluation.py is a script, so it is never
imported: ``ensemble_prediction`` (:110-117) is picked out of its syntax tree and executed in a namespace that holds the three
weights of :81-91 (or the case's own) and three stand-in models whose ``predict`` replays recorded float32 probability tables: the
"input" of a window is its row number.  The per-song counters (:2096-2172 for original songs, whose instruments are judged once per
song; :2471-2604 for switched songs, judged window by window) are inline script code there; ``song_counters`` below restates them
line by line under the installed NumPy, which accumulates ``+=`` on float32 scalars in float32.  Only data is written: the tables,
the classes, the groups and the recorded results.

  python tests/golden/make_style_fixtures.py

Two cases, 400 windows in 13 groups.  ``a``: C = 2, the reference's weights, instruments per window (instr_row absent), groups of
300 (more than one pass of a 256-lane workgroup), 0, 1, 12, 9 and 8 windows.  ``b``: C = 3, weights 0.499 / 0.3 / 0.2, instruments
per song (instr_row = the group), groups of 20, 1, 0, 17, 22, 7 and 3 windows, the last with every class 255.  Both sprinkle 255s.
Assertions keep the fixture from going soft: every judge's hit rate lies in 20..80 %, the three judges' argmaxes disagree on at
least a quarter of the windows, the ensemble's argmax differs from the pitch judge's on at least 5 %, exact ties occur within rows
(the first index wins), at least ten rows have a partial sum exactly between two float32 values, and at least ten rows change
when the weighted sum is evaluated with fused multiply-adds.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402

JUDGES = ("pitch", "velocity", "instrument", "ensemble")
CASES = (
    dict(name="a", C=2, weights=(0.999 - 0.5, 0.999 - 0.5, 0.999 - 0.5), groups=(300, 0, 1, 12, 9, 8), per_song=False, all_left_out=()),
    dict(name="b", C=3, weights=(0.999 - 0.5, 0.3, 0.2), groups=(20, 1, 0, 17, 22, 7, 3), per_song=True, all_left_out=(6,)),
)


class _Replay:
    """a stand-in classifier: the input of a window is its row number in the recorded table"""

    def __init__(self, table):
        self.table = table

    def predict(self, x):
        return self.table[np.asarray(x, np.int64)]


def _reference_ensemble(models, weights):
    tree = ast.parse(open(os.path.join(mfx.REF, "vae_evaluation.py")).read())
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "ensemble_prediction"]
    assert len(picked) == 1
    ns = dict(np=np, pitches_classifier_model=models["pitch"], instrument_classifier_model=models["instrument"],
              velocity_classifier_model=models["velocity"], pitches_classifier_model_weight=weights[0],
              instrument_classifier_model_weight=weights[1], velocity_classifier_model_weight=weights[2])
    exec(compile(ast.Module(body=picked, type_ignores=[]), "<pinned>", "exec"), ns)
    return ns["ensemble_prediction"]


def song_counters(models, ensemble_prediction, windows, C, song_row):
    """accuracy and confidence of the four judges over the counted ``windows`` of one song of class ``C``.  ``song_row`` None: the
    switched block :2471-2604 (every window's instruments are judged); else the original block :2075-2172 (row ``song_row`` of the
    instrument table judges the song once, :2087-2094, and its figures are not divided, :2151)."""
    acc = dict.fromkeys(JUDGES, 0.0)                                                            # :2078-2085 / :2462-2469
    conf = dict.fromkeys(JUDGES, 0.0)
    per_window = {j: [] for j in JUDGES}
    ens_rows = {}

    def judge(name, prediction):
        conf[name] += prediction[C]                                                             # :2101-2102
        if np.argmax(prediction) == C:                                                          # :2103-2104
            acc[name] += 1
        per_window[name].append(int(np.argmax(prediction)))

    if song_row is not None:
        instrument_classifier_input = np.asarray([song_row])                                    # :2088
        judge("instrument", models["instrument"].predict(instrument_classifier_input)[0])       # :2089-2094
        per_window["instrument"] = per_window["instrument"] * len(windows)
    for w in windows:                                                                           # :2096 / :2471
        pitches_classifier_input = np.asarray([w])                                              # :2098 / :2497
        judge("pitch", models["pitch"].predict(pitches_classifier_input)[0])                    # :2099-2104 / :2498-2503
        velocity_classifier_input = np.asarray([w])                                             # :2109 / :2509
        judge("velocity", models["velocity"].predict(velocity_classifier_input)[0])             # :2110-2115 / :2510-2515
        if song_row is None:
            instrument_classifier_input = np.asarray([w])                                       # :2519
            judge("instrument", models["instrument"].predict(instrument_classifier_input)[0])   # :2520-2525
        e = ensemble_prediction(pitches_classifier_input, instrument_classifier_input, velocity_classifier_input)[0]   # :2118 / :2529
        ens_rows[w] = e
        judge("ensemble", e)                                                                    # :2119-2123 / :2530-2534
    num = len(windows)
    for name in JUDGES:
        if name == "instrument" and song_row is not None:
            continue                                                                            # :2151-2152: not divided
        acc[name] /= num                                                                        # :2126-2127 / :2553-2554
        conf[name] /= num
    return acc, conf, per_window, ens_rows


def _fused(p, i, v, weights):
    """the weighted sum as a compiler that contracts would evaluate it: fma(v, wv, fma(i, wi, p * wp)) / den.  A float32 product is
    exact in double and the double sum rounds at 2^-53, so rounding it to float32 is the fused result (up to a 2^-29 chance)"""
    wp, wi, wv = (np.float32(x) for x in weights)
    den = np.float32(weights[0] + weights[1] + weights[2])
    t = p * wp
    t = (i.astype(np.float64) * np.float64(wi) + t.astype(np.float64)).astype(np.float32)
    t = (v.astype(np.float64) * np.float64(wv) + t.astype(np.float64)).astype(np.float32)
    return t / den


def _tie_rows(p, i, v, weights):
    """rows in which one of the two float32 sums of the unfused evaluation lands exactly between two float32 values (the sum of two
    float32 terms is exact in double): round-to-even decides there, and a fused multiply-add, which still sees the bits the
    rounded product dropped, may decide the other way"""
    wp, wi, wv = (np.float32(x) for x in weights)
    a, b, c = p * wp, i * wi, v * wv

    def tie(x, y):
        exact = x.astype(np.float64) + y.astype(np.float64)
        r = exact.astype(np.float32)
        other = np.nextafter(r, np.where(exact > r, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        return (exact != r) & (np.abs(exact - r) == np.abs(other.astype(np.float64) - exact))
    return int(np.any(tie(a, b) | tie(a + b, c), axis=1).sum())


def _tables(rng, n, rows_i, C, cls_of_window, cls_of_row):
    def judge(rows, cls, skill):
        logits = rng.normal(0.0, 1.2, (rows, C))
        logits[np.arange(rows), cls] += skill
        e = np.exp(logits - logits.max(1, keepdims=True))
        p = (e / e.sum(1, keepdims=True)).astype(np.float32)
        tied = rng.random(rows) < 0.08          # exact ties: the first index must win
        for r in np.nonzero(tied)[0]:
            pattern = [0.5, 0.5] if C == 2 else [[0.375, 0.375, 0.25], [0.25, 0.375, 0.375], [0.375, 0.25, 0.375]][rng.integers(3)]
            p[r] = np.asarray(pattern, np.float32)
        return p
    return judge(n, cls_of_window, 0.5), judge(n, cls_of_window, 0.3), judge(rows_i, cls_of_row, 0.6 if rows_i == n else 6.0)


def build_case(rng, case):
    C, groups = case["C"], case["groups"]
    group_off = np.concatenate([[0], np.cumsum(groups)]).astype(np.int32)
    n, G = int(group_off[-1]), len(groups)
    song_class = rng.integers(0, C, G)
    true = np.repeat(song_class, groups).astype(np.int64)
    cls = true.astype(np.uint8)
    cls[rng.random(n) < 0.06] = 255
    for g in case["all_left_out"]:
        cls[group_off[g]:group_off[g + 1]] = 255
    for g in range(G):          # the one-window group and its like stay counted
        if groups[g] == 1:
            cls[group_off[g]] = song_class[g]
    rows_i = G if case["per_song"] else n
    # judged once per song, a few rows decide the instrument judge's rate: every other song's row leans to a wrong class
    leaning = np.where(np.arange(G) % 2 == 0, song_class, (song_class + 1) % C)
    p_pitch, p_vel, p_instr = _tables(rng, n, rows_i, C, true, leaning if case["per_song"] else true)
    models = dict(pitch=_Replay(p_pitch), velocity=_Replay(p_vel), instrument=_Replay(p_instr))
    ensemble_prediction = _reference_ensemble(models, case["weights"])
    instr_row = np.repeat(np.arange(G), groups).astype(np.int32) if case["per_song"] else np.arange(n, dtype=np.int32)

    # every window through the reference's function, one at a time as the script calls it (also the windows no group counts)
    ensemble = np.stack([ensemble_prediction(np.asarray([w]), np.asarray([instr_row[w]]), np.asarray([w]))[0] for w in range(n)])
    assert ensemble.dtype == np.float32
    judged_i = p_instr[instr_row]
    pred = np.stack([np.argmax(t, axis=1) for t in (p_pitch, p_vel, judged_i, ensemble)], axis=1).astype(np.uint8)

    count = np.zeros(G, np.int64)
    accuracy = np.full((G, 4), np.nan)
    confidence = np.full((G, 4), np.nan)
    confusion = np.zeros((4, C, C), np.int32)
    for g in range(G):
        windows = [w for w in range(group_off[g], group_off[g + 1]) if cls[w] != 255]
        count[g] = len(windows)
        if not windows:
            continue
        k = int(song_class[g])
        acc, conf, per_window, ens_rows = song_counters(models, ensemble_prediction, windows, k, g if case["per_song"] else None)
        for j, name in enumerate(JUDGES):
            accuracy[g, j], confidence[g, j] = float(acc[name]), float(conf[name])
            assert per_window[name] == pred[windows, j].tolist()
            for a in per_window[name]:
                confusion[j, k, a] += 1
        for w, e in ens_rows.items():
            assert np.array_equal(e.view(np.uint32), ensemble[w].view(np.uint32))

    counted = cls != 255
    for j, name in enumerate(JUDGES):
        rate = float((pred[counted, j] == cls[counted]).mean())
        print("case %s: %s hit rate %.1f %%" % (case["name"], name, 100 * rate))
        assert 0.2 <= rate <= 0.8, "the %s judge is too sure or too wrong: %.3f" % (name, rate)
    disagree = float(((pred[:, 0] != pred[:, 1]) | (pred[:, 0] != pred[:, 2])).mean())
    ens_vs_pitch = float((pred[:, 3] != pred[:, 0]).mean())
    ties = sum(int((np.sort(t, 1)[:, -1] == np.sort(t, 1)[:, -2]).sum()) for t in (p_pitch, p_vel, p_instr))
    fused = _fused(p_pitch, judged_i, p_vel, case["weights"])
    fma_rows = int(np.any(fused.view(np.uint32) != ensemble.view(np.uint32), axis=1).sum())
    halfway = _tie_rows(p_pitch, judged_i, p_vel, case["weights"])
    print("case %s: judges disagree on %.1f %%, ensemble differs from pitch on %.1f %%, %d tied rows, %d rows with a sum exactly between "
          "two float32 values, %d rows change under FMA" % (case["name"], 100 * disagree, 100 * ens_vs_pitch, ties, halfway, fma_rows))
    assert disagree >= 0.25 and ens_vs_pitch >= 0.05 and ties >= 5 and halfway >= 10 and fma_rows >= 10
    out = dict(p_pitch=p_pitch, p_vel=p_vel, p_instr=p_instr, cls=cls, group_off=group_off, weights=np.asarray(case["weights"], np.float64),
               ensemble=ensemble, pred=pred, count=count, accuracy=accuracy, confidence=confidence, confusion=confusion,
               song_class=song_class.astype(np.uint8), fma_rows=np.int64(fma_rows), halfway_rows=np.int64(halfway))
    if case["per_song"]:
        out["instr_row"] = instr_row
    return {"%s_%s" % (case["name"], k): v for k, v in out.items()}


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    rng = np.random.default_rng(20261021)
    out = {}
    for case in CASES:
        out.update(build_case(rng, case))
    path = os.path.join(HERE, "style_scores.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
