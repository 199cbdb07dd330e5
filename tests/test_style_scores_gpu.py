"""Style-transfer scoring on the device (csrc/style.hip, mvae_style_scores) against the NumPy mirror of midi_vae_amd.style - which
tests/test_style_scores_cpu.py pins to the reference's own ensemble and counters - and against those recorded results themselves;
the classifiers fed from device rolls; and the public surface that joins a decode to the judges.

Bounds (derived, not measured).  The ensemble: five float32 operations and a correctly rounded division per element, none fused, on
both sides: BIT-EQUAL.  Argmaxes follow from those bits and from the input bits: equal.  Counts, hits and the confusion counts are
integers (the latter integer atomics: exact in any order): equal.  An accuracy is hits / count, one double division: bit-equal.  A
confidence mean: the device adds at most ceil(n_g / 256) terms per lane one after the other and 8 tree levels on top, every
addition rounding once at 2^-53 relative to a partial sum of non-negative terms, then divides once; the mirror's math.fsum is the
exactly rounded sum: within (ceil(n_g / 256) + 8) * 2^-53 * max(mean, 2^-1022) of each other (style_contract.device_mean_ratio);
the largest ratio seen is printed."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import style as st
from tests import footprint as fp
from tests import style_contract as sc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    fx = sc.load_fixture()
    for f in fx.values():
        f["mirror"] = sc.mirror_of(f)
    return fx


def assert_scores(got, want, what):
    """device results against the mirror's, by the split of this file's docstring; returns the largest confidence ratio"""
    if want["ensemble"] is None:
        assert got["ensemble"] is None, what
    else:
        g, w = got["ensemble"], want["ensemble"]
        assert g.dtype == np.float32 and g.shape == w.shape, what
        bad = np.argwhere(~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))))
        assert bad.size == 0, "%s: %d ensemble values differ, first at %s: %r vs %r" % (what, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
    assert got["pred"].dtype == np.uint8 and np.array_equal(got["pred"], want["pred"]), "%s: pred" % what
    assert got["confusion"].dtype == np.int32 and np.array_equal(got["confusion"], want["confusion"]), "%s: confusion" % what
    gt, wt = got["table"], want["table"]
    assert gt.dtype == np.float64 and gt.shape == wt.shape, what
    assert sc.same_bits(gt[:, 0], wt[:, 0]) and sc.same_bits(gt[:, 1::2], wt[:, 1::2]), "%s: counts or accuracies" % what
    assert np.array_equal(np.isnan(gt), np.isnan(wt)), "%s: NaN in other places" % what
    worst = 0.0
    for g in range(gt.shape[0]):
        for c in (2, 4, 6, 8):
            if not np.isnan(wt[g, c]):
                worst = max(worst, sc.device_mean_ratio(gt[g, c], wt[g, c], int(wt[g, 0])))
    print("%s: largest |device - mirror| of a confidence mean over its bound: %.3g" % (what, worst))
    assert worst <= 1.0, what
    return worst


def to_dev(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


# ---- the reference's windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture(cases, case):
    fx = cases[case]
    got = st.scores(fx["p_pitch"], fx["p_vel"], fx["p_instr"], fx["cls"], fx["group_off"], fx["instr_row"], fx["weights"])
    assert_scores(got, fx["mirror"], "case %s" % case)
    assert np.array_equal(got["ensemble"].view(np.uint32), fx["ensemble"].view(np.uint32)), "against the reference's own ensemble"
    assert np.array_equal(got["pred"], fx["pred"]) and sc.same_bits(got["table"][:, 1::2], fx["accuracy"])
    assert np.array_equal(got["confusion"], fx["confusion"])
    tensors = st.scores(to_dev(fx["p_pitch"], torch.float32), to_dev(fx["p_vel"], torch.float32), to_dev(fx["p_instr"], torch.float32),
                        to_dev(fx["cls"], torch.uint8), to_dev(fx["group_off"], torch.int32), to_dev(fx["instr_row"], torch.int32), fx["weights"])
    for k in got:
        assert np.array_equal(got[k], tensors[k], equal_nan=True), "device tensors in: %s" % k


def _f64(buf):
    return np.ascontiguousarray(buf.bits()).view(np.uint64).view(np.float64)


def test_fixture_strided_and_guarded(cases):
    """case b with every leading dimension wider than it must be and different from the others: nothing is written outside
    [n x C] of the ld-strided ensemble rows, nothing beyond column 8 of the table, the pad columns of the inputs (NaN sentinels) are
    never used, every guard and every input as planted"""
    fx = cases["b"]
    n, C, G = fx["p_pitch"].shape[0], 3, len(fx["group_off"]) - 1
    lds = dict(p_pitch=5, p_vel=7, p_instr=4)
    LD_ENS, LD_TABLE = 6, 11
    ar, bufs = fp.Arena(DEV), {}
    for name, ld in lds.items():
        data = torch.full((fx[name].shape[0], ld), float("nan"))
        data[:, :C] = torch.from_numpy(fx[name])
        bufs[name] = ar.carve(name, tuple(data.shape), torch.float32, data=data)
    bufs["instr_row"] = ar.carve("instr_row", (n,), torch.int32, data=torch.from_numpy(fx["instr_row"]))
    bufs["cls"] = ar.carve("cls", (n,), torch.uint8, data=torch.from_numpy(fx["cls"]), guard="zero")
    bufs["group_off"] = ar.carve("group_off", (G + 1,), torch.int32, data=torch.from_numpy(fx["group_off"]))
    b_ens = ar.carve("ens", (n, LD_ENS), torch.float32)
    b_pred = ar.carve("pred", (n, 4), torch.uint8)
    b_table = ar.carve("table", (G, 2 * LD_TABLE), torch.float32)
    b_conf = ar.carve("confusion", (4, C, C), torch.int32, prefill=np.zeros((4, C, C), np.int32))
    ar.commit()
    table = b_table.t.view(torch.float64)
    assert table.shape == (G, LD_TABLE) and bufs["p_vel"].t.stride(0) == 7
    st.enqueue(bufs["p_pitch"].t[:, :C], bufs["p_vel"].t[:, :C], bufs["p_instr"].t[:, :C], bufs["cls"].t, bufs["group_off"].t, bufs["instr_row"].t,
               fx["weights"], b_ens.t[:, :C], b_pred.t, table, b_conf.t, torch.cuda.current_stream().cuda_stream)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(b_ens, np.s_[:, :C])
    ar.assert_untouched(b_ens, np.s_[:, C:])
    ar.assert_written(b_table, np.s_[:, :18])
    ar.assert_untouched(b_table, np.s_[:, 18:])
    for name in ("p_pitch", "p_vel", "p_instr", "instr_row", "cls", "group_off"):
        b = bufs[name]
        assert np.array_equal(b.bits(), ar.planted[b.body:b.body + b.nbytes].view(b.bits().dtype).reshape(b.shape)), name
    got = dict(ensemble=np.ascontiguousarray(b_ens.bits()[:, :C]).view(np.float32), pred=b_pred.bits().copy(),
               table=np.ascontiguousarray(_f64(b_table)[:, :9]), confusion=b_conf.bits().view(np.int32).copy())
    assert_scores(got, fx["mirror"], "strided")
    tight = st.scores(fx["p_pitch"], fx["p_vel"], fx["p_instr"], fx["cls"], fx["group_off"], fx["instr_row"], fx["weights"])
    assert np.array_equal(got["table"].view(np.uint64), tight["table"].view(np.uint64)), "the strides changed the sums"


# ---- shapes the fixture does not have ----------------------------------------------------------------------------------------------
def random_case(seed, C, groups, rows_i=None, nan_rows=()):
    """softmax-like float32 tables with exact ties, classes with 255s and one class that does not exist"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(groups)]).astype(np.int32)
    n = int(off[-1])
    def table(rows):
        e = np.exp(rng.normal(0.0, 1.5, (rows, C)))
        p = (e / e.sum(1, keepdims=True)).astype(np.float32)
        tie = rng.random(rows) < 0.1
        p[tie, rng.integers(0, C, int(tie.sum()))] = p[tie].max(1)          # a second copy of the maximum somewhere
        return p
    p = [table(n), table(n), table(n if rows_i is None else rows_i)]
    for r in nan_rows:
        p[r % 2][r % n, r % C] = np.nan
    cls = rng.integers(0, C, n).astype(np.uint8)
    cls[rng.random(n) < 0.05] = 255
    if n > 10:
        cls[rng.integers(0, n)] = min(C, 254)
    instr_row = None if rows_i is None else rng.integers(0, rows_i, n).astype(np.int32)
    return p, cls, off, instr_row


@pytest.mark.parametrize("C,groups", [(2, (1,)), (16, (256, 257, 0, 3)), (17, (40, 513)), (64, (300, 1, 77))], ids=lambda x: str(x))
def test_class_counts_and_group_lengths(C, groups):
    """one window; exactly one pass, one pass and one window, two passes and one window; 16 and 17 classes (the confusion counts are
    gathered in LDS up to 16 classes and go to memory directly above), 64 classes; NaN probabilities (the first NaN wins)"""
    p, cls, off, _ = random_case(100 * C + len(groups), C, groups, nan_rows=(0, 5) if C > 2 else ())
    w = (0.7, 0.2, 0.45)
    want = st.scores(p[0], p[1], p[2], cls, off, None, w, device=False)
    assert_scores(st.scores(p[0], p[1], p[2], cls, off, None, w), want, "C = %d, groups %r" % (C, groups))


def test_instrument_rows_out_of_range_and_malformed_groups():
    """instr_row below 0 and past n_instr_rows: 255 / NaN, never read (the table has exactly n_instr_rows rows inside guards and a
    read past it would meet sentinel NaNs; rows far outside would fault).  group_off with a descending pair (an empty group), an
    end past n and a start below 0 (both clamped)"""
    C, n, rows_i = 5, 300, 9
    p, cls, _, instr_row = random_case(77, C, (n,), rows_i=rows_i)
    instr_row[[0, 17, 256, 299]] = [-1, rows_i, 2 ** 31 - 1, -2 ** 31]
    cls[[0, 17, 256, 299]] = 1
    off = np.array([-5, 100, 90, 90, 290, n + 1000], np.int32)          # groups: [0, 100), empty, empty, [90, 290), [290, n)
    w = st.DEFAULT_WEIGHTS
    want = st._mirror(p[0], p[1], p[2], cls, off.astype(np.int64), instr_row.astype(np.int64), list(w))
    ar = fp.Arena(DEV)
    b_instr = ar.carve("p_instr", (rows_i, C), torch.float32, data=torch.from_numpy(p[2]))
    ar.commit()
    res = st.device_scores(to_dev(p[0], torch.float32), to_dev(p[1], torch.float32), b_instr.t, to_dev(cls, torch.uint8), to_dev(off, torch.int32),
                           to_dev(instr_row, torch.int32), w)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    ar.fetch()
    ar.assert_guards_intact()
    bad = [0, 17, 256, 299]
    assert np.all(got["pred"][bad, 2:] == 255) and np.all(np.isnan(got["ensemble"][bad])) and np.all(got["pred"][bad, :2] < C)
    assert list(want["table"][:, 0] > 0) == [True, False, False, True, True] and np.all(np.isnan(want["table"][:, [6, 8]][[0, 3, 4]]))
    # windows [90, 100) sit in two groups: both write the same bits
    assert_scores(got, want, "out-of-range rows, malformed groups")


@pytest.mark.parametrize("absent", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)], ids=lambda a: "without_" + "_".join(st.JUDGES[j] for j in a))
def test_absent_judges(cases, absent):
    """a NULL table: NaN columns in the table, 255 in pred, no ensemble, no confusion counts of that judge or of the ensemble"""
    fx = cases["b"]
    tables = [None if j in absent else fx[k] for j, k in enumerate(("p_pitch", "p_vel", "p_instr"))]
    want = st.scores(tables[0], tables[1], tables[2], fx["cls"], fx["group_off"], fx["instr_row"], fx["weights"], device=False)
    got = st.scores(tables[0], tables[1], tables[2], fx["cls"], fx["group_off"], fx["instr_row"], fx["weights"])
    assert_scores(got, want, "without %r" % (absent,))
    gone = list(absent) + [3]
    assert got["ensemble"] is None and np.all(got["pred"][:, gone] == 255) and got["confusion"][gone].sum() == 0
    cols = [c for j in gone for c in (1 + 2 * j, 2 + 2 * j)]
    assert np.all(np.isnan(got["table"][:, cols]))
    kept = [j for j in range(3) if j not in absent]
    full = cases["b"]["mirror"]
    assert np.array_equal(got["pred"][:, kept], full["pred"][:, kept]) and np.array_equal(got["confusion"][kept], full["confusion"][kept])


# ---- refusals and accepted forms -------------------------------------------------------------------------------------------------
def _contract_arena(fx):
    """the baseline of tests/style_contract.py on real, guarded buffers filled from case b"""
    ar, bufs = fp.Arena(DEV), {}
    rng = np.random.default_rng(1)

    def carve(name, shape, kind, out=False):
        if kind == "f64":
            bufs[name] = ar.carve(name, (shape[0], 2 * shape[1]), torch.float32)
        elif name == "confusion_out":
            bufs[name] = ar.carve(name, shape, torch.int32, prefill=np.zeros(shape, np.int32))
        elif out:
            bufs[name] = ar.carve(name, shape, torch.uint8 if kind == "u8" else torch.float32)
        elif kind == "f32":
            data = torch.full(shape, float("nan"))
            data[:, :sc.NC] = torch.from_numpy(fx[name][:shape[0]])
            bufs[name] = ar.carve(name, shape, torch.float32, data=data)
        elif name == "cls":
            bufs[name] = ar.carve(name, shape, torch.uint8, data=torch.from_numpy(fx["cls"][:shape[0]].copy()), guard="zero")
        elif name == "group_off":
            bufs[name] = ar.carve(name, shape, torch.int32, data=torch.tensor(sc.GROUP_OFF, dtype=torch.int32))
        else:
            bufs[name] = ar.carve(name, shape, torch.int32, data=torch.from_numpy(rng.integers(0, sc.G, shape).astype(np.int32)))
        return 0x1000

    sc.baseline(carve)
    ar.commit()
    return ar, bufs, (lambda name, shape, kind, out=False: bufs[name].t.data_ptr())


def _contract_mirror(bufs, mutate):
    """the mirror of mutate(baseline) on what the arena's inputs hold"""
    a = mutate(sc.baseline(lambda name, shape, kind, out=False: 1))
    host = {k: b.t.cpu().numpy() for k, b in bufs.items() if not b.is_output}
    tables = [host[k][:, :a.C] if getattr(a, k) else None for k in ("p_pitch", "p_vel", "p_instr")]
    return st._mirror(tables[0], tables[1], tables[2], host["cls"], np.asarray(sc.GROUP_OFF, np.int64),
                      host["instr_row"].astype(np.int64) if a.instr_row else None, list(a.weights))


def _contract_outputs(bufs, C):
    return dict(ensemble=np.ascontiguousarray(bufs["ens_out"].bits()[:, :C]).view(np.float32), pred=bufs["pred_out"].bits().copy(),
                table=np.ascontiguousarray(_f64(bufs["table_out"])[:, :9]), confusion=bufs["confusion_out"].bits().view(np.int32).copy())


def test_refused_calls_enqueue_nothing(cases):
    """the safe rows of tests/style_contract.py on real buffers: the promised code, and every byte of the arena - the tables, the
    sentinel-filled outputs, the guards - as planted; the baseline itself then runs inside its buffers"""
    ar, bufs, resolve = _contract_arena(cases["b"])
    lib, stream = hl.load(), torch.cuda.current_stream().cuda_stream
    safe = [r for r in sc.ROWS if r[3]]
    assert len(safe) >= 20
    for name, mutate, code, _ in safe:
        rc = sc.invoke(lib, mutate(sc.baseline(resolve)), stream)
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert sc.invoke(lib, sc.baseline(resolve), stream) == 0
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(bufs["ens_out"], np.s_[:, :sc.NC])
    ar.assert_untouched(bufs["ens_out"], np.s_[:, sc.NC:])
    ar.assert_written(bufs["pred_out"])
    ar.assert_written(bufs["table_out"], np.s_[:, :18])
    ar.assert_untouched(bufs["table_out"], np.s_[:, 18:])
    assert_scores(_contract_outputs(bufs, sc.NC), _contract_mirror(bufs, lambda a: a), "baseline")


@pytest.mark.parametrize("form", sc.ACCEPTED, ids=[f[0] for f in sc.ACCEPTED])
def test_accepted_forms_run_inside_their_buffers(cases, form):
    """every accepted form of the table: enqueued, the outputs it names written where the mirror says, the others untouched"""
    name, mutate = form
    ar, bufs, resolve = _contract_arena(cases["b"])
    a = mutate(sc.baseline(resolve))
    assert sc.invoke(hl.load(), a, torch.cuda.current_stream().cuda_stream) == 0, name
    ar.fetch()
    ar.assert_guards_intact()
    want = _contract_mirror(bufs, mutate)
    got = _contract_outputs(bufs, a.C)
    for field, buf in (("ens_out", "ens_out"), ("pred_out", "pred_out"), ("table_out", "table_out")):
        if not getattr(a, field):
            ar.assert_untouched(bufs[buf])
    ar.assert_untouched(bufs["ens_out"], np.s_[:, a.C:])
    ar.assert_untouched(bufs["table_out"], np.s_[:, 18:])
    if not a.confusion_out:
        assert not bufs["confusion_out"].bits().any()
    # compare what the form asked for; the mirror fills in what it did not
    if not a.ens_out:
        got["ensemble"] = want["ensemble"]
    if not a.pred_out:
        got["pred"] = want["pred"]
    if not a.table_out:
        got["table"] = want["table"]
    if not a.confusion_out:
        got["confusion"] = want["confusion"]
    elif a.C < sc.NC:
        got["confusion"] = np.ascontiguousarray(got["confusion"].reshape(-1)[:4 * a.C * a.C].reshape(4, a.C, a.C))
    assert_scores(got, want, name)


# ---- classifiers that read device rolls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["pitch", "velocity", "instrument"])
def test_predict_on_device_rolls_is_predict_on_host_arrays(kind, dtype):
    """37 windows at batch 16: the last engine batch has 5 windows in 16 padded columns, right after a full one whose columns 5..15
    are stale.  The device copy stages the same bytes the host staging does and zeroes the same pad: BIT-EQUAL probabilities, as a
    device tensor and read back"""
    from midi_vae_amd.classifier import StyleClassifier
    rng = np.random.default_rng(37)
    T, K, n, bs = 16, 13, 37, 16
    clf = StyleClassifier(kind, input_dim=K, num_classes=3, lstm_size=64, num_layers=2, compute_dtype=dtype, seed=6)
    if kind == "velocity":
        roll = np.where(rng.random((n, T)) < 0.4, 0.0, rng.random((n, T))).astype(np.float32)
        host_x = roll[..., None]
    else:
        roll = rng.integers(0, K, (n, T)).astype(np.uint8)
        host_x = roll
    want = clf.predict(host_x, batch_size=bs)
    assert want.shape == (n, 3) and want.dtype == np.float32 and np.all(np.abs(want.sum(1) - 1) < 1e-2) and len(np.unique(want[:, 0])) > 10
    dev_roll = torch.from_numpy(roll).to(DEV)
    clf.predict(dev_roll[:bs], batch_size=bs, as_device=True)          # a full batch first: every pad column of the next tail is stale
    got = clf.predict(dev_roll, batch_size=bs, as_device=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (n, 3) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "device roll, device result"
    assert np.array_equal(clf.predict(dev_roll, batch_size=bs).view(np.uint32), want.view(np.uint32)), "device roll, host result"
    assert np.array_equal(clf.predict(host_x, batch_size=bs, as_device=True).cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a strided view - the transpose of a time-major buffer, what a decode leaves behind - is the same roll
    tm = torch.zeros((T, 48), dtype=dev_roll.dtype, device=DEV)
    tm[:, :n] = dev_roll.t()
    assert np.array_equal(clf.predict(tm.t()[:n], batch_size=bs).view(np.uint32), want.view(np.uint32)), "strided device roll"
    eng = clf.engine
    name = "in.x_val" if kind == "velocity" else "in.x_idx"
    assert not eng._v(name, T, 16)[:, 5:].any(), "the pad columns of the last batch are not zero"
    with pytest.raises(ValueError):
        clf.predict(dev_roll.to(torch.float64), batch_size=bs)
    with pytest.raises(ValueError):
        eng.stage_device(dev_roll.t()[:8], 5)


# ---- the public surface: a decode joined to the judges --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """a tiny VAE (GRU, H = 64, Z = 16, T = 16, 4 voices, 3 style classes, instrument and velocity heads), three judges, 3 songs of
    2 to 5 windows"""
    from midi_vae_amd.classifier import StyleClassifier
    from midi_vae_amd.config import build_settings, create_kwargs
    from midi_vae_amd.model import VAE
    s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=16, input_length=4, output_length=4, max_voices=4, batch_size=8,
                       classes=("a", "b", "c"))
    m = VAE().create(compute_dtype="f32", seed=8, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z, m.spec.C) == (16, 4, 16, 3) and s["meta_velocity"] and s["meta_instrument"]
    mk = lambda kind, K, seed: StyleClassifier(kind, input_dim=K, num_classes=3, lstm_size=64, num_layers=2, compute_dtype="f32", seed=seed)
    judges = st.Judges(mk("pitch", s["output_dim"], 1), mk("velocity", 1, 2), mk("instrument", s["meta_instrument_dim"], 3),
                       weights=(0.499, 0.3, 0.2))
    rng = np.random.default_rng(88)
    zs = [rng.standard_normal((m_i, 16)) * 2.0 for m_i in (2, 5, 3)]
    return s, m, judges, zs, [2, 0, 1]


def _host_judges(judges, s, Y, I, V, bs):
    """host ``predict`` of the three judges on what process_decoder_indices returns, the way the reference feeds them (:2491-2520)"""
    T = s["output_length"]
    n = Y.shape[0] // T
    pitch_in = np.append(Y, np.zeros((Y.shape[0], 1)), axis=1)
    pitch_in[pitch_in.sum(1) == 0, -1] = 1
    return (judges.pitch.predict(pitch_in.reshape(n, T, -1), batch_size=bs), judges.velocity.predict(V.reshape(n, T, 1), batch_size=bs),
            judges.instrument.predict(np.asarray(I), batch_size=bs))


def _assert_style(got, table_row, ens_rows, what):
    """a reported ``style`` dict against the mirror's table row and ensemble rows"""
    assert got["windows"] == int(table_row[0]), what
    for j, name in enumerate(st.JUDGES):
        assert got[name]["accuracy"] == table_row[1 + 2 * j], (what, name)
        assert sc.device_mean_ratio(got[name]["confidence"], table_row[2 + 2 * j], got["windows"]) <= 1.0, (what, name)
    assert np.array_equal(got["ensemble_prediction"].view(np.uint32), ens_rows.view(np.uint32)), what


def test_switch_styles_against_the_host_route(tiny):
    from midi_vae_amd import events as ev
    from midi_vae_amd import packers as pk
    s, m, judges, zs, classes = tiny
    dec, T, bs = m.decoder, 16, 8
    S = [np.random.default_rng(i).standard_normal((z.shape[0], s["signature_vector_length"])) for i, z in enumerate(zs)]
    programs = [[0, 24, 40, 56], [8, 8, 8, 8], [0, 0, 120, 127]]
    got = dec.switch_styles(zs, classes, S=S, judges=judges, note_events=True, batch_size=bs, programs=programs)
    pairs = st.switch_pairs(classes, 3)
    assert [(d["song"], d["C"], d["C_switch"]) for d in got["pairs"]] == pairs and len(pairs) == 6

    # the host route: every switched window decoded in a call of its own, as the reference does (:2471-2483)
    Ys, Is, Vs, lengths, idx_rows = [], [], [], [], []
    for song, C, C_switch in pairs:
        switched, history = st.switched_latents(zs[song], C, C_switch)
        for i in range(switched.shape[0]):
            x = pk.prepare_decoder_input(s, switched[i:i + 1], C_switch, S[song][i:i + 1], history[i:i + 1])
            idx = dec.predict_indices(x, batch_size=bs)
            Y, I, V, D, N = pk.process_decoder_indices(s, idx)
            Ys.append(Y), Is.append(I[0]), Vs.append(V), idx_rows.append(idx)
        lengths.append(switched.shape[0])
    n = sum(lengths)
    notes = np.concatenate([r["notes"] for r in idx_rows], 0)
    instr = np.concatenate([r["instr"] for r in idx_rows], 0)
    velocity = np.concatenate(Vs).reshape(n, T)
    assert (notes != s["new_num_notes"]).any(), "the model decodes nothing to judge"
    tables = _host_judges(judges, s, np.concatenate(Ys, 0), Is, np.concatenate(Vs), bs)
    off = st.song_groups(lengths)
    own = st.scores(tables[0], tables[1], tables[2], np.repeat([C for _, C, _ in pairs], lengths).astype(np.uint8), off,
                    weights=judges.weights, device=False)
    target = st.scores(tables[0], tables[1], tables[2], np.repeat([t for _, _, t in pairs], lengths).astype(np.uint8), off,
                       weights=judges.weights, device=False)
    voted = ev.vote_for_programs(instr, lengths, s)
    starts = (~(velocity > s["velocity_threshold_such_that_it_is_a_played_note"])).astype(np.uint8)
    events = ev.note_events(notes, velocity.astype(np.float32), starts, lengths, s, device=False)
    lo = 0
    for k, (d, m_k) in enumerate(zip(got["pairs"], lengths)):
        what = "pair %d" % k
        assert np.array_equal(d["notes"], notes[lo:lo + m_k]) and np.array_equal(d["instr"], instr[lo:lo + m_k]), what
        assert d["velocity"].dtype == np.float32 and np.array_equal(d["velocity"].astype(np.float64), velocity[lo:lo + m_k]), what
        _assert_style(d["style"], own["table"][k], own["ensemble"][lo:lo + m_k], what)
        _assert_style(dict(d["style_target"], ensemble_prediction=d["style"]["ensemble_prediction"]), target["table"][k], own["ensemble"][lo:lo + m_k], what)
        assert d["voted_programs"] == voted[k] and d["instruments_switched"] == (voted[k] != programs[d["song"]]), what
        assert d["programs"] == (voted[k] if d["instruments_switched"] else programs[d["song"]]), what
        assert np.array_equal(d["events"], events[k]), what
        assert d["signature"].shape == (m_k, 15) and d["harmonicity"].shape == (m_k, 4, 4), what
        lo += m_k
    from midi_vae_amd import descriptors
    assert np.array_equal(np.concatenate([d["signature"] for d in got["pairs"]], 0), descriptors.signature_vectors(notes, s), equal_nan=True)
    assert np.array_equal(np.concatenate([d["harmonicity"] for d in got["pairs"]], 0), descriptors.harmonicity(notes, s), equal_nan=True)
    assert np.array_equal(got["switch_instruments_matrix"], st.switch_instruments_matrix(pairs, programs, voted, 3))
    assert got["switch_instruments_matrix"].sum() == 4 * len(pairs)
    plain = dec.switch_styles(zs, classes, S=S, batch_size=bs)
    assert plain["switch_instruments_matrix"] is None and all("style" not in d and "events" not in d for d in plain["pairs"])
    assert all(np.array_equal(a["notes"], b["notes"]) for a, b in zip(plain["pairs"], got["pairs"]))


def test_predict_songs_with_judges_against_the_host_route(tiny):
    from midi_vae_amd import packers as pk
    s, m, judges, zs, classes = tiny
    dec, T, bs = m.decoder, 16, 8
    xs = [pk.prepare_decoder_input(s, z, C, np.zeros((z.shape[0], s["signature_vector_length"])), None) for z, C in zip(zs, classes)]
    got = dec.predict_songs(xs, batch_size=bs, judges=judges, classes=classes)
    plain = dec.predict_songs(xs, batch_size=bs)
    Ys, Is, Vs, lengths = [], [], [], [z.shape[0] for z in zs]
    for x in xs:          # a whole song through process_decoder_indices: the velocity rules carry through it
        Y, I, V, D, N = pk.process_decoder_indices(s, dec.predict_indices(x, batch_size=bs))
        Ys.append(Y), Is.extend(I), Vs.append(V)
    tables = _host_judges(judges, s, np.concatenate(Ys, 0), Is, np.concatenate(Vs), bs)
    want = st.scores(tables[0], tables[1], tables[2], np.repeat(classes, lengths).astype(np.uint8), st.song_groups(lengths),
                     weights=judges.weights, device=False)
    lo = 0
    for i, (d, p, m_i) in enumerate(zip(got, plain, lengths)):
        assert sorted(set(d) - set(p)) == ["style"] and all(np.array_equal(d[k], p[k]) for k in p), i
        assert np.array_equal(d["velocity"].astype(np.float64), Vs[i].reshape(m_i, T)), i
        _assert_style(d["style"], want["table"][i], want["ensemble"][lo:lo + m_i], "song %d" % i)
        lo += m_i
    with pytest.raises(ValueError):
        dec.predict_songs(xs, batch_size=bs, judges=judges)


def test_latent_sweep_with_and_without_judges(tiny):
    from midi_vae_amd import sweep as sw
    s, m, judges, zs, classes = tiny
    dec, bs = m.decoder, 8
    z = zs[1][:2]
    plain = dec.latent_sweep(z, evaluations_per_dimension=2, batch_size=bs, return_rolls=True)
    got = dec.latent_sweep(z, evaluations_per_dimension=2, batch_size=bs, return_rolls=True, judges=judges)
    n, Z, K = 2, 16, 3
    assert sorted(set(got) - set(plain)) == ["style"] and got["style"].shape == (n, Z, K, 3) and got["style"].dtype == np.float32
    for key in ("table", "programs", "values", "notes", "velocity"):
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    # without judges: today's result, key for key - the host summaries of the same table
    today = sw.summarize_sweep(plain["table"], plain["programs"])
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a == b
    for i in range(n):
        for d in range(Z):
            a, b = plain["summaries"][i][d], today[0][i][d]
            assert list(a) == list(b) and not any("style" in k for k in a), (i, d)
            assert all(same(a[k][0], b[k][0]) and same(a[k][1], b[k][1]) for k in a), (i, d)
    assert plain["most_peaked"] == today[2] and plain["overall_best"] == today[3]
    # the class-0 probabilities: host predict on the rolls, the same classifier batches (windows in order, 8 at a time)
    T, V = 16, 4
    notes, vel = got["notes"].reshape(-1, T), got["velocity"].reshape(-1, T)
    instr = (got["programs"].reshape(-1, V) // 8).astype(np.uint8)
    want = np.stack([judges.pitch.predict(notes, batch_size=bs)[:, 0], judges.velocity.predict(vel[..., None], batch_size=bs)[:, 0],
                     judges.instrument.predict(instr, batch_size=bs)[:, 0]], axis=1)
    assert np.array_equal(got["style"].reshape(-1, 3).view(np.uint32), want.view(np.uint32))
    seen = set()
    for i in range(n):
        for d in range(Z):
            a = got["summaries"][i][d]
            b = sw.summarize(got["table"][i, d], got["programs"][i, d], style=got["style"][i, d])
            assert list(a) == list(b) and all(same(a[k][0], b[k][0]) and same(a[k][1], b[k][1]) for k in a), (i, d)
            rest, before = {k: v for k, v in a.items() if "style" not in k}, plain["summaries"][i][d]
            assert list(rest) == list(before) and all(same(rest[k][0], before[k][0]) and same(rest[k][1], before[k][1]) for k in rest), (i, d)
            styles = sorted(k.rsplit("_", 1)[0] for k in a if "style" in k)
            assert "mean_instrumentstyle" in styles and set(styles) <= {"mean_pitchstyle", "mean_velocitystyle", "mean_instrumentstyle"}
            assert ("mean_pitchstyle" in styles) == (got["table"][i, d, :, 0] > 0).any()
            assert ("mean_velocitystyle" in styles) == (got["table"][i, d, :, 9] > 0).any()
            seen.update(styles)
    assert len(seen) == 3, "the sweep never met a pitch or a note start: %r" % sorted(seen)
    assert any("style" in k for k in got["influence"]) and any("style" in k for k in got["overall_best"])


def test_score_originals_judges_a_songs_instruments_once(tiny):
    """the reference's original-songs block: one instrument row per song, whose figure is that single prediction (exactly: the
    mean of m copies of a float32 is that float32) and whose accuracy is 0 or 1"""
    s, m, judges, zs, classes = tiny
    rng = np.random.default_rng(61)
    lengths, T, bs = (3, 1, 6), 16, 8
    X_idx = [rng.integers(0, 61, (m_i, T)).astype(np.uint8) for m_i in lengths]
    V = [np.where(rng.random((m_i, T)) < 0.4, 0.0, rng.random((m_i, T))).astype(np.float32) for m_i in lengths]
    I_idx = [rng.integers(0, 16, 4).astype(np.uint8) for _ in lengths]
    got = st.score_originals(X_idx, V, I_idx, classes, judges, batch_size=bs)
    tables = (judges.pitch.predict(np.concatenate(X_idx, 0), batch_size=bs), judges.velocity.predict(np.concatenate(V, 0)[..., None], batch_size=bs),
              judges.instrument.predict(np.stack(I_idx, 0), batch_size=bs))
    want = st.scores(tables[0], tables[1], tables[2], np.repeat(classes, lengths).astype(np.uint8), st.song_groups(lengths),
                     np.repeat(np.arange(3), lengths), judges.weights, device=False)
    lo = 0
    for g, m_g in enumerate(lengths):
        _assert_style(got[g]["style"], want["table"][g], want["ensemble"][lo:lo + m_g], "song %d" % g)
        assert got[g]["style"]["instrument"]["confidence"] == float(tables[2][g, classes[g]])
        assert got[g]["style"]["instrument"]["accuracy"] == float(np.argmax(tables[2][g]) == classes[g])
        lo += m_g
