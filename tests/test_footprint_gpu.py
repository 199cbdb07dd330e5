"""Which memory the main kernels touch (GPU box only): guarded, sentinel-filled outputs for the recurrent, head, sampling, GEMM and
weight-preparation kernels (tests/footprint.py; the checker itself is checked in test_footprint_cpu.py).

The value tests (test_ops_gpu.py and its neighbours) hand every kernel tight ``torch.zeros`` outputs: a pad row written past the end
of a tensor, an element a kernel must write but does not, and a result that depends on what the output held before all pass there.
Here every case runs the kernel TWICE on the same inputs - once with every output (and every float input) carved from one arena,
neighbours guarding each other, sentinel NaNs everywhere; once into tight zero-filled buffers as the value tests do - and asserts

  1. the guards are intact;
  2. the documented extent is fully written, documented pad is exactly zero, documented gaps are untouched;
  3. every output that is not accumulated atomically is bit-identical between the two runs;
  4. the arena run passes the existing oracle check of that kernel (parity.assert_parity / assert_product / assert_bits, the problem
     builders and constants of tests/parity.py; no tolerance of its own);
  5. accumulated outputs (the heads' scalars, accumulate / split-K C, colsum_b) start from small integers and are driven with
     parity.integer_operands where the kernel allows: then they are bit-comparable too.  The heads' loss word is a sum of
     row_weight x cross-entropy - never integers, and its atomics arrive in any order: it is held to parity.LOSS_RTOL, the hit
     count beside it exactly.

Float inputs sit at their exact size in the arena with NaN sentinels behind them: an over-read that is USED fails point 4.  What
these tests cannot see: an over-read whose value is not used, and over-reads of index arrays (their guards hold the valid index 0
so that no gather can leave its table).  No test here plants an out-of-range index or hands a kernel a buffer below its documented
size.  Row isolation: one more launch with batch row 2 of the inputs NaN - every other row of every output keeps its bits."""
import copy

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops, sampling
from oracle import vae_oracle as vo
from tests import footprint as fp
from tests import parity as par
from tests.gpu_util import DEV, dev, host, pairing, tile16
from test_choice_decode_cpu import excluded_rows, integer_problem
from test_ops_gpu import seq_layouts
from test_rnn_handover_gpu import BF16, F32, Bwd, Fwd, Out, _waves, bwd_problem, fwd_problem
from test_small_ops_gpu import _tile16_offsets

pytestmark = pytest.mark.gpu

T3 = 3
NAN_ROW = 2


class Case(dict):
    """a dict whose keys read and write as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def zeros(shape, dt=torch.float32):
    return torch.zeros(tuple(shape), dtype=dt, device=DEV)


def carve_in(ar, name, t, guard="sentinel"):
    """a device tensor as an input at its exact size in the arena (None stays None)"""
    return None if t is None else ar.carve(name, tuple(t.shape), t.dtype, data=t.contiguous(), guard=guard)


def tensor(b):
    return None if b is None else b.t


def same_as_tight(bufs, tight, what, skip=()):
    """point 3: every output of the arena run has the bits of the tight zero-filled run"""
    for k, b in bufs.items():
        if b is not None and k not in skip:
            fp.assert_same_bits(b, tight[k], "%s %s" % (k, what))


def other_rows_keep_their_bits(got, clean, axis, what):
    """row isolation: ``got`` (the run with batch row NAN_ROW poisoned) against the clean run, both as integer arrays"""
    g, c = np.delete(got, NAN_ROW, axis=axis), np.delete(clean, NAN_ROW, axis=axis)
    diff = g != c
    assert not diff.any(), "%s: %d elements of rows other than %d changed with that row's inputs, first at %s" % (
        what, int(diff.sum()), NAN_ROW, tuple(int(i) for i in np.argwhere(diff)[0]))


def test_sentinels_survive_the_copies_of_gpu_util_as_bits():
    """host(): device -> float64 keeps the payload of both sentinels; dev(): float64 -> f32 keeps it as well"""
    ar = fp.Arena(DEV)
    f, h = ar.carve("f", (5, 3), torch.float32), ar.carve("h", (5, 3), torch.bfloat16)
    ar.commit().fetch()
    assert np.all(f.bits() == fp.F32_SENTINEL) and np.all(h.bits() == fp.BF16_SENTINEL)
    assert np.all(fp.f32_bits(host(f.t)) == fp.F32_SENTINEL) and np.all(fp.f32_bits(host(h.t)) == fp.BF16_SENTINEL << 16)
    back = dev(host(f.t))
    assert np.all(back.view(torch.int32).cpu().numpy().view(np.uint32) == fp.F32_SENTINEL)
    ar.assert_guards_intact()


# ---- recurrent kernels ------------------------------------------------------------------------------------------------------
SAVES = ["all", "hs", "none"]              # training (hs, cs, acts, h_last, c_last); the h sequence only; inference (h_last only)


def _fwd_outputs(fw, save, make):
    """the outputs of one save mode: ``make(name, shape, torch type)`` allocates"""
    T, B, H, GH, td = fw.T, fw.B, fw.H, fw.GH, fw.td
    train = save == "all"
    return dict(hs=make("hs", (T + 1, B, H), td) if save != "none" else None,
                cs=make("cs", (T + 1, B, H), td) if fw.lstm and train else None,
                acts=make("acts", (T, B, GH), td) if train else None,
                h_last=make("h_last", (B, H), torch.float32),
                c_last=make("c_last", (B, H), torch.float32) if fw.lstm and train else None)


def _fwd_in_arena(fw, save):
    """every float input and every output of ``fw`` carved from one arena: (arena, a copy of fw that launches on them, output Bufs)"""
    ar = fp.Arena(DEV)
    ins = {k: carve_in(ar, k, v, "zero" if k == "idx" else "sentinel") for k, v in fw.kw.items() if torch.is_tensor(v)}
    h0, c0 = carve_in(ar, "h0", fw.h0), carve_in(ar, "c0", fw.c0)
    bufs = _fwd_outputs(fw, save, ar.carve)
    ar.commit()
    fa = copy.copy(fw)
    fa.kw = dict(fw.kw)
    fa.kw.update({k: b.t for k, b in ins.items()})
    fa.h0, fa.c0 = h0.t, tensor(c0)
    return ar, fa, bufs


def _row_major(fw, t, rows, cols):
    return tile16(t, rows, cols, False, paired=pairing(fw.lay)) if fw.tiled else t


def _fwd_parity(fw, out, what):
    pb, T, B, H, GH = fw.pb, fw.T, fw.B, fw.H, fw.GH
    if out["hs"] is not None:
        par.assert_parity(host(out["hs"]), pb.hs, fw.dt, par.step_blocks, "hs " + what, values=True)
    if out["acts"] is not None:
        par.assert_parity(host(_row_major(fw, out["acts"], T * B, GH)), pb.acts, fw.dt, par.gate_blocks(pb.cellname), "acts " + what, values=True)
    if out["cs"] is not None:
        par.assert_parity(host(_row_major(fw, out["cs"], (T + 1) * B, H)), pb.cs, fw.dt, par.step_blocks, "cs " + what, values=True)
    par.assert_parity(host(out["h_last"]), pb.hs[-1], fw.dt, par.whole, "h_last " + what, values=True)
    if out["c_last"] is not None:
        par.assert_parity(host(out["c_last"]), pb.cs[-1], fw.dt, par.whole, "c_last " + what, values=True)


def _fwd_arena_run(fw, save, what):
    """points 1 and 2 of one forward launch into an arena; returns (arena, output Bufs)"""
    ar, fa, bufs = _fwd_in_arena(fw, save)
    fa.launch(Out({k: tensor(b) for k, b in bufs.items()}))
    ar.fetch()
    ar.assert_guards_intact()
    for k, b in bufs.items():
        if b is not None:
            ar.assert_written(b)               # (hs / cs slot 0 included: it receives h0 / c0)
    return ar, bufs


def _fwd_footprint(cellname, H, B, dt, xmode, lay, T, save):
    fw = Fwd(fwd_problem(cellname, H, T, B, dt, xmode), lay, dt)
    what = "(%s %s H=%d B=%d T=%d %s, layout %d, save %s)" % (cellname, "bf16" if dt == BF16 else "f32", H, B, T, xmode, lay, save)
    tight = _fwd_outputs(fw, save, lambda n, s, d: zeros(s, d))
    fw.launch(Out(tight))
    ar, bufs = _fwd_arena_run(fw, save, what)
    same_as_tight(bufs, tight, what)
    _fwd_parity(fw, {k: tensor(b) for k, b in bufs.items()}, what)
    return fw, bufs


def _poisoned_forward_problem(pb):
    """batch row NAN_ROW of every float input is NaN (an indexed input keeps its table: only that row's initial state is poisoned)"""
    p = par.Problem(pb)
    p.update(vars(pb))                     # (the builder sets xp, xs, ... as attributes: a copy of the dict alone loses them)
    for k, sl in (("h0", np.s_[NAN_ROW]), ("c0", np.s_[NAN_ROW]), ("xp0", np.s_[NAN_ROW]), ("xs", np.s_[:, NAN_ROW])):
        if p.get(k) is not None:
            p[k] = np.array(p[k], np.float64)
            p[k][sl] = np.nan
    if p.xmode == "dense":
        p["xp"] = np.array(p.xp, np.float64)
        p["xp"][:, NAN_ROW] = np.nan
    return p


def _fwd_row_isolation(fw, clean, what):
    fn = Fwd(_poisoned_forward_problem(fw.pb), fw.lay, fw.dt)
    ar, bufs = _fwd_arena_run(fn, "all", what + " (row %d NaN)" % NAN_ROW)
    assert np.isnan(bufs["h_last"].values()[NAN_ROW]).all(), "the poisoned row did not reach h_last " + what
    for k, b in bufs.items():
        if b is not None:
            other_rows_keep_their_bits(b.bits(), clean[k].bits(), b.bits().ndim - 2, "%s %s" % (k, what))


CELLNAMES = ["GRU", "LSTM", "SimpleRNN"]
# (64, 5): one partial workgroup; (64, 21): a full one and a partial one; f32 (256, 21): the 8-wave instantiation; LSTM (320, 5): late-x
GENERIC = ([(c, dt, 64, B) for c in CELLNAMES for dt in (F32, BF16) for B in (5, 21)] + [(c, F32, 256, 21) for c in CELLNAMES] +
           [("LSTM", dt, 320, 5) for dt in (F32, BF16)])


def _gid(case):
    return "-".join("bf16" if v == BF16 and i == 1 else "f32" if v == F32 and i == 1 else str(v) for i, v in enumerate(case))


@pytest.mark.parametrize("case", GENERIC, ids=_gid)
def test_generic_forward(case):
    """rnn.hip, forward: all four input modes at (64, 21), dense elsewhere; the three save modes; row isolation on the training save"""
    cellname, dt, H, B = case
    for xmode in (["dense", "index", "scalar", "const"] if (H, B) == (64, 21) else ["dense"]):
        for save in SAVES:
            fw, bufs = _fwd_footprint(cellname, H, B, dt, xmode, hl.ROWMAJOR, T3, save)
            if save == "all":
                _fwd_row_isolation(fw, bufs, "(%s %s)" % (cellname, xmode))


def _bwd_outputs(bw, make):
    T, B, H, GH, td = bw.T, bw.B, bw.H, bw.GH, bw.td
    return dict(da=make("da", (T, B, GH), td), rh=make("rh", (T, B, H), td) if bw.gru else None,
                dh0=make("dh0", (B, H), torch.float32), dc0=make("dc0", (B, H), torch.float32) if bw.lstm else None)


def _bwd_in_arena(bw):
    """every input and output of ``bw`` carved from one arena"""
    ar = fp.Arena(DEV)
    names = ("hs", "cs", "acts", "dext", "dlast", "dclast")
    ins = {k: carve_in(ar, k, getattr(bw, k)) for k in names}
    bufs = _bwd_outputs(bw, ar.carve)
    ar.commit()
    ba = copy.copy(bw)
    for k in names:
        setattr(ba, k, tensor(ins[k]))
    return ar, ba, bufs


def _bwd_launch_in_arena(bw):
    ar, ba, bufs = _bwd_in_arena(bw)
    ba.launch(Out({k: tensor(b) for k, b in bufs.items()}))
    ar.fetch()
    ar.assert_guards_intact()
    for b in bufs.values():
        if b is not None:
            ar.assert_written(b)
    return ar, bufs


def _bwd_footprint(cellname, H, B, dt, ext, lay, T):
    bw = Bwd(bwd_problem(cellname, H, T, B, dt, ext), lay, dt)
    what = "(%s %s H=%d B=%d T=%d ext=%s, layout %d)" % (cellname, "bf16" if dt == BF16 else "f32", H, B, T, ext, lay)
    tight = _bwd_outputs(bw, lambda n, s, d: zeros(s, d))
    bw.launch(Out(tight))
    ar, bufs = _bwd_launch_in_arena(bw)
    same_as_tight(bufs, tight, what)
    bw.check_parity(Out({k: tensor(b) for k, b in bufs.items()}), what)
    return bw, bufs


def _bwd_row_isolation(bw, clean, what):
    p = par.Problem(bw.pb)
    for k in ("dext", "dlast", "dclast", "hs_r", "cs_r", "acts_r"):
        if p.get(k) is not None:
            p[k] = np.array(p[k], np.float64)
            p[k][..., NAN_ROW, :] = np.nan
    with np.errstate(all="ignore"):
        bn = Bwd(p, bw.lay, bw.dt)
    ar, bufs = _bwd_launch_in_arena(bn)
    assert np.isnan(bufs["dh0"].values()[NAN_ROW]).all(), "the poisoned row did not reach dh0 " + what
    for k, b in bufs.items():
        if b is not None:
            other_rows_keep_their_bits(b.bits(), clean[k].bits(), b.bits().ndim - 2, "%s %s" % (k, what))


@pytest.mark.parametrize("ext", [True, False], ids=["ext", "noext"])
@pytest.mark.parametrize("case", GENERIC, ids=_gid)
def test_generic_backward(case, ext):
    """rnn.hip, BPTT with and without dhs_ext: da, rh (GRU), dh0, dc0 (LSTM); row isolation"""
    cellname, dt, H, B = case
    bw, bufs = _bwd_footprint(cellname, H, B, dt, ext, hl.ROWMAJOR, T3)
    _bwd_row_isolation(bw, bufs, "(%s ext=%s)" % (cellname, ext))


RES_B = 48
RES_T = [1, 3, 4]              # the single step, a pair plus a trailing step, pairs only


@pytest.mark.parametrize("T", RES_T)
@pytest.mark.parametrize("cellname", ["LSTM", "GRU"])
def test_resident_forward(cellname, T):
    """rnn_resident.hip / rnn_w8.hip, forward at H = 256, bf16, B = 48: every layout seq_layouts() gives, dense / index / const inputs
    (and scalar for TILE16), training and inference saves.  acts and cs are tiled: the whole buffer is the region."""
    for xmode in ("dense", "index", "const", "scalar"):
        for lay in seq_layouts(True, cellname, xmode):
            for save in ("all", "none"):
                _fwd_footprint(cellname, par.RES_H, RES_B, BF16, xmode, lay, T, save)


@pytest.mark.parametrize("T", RES_T)
@pytest.mark.parametrize("cellname", ["LSTM", "GRU"])
def test_resident_backward(cellname, T, monkeypatch):
    monkeypatch.delenv("MVAE_LSTM_BWD_W8", raising=False)
    for ext in (True, False):
        for lay in seq_layouts(True, cellname, forward=False):
            _bwd_footprint(cellname, par.RES_H, RES_B, BF16, ext, lay, T)


def test_resident_backward_lstm_on_two_waves_per_simd(monkeypatch):
    """MVAE_LSTM_BWD_W8=1: the LSTM BPTT of rnn_w8.hip (TILE16P data), as test_ops_gpu.py runs it"""
    monkeypatch.setenv("MVAE_LSTM_BWD_W8", "1")
    _bwd_footprint("LSTM", par.RES_H, RES_B, BF16, True, hl.TILE16P, T3)


# ---- phase launches ---------------------------------------------------------------------------------------------------------
PHASE = [(4, 16, "index"), (4, 32, "dense")]          # (T, B, input mode); the dense problem reads what the expansion producer writes
PHASE_CS, PHASE_BLOCKS = 2, 2


@pytest.mark.parametrize("cellname,lay", [("LSTM", hl.TILE16P), ("GRU", hl.TILE16P), ("GRU", hl.TILE16Q)])
def test_phase_launches(cellname, lay):
    """one mvae_rnn_fwd_multi of two problems (B = 16 and B = 32, T = 4) plus one xpand producer that feeds the second, and the
    matching mvae_rnn_bwd_multi: every output of every problem from ONE arena, bit-equal to the single launches into tight buffers"""
    H, GH = par.RES_H, vo.GATES[cellname] * par.RES_H
    (T0, B0, xm0), (T1, B1, _) = PHASE
    R, n = T1 * B1, T1 // PHASE_CS
    x = par.xpand_problem(GH, R, seed=GH + 1)
    xs, w, bias = dev(x.xs), dev(x.w), dev(x.bias)
    want = zeros((T1, B1, GH), torch.bfloat16)
    ops.outer_bias_tile16(xs, w, bias, want, R, GH)
    base = fwd_problem(cellname, H, T1, B1, BF16, "const", seed=par.phase_seed(1, cellname))
    p1 = par.Problem(base)
    p1.update(xmode="dense", xp=host(tile16(want, R, GH, False)), xp0=None)
    p1.hs, p1.cs, p1.acts = vo.rnn_forward(cellname, p1.xp, p1.U, p1.h0, p1.c0)
    fws = [Fwd(fwd_problem(cellname, H, T0, B0, BF16, xm0, seed=par.phase_seed(0, cellname)), lay, BF16), Fwd(p1, lay, BF16)]
    tight = [_fwd_outputs(fw, "all", lambda n_, s, d: zeros(s, d)) for fw in fws]
    fws[0].launch(Out(tight[0]))
    fws[1].launch(Out(tight[1]), xp=want)
    # the phase launch: inputs, the producer's out, its counters and every output of both problems in one arena
    ar = fp.Arena(DEV)
    ins = [{k: carve_in(ar, "%s[%d]" % (k, i), v, "zero" if k == "idx" else "sentinel") for k, v in fw.kw.items()
            if torch.is_tensor(v) and not (i == 1 and k == "xp")} for i, fw in enumerate(fws)]
    states = [(carve_in(ar, "h0[%d]" % i, fw.h0), carve_in(ar, "c0[%d]" % i, fw.c0)) for i, fw in enumerate(fws)]
    xin = [carve_in(ar, "xs", xs), carve_in(ar, "w", w), carve_in(ar, "bias", bias)]
    xout = ar.carve("xpand out", (T1, B1, GH), torch.bfloat16)
    done = ar.carve("chunk_done", (n,), torch.int32, prefill=np.zeros(n, np.int64))
    status = ar.carve("status", (1,), torch.int32, prefill=np.zeros(1, np.int64))
    bufs = [_fwd_outputs(fw, "all", lambda n_, s, d, i=i: ar.carve("%s[%d]" % (n_, i), s, d)) for i, fw in enumerate(fws)]
    ar.commit()
    fas = []
    for i, fw in enumerate(fws):
        fa = copy.copy(fw)
        fa.kw = dict(fw.kw)
        fa.kw.update({k: b.t for k, b in ins[i].items()})
        fa.h0, fa.c0 = states[i][0].t, tensor(states[i][1])
        fas.append(fa)
    waves = _waves(lay)
    xa = ops.xpand(xin[0].t, xin[1].t, xin[2].t, xout.t, R, GH, PHASE_CS * B1, done.t, PHASE_BLOCKS)
    args = [fas[0].launch(Out({k: tensor(b) for k, b in bufs[0].items()}), build_only=True),
            fas[1].launch(Out({k: tensor(b) for k, b in bufs[1].items()}), xp=xout.t, chunk_steps=PHASE_CS, wait_ready=done.t,
                          wait_value=waves * PHASE_BLOCKS, status=status.t, build_only=True)]
    assert ops.rnn_fwd_multi(args, [xa]) is True
    ar.fetch()
    ar.assert_guards_intact()
    assert status.bits().tolist() == [0] and done.bits().tolist() == [waves * PHASE_BLOCKS] * n
    ar.assert_written(xout)
    fp.assert_same_bits(xout, want, "the producer's out")
    for i, fw in enumerate(fws):
        what = "(forward problem %d of the phase launch)" % i
        for b in bufs[i].values():
            if b is not None:
                ar.assert_written(b)
        same_as_tight(bufs[i], tight[i], what)
        _fwd_parity(fw, {k: tensor(b) for k, b in bufs[i].items()}, what)

    # backward: the BPTT of the same two shapes, with and without an upstream gradient
    bws = [Bwd(bwd_problem(cellname, H, T, B, BF16, ext), lay, BF16) for (T, B, _), ext in zip(PHASE, (False, True))]
    tightb = [_bwd_outputs(bw, lambda n_, s, d: zeros(s, d)) for bw in bws]
    for bw, out in zip(bws, tightb):
        bw.launch(Out(out))
    ar = fp.Arena(DEV)
    names = ("hs", "cs", "acts", "dext", "dlast", "dclast")
    insb = [{k: carve_in(ar, "%s[%d]" % (k, i), getattr(bw, k)) for k in names} for i, bw in enumerate(bws)]
    bufsb = [_bwd_outputs(bw, lambda n_, s, d, i=i: ar.carve("%s[%d]" % (n_, i), s, d)) for i, bw in enumerate(bws)]
    ar.commit()
    argsb = []
    for i, bw in enumerate(bws):
        ba = copy.copy(bw)
        for k in names:
            setattr(ba, k, tensor(insb[i][k]))
        argsb.append(ba.launch(Out({k: tensor(b) for k, b in bufsb[i].items()}), build_only=True))
    assert ops.rnn_bwd_multi(argsb) is True
    ar.fetch()
    ar.assert_guards_intact()
    for i, bw in enumerate(bws):
        what = "(backward problem %d of the phase launch)" % i
        for b in bufsb[i].values():
            if b is not None:
                ar.assert_written(b)
        same_as_tight(bufsb[i], tightb[i], what)
        bw.check_parity(Out({k: tensor(b) for k, b in bufsb[i].items()}), what)


# ---- heads ------------------------------------------------------------------------------------------------------------------
SC0 = np.array([3.0, 5.0])             # what the two accumulated scalars hold before the launch


def _head_inputs(kind, dtype, N, H, R, two_hot, b_stride, b_valid, fused, nan_row):
    """device inputs and the float64 oracle of one head problem (kind 0: par.softmax_head_problem; kind 1: par.fused_head_problem)"""
    td = ops.torch_dtype(dtype)
    NP = ops.head_np(N)
    if kind == 0:
        _, hs_h, W, bias, tgt, rw, tgt2 = par.softmax_head_problem(N, H, R, seed=N, two_hot=two_hot)
    else:
        hs_h, W, rw, bias, y = par.fused_head_problem(1, 1, H, R, seed=R)
    if nan_row is not None:
        hs_h = hs_h.copy()
        hs_h[nan_row] = np.nan
    d = Case(kind=kind, dtype=dtype, td=td, N=N, NP=NP, H=H, R=R, b_stride=b_stride, b_valid=b_valid, fused=fused)
    d.hs = dev(hs_h, td)
    d.wt = zeros((NP, H), td)
    d.wc = torch.full((H, NP), 7.0, dtype=td, device=DEV) if fused else None
    pb = ops.PrepBatch()
    pb.transpose_convert(dev(W), d.wt, n_pad=NP)
    if fused:
        pb.convert_pad(dev(W), d.wc, NP)
    pb.run()
    torch.cuda.synchronize()
    Wq = host(d.wt)[:N].T
    d.bias, d.rw = dev(bias), dev(rw)
    d.counted = (np.arange(R) % b_stride < b_valid) if b_stride else np.ones(R, bool)
    if kind == 0:
        if b_stride and nan_row is None:        # padding rows whose target IS their argmax: hits if they were counted
            am_o = np.argmax(host(d.hs) @ Wq + bias, 1)
            tgt[~d.counted] = am_o[~d.counted]
            if two_hot:
                tgt2[~d.counted] = 255
        d.tgt, d.tgt2, d.y = dev(tgt, torch.uint8), (dev(tgt2, torch.uint8) if two_hot else None), None
        if nan_row is None:
            d.p, d.loss, d.dl, d.target = par.softmax_head_oracle(host(d.hs), Wq, bias, tgt, rw, 0.7, tgt2)
    else:
        d.tgt, d.tgt2, d.y = None, None, dev(y)
        if nan_row is None:
            p = vo.sigmoid(host(d.hs) @ Wq + bias)[:, 0]
            d.p, d.loss, d.dl, d.y_h = p, np.sum(rw * (p - y) ** 2), (rw * 2 * (p - y) * p * (1 - p))[:, None], y
    return d


def _head_launch(d, ins, out):
    ops.head(d.kind, d.dtype, d.R, d.H, d.N, ins["hs"], ins["wt"], ins["bias"], target_idx=ins["tgt"], target_val=ins["y"],
             row_weight=ins["rw"], grad_scale=0.7 if d.kind == 0 else 1.0, probs=out.get("probs"), argmax=out.get("argmax"),
             dlogits=out.get("dlogits"), scalars=out.get("scalars"), b_stride=d.b_stride, b_valid=d.b_valid, wc=ins["wc"],
             dhs=out.get("dhs"), target_idx2=ins["tgt2"])


def _head_arena(d, inference=False):
    """one launch with every input and output in one arena; points 1 and 2.  ``inference``: only argmax is passed - the probs and
    dlogits buffers beside it must stay untouched"""
    ar = fp.Arena(DEV)
    ins = {k: carve_in(ar, k, d[k], "zero" if k in ("tgt", "tgt2") else "sentinel") for k in ("hs", "wt", "bias", "tgt", "tgt2", "y", "rw", "wc")}
    R, N, NP, H = d.R, d.N, d.NP, d.H
    bufs = dict(probs=ar.carve("probs", (R, N) if d.kind == 0 else (R,), torch.float32), argmax=ar.carve("argmax", (R,), torch.uint8),
                dlogits=ar.carve("dlogits", (R, NP), d.td), dhs=ar.carve("dhs", (R, H), d.td) if d.fused else None,
                scalars=ar.carve("scalars", (4,), torch.float32, prefill=SC0, region=np.s_[:2]))
    ar.commit()
    passed = {k: tensor(b) for k, b in bufs.items()}
    if inference:
        passed = dict(argmax=bufs["argmax"].t)
    _head_launch(d, {k: tensor(b) for k, b in ins.items()}, passed)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(bufs["argmax"])
    ar.assert_untouched(bufs["scalars"], np.s_[2:])          # two words: the words behind them stay
    if inference:
        for k in ("probs", "dlogits"):
            ar.assert_untouched(bufs[k])
        assert np.array_equal(bufs["scalars"].values()[:2], SC0)
        return ar, bufs
    ar.assert_written(bufs["probs"])
    if d.kind == 0:
        ar.assert_written(bufs["dlogits"], np.s_[:, :N])
        if NP > N:
            ar.assert_zero(bufs["dlogits"], np.s_[:, N:])     # the softmax head writes [N, NP) as zeros
    else:
        ar.assert_written(bufs["dlogits"], np.s_[:, :1])
        ar.assert_untouched(bufs["dlogits"], np.s_[:, 1:])    # the sigmoid head stores column 0 only: [1, NP) are the caller's
    if d.fused:
        ar.assert_written(bufs["dhs"])                       # (TILE16: the whole buffer is the region)
    return ar, bufs


def _head_tight(d, inference=False):
    R, N, NP, H = d.R, d.N, d.NP, d.H
    out = dict(probs=zeros((R, N) if d.kind == 0 else (R,)), argmax=zeros((R,), torch.uint8), dlogits=zeros((R, NP), d.td),
               dhs=zeros((R, H), d.td) if d.fused else None, scalars=zeros((2,)))
    _head_launch(d, d, dict(argmax=out["argmax"]) if inference else out)
    torch.cuda.synchronize()
    return out


def _head_footprint(kind, dtype, N, H, R, two_hot=False, b_stride=0, b_valid=0, fused=False):
    d = _head_inputs(kind, dtype, N, H, R, two_hot, b_stride, b_valid, fused, None)
    what = "(kind %d %s N=%d H=%d R=%d)" % (kind, "bf16" if dtype == BF16 else "f32", N, H, R)
    tight = _head_tight(d)
    ar, bufs = _head_arena(d)
    # 3. bit-identical to the tight run: everything but the atomically accumulated scalars; dlogits of kind 1 in column 0 only
    fp.assert_same_bits(bufs["probs"], tight["probs"], "probs " + what)
    fp.assert_same_bits(bufs["argmax"], tight["argmax"], "argmax " + what)
    cols = np.s_[:, :1] if kind == 1 else np.s_[:, :]
    fp.assert_same_bits(bufs["dlogits"].bits()[cols], fp.bits_of(tight["dlogits"])[cols], "dlogits " + what)
    if fused:
        fp.assert_same_bits(bufs["dhs"], tight["dhs"], "dhs " + what)
    # 4. the oracle checks of test_ops_gpu.py on the arena run
    probs, dl, sc = bufs["probs"].values(), bufs["dlogits"].values(), bufs["scalars"].values()[:2] - SC0
    if kind == 0:
        par.assert_parity(probs, d.p, dtype, par.row_blocks, "probs " + what, values=True)
        par.assert_parity(dl[:, :N], d.dl, dtype, par.row_blocks, "dlogits " + what)
        assert np.array_equal(bufs["argmax"].bits(), np.argmax(probs, 1))
        match = np.argmax(probs, 1) == np.argmax(d.target, 1)
        hits = np.sum(match & d.counted)
        if b_stride:
            assert np.sum(match & ~d.counted) > R // 8
    else:
        par.assert_parity(probs[:, None], d.p[:, None], dtype, par.row_blocks, "probs " + what, values=True)
        par.assert_parity(dl[:, :1], d.dl, dtype, par.row_blocks, "dlogits " + what)
        hits = np.sum(np.round(probs.astype(np.float32)) == d.y_h.astype(np.float32))
        assert np.array_equal(bufs["argmax"].bits(), np.round(probs.astype(np.float32)).astype(np.uint8))
    # 5. the scalars started from 3 and 5: the hit count is exact (and so equal to the tight run's), the loss within LOSS_RTOL (the
    #    3.0 it was added to costs half an ulp of the sum, 1e-7 relative: far inside)
    assert sc[1] == hits and sc[1] == host(tight["scalars"])[1], (sc, hits, host(tight["scalars"]))
    par.assert_rel(sc[0], d.loss, par.LOSS_RTOL, "loss " + what)
    if fused:
        want = dl[:, :N if kind == 0 else 1] @ host(d.wc)[:, :N if kind == 0 else 1].T
        assert np.abs(want).max() > 0
        par.assert_parity(host(tile16(bufs["dhs"].t, R, H, False)), want, dtype, par.row_blocks, "dhs " + what)
    return d, bufs


def _head_row_isolation(d, clean, what):
    """hs row NAN_ROW is NaN: every other row of probs, argmax, dlogits and dhs keeps its bits (the scalars take the NaN)"""
    dn = _head_inputs(d.kind, d.dtype, d.N, d.H, d.R, d.tgt2 is not None, d.b_stride, d.b_valid, d.fused, NAN_ROW)
    for k in ("tgt", "tgt2"):
        dn[k] = d[k]                       # (the clean run's targets: padding rows were retargeted there)
    ar, bufs = _head_arena(dn)
    assert np.isnan(bufs["probs"].values()[NAN_ROW]).all()
    for k in ("probs", "argmax", "dlogits"):
        g, c = bufs[k].bits(), clean[k].bits()
        if k == "dlogits" and d.kind == 1:
            g, c = g[:, :1], c[:, :1]
        other_rows_keep_their_bits(g, c, 0, "%s %s" % (k, what))
    if d.fused:
        rm = lambda b: fp.bits_of(tile16(b.t, d.R, d.H, False))
        other_rows_keep_their_bits(rm(bufs["dhs"]), rm(clean["dhs"]), 0, "dhs " + what)


HEAD_N = [7, 17, 61, 100, 129, 192]           # 1, 2, 4, 8, 9 and 12 column tiles


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", HEAD_N)
def test_softmax_head(N, dtype):
    """R = 70: not a multiple of 16, and under bf16 with N <= 64 a wave's second row tile is partly or wholly beyond R"""
    d, bufs = _head_footprint(0, dtype, N, 64, 70)
    _head_row_isolation(d, bufs, "(N=%d)" % N)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,H", [(n, 64) for n in HEAD_N] + [(61, 256)])
def test_softmax_head_with_the_fused_input_gradient(N, H, dtype):
    d, bufs = _head_footprint(0, dtype, N, H, 48, fused=True)
    _head_row_isolation(d, bufs, "(fused, N=%d H=%d)" % (N, H))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_head_two_hot_padding_rows_and_inference(dtype):
    _head_footprint(0, dtype, 61, 64, 70, two_hot=True)
    _head_footprint(0, dtype, 61, 64, 70, b_stride=10, b_valid=7)
    # inference: argmax only - the probs / dlogits buffers that were not passed stay untouched, the scalars keep their values
    d = _head_inputs(0, dtype, 61, 64, 70, False, 0, 0, False, None)
    tight = _head_tight(d, inference=True)
    ar, bufs = _head_arena(d, inference=True)
    fp.assert_same_bits(bufs["argmax"], tight["argmax"], "argmax (inference)")
    top2 = np.sort(d.p, 1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4            # (f32 evaluation errors are ~1e-6 of a probability)
    assert clear.sum() > 60 and np.array_equal(bufs["argmax"].bits()[clear], np.argmax(d.p, 1)[clear])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,fused", [(70, False), (48, True)])
def test_sigmoid_head(R, fused, dtype):
    """kind 1 stores column 0 of dlogits only: columns [1, NP) are asserted UNTOUCHED (include/midivae_hip.h, mvae_head_args.dlogits)"""
    d, bufs = _head_footprint(1, dtype, 1, 64, R, fused=fused)
    _head_row_isolation(d, bufs, "(sigmoid, R=%d)" % R)


@pytest.mark.parametrize("dtype,H,N", [(F32, 16, 7), (BF16, 32, 17)], ids=["f32", "bf16"])
def test_softmax_head_grid_stride(dtype, H, N):
    """R = 65536 + 70: the bounded grid walks the rows again, the last pass ends in a partial tile"""
    _head_footprint(0, dtype, N, H, 65536 + 70)


# ---- mvae_head_sample -------------------------------------------------------------------------------------------------------
def _designed(cdf, seed, min_bin=1e-3):
    """per row: a bin of the float64 CDF at least ``min_bin`` wide and the f32 uniform at its middle (test_choice_decode_gpu.designed)"""
    rng = np.random.default_rng(seed)
    lo = np.concatenate([np.zeros((cdf.shape[0], 1)), cdf[:, :-1]], axis=1)
    ok = (cdf - lo) >= min_bin
    assert ok.any(axis=1).all()
    k = np.argmax(np.where(ok, rng.random(cdf.shape), -1.0), axis=1)
    rows = np.arange(cdf.shape[0])
    return k, (0.5 * (lo[rows, k] + cdf[rows, k])).astype(np.float32)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [7, 61, 129])
@pytest.mark.parametrize("supplied", [True, False], ids=["supplied", "generated"])
def test_head_sample(supplied, N, dtype):
    """out (R) uint8 is written, the bytes behind it stay; the draws are the mirror's (midi_vae_amd/sampling.py) and the tight run's.
    Supplied uniforms: u_stride = 2, tries = 2, both designed (the middle of a CDF bin); generated ones: Philox in the kernel."""
    R, H, td = 70, 64, ops.torch_dtype(dtype)
    hs, W, bias, logits = integer_problem(R, H, N, seed=1000 * N + H)
    NP = ops.head_np(N)
    wt = zeros((NP, H), td)
    ops.transpose_convert(dev(W), wt, n_pad=NP)
    cdf = sampling.cdf_bins(logits, 1.0, from_logits=True)
    if supplied:
        (k1, u1), (k2, u2) = _designed(cdf, 5), _designed(cdf, 6)
        u, cutoff = np.stack([u1, u2], axis=1), 0.05
        q = np.diff(np.concatenate([np.zeros((R, 1)), cdf], axis=1), axis=1)
        p1, p2 = q[np.arange(R), k1], q[np.arange(R), k2]
        check = (np.abs(p1 - cutoff) > 1e-4) & (np.abs(p2 - cutoff) > 1e-4)          # (the cutoff comparison itself is not at its edge)
        want = np.where(p1 > cutoff, k1, k2)
        assert np.array_equal(sampling.choice_index_rows(logits, u, 1.0, tries=2, cutoff=cutoff, from_logits=True), want)
        kw = dict(u_stride=2, tries=2, cutoff=cutoff)
    else:
        u = sampling.uniforms(77, 3, 1, R, 1).reshape(-1)
        want = sampling.choice_index_rows(logits, u, 1.0, from_logits=True)
        check = ~excluded_rows(cdf, u, N)
        kw = dict(seed=77, head_id=3, T=R)
    assert check.sum() > R // 2
    ud = dev(np.asarray(u, np.float32)) if supplied else None
    tight = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
    ops.head_sample(dtype, R, H, N, dev(hs, td), wt, dev(bias), tight, uniforms=ud, **kw)
    ar = fp.Arena(DEV)
    ins = dict(hs=carve_in(ar, "hs", dev(hs, td)), wt=carve_in(ar, "wt", wt), bias=carve_in(ar, "bias", dev(bias)), u=carve_in(ar, "uniforms", ud))
    out = ar.carve("out", (R,), torch.uint8)
    ar.commit()
    ops.head_sample(dtype, R, H, N, ins["hs"].t, ins["wt"].t, ins["bias"].t, out.t, uniforms=tensor(ins["u"]), **kw)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(out)
    fp.assert_same_bits(out, tight, "out")
    assert np.array_equal(out.bits()[check], want[check]), np.nonzero((out.bits() != want) & check)[0]


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
def _rounded(a, dt):
    return host(dev(a, dt))


def _gemm_footprint(M, N, K, a_dt, b_dt, c_dt=torch.float32, ta=False, tb=False, alpha=1.0, bias=False, accumulate=False, split_k=1,
                    ldb=None, pad=4, onehot=False, colsum=False, what="", **kw):
    """one mvae_gemm call, C (M, ldc) with ldc = N + pad (TILE16: N) from an arena and a tight one.  Store mode: random operands,
    C starts as sentinels - columns < N written, the gap [N, ldc) untouched, the rows before 0 and after M - 1 are the guards; the
    unit bound of parity.assert_product.  Accumulate mode: small-integer operands onto small integers in columns < N (sentinels in
    the gap) - bit-equal to float64 in every arrival order (parity.assert_bits), and to the tight run.  Returns the arena's C."""
    rng = np.random.default_rng(M + N + K + split_k)
    integer = accumulate
    tile = kw.get("c_layout") == hl.TILE16
    ldc = N if tile else N + pad
    ar_, ac_ = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    ldb = ldb or bc
    make = (lambda sh: par.integer_operands(rng, sh)) if integer else (lambda sh: rng.standard_normal(sh))
    if onehot:
        idx = rng.integers(0, M, (K,))
        Ad = dev(idx, torch.uint8)
        opA = np.zeros((M, K))
        opA[idx, np.arange(K)] = 1.0
    else:
        Ad = dev(make((ar_, ac_)), a_dt)
        Ah = host(Ad)
    Bm = make((br, ldb))
    if ldb > bc:
        Bm[:, bc:(bc + 7) // 8 * 8] = 0            # the last 16-byte load of a row of the narrow-N path: zero, as the callers keep it
    Bd = dev(Bm, b_dt)
    Bh = host(Bd)[:, :bc]
    f32_path = a_dt == torch.float32 and b_dt == torch.float32 and not onehot
    if not f32_path:
        Bh = par.bf16_round(Bh)
        if not onehot:
            Ah = par.bf16_round(Ah)
    if not onehot:
        opA = Ah.T if ta else Ah
    opB = Bh.T if tb else Bh
    bias_h = _rounded(make((N,)), torch.float32) if bias else None
    c0 = par.integer_operands(rng, (M, N)) if accumulate else None
    cs0 = par.integer_operands(rng, (N,)) if colsum else None
    call = dict(trans_a=ta or onehot, trans_b=tb, ldb=ldb, ldc=ldc, accumulate=accumulate, split_k=split_k, alpha=alpha,
                a_kind=hl.ONEHOT if onehot else None, **kw)
    # the tight run
    Ct = zeros((M, ldc), c_dt)
    if accumulate:
        Ct[:, :N] = dev(c0)
    cst = dev(cs0) if colsum else None
    ops.gemm(Ad, Bd, Ct, M, N, K, bias=dev(bias_h) if bias else None, colsum_b=cst, **call)
    # the arena run
    ar = fp.Arena(DEV)
    A_, B_ = carve_in(ar, "A", Ad, "zero" if onehot else "sentinel"), carve_in(ar, "B", Bd)
    bias_ = carve_in(ar, "bias", dev(bias_h)) if bias else None
    C = ar.carve("C", (M, ldc), c_dt, prefill=c0, region=np.s_[:, :N]) if accumulate else ar.carve("C", (M, ldc), c_dt)
    cs = ar.carve("colsum_b", (N,), torch.float32, prefill=cs0) if colsum else None
    ar.commit()
    ops.gemm(A_.t, B_.t, C.t, M, N, K, bias=tensor(bias_), colsum_b=tensor(cs), **call)
    ar.fetch()
    ar.assert_guards_intact()
    if not accumulate:
        ar.assert_written(C, None if tile else np.s_[:, :N])
    if not tile:
        ar.assert_untouched(C, np.s_[:, N:])
    fp.assert_same_bits(C.bits()[:, :N], fp.bits_of(Ct)[:, :N], "C " + what)
    al = np.float64(np.float32(alpha))
    storage = "bf16" if c_dt == torch.bfloat16 else "f32"
    got = host(tile16(C.t, M, N, False)) if tile else C.values()[:, :N]
    want = al * (opA @ opB) + (bias_h if bias else 0.0) + (c0 if accumulate else 0.0)
    if integer:
        par.assert_bits(got, want, storage, what + " (integers)")
    else:
        par.assert_product(got, want, par.product_unit(opA, opB, al, [bias_h] if bias else []), "f32" if f32_path else "bf16", what,
                           out_bf16=storage == "bf16")
    if colsum:
        fp.assert_same_bits(cs, cst, "colsum_b " + what)
        par.assert_bits(cs.values(), cs0 + opB.sum(0), "f32", "colsum_b " + what)
    return C


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_generic(ta, tb, dt):
    """gemm_k at (50, 61, 33): one partial 64 x 64 tile; store (with bias, f32 and the operand type as output) and split-K"""
    _gemm_footprint(50, 61, 33, dt, dt, ta=ta, tb=tb, bias=True, what="store")
    if dt == torch.bfloat16:
        _gemm_footprint(50, 61, 33, dt, dt, c_dt=dt, ta=ta, tb=tb, bias=True, what="store, bf16 out")
    _gemm_footprint(50, 61, 33, dt, dt, ta=ta, tb=tb, accumulate=True, split_k=3, alpha=0.5, what="split-K")


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 64)])
def test_gemm_fast_store(M, N, K):
    """gemm_fast_k, store mode, bf16 operands: f32 and bf16 C with ldc = N + 4"""
    bf = torch.bfloat16
    for c_dt in (torch.float32, bf):
        _gemm_footprint(M, N, K, bf, bf, c_dt=c_dt, tb=True, bias=True, what="fast store")


@pytest.mark.parametrize("M", [61, 200])
def test_gemm_onehot_accumulate(M):
    """one-hot A on the fast kernel: a full 128-row tile is computed, rows >= M are never stored (M = 61: one tile; 200: two)"""
    _gemm_footprint(M, 256, 1024, None, torch.bfloat16, accumulate=True, split_k=4, alpha=0.5, onehot=True, what="one-hot A")


@pytest.mark.parametrize("N", [61, 77, 200])
def test_gemm_fast_narrow_last_tile(N):
    """C += A^T B with a narrow last N tile (N = 200: a full tile and a narrow one), ldb = N rounded up to 8"""
    bf = torch.bfloat16
    _gemm_footprint(256, N, 1024, bf, bf, ta=True, accumulate=True, split_k=4, alpha=0.5, ldb=(N + 7) // 8 * 8, what="narrow N")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_tile16_output(dt):
    """c_layout = TILE16 at (32, 48, 64), the generic kernel in both types: the whole buffer is the region, and ldc does not apply"""
    _gemm_footprint(32, 48, 64, dt, dt, c_dt=dt, tb=True, bias=True, c_layout=hl.TILE16, what="TILE16")


def test_gemm_colsum_b_beside_c():
    bf = torch.bfloat16
    _gemm_footprint(128, 256, 1024, bf, bf, ta=True, accumulate=True, split_k=2, alpha=0.25, colsum=True, what="C and colsum_b")


def _weight_gradient_problems(rng, K, N):
    """three problems of the batched weight-gradient launches: dense A with fused column sums, dense A, one-hot A"""
    bf = torch.bfloat16
    A1, A2 = par.integer_operands(rng, (K, 256)), par.integer_operands(rng, (K, 128))
    idx = rng.integers(0, 61, (K,))
    A3 = np.zeros((K, 61))
    A3[np.arange(K), idx] = 1.0
    Bi = par.integer_operands(rng, (K, N))
    dv = dict(A1=dev(A1, bf), A2=dev(A2, bf), A3=dev(idx, torch.uint8), B=dev(Bi, bf))
    c0 = [par.integer_operands(rng, (m, N)) for m in (256, 128, 61)]
    cs0 = par.integer_operands(rng, (N,))
    want = [c + 0.5 * (a.T @ Bi) for c, a in zip(c0, (A1, A2, A3))]
    return dv, c0, cs0, want, cs0 + Bi.sum(0)


def _weight_gradient_launch(launch, dv, Cs, cs, N, K, ldc, **kw):
    common = dict(trans_a=True, accumulate=True, alpha=0.5, ldc=ldc, build_only=True, **kw)
    launch([ops.gemm(dv["A1"], dv["B"], Cs[0], 256, N, K, split_k=4, colsum_b=cs, **common),
            ops.gemm(dv["A2"], dv["B"], Cs[1], 128, N, K, split_k=2, **common),
            ops.gemm(dv["A3"], dv["B"], Cs[2], 61, N, K, split_k=8, a_kind=hl.ONEHOT, **common)])


@pytest.mark.parametrize("kind", ["multi", "kstream"])
def test_gemm_batched_weight_gradients(kind):
    """mvae_gemm_multi and mvae_gemm_kstream_multi (counters already at their value): three problems, their Cs (ldc = N + 4) and the
    colsum_b adjacent in one arena; small-integer operands: bit-equal to float64 and to the tight run"""
    rng = np.random.default_rng(31)
    N, rows, nch = 256, 1024, 2
    K, ldc = rows * nch, N + 4
    dv, c0, cs0, want, want_cs = _weight_gradient_problems(rng, K, N)
    ms = (256, 128, 61)
    counters = torch.full((nch,), 9, dtype=torch.int32, device=DEV)
    status = zeros((1,), torch.int32)
    if kind == "multi":
        kw = {}
        launch = lambda ps: ops.gemm_multi(ps) == len(ps) or pytest.fail("mvae_gemm_multi did not take the problems")
    else:
        kw = dict(k_wait=counters, k_wait_value=9, k_chunk_rows=rows, k_reverse=True, chunk_status=status)
        launch = ops.gemm_kstream_multi
    tight = [zeros((m, ldc)) for m in ms]
    for t, c in zip(tight, c0):
        t[:, :N] = dev(c)
    cst = dev(cs0)
    _weight_gradient_launch(launch, dv, tight, cst, N, K, ldc, **kw)
    ar = fp.Arena(DEV)
    ins = {k: carve_in(ar, k, v, "zero" if k == "A3" else "sentinel") for k, v in dv.items()}
    Cs, cs = [], None
    for i, (m, c) in enumerate(zip(ms, c0)):
        Cs.append(ar.carve("C%d" % i, (m, ldc), torch.float32, prefill=c, region=np.s_[:, :N]))
        if i == 0:
            cs = ar.carve("colsum_b", (N,), torch.float32, prefill=cs0)
    ar.commit()
    _weight_gradient_launch(launch, {k: b.t for k, b in ins.items()}, [b.t for b in Cs], cs.t, N, K, ldc, **kw)
    ar.fetch()
    ar.assert_guards_intact()
    assert int(status.item()) == 0
    for i, C in enumerate(Cs):
        ar.assert_untouched(C, np.s_[:, N:])
        fp.assert_same_bits(C.bits()[:, :N], fp.bits_of(tight[i])[:, :N], "C%d" % i)
        par.assert_bits(C.values()[:, :N], want[i], "f32", "C%d (integers)" % i)
    fp.assert_same_bits(cs, cst, "colsum_b")
    par.assert_bits(cs.values(), want_cs, "f32", "colsum_b (integers)")


@pytest.mark.parametrize("lay", [hl.TILE16, hl.ROWMAJOR])
@pytest.mark.parametrize("which", ["chunked", "weights-stationary"])
def test_gemm_persistent_launches(which, lay):
    """the chunked persistent launch of gemm_fast_k (K = 768, two workgroups, one row block per chunk) and the weights-stationary
    projection (K = 256, N = 768, 8 row blocks per chunk) at the smallest shapes test_ops_gpu.py runs them, counters at their wait
    value: C (bf16; row-major with ldc = N + 8) and the published counters in one arena; bit-equal to the plain GEMM into a tight C"""
    if which == "chunked":
        N, K, blocks, rows, nchunks = 256, 768, 2, 128, 3
    else:
        N, K, blocks, rows, nchunks = 768, 256, 8 * (768 // 128), 8 * 128, 3
    M = rows * nchunks
    ldc = N if lay == hl.TILE16 else N + 8
    rng = np.random.default_rng(K + lay)
    A, W = dev(rng.standard_normal((M, K)) * 0.5, torch.bfloat16), dev(rng.standard_normal((N, K)) * 0.1, torch.bfloat16)
    bias = dev(rng.standard_normal((N,)))
    tight = zeros((M, ldc), torch.bfloat16)
    ops.gemm(A, W, tight, M, N, K, trans_b=True, bias=bias, c_layout=lay, ldc=ldc)
    ar = fp.Arena(DEV)
    A_, W_, b_ = carve_in(ar, "A", A), carve_in(ar, "W", W), carve_in(ar, "bias", bias)
    ready = ar.carve("chunk_wait", (nchunks,), torch.int32, data=np.full(nchunks, 5))
    C = ar.carve("C", (M, ldc), torch.bfloat16)
    done = ar.carve("chunk_done", (nchunks,), torch.int32, prefill=np.zeros(nchunks, np.int64))
    status = ar.carve("chunk_status", (1,), torch.int32, prefill=np.zeros(1, np.int64))
    ar.commit()
    ops.gemm(A_.t, W_.t, C.t, M, N, K, trans_b=True, bias=b_.t, c_layout=lay, ldc=ldc, max_blocks=blocks, chunk_rows=rows,
             chunk_wait=ready.t, chunk_wait_value=5, chunk_done=done.t, chunk_status=status.t)
    ar.fetch()
    ar.assert_guards_intact()
    assert status.bits().tolist() == [0] and done.bits().tolist() == [4 * blocks] * nchunks
    if lay == hl.TILE16:
        ar.assert_written(C)
    else:
        ar.assert_written(C, np.s_[:, :N])
        ar.assert_untouched(C, np.s_[:, N:])
    fp.assert_same_bits(C.bits()[:, :N], fp.bits_of(tight)[:, :N], "C")
    out = host(tile16(C.t, M, N, False)) if lay == hl.TILE16 else C.values()[:, :N]
    ref = host(A) @ host(W).T + host(bias)
    par.assert_product(out, ref, par.product_unit(host(A), host(W).T, extra=[host(bias)]), "bf16", which, out_bf16=True)


# ---- mvae_prepare_batch and the layout writers ---------------------------------------------------------------------------------
def test_prepare_batch_all_job_kinds_back_to_back():
    """one launch with all eight job kinds, their destinations carved back to back: bit-equal to the same jobs into tight buffers, and
    to float64 where the job is exact (conversions, W + b in f32 then rounded, transposes, zero fills, broadcasts)"""
    rng = np.random.default_rng(41)
    bf, f32 = torch.bfloat16, torch.float32
    H = 64
    src = dict(U=dev(rng.standard_normal((H, 3 * H)) * 0.1), Wt=dev(rng.standard_normal((7, 192))), bt=dev(rng.standard_normal(192)),
               Wp=dev(rng.standard_normal((7, 1024))), bp=dev(rng.standard_normal(1024)), Wq=dev(rng.standard_normal((7, 768))),
               bq=dev(rng.standard_normal(768)), W61=dev(rng.standard_normal((64, 61))), W129=dev(rng.standard_normal((64, 129))),
               x=dev(rng.standard_normal(1001)), x2=dev(rng.standard_normal(1001)), row=dev(rng.standard_normal(192)))
    dests = [("pack f32 fwd", (3 * H * H,), f32), ("pack f32 bwd", (3 * H * H,), f32), ("pack bf16 fwd", (3 * H * H,), bf),
             ("pack bf16 bwd", (3 * H * H,), bf), ("table", (7, 192), bf), ("table paired", (7, 1024), bf), ("table paired8", (7, 768), bf),
             ("wt61", (64, 64), bf), ("wt129", (144, 64), f32), ("to bf16", (1001,), bf), ("to f32", (1001,), f32), ("zero bf16", (6,), bf),
             ("zero f32", (3,), f32), ("wc", (64, 64), bf), ("counter", (1,), torch.int32), ("rows", (5, 192), f32)]

    def jobs(t):
        pb = ops.PrepBatch()
        pb.pack_recurrent(src["U"], t["pack f32 fwd"], 0); pb.pack_recurrent(src["U"], t["pack f32 bwd"], 1)
        pb.pack_recurrent(src["U"], t["pack bf16 fwd"], 0); pb.pack_recurrent(src["U"], t["pack bf16 bwd"], 1)
        pb.make_table(src["Wt"], src["bt"], t["table"]); pb.make_table(src["Wp"], src["bp"], t["table paired"], paired=True)
        pb.make_table(src["Wq"], src["bq"], t["table paired8"], paired=8)
        pb.transpose_convert(src["W61"], t["wt61"], n_pad=64); pb.transpose_convert(src["W129"], t["wt129"], n_pad=144)
        pb.convert(src["x"], t["to bf16"]); pb.convert(src["x2"], t["to f32"])      # (the source of a CONVERT job is f32)
        pb.zero(t["zero bf16"]); pb.zero(t["zero f32"])
        pb.convert_pad(src["W61"], t["wc"], 64)
        pb.add_i32(t["counter"], 3)
        pb.broadcast_rows(src["row"], t["rows"], 5)
        pb.run()
        return pb

    tight = {n: zeros(s, d) for n, s, d in dests}
    tight["counter"].fill_(4)
    keep = jobs(tight)
    ar = fp.Arena(DEV)
    bufs = {n: (ar.carve(n, s, d, prefill=np.array([4])) if n == "counter" else ar.carve(n, s, d)) for n, s, d in dests}
    ar.commit()
    keep2 = jobs({n: b.t for n, b in bufs.items()})
    ar.fetch()
    ar.assert_guards_intact()
    for n, b in bufs.items():
        if n != "counter":
            ar.assert_written(b)
        fp.assert_same_bits(b, tight[n], n)
    assert bufs["counter"].bits().tolist() == [7]            # (the counter sits between sentinel words: the guards)
    ar.assert_zero(bufs["wt61"], np.s_[61:])                 # rows [N, N_pad) of a transposed copy: exactly zero
    ar.assert_zero(bufs["wt129"], np.s_[129:])
    ar.assert_zero(bufs["wc"], np.s_[:, 61:])
    ar.assert_zero(bufs["zero bf16"])
    ar.assert_zero(bufs["zero f32"])
    h = lambda k: host(src[k])
    par.assert_bits(bufs["table"].values(), par.cast(h("Wt") + h("bt"), "f32"), "bf16", "table")
    par.assert_bits(bufs["wt61"].values()[:61], h("W61").T, "bf16", "wt61")
    par.assert_bits(bufs["wt129"].values()[:129], h("W129").T, "f32", "wt129")
    par.assert_bits(bufs["wc"].values()[:, :61], h("W61"), "bf16", "wc")
    par.assert_bits(bufs["to bf16"].values(), h("x"), "bf16", "convert to bf16")
    par.assert_bits(bufs["to f32"].values(), h("x2"), "f32", "convert to f32")
    par.assert_bits(bufs["rows"].values(), np.broadcast_to(h("row"), (5, 192)), "f32", "broadcast rows")
    assert keep and keep2


@pytest.mark.parametrize("dt,storage", [(torch.float32, "f32"), (torch.bfloat16, "bf16")])
def test_relayout_gather2_and_outer_bias(dt, storage):
    """mvae_relayout (all six modes at (32, 256)), mvae_gather2_tile16 (both layouts) and mvae_outer_bias_tile16 at (16, 768): the
    whole destination is written, nothing around it; the round trip is the identity, the tiled image the header's offset formula"""
    rng = np.random.default_rng(43)
    rows, cols = 32, 256
    a = dev(rng.standard_normal((rows, cols)), dt)
    for paired in (False, True, "q"):
        ar = fp.Arena(DEV)
        a_ = carve_in(ar, "src", a)
        tiled, back = ar.carve("tiled", (rows, cols), dt), ar.carve("back", (rows, cols), dt)
        ar.commit()
        ops.relayout(a_.t, tiled.t, rows, cols, True, paired=paired)
        ops.relayout(tiled.t, back.t, rows, cols, False, paired=paired)
        ar.fetch()
        ar.assert_guards_intact()
        ar.assert_written(tiled)
        ar.assert_written(back)
        fp.assert_same_bits(back, a, "round trip, paired=%s" % paired)
        fp.assert_same_bits(tiled, tile16(a, rows, cols, True, paired=paired), "tiled, paired=%s" % paired)
        if paired is False:
            assert np.array_equal(tiled.bits().ravel()[_tile16_offsets(rows, cols)].reshape(rows, cols), fp.bits_of(a))
    R, N, K1, K2 = 48, 768, 61, 16
    t1, t2 = dev(rng.standard_normal((K1, N)), dt), dev(rng.standard_normal((K2, N)), dt)
    i1, i2 = rng.integers(0, K1, R), rng.integers(0, K2, R)
    for layout in (hl.TILE16, hl.ROWMAJOR):
        tight = zeros((R, N), dt)
        ops.gather2_tile16(dev(i1, torch.uint8), dev(i2, torch.uint8), t1, t2, tight, R, N, layout=layout)
        ar = fp.Arena(DEV)
        ins = [carve_in(ar, "idx", dev(i1, torch.uint8), "zero"), carve_in(ar, "idx2", dev(i2, torch.uint8), "zero"),
               carve_in(ar, "table", t1), carve_in(ar, "table2", t2)]
        out = ar.carve("out", (R, N), dt)
        ar.commit()
        ops.gather2_tile16(ins[0].t, ins[1].t, ins[2].t, ins[3].t, out.t, R, N, layout=layout)
        ar.fetch()
        ar.assert_guards_intact()
        ar.assert_written(out)
        fp.assert_same_bits(out, tight, "gather2, layout %d" % layout)
        got = out.values()
        if layout == hl.TILE16:
            got = got.ravel()[_tile16_offsets(R, N)].reshape(R, N)
        par.assert_bits(got, host(t1)[i1] + host(t2)[i2], storage, "gather2")
    R, N = 16, 768
    xs, w, b = dev(rng.random(R)), dev(rng.standard_normal(N)), dev(rng.standard_normal(N))
    tight = zeros((R, N), dt)
    ops.outer_bias_tile16(xs, w, b, tight, R, N)
    ar = fp.Arena(DEV)
    ins = [carve_in(ar, "xs", xs), carve_in(ar, "w", w), carve_in(ar, "bias", b)]
    out = ar.carve("out", (R, N), dt)
    ar.commit()
    ops.outer_bias_tile16(ins[0].t, ins[1].t, ins[2].t, out.t, R, N)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(out)
    fp.assert_same_bits(out, tight, "outer_bias")
    # the bound of test_small_ops_gpu.test_outer_bias_tile16: half an ulp of a bf16 output plus two f32 units (the multiply, the add)
    got = out.values().ravel()[_tile16_offsets(R, N)].reshape(R, N)
    want = host(xs)[:, None] * host(w)[None] + host(b)[None]
    bound = 2.0 * par.product_unit(host(xs)[:, None], host(w)[None], extra=[host(b)[None]]) + (par.half_ulp_bf16(want) if storage == "bf16" else 0.0)
    assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) / bound).max())
