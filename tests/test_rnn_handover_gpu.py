"""The recurrent kernels in the calling conventions the engine uses and test_ops_gpu.py never passes (GPU box only).

test_ops_gpu.py and test_hidden_sizes_gpu.py hold every recurrent kernel to the float64 oracle in ONE convention: one launch, packed
(B, H) states, no hand-over fields.  Here the same kernels (generic ROWMAJOR; resident phased TILE16; slot-interleaved TILE16P;
two-waves-per-SIMD TILE16Q, and the LSTM BPTT of rnn_w8.hip under MVAE_LSTM_BWD_W8=1) run the way the engine calls them, and what
is pinned at kernel level is

  1. states as column blocks of wider buffers (h0_ld / h_last_ld / dh_last_ld / dh0_ld; c_last and dc_last share them): bit-equal
     to the packed launch, the sentinel columns around the block untouched, the strided run within parity.BOUNDS of the oracle;
  2. a sequence as consecutive launches over time chunks with the f32 state carried (h_last -> h0, c_last -> c0; dh0 -> dh_last,
     dc0 -> dc_last): bit-equal to the single launch in BOTH directions, and within the bounds of the whole-sequence oracle;
  3. the chunk counters without a partner: counters 0 .. ceil(T / cs) - 1 move by mvae_rnn_producer_waves * B / 16 per launch,
     exactly and cumulatively, nothing else moves, status stays 0, waits on counters already at their value (the >= edge) change
     no bit of any output - chunk_steps 1 (publishing and the backward kernels), 2, 3, 16 at T = 1, cs - 1, cs, cs + 1, 2 cs, 2 cs + 1;
  4. a live partner: inputs that are NaN until a second queue writes a chunk and publishes its counter - a read in front of its
     wait poisons the output - and snapshots taken by a second queue the moment a chunk's counter has its value;
  5. the phase launches mvae_rnn_fwd_multi / mvae_rnn_bwd_multi (problems of different T, B, input mode, upstream gradient; an
     expansion producer in both variants feeding a dense-input recurrence): every problem bit-equal to its single launch;
  6. what the entry points refuse: one-step chunks with wait_ready in the forward direction, signal_done without hs, mixed
     phase launches, families that do not take a cell or an input mode.

Nearly every assertion is bit-equality or an exact integer; the rest are parity.assert_parity with parity.BOUNDS unchanged
(margins on the MI355X, every test of this file: profiles/r11_handover_margins.txt - the same ratios as the packed single launches,
since the outputs are the same bits).  The device-side waits give up after about 3 s and set ``status``: a missed publish shows as a non-zero status,
a missed wait as NaN, never as a hang.  What stays covered at engine level only: stale L2 data left by an EARLIER launch on the
same buffers (a snapshot compared with the final tensor of the same launch cannot show it).
"""
import functools

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from oracle import vae_oracle as vo
from tests import parity as par
from tests.gpu_util import DEV, _paired8_columns, _paired_columns, dev, host, no_host_sync, pairing, tile16, two_queues

pytestmark = pytest.mark.gpu

CELL = {"GRU": hl.GRU, "LSTM": hl.LSTM, "SimpleRNN": hl.RNN}
BF16, F32 = hl.BF16, hl.F32
RH, RB, T7 = par.RES_H, par.RES_B, par.HANDOVER_T
SENT = par.STATE_SENTINEL

# family -> (seq_layout, cells, forward input modes); "w8lstm": the LSTM BPTT of rnn_w8.hip (TILE16P data, MVAE_LSTM_BWD_W8=1)
FAMILIES = {
    "generic": (hl.ROWMAJOR, ["LSTM", "GRU", "SimpleRNN"], ["dense", "index", "scalar", "const"]),
    "phased": (hl.TILE16, ["LSTM", "GRU"], ["dense", "index", "scalar", "const"]),
    "il": (hl.TILE16P, ["LSTM", "GRU"], ["dense", "index", "const"]),
    "w8": (hl.TILE16Q, ["GRU"], ["dense", "index", "const"]),
    "w8lstm": (hl.TILE16P, ["LSTM"], []),
}


def _shapes(fam):
    return par.GENERIC_SHAPES if fam == "generic" else [(RH, RB, BF16)]


FWD_CASES = [(fam, c, H, B, dt, xm) for fam in ("generic", "phased", "il", "w8") for c in FAMILIES[fam][1] for H, B, dt in _shapes(fam)
             for xm in FAMILIES[fam][2]]
BWD_CASES = [(fam, c, H, B, dt, ext) for fam in FAMILIES for c in FAMILIES[fam][1] for H, B, dt in _shapes(fam) for ext in (True, False)]
PIPE_FWD = [("il", "LSTM"), ("il", "GRU"), ("w8", "GRU")]
PIPE_BWD = [("il", "LSTM"), ("il", "GRU"), ("w8", "GRU"), ("w8lstm", "LSTM")]


def _id(case):
    return "-".join("bf16" if v == BF16 and i == 4 else "f32" if v == F32 and i == 4 else str(v) for i, v in enumerate(case))


def _env(fam, monkeypatch):
    if fam == "w8lstm":
        monkeypatch.setenv("MVAE_LSTM_BWD_W8", "1")
    else:
        monkeypatch.delenv("MVAE_LSTM_BWD_W8", raising=False)


def _rnd(dt):
    return lambda a: par.cast(a, "bf16" if dt == BF16 else "f32")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def assert_same_bits(got, want, what):
    if want is None:
        assert got is None, what
        return
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    diff = g != w
    par._record("bits:device", what, mismatches=float(diff.sum()))
    assert not bool(diff.any()), "%s: %d of %d elements differ, first at %s" % (
        what, int(diff.sum()), diff.numel(), tuple(int(i) for i in diff.nonzero()[0]))


class Out(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def fwd_problem(cellname, H, T, B, dt, xmode, seed=None):
    return par.rnn_forward_inputs(cellname, H, T, B, xmode, seed=H + B + T if seed is None else seed, rnd=_rnd(dt))


@functools.lru_cache(maxsize=None)
def bwd_problem(cellname, H, T, B, dt, ext):
    U, hs, cs, acts, dext, dlast = par.rnn_backward_problem(cellname, H, T, B, ext, _rnd(dt))
    return par.Problem(cellname=cellname, H=H, T=T, B=B, U=U, hs_r=hs, cs_r=cs, acts_r=acts, dext=dext, dlast=dlast,
                       dclast=par.carried_cell_gradient(H, B) if cellname == "LSTM" else None)


class Fwd(object):
    """the device side of one forward problem (par.rnn_forward_inputs) in one kernel family"""

    def __init__(self, pb, lay, dt):
        self.pb, self.lay, self.dt, self.cell, self.td = pb, lay, dt, CELL[pb.cellname], ops.torch_dtype(dt)
        self.T, self.B, self.H, self.GH = pb.T, pb.B, pb.H, pb.G * pb.H
        self.tiled, self.lstm = lay != hl.ROWMAJOR, pb.cellname == "LSTM"
        self.up = ops.pack_recurrent(dev(pb.U), self.cell, dt, 0)
        kw = {}
        if pb.xmode == "dense":
            xp = dev(pb.xp, self.td)
            kw["xp"] = tile16(xp, self.T * self.B, self.GH, True) if self.tiled else xp
        elif pb.xmode == "index":
            table, tl = pb.table, hl.TABLE_ROWMAJOR
            if lay == hl.TILE16P:
                table, tl = _paired_columns(table), hl.TABLE_PAIRED
            elif lay == hl.TILE16Q:
                table, tl = _paired8_columns(table), hl.TABLE_PAIRED8
            kw.update(idx=dev(pb.idx, torch.uint8), table=dev(table, self.td), table_layout=tl)
        elif pb.xmode == "scalar":
            kw.update(xs=dev(pb.xs), w_row=dev(pb.w_row), bias=dev(pb.bias))
        else:
            kw["xp0"] = dev(pb.xp0, self.td)
        self.kw = kw
        self.h0, self.c0 = dev(pb.h0), (dev(pb.c0) if self.lstm else None)

    def buffers(self, save="all"):
        z = lambda *s: torch.zeros(s, dtype=self.td, device=DEV)
        return Out(hs=z(self.T + 1, self.B, self.H), cs=z(self.T + 1, self.B, self.H) if self.lstm and save == "all" else None,
                   acts=z(self.T, self.B, self.GH) if save == "all" else None,
                   h_last=torch.zeros((self.B, self.H), device=DEV), c_last=torch.zeros((self.B, self.H), device=DEV) if self.lstm else None)

    def launch(self, out, t0=0, t1=None, h0=None, c0=None, h_last=None, c_last=None, **extra):
        """steps [t0, t1) into the time slices of ``out`` (a time slice of a tiled array is contiguous: B % 16 == 0)"""
        t1 = self.T if t1 is None else t1
        kw = dict(self.kw)
        for k in ("xp", "idx", "xs"):
            if k in kw:
                kw[k] = kw[k][t0:t1]
        kw.update(extra)
        cut = lambda a, n: None if a is None else a[t0:t1 + n]
        return ops.rnn_fwd(self.cell, self.dt, t1 - t0, self.B, self.H, self.up, h0=self.h0 if h0 is None else h0,
                           c0=self.c0 if c0 is None else c0, hs=cut(out.hs, 1), cs=cut(out.cs, 1), acts=cut(out.acts, 0),
                           h_last=out.h_last if h_last is None else h_last, c_last=out.c_last if c_last is None else c_last,
                           seq_layout=self.lay, **kw)

    def check_parity(self, out, what, h_last=None, c_last=None, oracle=None):
        hs_o, cs_o, acts_o = oracle or (self.pb.hs, self.pb.cs, self.pb.acts)
        T, B, H, GH, pr = self.T, self.B, self.H, self.GH, pairing(self.lay)
        par.assert_parity(host(out.hs), hs_o, self.dt, par.step_blocks, "hs " + what, values=True)
        if out.acts is not None:
            acts = tile16(out.acts, T * B, GH, False, paired=pr) if self.tiled else out.acts
            par.assert_parity(host(acts), acts_o, self.dt, par.gate_blocks(self.pb.cellname), "acts " + what, values=True)
        if out.cs is not None:
            cs = tile16(out.cs, (T + 1) * B, H, False, paired=pr) if self.tiled else out.cs
            par.assert_parity(host(cs), cs_o, self.dt, par.step_blocks, "cs " + what, values=True)
        par.assert_parity(host(out.h_last if h_last is None else h_last), hs_o[-1], self.dt, par.whole, "h_last " + what, values=True)
        if self.lstm:
            par.assert_parity(host(out.c_last if c_last is None else c_last), cs_o[-1], self.dt, par.whole, "c_last " + what, values=True)

    def assert_same(self, got, want, what):
        for k in ("hs", "cs", "acts", "h_last", "c_last"):
            assert_same_bits(got[k], want[k], "%s %s" % (k, what))


class Bwd(object):
    """the device side of one BPTT problem (saved sequences as the forward kernel of the family stores them)"""

    def __init__(self, pb, lay, dt):
        self.pb, self.lay, self.dt, self.cell, self.td = pb, lay, dt, CELL[pb.cellname], ops.torch_dtype(dt)
        self.T, self.B, self.H = pb.T, pb.B, pb.H
        self.GH = vo.GATES[pb.cellname] * pb.H
        self.tiled, self.lstm, self.gru = lay != hl.ROWMAJOR, pb.cellname == "LSTM", pb.cellname == "GRU"
        T, B, H, GH, td, pr = self.T, self.B, self.H, self.GH, self.td, pairing(lay)
        self.ut = ops.pack_recurrent(dev(pb.U), self.cell, dt, 1)
        self.hs = dev(pb.hs_r, td)
        self.acts, self.cs = dev(pb.acts_r, td), (dev(pb.cs_r, td) if self.lstm else None)
        self.dext = dev(pb.dext, td) if pb.dext is not None else None
        if self.tiled:
            self.acts = tile16(self.acts, T * B, GH, True, paired=pr)
            self.cs = tile16(self.cs, (T + 1) * B, H, True, paired=pr) if self.lstm else None
            self.dext = tile16(self.dext, T * B, H, True) if self.dext is not None else None
        self.dlast, self.dclast = dev(pb.dlast), (dev(pb.dclast) if pb.get("dclast") is not None else None)
        self.want = vo.rnn_backward(pb.cellname, pb.hs_r, pb.cs_r, pb.acts_r, pb.U, pb.dext, pb.dlast, dc_last=pb.get("dclast"))

    def buffers(self):
        z = lambda *s: torch.zeros(s, dtype=self.td, device=DEV)
        return Out(da=z(self.T, self.B, self.GH), rh=z(self.T, self.B, self.H) if self.gru else None,
                   dh0=torch.zeros((self.B, self.H), device=DEV), dc0=torch.zeros((self.B, self.H), device=DEV) if self.lstm else None)

    def launch(self, out, t0=0, t1=None, dh_last=None, dc_last=None, dh0=None, dc0=None, **extra):
        t1 = self.T if t1 is None else t1
        cut = lambda a, n: None if a is None else a[t0:t1 + n]
        kw = dict(dhs_ext=cut(self.dext, 0))
        kw.update(extra)
        return ops.rnn_bwd(self.cell, self.dt, t1 - t0, self.B, self.H, self.ut, cut(self.hs, 1), cut(self.cs, 1), cut(self.acts, 0),
                           cut(out.da, 0), dh_last=self.dlast if dh_last is None else dh_last,
                           dc_last=self.dclast if dc_last is None else dc_last, rh=cut(out.rh, 0),
                           dh0=out.dh0 if dh0 is None else dh0, dc0=out.dc0 if dc0 is None else dc0, seq_layout=self.lay, **kw)

    def check_parity(self, out, what, dh0=None, dc0=None):
        da_o, _, dh0_o, dc0_o = self.want
        name = self.pb.cellname
        par.assert_parity(host(out.da), da_o, self.dt, par.gate_blocks(name), "da " + what)
        par.assert_parity(host(out.dh0 if dh0 is None else dh0), dh0_o, self.dt, par.whole, "dh0 " + what)
        if self.lstm:
            par.assert_parity(host(out.dc0 if dc0 is None else dc0), dc0_o, self.dt, par.whole, "dc0 " + what)
        if self.gru:
            H = self.H
            par.assert_parity(host(out.rh), self.pb.acts_r[:, :, H:2 * H] * self.pb.hs_r[:-1], self.dt, par.step_blocks, "rh " + what,
                              values=True)

    def assert_same(self, got, want, what):
        for k in ("da", "rh", "dh0", "dc0"):
            assert_same_bits(got[k], want[k], "%s %s" % (k, what))


def column_block(value, ld, off, H):
    """a (B, ld) f32 buffer of sentinels with ``value`` (B, H) in columns [off, off + H): (buffer, view of the block)"""
    B = value.shape[0]
    wide = torch.full((B, ld), SENT, device=DEV)
    wide[:, off:off + H] = value
    return wide, wide[:, off:off + H]


def assert_block_only(wide, off, H, what):
    outside = torch.cat([wide[:, :off], wide[:, off + H:]], 1)
    assert bool((outside == SENT).all()), "%s: %d sentinel columns were written" % (what, int((outside != SENT).sum()))


# ---- 1. states as column blocks of wider buffers -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_states_as_column_blocks(case):
    """h0 / c0 read from columns [H, 2H) of (B, 3H) buffers, h_last / c_last written into columns [2H, 3H) of (B, 4H) buffers (two
    different strides: one taken for the other reads or writes the wrong block): every output bit-equal to the packed launch, the
    sentinel columns untouched, the strided run within the oracle bounds"""
    fam, cellname, H, B, dt, xmode = case
    fw = Fwd(fwd_problem(cellname, H, T7, B, dt, xmode), FAMILIES[fam][0], dt)
    packed, strided = fw.buffers(), fw.buffers()
    fw.launch(packed)
    ld_in, ld_out = par.STATE_LD_FACTOR * H, 4 * H
    h0_w, h0_v = column_block(fw.h0, ld_in, H, H)
    c0_w, c0_v = column_block(fw.c0, ld_in, H, H) if fw.lstm else (None, None)
    hl_w, hl_v = column_block(torch.full((B, H), SENT, device=DEV), ld_out, 2 * H, H)
    cl_w, cl_v = column_block(torch.full((B, H), SENT, device=DEV), ld_out, 2 * H, H) if fw.lstm else (None, None)
    keep = [h0_w.clone(), c0_w.clone() if fw.lstm else None]
    fw.launch(strided, h0=h0_v, c0=c0_v, h_last=hl_v, c_last=cl_v, h0_ld=ld_in, h_last_ld=ld_out)
    torch.cuda.synchronize()
    strided["h_last"], strided["c_last"] = hl_v.contiguous(), (cl_v.contiguous() if fw.lstm else None)
    fw.assert_same(strided, packed, "(column blocks vs packed)")
    assert_block_only(hl_w, 2 * H, H, "h_last")
    assert_same_bits(h0_w, keep[0], "the h0 buffer")
    if fw.lstm:
        assert_block_only(cl_w, 2 * H, H, "c_last")
        assert_same_bits(c0_w, keep[1], "the c0 buffer")
    fw.check_parity(strided, "(column blocks, %s)" % fam)


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_states_as_column_blocks(case, monkeypatch):
    """dh_last / dc_last read with dh_last_ld = 3H (columns [H, 2H)), dh0 / dc0 written with dh0_ld = 4H (columns [2H, 3H)), with
    and without an upstream gradient per step: as the forward test"""
    fam, cellname, H, B, dt, ext = case
    _env(fam, monkeypatch)
    bw = Bwd(bwd_problem(cellname, H, T7, B, dt, ext), FAMILIES[fam][0], dt)
    packed, strided = bw.buffers(), bw.buffers()
    bw.launch(packed)
    ld_in, ld_out = par.STATE_LD_FACTOR * H, 4 * H
    dl_w, dl_v = column_block(bw.dlast, ld_in, H, H)
    dcl_w, dcl_v = column_block(bw.dclast, ld_in, H, H) if bw.lstm else (None, None)
    d0_w, d0_v = column_block(torch.full((B, H), SENT, device=DEV), ld_out, 2 * H, H)
    dc0_w, dc0_v = column_block(torch.full((B, H), SENT, device=DEV), ld_out, 2 * H, H) if bw.lstm else (None, None)
    keep = [dl_w.clone(), dcl_w.clone() if bw.lstm else None]
    bw.launch(strided, dh_last=dl_v, dc_last=dcl_v, dh0=d0_v, dc0=dc0_v, dh_last_ld=ld_in, dh0_ld=ld_out)
    torch.cuda.synchronize()
    strided["dh0"], strided["dc0"] = d0_v.contiguous(), (dc0_v.contiguous() if bw.lstm else None)
    bw.assert_same(strided, packed, "(column blocks vs packed)")
    assert_block_only(d0_w, 2 * H, H, "dh0")
    assert_same_bits(dl_w, keep[0], "the dh_last buffer")
    if bw.lstm:
        assert_block_only(dc0_w, 2 * H, H, "dc0")
        assert_same_bits(dcl_w, keep[1], "the dc_last buffer")
    bw.check_parity(strided, "(column blocks, %s)" % fam)


# ---- 2. a sequence as consecutive launches ---------------------------------------------------------------------------------------
def _split_lengths(fam, cellname):
    """T = 7 for every family; T = 8 as 3 + 5 as well where the step loop is unrolled by two around the hand-over (il / w8 GRU)"""
    return [T7, 8] if cellname == "GRU" and fam in ("il", "w8") else [T7]


@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_as_consecutive_launches_carries_the_f32_state(case):
    """chunk k + 1 starts from h_last (and c_last, f32: 'without rounding the carried state') of chunk k; hs / cs / acts are time
    slices of the full buffers (slot t0 of hs is rewritten by the next chunk with the same value).  Bit-equal to the single launch -
    the state passes through memory as the f32 it is in registers, and a step does the same arithmetic wherever it stands in a
    launch - and within the bounds of the whole-sequence oracle"""
    fam, cellname, H, B, dt, xmode = case
    for T in _split_lengths(fam, cellname):
        fw = Fwd(fwd_problem(cellname, H, T, B, dt, xmode), FAMILIES[fam][0], dt)
        single = fw.buffers()
        fw.launch(single)
        for lengths in par.TIME_SPLITS[T]:
            out, h, c = fw.buffers(), fw.h0, fw.c0
            for t0, t1 in par.split_bounds(lengths):
                nh, nc = torch.zeros((B, H), device=DEV), (torch.zeros((B, H), device=DEV) if fw.lstm else None)
                fw.launch(out, t0, t1, h0=h, c0=c, h_last=nh, c_last=nc)
                h, c = nh, nc
            torch.cuda.synchronize()
            out["h_last"], out["c_last"] = h, c
            what = "(T = %d as %s)" % (T, "+".join(map(str, lengths)))
            fw.assert_same(out, single, what)
            fw.check_parity(out, what)


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_as_consecutive_launches_carries_the_f32_state(case, monkeypatch):
    """from the last time chunk to the first with dh_last <- dh0, dc_last <- dc0.  Bit-equal to the single launch in EVERY family:
    each BPTT kernel forms a step's gradient as d = dh + dhs_ext[t] from the carried dh (rnn.hip rnn_bwd_k, rnn_resident.hip
    rnn_bwd_res_k / lstm_bwd_il_body / gru_bwd_il_body, rnn_w8.hip gru_bwd_w8_body / lstm_bwd_w8_body: ``d = dh; d += ext``), never
    by starting the matrix accumulator of step t + 1 from dhs_ext[t] - so dh_last + dhs_ext[T - 1] of a chunk is the very addition
    the single launch does at that step, dh0 leaves as the f32 accumulator it is, and the order of additions is the same.  Also
    within the bounds of the whole-sequence oracle (which gets dc_last on top of dh_last: both enter the last chunk)"""
    fam, cellname, H, B, dt, ext = case
    _env(fam, monkeypatch)
    for T in _split_lengths(fam, cellname):
        bw = Bwd(bwd_problem(cellname, H, T, B, dt, ext), FAMILIES[fam][0], dt)
        single = bw.buffers()
        bw.launch(single)
        for lengths in par.TIME_SPLITS[T]:
            out, dh, dc = bw.buffers(), bw.dlast, bw.dclast
            for t0, t1 in reversed(par.split_bounds(lengths)):
                nh, nc = torch.zeros((B, H), device=DEV), (torch.zeros((B, H), device=DEV) if bw.lstm else None)
                bw.launch(out, t0, t1, dh_last=dh, dc_last=dc, dh0=nh, dc0=nc)
                dh, dc = nh, nc
            torch.cuda.synchronize()
            out["dh0"], out["dc0"] = dh, dc
            what = "(T = %d as %s)" % (T, "+".join(map(str, lengths)))
            bw.assert_same(out, single, what)
            bw.check_parity(out, what)


# ---- 3. chunk counters without a live partner ----------------------------------------------------------------------------------
GUARD, SPARE = 4, 2


def guarded(n, fill):
    """n words of ``fill`` between GUARD sentinel words in front and behind: (whole array, the n words)"""
    t = torch.full((n + 2 * GUARD,), par.WORD_SENTINEL, dtype=torch.int32, device=DEV)
    t[GUARD:GUARD + n] = fill
    return t, t[GUARD:GUARD + n]


def assert_counters(whole, fill, moved, what):
    """words 0 .. len(moved) - 1 of the guarded array = fill + moved, every other word as it was"""
    got = whole.cpu().numpy().astype(np.int64)
    want = np.full(got.shape, par.WORD_SENTINEL, np.int64)
    want[GUARD:-GUARD] = fill
    want[GUARD:GUARD + len(moved)] += np.asarray(moved, np.int64)
    assert np.array_equal(got, want), "%s: counters %s, expected %s" % (what, got.tolist(), want.tolist())


def _waves(lay):
    return int(hl.load().mvae_rnn_producer_waves(lay))


def _counter_variants(cs, forward, ext=True):
    """(value the wait_ready words hold or None = no waits, wait_value): no waits; wait_value 0 (= 1) on words at 1; a non-zero
    value on words at exactly that value.  Waits need a dense input / an upstream gradient, forward also chunk_steps >= 2"""
    if (forward and cs == 1) or not ext:
        return [(None, 0)]
    return [(None, 0), (1, 0), (5, 5)]


def _counter_run(run, launch, same, lay, T, cs, variants, what):
    """``launch(out, **pipe)`` with signal_done (and waits that never wait) against the plain launch ``run``: exact counters, twice"""
    per = par.expected_counters(T, cs, _waves(lay), RB)
    assert len(per) == par.chunk_count(T, cs)
    for ready_val, wait_value in variants:
        for fill in (0, 1000):
            whole, cnt = guarded(len(per) + SPARE, fill)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            pipe = dict(chunk_steps=cs, signal_done=cnt, status=status)
            rwhole = None
            if ready_val is not None:
                rwhole, ready = guarded(len(per), ready_val)
                pipe.update(wait_ready=ready, wait_value=wait_value)
            for n in (1, 2):                                        # the engine's counters are cumulative
                out = launch(**pipe)
                torch.cuda.synchronize()
                w = "%s T=%d cs=%d ready=%s launch %d" % (what, T, cs, ready_val, n)
                assert int(status.item()) == 0, w
                assert_counters(whole, fill, [n * p for p in per], w)
                if rwhole is not None:
                    assert_counters(rwhole, ready_val, [], w + " (wait_ready)")
                same(out, run, w)


@pytest.mark.parametrize("cs", par.COUNTER_CS)
@pytest.mark.parametrize("save", ["all", "hs"])
@pytest.mark.parametrize("fam,cellname", PIPE_FWD)
def test_forward_chunk_counters_without_a_partner(fam, cellname, save, cs):
    lay = FAMILIES[fam][0]
    for T in par.counter_lengths(cs):
        fw = Fwd(fwd_problem(cellname, RH, T, RB, BF16, "dense", seed=40 + T), lay, BF16)
        plain = fw.buffers(save)
        fw.launch(plain)

        def launch(**pipe):
            out = fw.buffers(save)
            fw.launch(out, **pipe)
            return out
        _counter_run(plain, launch, fw.assert_same, lay, T, cs, _counter_variants(cs, True), "%s %s save=%s" % (fam, cellname, save))
    # publishing needs hs: refused as mvae_rnn_fwd documents (signal_done && !hs), nothing launched, no counter moved
    whole, cnt = guarded(4, 0)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.rnn_fwd(fw.cell, BF16, fw.T, RB, RH, fw.up, xp=fw.kw["xp"], h0=fw.h0, c0=fw.c0, h_last=plain.h_last, seq_layout=lay,
                    chunk_steps=cs, signal_done=cnt)
    torch.cuda.synchronize()
    assert_counters(whole, 0, [], "refused launch")


@pytest.mark.parametrize("cs", par.COUNTER_CS)
@pytest.mark.parametrize("ext", [True, False])
@pytest.mark.parametrize("fam,cellname", PIPE_BWD)
def test_backward_chunk_counters_without_a_partner(fam, cellname, ext, cs, monkeypatch):
    _env(fam, monkeypatch)
    lay = FAMILIES[fam][0]
    for T in par.counter_lengths(cs):
        bw = Bwd(bwd_problem(cellname, RH, T, RB, BF16, ext), lay, BF16)
        plain = bw.buffers()
        bw.launch(plain)

        def launch(**pipe):
            out = bw.buffers()
            bw.launch(out, **pipe)
            return out
        _counter_run(plain, launch, bw.assert_same, lay, T, cs, _counter_variants(cs, False, ext), "%s %s ext=%s" % (fam, cellname, ext))


# ---- 4. a live partner -------------------------------------------------------------------------------------------------------------
def _live_value(T):
    """(value the producer publishes, wait_value): 0 means 1 at T = 8, a non-zero value at T = 9"""
    return (1, 0) if T == 8 else (3, 3)


@pytest.mark.parametrize("T", par.LIVE_T)
@pytest.mark.parametrize("cs", par.LIVE_CS_FWD)
@pytest.mark.parametrize("fam,cellname", PIPE_FWD)
def test_forward_waits_for_every_chunk_of_a_live_producer(fam, cellname, cs, T):
    """the kernel is launched FIRST on a dense xp that is NaN; a second queue copies the true xp over it chunk after chunk, first chunk
    to last, and publishes each chunk - the host is orders of magnitude slower than a 2 us step, so a read in front of its wait
    meets NaN.  Bit-equal to the un-pipelined launch on the true data, status 0"""
    lay = FAMILIES[fam][0]
    fw = Fwd(fwd_problem(cellname, RH, T, RB, BF16, "dense", seed=60 + T), lay, BF16)
    plain, out = fw.buffers(), fw.buffers()
    fw.launch(plain)
    true_xp = fw.kw["xp"]
    live_xp = torch.full_like(true_xp, float("nan"))
    n = par.chunk_count(T, cs)
    value, wait_value = _live_value(T)
    ready = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s1, s2 = two_queues()
    with no_host_sync():
        with torch.cuda.stream(s1):
            fw.launch(out, xp=live_xp, chunk_steps=cs, wait_ready=ready, wait_value=wait_value, status=status)
        with torch.cuda.stream(s2):
            for k in range(n):
                a, b = par.chunk_steps_of(k, T, cs)
                live_xp[a:b].copy_(true_xp[a:b])
                ops.stream_write_value32(ready[k:k + 1], value, stream=s2)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    fw.assert_same(out, plain, "(%s %s behind a live producer, T=%d cs=%d)" % (fam, cellname, T, cs))


@pytest.mark.parametrize("T", par.LIVE_T)
@pytest.mark.parametrize("cs", par.LIVE_CS_BWD)
@pytest.mark.parametrize("fam,cellname", PIPE_BWD)
def test_backward_waits_for_every_chunk_of_a_live_producer(fam, cellname, cs, T, monkeypatch):
    """as the forward test with dhs_ext (TILE16) as the gated input, written and published from the LAST chunk to the first - the
    order BPTT consumes them in; one-step chunks included (the backward kernels request the upstream gradient one step ahead,
    behind the wait at the start of every chunk's last-processed step)"""
    _env(fam, monkeypatch)
    lay = FAMILIES[fam][0]
    bw = Bwd(bwd_problem(cellname, RH, T, RB, BF16, True), lay, BF16)
    plain, out = bw.buffers(), bw.buffers()
    bw.launch(plain)
    true_d = bw.dext
    live_d = torch.full_like(true_d, float("nan"))
    n = par.chunk_count(T, cs)
    value, wait_value = _live_value(T)
    ready = torch.zeros(n, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s1, s2 = two_queues()
    with no_host_sync():
        with torch.cuda.stream(s1):
            bw.launch(out, dhs_ext=live_d, chunk_steps=cs, wait_ready=ready, wait_value=wait_value, status=status)
        with torch.cuda.stream(s2):
            for k in range(n - 1, -1, -1):
                a, b = par.chunk_steps_of(k, T, cs)
                live_d[a:b].copy_(true_d[a:b])
                ops.stream_write_value32(ready[k:k + 1], value, stream=s2)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    bw.assert_same(out, plain, "(%s %s behind a live producer, T=%d cs=%d)" % (fam, cellname, T, cs))


def _follow(s1, s2, launch, cnt, per, order, copies):
    """s2 waits for every chunk's counter in the kernel's own publishing order and copies that chunk's rows the moment it is
    released; then the kernel on s1 with signal_done.  Behind the kernel s1 copies the counters as the kernel left them - asserted
    exact here too - and only then (also behind a refused launch) writes the expected value into every counter: a kernel that
    published too little cannot leave s2 waiting for ever, and fails by its own counters, not by a later snapshot that is right."""
    left = torch.full_like(cnt, -1)
    with no_host_sync():
        with torch.cuda.stream(s2):
            for k, _ in order:
                ops.stream_wait_value32(cnt[k:k + 1], per[k], stream=s2)
                copies(k)
        with torch.cuda.stream(s1):
            try:
                launch()
                left.copy_(cnt)
            finally:
                for k in range(len(per)):
                    ops.stream_write_value32(cnt[k:k + 1], per[k], stream=s1)
    torch.cuda.synchronize()
    assert left.cpu().tolist() == list(per), "counters as the kernel left them: %s, expected %s" % (left.cpu().tolist(), list(per))


@pytest.mark.parametrize("T", par.LIVE_T)
@pytest.mark.parametrize("cs", par.LIVE_CS_FWD)
@pytest.mark.parametrize("fam,cellname", PIPE_FWD)
def test_forward_counters_follow_the_data(fam, cellname, cs, T):
    """a second queue waits for counter k = waves * B / 16 and copies the hs slots of chunk k (slots k cs + 1 .. min((k + 1) cs, T);
    slot 0 with chunk 0) into a snapshot, as the engine releases the projection GEMM of the layer above: the snapshot is bit-equal
    to the final hs - the slots are stored write-through before the counter moves, and no chunk is published a chunk early"""
    lay = FAMILIES[fam][0]
    fw = Fwd(fwd_problem(cellname, RH, T, RB, BF16, "dense", seed=60 + T), lay, BF16)
    plain, out = fw.buffers(), fw.buffers()
    fw.launch(plain)
    per = par.expected_counters(T, cs, _waves(lay), RB)
    cnt = torch.zeros(len(per), dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    snap = torch.full_like(out.hs, float("nan"))

    def copies(k):
        a, b = par.chunk_steps_of(k, T, cs)
        lo = a + (1 if k else 0)
        snap[lo:b + 1].copy_(out.hs[lo:b + 1])
    s1, s2 = two_queues()
    _follow(s1, s2, lambda: fw.launch(out, chunk_steps=cs, signal_done=cnt, status=status), cnt, per, par.publish_order(T, cs, True), copies)
    assert int(status.item()) == 0
    fw.assert_same(out, plain, "(publishing, T=%d cs=%d)" % (T, cs))
    assert_same_bits(snap, out.hs, "hs snapshots taken at the counters")


@pytest.mark.parametrize("T", par.LIVE_T)
@pytest.mark.parametrize("cs", par.LIVE_CS_BWD)
@pytest.mark.parametrize("fam,cellname", PIPE_BWD)
def test_backward_counters_follow_the_data(fam, cellname, cs, T, monkeypatch):
    """the da rows (GRU: and the rh rows) of chunk k, copied by a second queue once counter k has its value, chunks in descending
    order - how the engine releases a layer's weight-gradient GEMMs"""
    _env(fam, monkeypatch)
    lay = FAMILIES[fam][0]
    bw = Bwd(bwd_problem(cellname, RH, T, RB, BF16, True), lay, BF16)
    plain, out = bw.buffers(), bw.buffers()
    bw.launch(plain)
    per = par.expected_counters(T, cs, _waves(lay), RB)
    cnt = torch.zeros(len(per), dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    snap_da = torch.full_like(out.da, float("nan"))
    snap_rh = torch.full_like(out.rh, float("nan")) if bw.gru else None

    def copies(k):
        a, b = par.chunk_steps_of(k, T, cs)
        snap_da[a:b].copy_(out.da[a:b])
        if bw.gru:
            snap_rh[a:b].copy_(out.rh[a:b])
    s1, s2 = two_queues()
    _follow(s1, s2, lambda: bw.launch(out, chunk_steps=cs, signal_done=cnt, status=status), cnt, per, par.publish_order(T, cs, False), copies)
    assert int(status.item()) == 0
    bw.assert_same(out, plain, "(publishing, T=%d cs=%d)" % (T, cs))
    assert_same_bits(snap_da, out.da, "da snapshots taken at the counters")
    if bw.gru:
        assert_same_bits(snap_rh, out.rh, "rh snapshots taken at the counters")


# ---- 5. phase launches called directly ----------------------------------------------------------------------------------------
PHASE_FAMILIES = [("il", "LSTM"), ("il", "GRU"), ("w8", "GRU")]


@pytest.mark.parametrize("save", ["all", "hs"])
@pytest.mark.parametrize("fam,cellname", PHASE_FAMILIES)
def test_phase_forward_equals_the_single_launches(fam, cellname, save):
    """mvae_rnn_fwd_multi on problems of different T, B (1, 2, 3 row tiles: every base[] differs), weights and input mode: every
    problem bit-equal to its single launch, and within the oracle bounds"""
    lay = FAMILIES[fam][0]
    fws = [Fwd(fwd_problem(cellname, RH, T, B, BF16, xm, seed=par.phase_seed(i, cellname)), lay, BF16)
           for i, (T, B, xm, _) in enumerate(par.PHASE_PROBLEMS)]
    singles, multis = [fw.buffers(save) for fw in fws], [fw.buffers(save) for fw in fws]
    for fw, out in zip(fws, singles):
        fw.launch(out)
    args = [fw.launch(out, build_only=True) for fw, out in zip(fws, multis)]
    assert ops.rnn_fwd_multi(args) is True
    torch.cuda.synchronize()
    for i, (fw, s, m) in enumerate(zip(fws, singles, multis)):
        fw.assert_same(m, s, "(problem %d of the phase launch)" % i)
        fw.check_parity(m, "(problem %d of the phase launch, %s)" % (i, fam))


@pytest.mark.parametrize("fam,cellname", PHASE_FAMILIES)
def test_phase_backward_equals_the_single_launches(fam, cellname):
    lay = FAMILIES[fam][0]
    bws = []
    for i, (T, B, _, ext) in enumerate(par.PHASE_PROBLEMS):
        rnd = _rnd(BF16)
        f = fwd_problem(cellname, RH, T, B, BF16, "dense", seed=par.phase_seed(i, cellname) + 1)
        rng = np.random.default_rng(par.phase_seed(i, cellname) + 2)
        pb = par.Problem(cellname=cellname, H=RH, T=T, B=B, U=f.U, hs_r=rnd(f.hs), cs_r=rnd(f.cs) if f.cs is not None else None,
                         acts_r=rnd(f.acts), dext=rnd(rng.standard_normal((T, B, RH)) * 0.1) if ext else None,
                         dlast=rng.standard_normal((B, RH)) * 0.1, dclast=par.carried_cell_gradient(RH, B) if cellname == "LSTM" else None)
        bws.append(Bwd(pb, lay, BF16))
    singles, multis = [bw.buffers() for bw in bws], [bw.buffers() for bw in bws]
    for bw, out in zip(bws, singles):
        bw.launch(out)
    args = [bw.launch(out, build_only=True) for bw, out in zip(bws, multis)]
    assert ops.rnn_bwd_multi(args) is True
    torch.cuda.synchronize()
    for i, (bw, s, m) in enumerate(zip(bws, singles, multis)):
        bw.assert_same(m, s, "(problem %d of the phase launch)" % i)
        bw.check_parity(m, "(problem %d of the phase launch, %s)" % (i, fam))


@pytest.mark.parametrize("blocks", par.XPAND_BLOCKS)
@pytest.mark.parametrize("variant", ["outer", "table"])
@pytest.mark.parametrize("fam,cellname", PHASE_FAMILIES)
def test_phase_forward_behind_an_expansion_producer(fam, cellname, variant, blocks):
    """an ``xpand`` producer inside the launch - the 1-feature expansion xs w + bias, or the rows table[idx] of a one-hot layer - wired
    as Engine._xpand_problem does (chunk_rows = cs B, the consumer waits for waves * blocks per chunk, producer first): ``out`` is
    bit-equal to mvae_outer_bias_tile16 / the gathered rows, every chunk_done word = waves * blocks, and the dense-input recurrence
    that follows it chunk by chunk is bit-equal to its single launch on that ``out``"""
    lay = FAMILIES[fam][0]
    T, cs, B = par.XPAND_T, par.XPAND_CS, par.XPAND_B
    GH, R, n = vo.GATES[cellname] * RH, T * B, T // cs
    x = par.xpand_problem(GH, R, seed=blocks + GH)
    td = torch.bfloat16
    out, want = torch.full((T, B, GH), float("nan"), dtype=td, device=DEV), torch.zeros((T, B, GH), dtype=td, device=DEV)
    whole, done = guarded(n, 0)
    keep = []
    if variant == "outer":
        keep = [dev(x.xs), dev(x.w), dev(x.bias)]
        ops.outer_bias_tile16(keep[0], keep[1], keep[2], want, R, GH)
        xa = ops.xpand(keep[0], keep[1], keep[2], out, R, GH, cs * B, done, blocks)
    else:
        keep = [dev(x.idx, torch.uint8), dev(x.table, td)]
        want = tile16(keep[1][keep[0].long()].contiguous().view(T, B, GH), R, GH, True)
        xa = ops.xpand(None, None, None, out, R, GH, cs * B, done, blocks, idx=keep[0], table=keep[1])
    xp_rm = host(tile16(want, R, GH, False))
    base = fwd_problem(cellname, RH, T, B, BF16, "const", seed=7 + blocks)          # (its U, h0, c0)
    pb = par.Problem(base)
    pb.update(xmode="dense", xp=xp_rm, xp0=None)
    fw = Fwd(pb, lay, BF16)
    oracle = vo.rnn_forward(cellname, xp_rm, pb.U, pb.h0, pb.c0)
    single, multi = fw.buffers(), fw.buffers()
    fw.launch(single, xp=want)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    waves = _waves(lay)
    arg = fw.launch(multi, xp=out, chunk_steps=cs, wait_ready=done, wait_value=waves * blocks, status=status, build_only=True)
    assert ops.rnn_fwd_multi([arg], [xa]) is True
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert_same_bits(out, want, "the producer's out")
    assert_counters(whole, 0, [waves * blocks] * n, "chunk_done")
    fw.assert_same(multi, single, "(behind the %s producer, %d blocks)" % (variant, blocks))
    fw.check_parity(multi, "(behind the %s producer)" % variant, oracle=oracle)
    assert keep


def test_what_the_entry_points_refuse(monkeypatch):
    """nothing is launched by any of these: phase launches of mixed cell types, with a SCALAR input or mixed save modes
    (MVAE_E_UNSUPPORTED: launch them one by one), an indexed problem with a row-major table, n > 8, n_xpand > 2 (MVAE_E_ARG); one-step
    chunks with wait_ready in the forward direction (the kernels read xp one or two steps ahead and wait once per chunk); families
    that do not take a cell, an input mode or the hand-over fields"""
    monkeypatch.delenv("MVAE_LSTM_BWD_W8", raising=False)
    T, B = 4, 16
    P, Q = hl.TILE16P, hl.TILE16Q
    mk = lambda c, xm, lay: Fwd(fwd_problem(c, RH, T, B, BF16, xm, seed=5), lay, BF16)
    lstm, gru, gruq, sca = mk("LSTM", "dense", P), mk("GRU", "dense", P), mk("GRU", "dense", Q), mk("LSTM", "scalar", P)
    keep = []                                   # (the buffers of built problems stay alive until their launch call returns)

    def built(fw, save="all", **kw):
        out = fw.buffers(save)
        keep.append(out)
        return fw.launch(out, build_only=True, **kw)
    assert ops.rnn_fwd_multi([built(lstm), built(gru)]) is False                       # mixed cell types
    assert ops.rnn_fwd_multi([built(lstm), built(sca)]) is False                       # a SCALAR input
    assert ops.rnn_fwd_multi([built(lstm), built(lstm, "hs")]) is False                # mixed save modes
    assert ops.rnn_fwd_multi([built(gruq), built(gruq, "hs")]) is False
    idx = mk("LSTM", "index", hl.TILE16)                                               # (its table is row-major)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.rnn_fwd_multi([built(lstm), _with_layout(idx, P, keep)])
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.rnn_fwd_multi([built(lstm) for _ in range(9)])                             # n > 8
    GH = 4 * RH
    xo = torch.zeros((T, B, GH), dtype=torch.bfloat16, device=DEV)
    xs, w, bias = torch.zeros(T * B, device=DEV), torch.zeros(GH, device=DEV), torch.zeros(GH, device=DEV)
    done = torch.zeros(2, dtype=torch.int32, device=DEV)
    xa = [ops.xpand(xs, w, bias, xo, T * B, GH, 2 * B, done, 2) for _ in range(3)]
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.rnn_fwd_multi([built(lstm)], xa)                                           # n_xpand > 2
    ready = torch.ones(T, dtype=torch.int32, device=DEV)
    for fw in (lstm, gru, gruq):                                                       # one-step chunks with wait_ready
        with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
            fw.launch(fw.buffers(), chunk_steps=1, wait_ready=ready)
        with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
            ops.rnn_fwd_multi([built(fw, chunk_steps=1, wait_ready=ready)])
        with pytest.raises(RuntimeError, match="MVAE_E_ARG"):                          # ... hand-over fields without a chunk length
            fw.launch(fw.buffers(), wait_ready=ready)
    idxp = mk("LSTM", "index", P)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):                              # waits gate a DENSE input only
        idxp.launch(idxp.buffers(), chunk_steps=2, wait_ready=ready)
    for c, xm, lay in (("LSTM", "scalar", P), ("LSTM", "dense", Q), ("GRU", "scalar", Q)):     # not these families'
        fw = mk(c, xm, lay)
        with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):
            fw.launch(fw.buffers())
    for lay in (hl.ROWMAJOR, hl.TILE16):                                               # only the il / w8 kernels poll and publish
        fw = mk("LSTM", "dense", lay)
        with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):
            fw.launch(fw.buffers(), chunk_steps=2, signal_done=done)
    rnn = Fwd(fwd_problem("SimpleRNN", RH, T, B, BF16, "dense", seed=5), hl.TILE16, BF16)
    with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):
        rnn.launch(rnn.buffers())
    bl, bg = (Bwd(bwd_problem(c, RH, T, B, BF16, True), P, BF16) for c in ("LSTM", "GRU"))

    def bbuilt(bw, **kw):
        out = bw.buffers()
        keep.append(out)
        return bw.launch(out, build_only=True, **kw)
    assert ops.rnn_bwd_multi([bbuilt(bl), bbuilt(bg)]) is False                        # mixed cell types
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.rnn_bwd_multi([bbuilt(bl) for _ in range(9)])
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):                              # waits gate dhs_ext
        bl.launch(bl.buffers(), dhs_ext=None, chunk_steps=2, wait_ready=ready)
    blq = Bwd(bwd_problem("LSTM", RH, T, B, BF16, True), Q, BF16)
    with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):                      # the w8 LSTM BPTT takes TILE16P data, under its switch
        blq.launch(blq.buffers())
    torch.cuda.synchronize()


def _with_layout(fw, lay, keep):
    """the problem of ``fw`` (an indexed input with a ROW-MAJOR table) declared for another sequence layout"""
    out = fw.buffers()
    keep.append(out)
    saved, fw.lay = fw.lay, lay
    try:
        return fw.launch(out, build_only=True)
    finally:
        fw.lay = saved
