"""Operator-level parity: every C-ABI kernel vs the float64 oracle on seeded inputs (GPU box only).

Tolerances: f32 mode (exact-f32 MFMA, f32 storage) rtol/atol 2e-4 class against float64; bf16 mode (bf16 MFMA
operands + bf16 sequence storage, f32 accumulate/state) 3e-2 class.  Integer outputs (argmax) are bit-exact.
``close(got, want, tol)`` bounds |err| by tol * (1 + |want|): an absolute floor of tol, far above the recurrent kernels'
gate gradients (~2.5e-3), dh0 / dc0 without an upstream gradient and the heads' d(logits) and dhs (~1/R) - a zero gradient
passes it.  So the recurrent and head tests also check every output block by block at its own scale (tests/parity.py:
per (time step, gate) for acts / da, per time step for hs / cs, per row for probabilities, d(logits) and dhs, the whole
tensor for h_last / dh0 / dc0; elementwise against rtol |want| + floor * block RMS and normwise, one table of constants per
mode), and the heads' loss to a relative 1e-4 (the oracle is given the kernel's rounded hs and W).  The bf16 constants
come from a rounding model of a correct kernel and the margins measured on the MI355X (profiles/r08_parity_margins.txt).
The GEMM and reduction tests keep their ``close`` / ``assert_allclose`` calls, sized for unrounded operands, and beside them hold
every output to the f32 accumulation unit of its own element (parity.assert_product: c_acc units + half an ulp of a bf16 output,
normwise, zero stays zero - constants from a CPU model of a correct accumulation, test_parity_gemm_cpu.py), and run every path
once more on small-integer operands, where the result must be BIT-equal to float64 (parity.assert_bits).  The kernels of
csrc/misc.hip and csrc/latent.hip have files of their own: test_small_ops_gpu.py, test_latent_ops_gpu.py.  Margins measured on
the MI355X against the new bounds: profiles/r09_op_parity_margins.txt.
Saturation: the ``*_saturated`` / ``*_clipped_rows`` / ``*_extremes`` tests run the same paths on problems that sit ON the kinks
(tests/parity.py: clipped hard-sigmoid gates and planted +-60 rows, a cell state past the range of e^{2c}, target probabilities
beyond both clips of the cross-entropy, sigmoid logits of +-100 and 0) with the same bounds, exact zeros where the derivative is
zero, and the forward kernels' own buffers handed to the backward kernels; margins: profiles/r10_saturation_margins.txt.
"""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from oracle import vae_oracle as vo
from tests import parity as par
from tests.gpu_util import (DEV, _paired8_columns, _paired_columns, close, dev, host, no_host_sync, pairing,  # noqa: F401
                            tile16, two_queues)

pytestmark = pytest.mark.gpu

CELLS = [("GRU", hl.GRU), ("LSTM", hl.LSTM), ("SimpleRNN", hl.RNN)]
DTYPES = [(hl.F32, 3e-4), (hl.BF16, 4e-2)]


def seq_layouts(res, cellname, xmode="dense", forward=True):
    """sequence layouts (= kernel families) to exercise: generic row-major; resident phased (TILE16); for LSTM / GRU
    without a scalar input also the slot-interleaved kernels (TILE16P: saved activations in tile pairs); for GRU the
    two-waves-per-SIMD kernels (TILE16Q: tiles j and j + 8 paired)"""
    if not res:
        return [hl.ROWMAJOR]
    lays = [hl.TILE16, hl.TILE16P] if (cellname in ("LSTM", "GRU") and xmode != "scalar") else [hl.TILE16]
    if cellname == "GRU" and xmode != "scalar" and (forward or W8_BACKWARD):
        lays.append(hl.TILE16Q)
    return lays


W8_BACKWARD = True       # (the two-waves-per-SIMD BPTT kernel)


def resident(H, B, dtype, cell):
    """the shapes the resident-weights kernels take (TILE16 sequence layout)"""
    return H == 256 and B % 16 == 0 and dtype == hl.BF16 and cell != hl.RNN


_rnn_problem = par.rnn_problem         # (shared with test_parity_cpu.py: the same problems on the CPU)


def test_paired_lookup_table_layout_and_its_rejection():
    """PrepBatch.make_table(paired=True) writes the NumPy permutation; mvae_rnn_fwd refuses a table in the wrong layout"""
    rng = np.random.default_rng(3)
    K, N = 7, 1024
    W, b = rng.standard_normal((K, N)), rng.standard_normal(N)
    plain = torch.zeros((K, N), dtype=torch.bfloat16, device=DEV)
    paired = torch.zeros_like(plain)
    ops.make_table(dev(W), dev(b), plain)
    ops.make_table_paired(dev(W), dev(b), paired)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(paired), _paired_columns(host(plain)))
    T, B, H = 4, 16, 256
    up = ops.pack_recurrent(dev(rng.standard_normal((H, 4 * H)) * 0.05), hl.LSTM, hl.BF16, 0)
    idx = dev(rng.integers(0, K, (T, B)), torch.uint8)
    hs = torch.zeros((T + 1, B, H), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):         # the slot-interleaved kernels need the paired table
        ops.rnn_fwd(hl.LSTM, hl.BF16, T, B, H, up, idx=idx, table=plain, hs=hs, seq_layout=hl.TILE16P)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):         # ... and nothing else takes it
        ops.rnn_fwd(hl.LSTM, hl.BF16, T, B, H, up, idx=idx, table=paired, hs=hs, seq_layout=hl.TILE16, table_layout=hl.TABLE_PAIRED)


@pytest.mark.parametrize("cellname,cell", CELLS)
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("xmode", ["dense", "index", "scalar", "const"])
@pytest.mark.parametrize("H,B", [(64, 5), (128, 37), (256, 21), (256, 32)])
def test_rnn_forward(cellname, cell, dtype, tol, xmode, H, B):
    T = 9
    rng, G, U, W, b, h0, c0 = _rnn_problem(cellname, H, T, B, seed=H + B)
    GH = G * H
    td = ops.torch_dtype(dtype)
    kw = {}
    if xmode == "dense":
        xp = rng.standard_normal((T, B, GH)) * 0.5
        if dtype == hl.BF16:
            xp = host(dev(xp, td))       # the kernel sees bf16-rounded inputs; give the oracle the same
        kw["xp"] = dev(xp, td)
    elif xmode == "index":
        idx = rng.integers(0, 7, (T, B))
        table = host(dev(W + b, td))
        xp = table[idx]
        kw["idx"], kw["table"] = dev(idx, torch.uint8), dev(table, td)
    elif xmode == "scalar":
        xs = rng.random((T, B))
        xp = xs[..., None] * W[0] + b
        kw["xs"], kw["w_row"], kw["bias"] = dev(xs), dev(W[0]), dev(b)
    else:
        xp0 = host(dev(rng.standard_normal((B, GH)) * 0.5, td))
        xp = np.broadcast_to(xp0[None], (T, B, GH)).copy()
        kw["xp0"] = dev(xp0, td)
    hs_o, cs_o, acts_o = vo.rnn_forward(cellname, xp, U, h0, c0 if cellname == "LSTM" else None)
    _rnn_forward_run(cellname, cell, dtype, tol, xmode, T, B, H, U, h0, c0, kw, (hs_o, cs_o, acts_o))


def _rnn_forward_run(cellname, cell, dtype, tol, xmode, T, B, H, U, h0, c0, kw, oracle, keep_device=False):
    """the forward kernel of every sequence layout the shape takes, on the inputs ``kw`` (row-major device tensors), against the
    oracle's (hs, cs, acts): ``close`` and the parity bounds.  Returns one dict per layout: the outputs as row-major float64 and the
    worst ratio to the bounds per output; ``keep_device``: also the kernel's own buffers, untouched and in their layout."""
    hs_o, cs_o, acts_o = oracle
    GH = vo.GATES[cellname] * H
    td = ops.torch_dtype(dtype)
    kw = dict(kw)
    up = ops.pack_recurrent(dev(U), cell, dtype, 0)
    res = resident(H, B, dtype, cell)
    if res and "xp" in kw:
        kw["xp"] = tile16(kw["xp"], T * B, GH, True)
    runs = []
    for lay in seq_layouts(res, cellname, xmode):
        hs = torch.zeros((T + 1, B, H), dtype=td, device=DEV)
        cs = torch.zeros((T + 1, B, H), dtype=td, device=DEV) if cellname == "LSTM" else None
        acts = torch.zeros((T, B, GH), dtype=td, device=DEV)
        h_last = torch.zeros((B, H), device=DEV)
        kwl = dict(kw)
        if xmode == "index" and cellname in ("LSTM", "GRU") and lay == hl.TILE16P:
            # the slot-interleaved LSTM / GRU kernels gather tile pairs: MVAE_TABLE_PAIRED column order (include/midivae_hip.h), built
            # here in NumPy - the device's own permutation (PrepBatch.make_table(paired=True)) is checked against it below
            kwl["table"], kwl["table_layout"] = dev(_paired_columns(host(kw["table"])), td), hl.TABLE_PAIRED
        if xmode == "index" and lay == hl.TILE16Q:
            kwl["table"], kwl["table_layout"] = dev(_paired8_columns(host(kw["table"])), td), hl.TABLE_PAIRED8
        ops.rnn_fwd(cell, dtype, T, B, H, up, h0=dev(h0), c0=dev(c0) if cellname == "LSTM" else None, hs=hs, cs=cs,
                    acts=acts, h_last=h_last, seq_layout=lay, **kwl)
        torch.cuda.synchronize()
        own = dict(hs=hs, cs=cs, acts=acts) if keep_device else None
        if res:
            acts = tile16(acts, T * B, GH, False, paired=pairing(lay))
            if cs is not None:
                cs = tile16(cs, (T + 1) * B, H, False, paired=pairing(lay))
        what = " (layout %d)" % lay
        close(host(hs), hs_o, tol, "hs" + what)
        close(host(acts), acts_o, tol, "acts" + what)
        close(host(h_last), hs_o[-1], tol, "h_last" + what)
        if cs is not None:
            close(host(cs), cs_o, tol, "cs" + what)
        ratios = dict(hs=par.assert_parity(host(hs), hs_o, dtype, par.step_blocks, "hs" + what, values=True),
                      acts=par.assert_parity(host(acts), acts_o, dtype, par.gate_blocks(cellname), "acts" + what, values=True),
                      h_last=par.assert_parity(host(h_last), hs_o[-1], dtype, par.whole, "h_last" + what, values=True))
        if cs is not None:
            ratios["cs"] = par.assert_parity(host(cs), cs_o, dtype, par.step_blocks, "cs" + what, values=True)
        runs.append(dict(lay=lay, res=res, hs=host(hs), cs=host(cs) if cs is not None else None, acts=host(acts), h_last=host(h_last),
                         ratios=ratios, own=own))
    return runs


@pytest.mark.parametrize("xmode", ["dense", "index", "const"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 33])
def test_gru_forward_two_waves_per_simd_short_odd_and_long(xmode, T):
    """rnn_w8.hip (seq_layout TILE16Q): the step loop is unrolled by two with half of every step deferred into the next one and
    hand-counted memory waits - lengths 1..7 and a longer odd one, every input mode, training / h-sequence-only / inference saves."""
    H, B, cellname, cell = 256, 48, "GRU", hl.GRU
    rng, G, U, W, b, h0, c0 = _rnn_problem(cellname, H, T, B, seed=100 + T)
    GH, td = G * H, torch.bfloat16
    kw = {}
    if xmode == "dense":
        xp = host(dev(rng.standard_normal((T, B, GH)) * 0.5, td))
        kw["xp"] = tile16(dev(xp, td), T * B, GH, True)
    elif xmode == "index":
        idx = rng.integers(0, 61, (T, B))
        table = host(dev(rng.standard_normal((61, GH)) * 0.5, td))
        xp = table[idx]
        kw.update(idx=dev(idx, torch.uint8), table=dev(_paired8_columns(table), td), table_layout=hl.TABLE_PAIRED8)
    else:
        xp0 = host(dev(rng.standard_normal((B, GH)) * 0.5, td))
        xp = np.broadcast_to(xp0[None], (T, B, GH)).copy()
        kw["xp0"] = dev(xp0, td)
    hs_o, _, acts_o = vo.rnn_forward(cellname, xp, U, h0, None)
    up = ops.pack_recurrent(dev(U), cell, hl.BF16, 0)
    tol = dict(DTYPES)[hl.BF16]
    for save in ("all", "hs", "none"):
        hs = torch.zeros((T + 1, B, H), dtype=td, device=DEV) if save != "none" else None
        acts = torch.zeros((T, B, GH), dtype=td, device=DEV) if save == "all" else None
        h_last = torch.zeros((B, H), device=DEV)
        ops.rnn_fwd(cell, hl.BF16, T, B, H, up, h0=dev(h0), hs=hs, acts=acts, h_last=h_last, seq_layout=hl.TILE16Q, **kw)
        torch.cuda.synchronize()
        close(host(h_last), hs_o[-1], tol, "h_last (%s)" % save)
        if hs is not None:
            close(host(hs), hs_o, tol, "hs (%s)" % save)
        if acts is not None:
            close(host(tile16(acts, T * B, GH, False, paired="q")), acts_o, tol, "acts")
        par.assert_parity(host(h_last), hs_o[-1], hl.BF16, par.whole, "h_last (%s)" % save, values=True)
        if hs is not None:
            par.assert_parity(host(hs), hs_o, hl.BF16, par.step_blocks, "hs (%s)" % save, values=True)
        if acts is not None:
            par.assert_parity(host(tile16(acts, T * B, GH, False, paired="q")), acts_o, hl.BF16, par.gate_blocks(cellname), "acts",
                              values=True)


def test_paired8_table_and_tile16q_relayout():
    """the device's MVAE_TABLE_PAIRED8 permutation and the TILE16Q relayout against their definitions in include/midivae_hip.h"""
    rng = np.random.default_rng(5)
    K, N = 61, 768
    W, b = rng.standard_normal((K, N)), rng.standard_normal(N)
    tab, plain = (torch.zeros((K, N), dtype=torch.bfloat16, device=DEV) for _ in range(2))
    pb = ops.PrepBatch()
    pb.make_table(dev(W), dev(b), tab, paired=8)
    pb.make_table(dev(W), dev(b), plain)
    pb.run()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(tab), _paired8_columns(host(plain)))
    rows, cols = 32, 768
    a = rng.standard_normal((rows, cols))
    m, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    off = (((m // 16) * (cols // 32) + (c // 256) * 8 + (c // 16) % 8) * 64 + ((c % 16) // 4) * 16 + m % 16) * 8 + ((c // 128) % 2) * 4 + c % 4
    want = np.empty(rows * cols)
    want[off.ravel()] = host(dev(a, torch.bfloat16)).ravel()
    got = tile16(dev(a, torch.bfloat16), rows, cols, True, paired="q")
    np.testing.assert_array_equal(host(got).ravel(), want)
    back = tile16(got, rows, cols, False, paired="q")
    np.testing.assert_array_equal(host(back), host(dev(a, torch.bfloat16)))


def test_rnn_forward_zero_initial_state_and_inference_mode():
    """h0/c0 NULL = zeros; hs/cs/acts NULL = inference: only the final state is produced."""
    rng, G, U, W, b, h0, c0 = _rnn_problem("LSTM", 64, 6, 16, seed=3)
    xp = rng.standard_normal((6, 16, G * 64)) * 0.5
    hs_o, _, _ = vo.rnn_forward("LSTM", xp, U, np.zeros((16, 64)), np.zeros((16, 64)))
    h_last = torch.zeros((16, 64), device=DEV)
    ops.rnn_fwd(hl.LSTM, hl.F32, 6, 16, 64, ops.pack_recurrent(dev(U), hl.LSTM, hl.F32, 0), xp=dev(xp), h_last=h_last)
    torch.cuda.synchronize()
    close(host(h_last), hs_o[-1], 3e-4)


@pytest.mark.parametrize("cellname,cell", CELLS)
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("H,B,ext", [(64, 5, True), (128, 20, False), (256, 19, True), (256, 33, False), (256, 32, True),
                                     (256, 16, False)])
def test_rnn_backward(cellname, cell, dtype, tol, H, B, ext):
    _rnn_backward_case(cellname, cell, dtype, tol, H, B, ext, T=8)


@pytest.mark.parametrize("cellname,cell", [c for c in CELLS if c[0] in ("GRU", "LSTM")])
@pytest.mark.parametrize("T", [1, 2, 3, 7])
def test_rnn_backward_resident_kernels_short_and_odd_lengths(cellname, cell, T):
    """The slot-interleaved backward kernels process time steps in pairs (alternating prefetch buffers) with a single
    trailing step for odd T: lengths 1, 2, 3 and 7 at H=256 bf16, with and without an upstream gradient."""
    for ext in (True, False):
        _rnn_backward_case(cellname, cell, hl.BF16, dict(DTYPES)[hl.BF16], 256, 32, ext, T=T)


@pytest.mark.parametrize("T,ext", [(1, True), (2, False), (7, True), (8, False)])
def test_lstm_backward_two_waves_per_simd_experiment_keeps_parity(T, ext, monkeypatch):
    """MVAE_LSTM_BWD_W8=1: the LSTM BPTT on 8 waves per workgroup with a quarter of U^T streamed from L2 (rnn_w8.hip) - slower than
    the 4-wave kernel (in-order vmcnt) and off by default, but the same function of the same data"""
    monkeypatch.setenv("MVAE_LSTM_BWD_W8", "1")
    _rnn_backward_case("LSTM", hl.LSTM, hl.BF16, dict(DTYPES)[hl.BF16], 256, 32, ext, T=T)


def _rnn_backward_case(cellname, cell, dtype, tol, H, B, ext, T, saturated=False):
    """``saturated``: the problem of par.rnn_saturated_problem (clipped gates, planted rows) instead of par.rnn_backward_problem,
    and beyond the same checks: a gate whose SAVED value is exactly 0 or 1 has a gradient of exactly zero, and rh = r * h exactly
    where r is clipped"""
    GH = vo.GATES[cellname] * H
    td = ops.torch_dtype(dtype)
    rnd = (lambda a: host(dev(a, td))) if dtype == hl.BF16 else (lambda a: a)
    if saturated:
        pb = par.rnn_saturated_problem(cellname, H, T, B, par.saturated_seed(H, T, B), lambda a: host(dev(a, td)))
        U, hs_o, cs_o, acts_o, dext, dlast = pb.U, pb.hs_r, pb.cs_r, pb.acts_r, (pb.dext if ext else None), pb.dlast
    else:
        U, hs_o, cs_o, acts_o, dext, dlast = par.rnn_backward_problem(cellname, H, T, B, ext, rnd)
    da_o, dU_o, dh0_o, dc0_o = vo.rnn_backward(cellname, hs_o, cs_o, acts_o, U, dext, dlast)

    ut = ops.pack_recurrent(dev(U), cell, dtype, 1)
    res = resident(H, B, dtype, cell)
    for lay in seq_layouts(res, cellname, forward=False):
        da = torch.zeros((T, B, GH), dtype=td, device=DEV)
        rh = torch.zeros((T, B, H), dtype=td, device=DEV)
        dh0 = torch.zeros((B, H), device=DEV)
        dc0 = torch.zeros((B, H), device=DEV)
        acts_d, cs_d = dev(acts_o, td), dev(cs_o, td) if cs_o is not None else None
        dext_d = dev(dext, td) if ext else None
        if res:
            pr = pairing(lay)
            acts_d = tile16(acts_d, T * B, GH, True, paired=pr)
            cs_d = tile16(cs_d, (T + 1) * B, H, True, paired=pr) if cs_d is not None else None
            dext_d = tile16(dext_d, T * B, H, True) if ext else None
        ops.rnn_bwd(cell, dtype, T, B, H, ut, dev(hs_o, td), cs_d, acts_d, da, dhs_ext=dext_d, dh_last=dev(dlast), rh=rh,
                    dh0=dh0, dc0=dc0, seq_layout=lay)
        torch.cuda.synchronize()
        what = " (layout %d)" % lay
        close(host(da), da_o, tol, "da" + what)
        close(host(dh0), dh0_o, tol, "dh0" + what)
        if cellname == "LSTM":
            close(host(dc0), dc0_o, tol, "dc0" + what)
        if cellname == "GRU":
            close(host(rh), acts_o[:, :, H:2 * H] * hs_o[:-1], tol, "rh" + what)
        par.assert_parity(host(da), da_o, dtype, par.gate_blocks(cellname), "da" + what)
        par.assert_parity(host(dh0), dh0_o, dtype, par.whole, "dh0" + what)
        if cellname == "LSTM":
            par.assert_parity(host(dc0), dc0_o, dtype, par.whole, "dc0" + what)
        if saturated:
            _saturated_backward_checks(cellname, H, acts_o, hs_o, host(da), host(rh), what)


def _saturated_backward_checks(cellname, H, acts, hs, da, rh, what):
    """acts / hs: the saved sequences the kernel was handed (row-major float64); at least 10 % of the gates must be clipped per side"""
    if cellname == "SimpleRNN":
        return
    n = par.assert_clipped_gates_have_no_gradient(cellname, acts, da, "da" + what)
    lo, hi = par.clipped_share(cellname, acts)
    assert lo >= 0.10 and hi >= 0.10 and n > 0, (lo, hi)
    if cellname == "GRU":
        r = acts[:, :, H:2 * H]
        clipped = (r == 0.0) | (r == 1.0)
        assert np.array_equal(rh[clipped], (r * hs[:-1])[clipped]), "rh at a clipped reset gate" + what


@pytest.mark.parametrize("cellname,cell", CELLS)
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("xmode", ["dense", "index"])
@pytest.mark.parametrize("H,B", par.SAT_FWD_SHAPES)
def test_rnn_forward_saturated(cellname, cell, dtype, tol, xmode, H, B):
    """test_rnn_forward on par.rnn_saturated_problem: pre-activation inputs of standard deviation 2 - 14 to 34 % of the hard-sigmoid
    gate values clipped at 0 and as many at 1 - and the planted rows +60 / -60 / alternating (tanh of +-60: e^{2x} = inf in the
    hardware form); dense input and table rows that carry the large values; every sequence layout of the shape.  (H = 384, 512:
    test_hidden_sizes_gpu.py)"""
    _rnn_forward_saturated_case(cellname, cell, dtype, tol, xmode, H, B, par.SAT_T_FWD)


def _rnn_forward_saturated_case(cellname, cell, dtype, tol, xmode, H, B, T, keep_device=False):
    td = ops.torch_dtype(dtype)
    pb = par.rnn_saturated_problem(cellname, H, T, B, par.saturated_seed(H, T, B), lambda a: host(dev(a, td)), xmode)
    if xmode == "dense":
        kw = dict(xp=dev(pb.xp, td))
    elif xmode == "index":
        kw = dict(idx=dev(pb.idx, torch.uint8), table=dev(pb.table, td))
    else:
        kw = dict(xp0=dev(pb.xp0, td))
    if cellname != "SimpleRNN":
        lo, hi = par.clipped_share(cellname, pb.acts)
        assert lo >= 0.10 and hi >= 0.10, (lo, hi)
    runs = _rnn_forward_run(cellname, cell, dtype, tol, xmode, T, B, H, pb.U, pb.h0, pb.c0, kw, (pb.hs, pb.cs, pb.acts),
                            keep_device=keep_device)
    for run in runs:
        for a in (run["hs"], run["cs"], run["acts"], run["h_last"]):
            assert a is None or np.all(np.isfinite(a))
    return pb, runs


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("xmode", ["dense", "const"])
def test_lstm_forward_cell_state_beyond_the_range_of_exp(dtype, tol, xmode):
    """T = 64 with the forget gate of the planted rows pinned at 1: their cell state grows by one per step to 64.8, and e^{2c}
    leaves the f32 range at c = 44.4 - tanh_fast then rests on rcp(inf) = 0.  bf16 on both resident layouts, f32 on the generic
    kernel.  Everything stays finite and within the bounds, and the planted rows' h is EXACTLY the oracle's (cast to the storage
    type) wherever that is decided beyond any rounding: units whose gates are all clipped at 0 (c = h = 0), and units with
    |c| > 12, where 1 - tanh(c) < 8e-11 - far below half an ulp of 1 in f32 - and o = 1."""
    H, T, B = par.SAT_LONG
    pb, runs = _rnn_forward_saturated_case("LSTM", hl.LSTM, dtype, tol, xmode, H, B, T)
    assert np.abs(pb.cs).max() > 45
    assert [r["lay"] for r in runs] == ([hl.TILE16, hl.TILE16P] if dtype == hl.BF16 else [hl.ROWMAJOR])
    want = par.cast(pb.hs[:, 1:4], "bf16" if dtype == hl.BF16 else "f32")
    decided = (pb.hs[:, 1:4] == 0.0) | (np.abs(pb.cs[:, 1:4]) > 12.0)
    assert decided.mean() > 0.5 and np.all(np.isin(want[decided], (0.0, 1.0, -1.0)))
    for run in runs:
        assert np.array_equal(run["hs"][:, 1:4][decided], want[decided]), "planted rows (layout %d)" % run["lay"]


@pytest.mark.parametrize("cellname,cell", CELLS)
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("H,B", par.SAT_BWD_SHAPES)
@pytest.mark.parametrize("ext", [True, False])
def test_rnn_backward_saturated(cellname, cell, dtype, tol, H, B, ext):
    """BPTT on the saturated problem's sequences (the oracle's, rounded to the storage type): the zero branch of every
    hard-sigmoid derivative.  (H = 384, 512: test_hidden_sizes_gpu.py)"""
    _rnn_backward_case(cellname, cell, dtype, tol, H, B, ext, T=par.SAT_T_BWD, saturated=True)


@pytest.mark.parametrize("cellname,cell", [c for c in CELLS if c[0] in ("GRU", "LSTM")])
@pytest.mark.parametrize("T,ext", [(3, True), (3, False), (7, True), (7, False), (64, True)])
def test_rnn_backward_saturated_resident_kernels_odd_and_long(cellname, cell, T, ext):
    """the pair-unrolled loop's tail (T = 3, 7 at B = 32) and the long window (T = 64, B = 16, an upstream gradient per step: with
    dh_last alone the gradient decays to 3e-16 over 64 saturated steps and the rounding model itself reaches 0.8 x the bound)"""
    _rnn_backward_case(cellname, cell, hl.BF16, dict(DTYPES)[hl.BF16], 256, 16 if T == 64 else 32, ext, T=T, saturated=True)


@pytest.mark.parametrize("T,ext", [(7, True), (7, False), (8, True), (8, False)])
def test_lstm_backward_two_waves_per_simd_experiment_saturated(T, ext, monkeypatch):
    """MVAE_LSTM_BWD_W8=1 (rnn_w8.hip: its own forms of the hard-sigmoid derivative) on the saturated problem"""
    monkeypatch.setenv("MVAE_LSTM_BWD_W8", "1")
    _rnn_backward_case("LSTM", hl.LSTM, hl.BF16, dict(DTYPES)[hl.BF16], 256, 32, ext, T=T, saturated=True)


@pytest.mark.parametrize("cellname,cell", [c for c in CELLS if c[0] in ("GRU", "LSTM")])
@pytest.mark.parametrize("dtype,H,B", [(hl.BF16, 256, 32), (hl.F32, 64, 5)])
def test_rnn_saturated_forward_hands_over_to_backward(cellname, cell, dtype, H, B):
    """The forward kernel's OWN hs / cs / acts buffers, untouched and in their layout, go to the backward kernel of the same layout
    (the BPTT tests above always re-layout the oracle's activations).  Compared with the oracle's BPTT on those same sequences,
    downloaded and un-tiled: both sides see the same clipped set, so this is as well conditioned as the other BPTT cases and the
    ordinary bounds apply - the bf16 gradient check of the saturated regime."""
    T, tol = par.SAT_T_FWD, dict(DTYPES)[dtype]
    GH, td = vo.GATES[cellname] * H, ops.torch_dtype(dtype)
    pb, runs = _rnn_forward_saturated_case(cellname, cell, dtype, tol, "dense", H, B, T, keep_device=True)
    ut = ops.pack_recurrent(dev(pb.U), cell, dtype, 1)
    assert len(runs) == ((3 if cellname == "GRU" else 2) if dtype == hl.BF16 else 1)
    for run in runs:
        lay, own = run["lay"], run["own"]
        hs, cs, acts = run["hs"], run["cs"], run["acts"]                      # what the kernel stored, row-major float64
        da_o, _, dh0_o, dc0_o = vo.rnn_backward(cellname, hs, cs, acts, pb.U, pb.dext, pb.dlast)
        da = torch.zeros((T, B, GH), dtype=td, device=DEV)
        rh = torch.zeros((T, B, H), dtype=td, device=DEV)
        dh0, dc0 = torch.zeros((B, H), device=DEV), torch.zeros((B, H), device=DEV)
        dext_d = dev(pb.dext, td)
        if run["res"]:
            dext_d = tile16(dext_d, T * B, H, True)
        ops.rnn_bwd(cell, dtype, T, B, H, ut, own["hs"], own["cs"], own["acts"], da, dhs_ext=dext_d, dh_last=dev(pb.dlast), rh=rh,
                    dh0=dh0, dc0=dc0, seq_layout=lay)
        torch.cuda.synchronize()
        what = " (hand-over, layout %d)" % lay
        close(host(da), da_o, tol, "da" + what)
        close(host(dh0), dh0_o, tol, "dh0" + what)
        par.assert_parity(host(da), da_o, dtype, par.gate_blocks(cellname), "da" + what)
        par.assert_parity(host(dh0), dh0_o, dtype, par.whole, "dh0" + what)
        if cellname == "LSTM":
            close(host(dc0), dc0_o, tol, "dc0" + what)
            par.assert_parity(host(dc0), dc0_o, dtype, par.whole, "dc0" + what)
        _saturated_backward_checks(cellname, H, acts, hs, host(da), host(rh), what)


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("M,N,K", [(50, 61, 33), (300, 192, 256), (128, 128, 1000), (256, 384, 1024), (512, 128, 192)])
def test_gemm(ta, tb, dtype, tol, M, N, K):
    rng = np.random.default_rng(M + N + K)
    td = ops.torch_dtype(dtype)
    A = rng.standard_normal((K, M) if ta else (M, K))
    B = rng.standard_normal((N, K) if tb else (K, N))
    bias = rng.standard_normal((N,))
    Ad, Bd = dev(A, td), dev(B, td)
    A, B = host(Ad), host(Bd)
    want = (A.T if ta else A) @ (B.T if tb else B)
    C = torch.zeros((M, N), device=DEV)
    ops.gemm(Ad, Bd, C, M, N, K, trans_a=ta, trans_b=tb, bias=dev(bias), act=hl.ACT_TANH, alpha=0.05)
    torch.cuda.synchronize()
    close(host(C), np.tanh(0.05 * want + bias), tol * 10, "tanh epilogue")
    kind = "bf16" if dtype == hl.BF16 else "f32"
    opA, opB, bias32 = (A.T if ta else A), (B.T if tb else B), host(dev(bias))
    par.assert_elementwise(host(C), np.tanh(np.float64(np.float32(0.05)) * want + bias32), "tanh epilogue")
    # split-K atomic accumulate into an f32 C that already holds data
    C2 = torch.ones((M, N), device=DEV)
    ops.gemm(Ad, Bd, C2, M, N, K, trans_a=ta, trans_b=tb, accumulate=True, split_k=3)
    torch.cuda.synchronize()
    close(host(C2), 1.0 + want, tol * np.sqrt(K), "split-k")
    par.assert_product(host(C2), 1.0 + want, par.product_unit(opA, opB, extra=[1.0]), kind, "split-k")
    if dtype == hl.BF16:
        C3 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        ops.gemm(Ad, Bd, C3, M, N, K, trans_a=ta, trans_b=tb)
        torch.cuda.synchronize()
        close(host(C3), want, 2e-2 * np.sqrt(K), "bf16 out")
        par.assert_product(host(C3), want, par.product_unit(opA, opB), kind, "bf16 out", out_bf16=True)
    # exact-arithmetic operands: small integers, alpha a power of two - every summation order gives the same bits
    Ai, Bi = par.integer_operands(rng, A.shape), par.integer_operands(rng, B.shape)
    bi, ci = par.integer_operands(rng, (N,)), par.integer_operands(rng, (M, N))
    wi = 0.5 * ((Ai.T if ta else Ai) @ (Bi.T if tb else Bi))
    C4, C5 = torch.zeros((M, N), device=DEV), dev(ci)
    ops.gemm(dev(Ai, td), dev(Bi, td), C4, M, N, K, trans_a=ta, trans_b=tb, bias=dev(bi), alpha=0.5)
    ops.gemm(dev(Ai, td), dev(Bi, td), C5, M, N, K, trans_a=ta, trans_b=tb, accumulate=True, split_k=3, alpha=0.5)
    torch.cuda.synchronize()
    par.assert_bits(host(C4), wi + bi, "f32", "integers, store with bias")
    par.assert_bits(host(C5), wi + ci, "f32", "integers, split-k")
    if dtype == hl.BF16:
        C6 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        ops.gemm(dev(Ai, td), dev(Bi, td), C6, M, N, K, trans_a=ta, trans_b=tb, alpha=0.5)
        torch.cuda.synchronize()
        assert np.mean(par.bf16_round(wi) != wi) > 0.1 or K < 64          # most elements need more than 8 bits: rounding shows
        par.assert_bits(host(C6), wi, "bf16", "integers, bf16 out")


@pytest.mark.parametrize("N", [1024, 768])
@pytest.mark.parametrize("chunk_tiles,reverse", [(8, False), (16, True), (24, False), (40, True)])
@pytest.mark.parametrize("epi", ["tile16_handover", "tile16_plain", "rowmajor"])
def test_weights_stationary_projection_equals_the_tiled_gemm(N, chunk_tiles, reverse, epi):
    """proj_ws_k (csrc/gemm.hip): x*W + b between two time-pipelined layers as a persistent launch of 8 * N/128 workgroups - weight
    fragments and accumulators in accumulator registers, A tiles double-buffered in LDS, requested with un-tracked loads and a
    hand-counted vmcnt.  Against the tiled kernel on the same operands: same MFMA order over k, so BIT-identical - with 1, 2, 3 and
    5 row blocks per workgroup and chunk (the prologue, the first block without stores in flight, the steady state, an odd tail),
    both chunk orders, all three epilogues; the chunk counters say every wave published every chunk."""
    rng = np.random.default_rng(N + chunk_tiles)
    H, nchunks = 256, 3
    rows = chunk_tiles * 128
    M = nchunks * rows
    A = dev(rng.standard_normal((M, H)), torch.bfloat16)
    W = dev(rng.standard_normal((N, H)) * 0.1, torch.bfloat16)
    bias = dev(rng.standard_normal((N,)))
    lay = hl.ROWMAJOR if epi == "rowmajor" else hl.TILE16
    want = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    ops.gemm(A, W, want, M, N, H, trans_b=True, bias=bias, c_layout=lay)
    blocks = 8 * (N // 128)
    ready = torch.full((nchunks,), 7, dtype=torch.int32, device=DEV)
    done = torch.zeros((nchunks,), dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    for rep in range(2):
        ops.gemm(A, W, got, M, N, H, trans_b=True, bias=bias, c_layout=lay, max_blocks=blocks, chunk_rows=rows, chunk_reverse=reverse,
                 chunk_wait=ready, chunk_wait_value=7, chunk_done=done if epi != "tile16_plain" else None, chunk_status=status)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert int(status.item()) == 0
    if epi != "tile16_plain":
        assert done.tolist() == [2 * 4 * blocks] * nchunks
    # close to the float64 product as well (the tiled kernel is itself checked against the oracle in test_gemm)
    ref = host(A) @ host(W).T + host(bias)
    out = host(tile16(got, M, N, False) if lay == hl.TILE16 else got)
    close(out, ref, 2e-2 * np.sqrt(H) * 0.1 + 1e-2, "projection")
    par.assert_product(out, ref, par.product_unit(host(A), host(W).T, extra=[host(bias)]), "bf16", "projection", out_bf16=True)


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16])
def test_gemm_tile16_output_and_relayout_roundtrip(dtype):
    rng = np.random.default_rng(1)
    M, N, K = 320, 192, 64
    td = ops.torch_dtype(dtype)
    A, B = dev(rng.standard_normal((M, K)), td), dev(rng.standard_normal((N, K)), td)
    bias = dev(rng.standard_normal((N,)))
    C_rm = torch.zeros((M, N), dtype=td, device=DEV)
    C_t = torch.zeros((M, N), dtype=td, device=DEV)
    ops.gemm(A, B, C_rm, M, N, K, trans_b=True, bias=bias)
    ops.gemm(A, B, C_t, M, N, K, trans_b=True, bias=bias, c_layout=hl.TILE16)
    back = tile16(C_t, M, N, False)
    torch.cuda.synchronize()
    assert torch.equal(back, C_rm)
    # the layout formula of include/midivae_hip.h, restated on the host
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    off = (((m // 16) * (N // 16) + n // 16) * 64 + ((n % 16) // 4) * 16 + m % 16) * 4 + n % 4
    want = np.empty(M * N)
    want[off.ravel()] = host(C_rm).ravel()
    assert np.array_equal(host(C_t).ravel(), want)
    assert torch.equal(tile16(back, M, N, True), C_t)
    if N % 32 == 0:      # TILE16P round trip (same values, tile pairs interleaved per lane)
        pr = tile16(back, M, N, True, paired=True)
        assert torch.equal(tile16(pr, M, N, False, paired=True), back)
        assert not torch.equal(pr, C_t)


def test_gemm_leading_dimensions_and_column_blocks():
    """GRU candidate-kernel gradient: dU[:, 2H:] = rh^T da[:, 2H:] written into a column block of dU."""
    rng = np.random.default_rng(5)
    R, H = 200, 64
    rh, da = rng.standard_normal((R, H)), rng.standard_normal((R, 3 * H))
    dU = torch.zeros((H, 3 * H), device=DEV)
    rh_d, da_d = dev(rh), dev(da)
    ops.gemm(rh_d, da_d[:, 2 * H:], dU[:, 2 * H:], H, H, R, trans_a=True, ldb=3 * H, ldc=3 * H, accumulate=True, split_k=2)
    torch.cuda.synchronize()
    want = np.zeros((H, 3 * H))
    want[:, 2 * H:] = rh.T @ da[:, 2 * H:]
    close(host(dU), want, 1e-4)
    rh, da = host(rh_d), host(da_d)                        # (the f32 values the kernel was handed)
    unit = np.zeros((H, 3 * H))                            # the untouched column blocks: exactly zero
    want[:, 2 * H:], unit[:, 2 * H:] = rh.T @ da[:, 2 * H:], par.product_unit(rh.T, da[:, 2 * H:])
    par.assert_product(host(dU), want, unit, "f32", "dU column block")


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 1e-5), (hl.BF16, 1e-2)])
def test_gemm_onehot_table_gradient(dtype, tol):
    rng = np.random.default_rng(9)
    R, D, N = 1024, 61, 256
    idx = rng.integers(0, D, (R,))
    da = rng.standard_normal((R, N))
    dad = dev(da, ops.torch_dtype(dtype))
    da = host(dad)
    want = np.zeros((D, N))
    np.add.at(want, idx, da)
    out = torch.zeros((D, N), device=DEV)
    ops.gemm(dev(idx, torch.uint8), dad, out, D, N, R, trans_a=True, a_kind=hl.ONEHOT, accumulate=True, split_k=4)
    torch.cuda.synchronize()
    close(host(out), want, tol * 10)
    A1 = np.zeros((R, D))
    A1[np.arange(R), idx] = 1.0
    par.assert_product(host(out), want, par.product_unit(A1.T, da), "bf16" if dtype == hl.BF16 else "f32", "table gradient")
    dai = par.integer_operands(rng, (R, N))                # integers: exact in every order
    outi = dev(par.integer_operands(np.random.default_rng(1), (D, N)))
    wanti = host(outi) + 0.5 * (A1.T @ dai)
    ops.gemm(dev(idx, torch.uint8), dev(dai, ops.torch_dtype(dtype)), outi, D, N, R, trans_a=True, a_kind=hl.ONEHOT, accumulate=True,
             split_k=4, alpha=0.5)
    torch.cuda.synchronize()
    par.assert_bits(host(outi), wanti, "f32", "table gradient of integers")


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("N", [61, 16, 3, 77, 128])
def test_softmax_head(dtype, tol, N):
    """N = 77 and 128 (no padding column): the 8-tile instantiation ('1hot-instrument' input, attach_instruments)"""
    _softmax_head_case(dtype, tol, N, H=64, R=333)


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("N,H,R,two_hot,b_stride", [(61, 128, 333, False, 0), (128, 320, 333, False, 0), (77, 512, 333, False, 0),
                                                    (61, 64, 65536 + 37, False, 0), (128, 128, 65536 + 37, True, 0),
                                                    (77, 256, 333, True, 0), (61, 64, 16 * 21, False, 16), (128, 64, 16 * 21, True, 16)])
def test_softmax_head_wide_long_two_hot_and_padding_rows(dtype, tol, N, H, R, two_hot, b_stride):
    """H up to 512 (the k loop), R = 65536 + 37 rows (the bounded grid walks the rows again: the LDS stage tile is reused - a
    T = 512 x B = 256 step has 131072), two-hot targets (target_idx2, 255 on some rows: attach_instruments) and padding rows
    (b_stride / b_valid: rows b >= 11 of every 16 carry targets equal to their argmax and must not count as hits)"""
    _softmax_head_case(dtype, tol, N, H=H, R=R, two_hot=two_hot, b_stride=b_stride, b_valid=11 if b_stride else 0)


def _softmax_head_case(dtype, tol, N, H, R, two_hot=False, b_stride=0, b_valid=0):
    rng, hs_h, W, bias, tgt, rw, tgt2 = par.softmax_head_problem(N, H, R, seed=N, two_hot=two_hot)
    td = ops.torch_dtype(dtype)
    hs = dev(hs_h, td)
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=td, device=DEV)
    ops.transpose_convert(dev(W), wt, n_pad=NP)
    Wq = host(wt)[:N].T
    counted = (np.arange(R) % b_stride < b_valid) if b_stride else np.ones(R, bool)
    if b_stride:                                  # padding rows whose target IS their argmax: hits if they were counted
        am_o = np.argmax(host(hs) @ Wq + bias, 1)
        tgt[~counted] = am_o[~counted]
        if two_hot:
            tgt2[~counted] = 255
    p, want_loss, want_dl, y = par.softmax_head_oracle(host(hs), Wq, bias, tgt, rw, 0.7, tgt2)
    probs = torch.zeros((R, N), device=DEV)
    am = torch.zeros((R,), dtype=torch.uint8, device=DEV)
    dl = torch.zeros((R, NP), dtype=td, device=DEV)
    sc = torch.zeros((2,), device=DEV)
    ops.head(0, dtype, R, H, N, hs, wt, dev(bias), target_idx=dev(tgt, torch.uint8), row_weight=dev(rw), grad_scale=0.7,
             probs=probs, argmax=am, dlogits=dl, scalars=sc, b_stride=b_stride, b_valid=b_valid,
             target_idx2=dev(tgt2, torch.uint8) if two_hot else None)
    torch.cuda.synchronize()
    close(host(probs), p, tol, "probs")
    close(host(dl)[:, :N], want_dl, tol, "dlogits")
    assert np.all(host(dl)[:, N:] == 0)
    close(host(sc)[0], want_loss, tol * 5, "loss")
    # argmax is bit-exact w.r.t. the probabilities the kernel itself returned (first maximum)
    assert np.array_equal(am.cpu().numpy(), np.argmax(probs.cpu().numpy(), axis=1).astype(np.uint8))
    # a hit: the first maximum is the target row's first hot column (index 0 for an all-zero row), on rows that count
    match = np.argmax(probs.cpu().numpy(), 1) == np.argmax(y, 1)
    assert host(sc)[1] == np.sum(match & counted)
    if b_stride:
        assert np.sum(match & ~counted) > R // 4
    par.assert_parity(host(probs), p, dtype, par.row_blocks, "probs", values=True)
    par.assert_parity(host(dl)[:, :N], want_dl, dtype, par.row_blocks, "dlogits")
    par.assert_rel(host(sc)[0], want_loss, par.LOSS_RTOL, "loss")


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16])
@pytest.mark.parametrize("want_probs", [True, False])
@pytest.mark.parametrize("N,H", [(61, 64), (61, 256), (16, 256)])
def test_softmax_head_argmax_planted_ties(dtype, want_probs, N, H):
    """The fused argmax follows the reference's decode rule (reference vae_definition.py:1048-1067: np.argmax = FIRST maximum;
    a row that sums to zero -> index 0) with ties PLANTED on the device: identical weight columns give bit-identical logits, so
    the maximum is shared by 2 / 3 / all columns - with and without the probability output (the decode-only path writes no
    probabilities), in both arithmetic modes, across both 16-column halves of a lane group and the 64-column boundary."""
    rng = np.random.default_rng(7 + N)
    R = 16 * 9 + 5
    td = ops.torch_dtype(dtype)
    hs_h = rng.standard_normal((R, H))
    W = rng.standard_normal((H, N)) * 0.3
    bias = rng.standard_normal((N,)) * 0.1
    # columns that tie: (a) two adjacent, (b) two across the 16-column boundary, (c) three incl. the last column
    groups = [(3, 4), (5, N - 1)] if N <= 16 else [(3, 4), (14, 17), (20, 40, N - 1)]
    Wt = W.copy()
    bt = bias.copy()
    big = 5.0 * np.abs(hs_h @ W + bias).max()
    for gi, grp in enumerate(groups):
        for c in grp:
            Wt[:, c] = W[:, grp[0]]
            bt[c] = bias[grp[0]]
    NP = ops.head_np(N)
    am_all = {}
    for gi, grp in enumerate(groups + [tuple(range(N))]):
        Wg, bg = Wt.copy(), bt.copy()
        if len(grp) == N:                          # every logit equal: all-zero weights and equal biases -> index 0
            Wg[:], bg[:] = 0.0, 0.25
        else:
            for c in grp:                          # lift the tied columns above every other column of every row
                bg[c] = bt[grp[0]] + big
        wt = torch.zeros((NP, H), dtype=td, device=DEV)
        ops.transpose_convert(dev(Wg), wt, n_pad=NP)
        hs = dev(hs_h, td)
        probs = torch.zeros((R, N), device=DEV) if want_probs else None
        am = torch.full((R,), 255, dtype=torch.uint8, device=DEV)
        sc = torch.zeros((2,), device=DEV)
        ops.head(0, dtype, R, H, N, hs, wt, dev(bg), probs=probs, argmax=am, scalars=sc)
        torch.cuda.synchronize()
        got = am.cpu().numpy()
        assert np.all(got == min(grp)), (grp, np.unique(got))
        if want_probs:
            p = probs.cpu().numpy()
            for c in grp[1:]:
                assert np.array_equal(p[:, c], p[:, grp[0]])          # the tie is exact on the device
            assert np.array_equal(got, np.argmax(p, axis=1).astype(np.uint8))


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
def test_sigmoid_head(dtype, tol):
    rng = np.random.default_rng(2)
    R, H = 150, 64
    td = ops.torch_dtype(dtype)
    hs = dev(rng.standard_normal((R, H)), td)
    W = rng.standard_normal((H, 1)) * 0.3
    bias = np.array([0.1])
    y = np.where(rng.random(R) < 0.5, 0.0, 0.5 + 0.5 * rng.random(R))
    y[:10] = 1.0
    rw = rng.random((R,)) / R
    wt = torch.zeros((16, H), dtype=td, device=DEV)
    ops.transpose_convert(dev(W), wt, n_pad=16)
    p = vo.sigmoid(host(hs) @ host(wt)[:1].T + bias)[:, 0]
    probs = torch.zeros((R,), device=DEV)
    dl = torch.zeros((R, 16), dtype=td, device=DEV)
    sc = torch.zeros((2,), device=DEV)
    ops.head(1, dtype, R, H, 1, hs, wt, dev(bias), target_val=dev(y), row_weight=dev(rw), grad_scale=1.0, probs=probs,
             dlogits=dl, scalars=sc)
    torch.cuda.synchronize()
    close(host(probs), p, tol)
    close(host(dl)[:, 0], rw * 2 * (p - y) * p * (1 - p), tol)
    close(host(sc)[0], np.sum(rw * (p - y) ** 2), tol * 5)
    assert host(sc)[1] == np.sum(np.round(probs.cpu().numpy()) == y.astype(np.float32))
    par.assert_parity(host(probs)[:, None], p[:, None], dtype, par.row_blocks, "probs", values=True)
    par.assert_parity(host(dl)[:, :1], (rw * 2 * (p - y) * p * (1 - p))[:, None], dtype, par.row_blocks, "dlogits")
    assert np.all(host(dl)[:, 1:] == 0)
    par.assert_rel(host(sc)[0], np.sum(rw * (p - y) ** 2), par.LOSS_RTOL, "loss")


def test_latent_block():
    rng = np.random.default_rng(4)
    B, Z, Cn = 37, 24, 4
    mu, lv = rng.standard_normal((B, Z)) * 0.5, rng.standard_normal((B, Z)) * 0.3
    eps = rng.standard_normal((B, Z)) * 0.01
    tgt = rng.integers(0, Cn, (B,))
    beta, pm, ps, sw = 0.1, 0.2, 1.5, 0.3
    z_o = mu + np.exp(lv / 2) * eps
    kl = np.mean(beta * (-0.5 * np.sum(1 + lv - 2 * np.log(ps) - ((mu - pm) ** 2 + np.exp(lv)) / ps ** 2, 1)))
    p = vo.softmax(z_o[:, :Cn])
    y = np.eye(Cn)[tgt]
    ce = np.mean(vo._cce(p, y))
    z = torch.zeros((B, Z), device=DEV)
    sp = torch.zeros((B, Cn), device=DEV)
    sc = torch.zeros((3,), device=DEV)
    ops.latent_fwd(B, Z, Cn, beta, pm, ps, 1.0 / B, dev(mu), dev(lv), dev(eps), z, sc, style_target=dev(tgt, torch.uint8),
                   style_probs=sp)
    torch.cuda.synchronize()
    close(host(z), z_o, 1e-5)
    close(host(sp), p, 1e-5)
    close(host(sc)[:2], [kl, ce], 1e-4)
    assert host(sc)[2] == np.sum(np.argmax(p, 1) == tgt)
    dz = rng.standard_normal((B, Z)) * 0.1
    dzt = dz.copy()
    dzt[:, :Cn] += sw * vo._cce_grad_logits(p, y) / B
    dmu_o = dzt + beta * (mu - pm) / ps ** 2 / B
    dlv_o = dzt * eps * 0.5 * np.exp(lv / 2) + beta * (-0.5) * (1 - np.exp(lv) / ps ** 2) / B
    dmu, dlv = torch.zeros((B, Z), device=DEV), torch.zeros((B, Z), device=DEV)
    ops.latent_bwd(B, Z, Cn, beta, pm, ps, sw, 1.0 / B, dev(mu), dev(lv), dev(eps), dev(dz), dmu, dlv, style_probs=sp,
                   style_target=dev(tgt, torch.uint8))
    torch.cuda.synchronize()
    close(host(dmu), dmu_o, 1e-5)
    close(host(dlv), dlv_o, 1e-5)
    # (at its own scale, with ldz / lddz, row weights, Z up to 256 and eps at epsilon_std = 1: tests/test_latent_ops_gpu.py)


@pytest.mark.parametrize("N,ldx", [(1024, 1024), (256, 256), (64, 64), (8, 16), (61, 64), (1, 16)])
def test_colsum_bf16_vector_path_plain_and_weighted(N, ldx):
    """16-byte loads, 8 columns per thread, LDS reduction + atomics; also with per-row weights (scalar-input dW)."""
    rng = np.random.default_rng(N)
    R = 4099
    X = dev(rng.standard_normal((R, ldx)), torch.bfloat16)
    wgt = rng.random(R)
    out = torch.full((N,), 0.5, device=DEV)              # accumulates on top of what is there
    ops.colsum(X, R, N, out, ldx=ldx)
    outw = torch.zeros((N,), device=DEV)
    ops.colsum_weighted(X, dev(wgt), R, N, outw, ldx=ldx)
    torch.cuda.synchronize()
    Xh = host(X)[:, :N]
    close(host(out), 0.5 + Xh.sum(0), 2e-4 * np.sqrt(R))
    close(host(outw), (Xh * wgt[:, None].astype(np.float32)).sum(0), 2e-4 * np.sqrt(R))
    w32 = wgt.astype(np.float32).astype(np.float64)
    par.assert_product(host(out), 0.5 + Xh.sum(0), par.sum_unit(Xh, extra=[0.5]), "sum", "colsum")
    par.assert_product(host(outw), w32 @ Xh, par.sum_unit(Xh, w32), "sum", "colsum_weighted")


def test_prepare_batch_matches_single_calls():
    """mvae_prepare_batch = the single weight-preparation calls, bit for bit, in one launch."""
    rng = np.random.default_rng(13)
    H, GH, K = 256, 1024, 61
    U, W, b, Wd = (dev(rng.standard_normal(sh)) for sh in ((H, GH), (K, GH), (GH,), (H, GH)))
    bf = torch.bfloat16
    want = [ops.pack_recurrent(U, hl.LSTM, hl.BF16, 0), ops.pack_recurrent(U, hl.LSTM, hl.BF16, 1),
            torch.zeros((K, GH), dtype=bf, device=DEV), torch.zeros((GH, H), dtype=bf, device=DEV),
            torch.zeros((H, GH), dtype=bf, device=DEV), torch.zeros((64, H), dtype=bf, device=DEV)]
    Wh = dev(rng.standard_normal((H, 61)))
    ops.make_table(W, b, want[2]); ops.transpose_convert(Wd, want[3]); ops.convert(Wd, want[4])
    ops.transpose_convert(Wh, want[5], n_pad=64)
    got = [torch.zeros_like(w) for w in want]
    pb = ops.PrepBatch()
    pb.pack_recurrent(U, got[0], 0); pb.pack_recurrent(U, got[1], 1); pb.make_table(W, b, got[2])
    pb.transpose_convert(Wd, got[3]); pb.convert(Wd, got[4]); pb.transpose_convert(Wh, got[5], n_pad=64)
    pb.run()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_outer_bias_tile16():
    rng = np.random.default_rng(12)
    R, N = 48, 1024
    xs, w, b = rng.random(R), rng.standard_normal(N), rng.standard_normal(N)
    out = torch.zeros((R, N), dtype=torch.bfloat16, device=DEV)
    ops.outer_bias_tile16(dev(xs), dev(w), dev(b), out, R, N)
    back = tile16(out, R, N, False)
    torch.cuda.synchronize()
    close(host(back), xs[:, None] * w[None] + b[None], 1e-2)
    xs, w, b = (host(dev(a)) for a in (xs, w, b))          # (the f32 values the kernel was handed)
    want = xs[:, None] * w[None] + b[None]                 # within half an ulp of bf16 plus two f32 units (the multiply, the add)
    assert np.all(np.abs(host(back) - want) <= par.half_ulp_bf16(want) + 2.0 * par.product_unit(xs[:, None], w[None], extra=[b[None]]))


def test_sum_over_time_split_and_accumulate():
    rng = np.random.default_rng(8)
    T, BN = 96, 16 * 1024
    X = dev(rng.standard_normal((T, BN)), torch.bfloat16)
    out = torch.full((BN,), 7.0, device=DEV)             # overwritten without accumulate
    ops.sum_over_time(X, T, BN, out)
    acc = torch.zeros((BN,), device=DEV)
    ops.sum_over_time(X[:40], 40, BN, acc)
    ops.sum_over_time(X[40:], T - 40, BN, acc, accumulate=True)
    torch.cuda.synchronize()
    want = host(X).sum(0)
    close(host(out), want, 1e-4)
    close(host(acc), want, 1e-4)
    par.assert_product(host(out), want, par.sum_unit(host(X)), "sum", "sum_over_time")
    par.assert_product(host(acc), want, par.sum_unit(host(X)), "sum", "sum_over_time in two parts")


def test_gemm_fast_narrow_n_accumulate():
    """Head kernel gradient: dW (H, 61) += hs^T (H, R) dl (R, 64 padded): one narrow N tile on the fast path."""
    rng = np.random.default_rng(9)
    R, H, N, NP = 4096, 256, 61, 64
    A = dev(rng.standard_normal((R, H)), torch.bfloat16)
    Bm = rng.standard_normal((R, NP))
    Bm[:, N:] = 0
    Bd = dev(Bm, torch.bfloat16)
    C = torch.ones((H, N), device=DEV)
    ops.gemm(A, Bd, C, H, N, R, trans_a=True, ldb=NP, accumulate=True, split_k=4)
    torch.cuda.synchronize()
    want = 1.0 + host(A).T.astype(np.float64) @ host(Bd)[:, :N].astype(np.float64)
    close(host(C), want, 2e-3 * np.sqrt(R) / 8)
    par.assert_product(host(C), want, par.product_unit(host(A).T, host(Bd)[:, :N], extra=[1.0]), "bf16", "narrow N")


def test_reductions_and_elementwise():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((1000, 192))
    out = torch.zeros((192,), device=DEV)
    ops.colsum(dev(X), 1000, 192, out)
    Xt = rng.standard_normal((11, 500))
    out2 = torch.zeros((500,), device=DEV)
    ops.sum_over_time(dev(Xt, torch.bfloat16), 11, 500, out2)
    y, dy = np.tanh(rng.standard_normal(777)), rng.standard_normal(777)
    dx = torch.zeros((777,), device=DEV)
    ops.tanh_bwd(dev(y), dev(dy), dx)
    W, b = rng.standard_normal((7, 48)), rng.standard_normal(48)
    tab = torch.zeros((7, 48), device=DEV)
    ops.make_table(dev(W), dev(b), tab)
    torch.cuda.synchronize()
    close(host(out), X.sum(0), 1e-4)
    close(host(out2), host(dev(Xt, torch.bfloat16)).sum(0), 1e-5)
    close(host(dx), dy * (1 - y * y), 1e-6)
    close(host(tab), W + b, 1e-6)
    X32 = host(dev(X))
    par.assert_product(host(out), X32.sum(0), par.sum_unit(X32), "sum", "colsum f32")
    Xt16 = host(dev(Xt, torch.bfloat16))
    par.assert_product(host(out2), Xt16.sum(0), par.sum_unit(Xt16), "sum", "sum_over_time bf16")
    y32, dy32 = host(dev(y)), host(dev(dy))
    par.assert_elementwise(host(dx), dy32 * (1 - y32 * y32), "tanh_bwd")
    par.assert_bits(host(tab), host(dev(W)) + host(dev(b)), "f32", "make_table: one f32 addition")


def test_adam_keep_count_and_prep_add_i32_job():
    """mvae_adam_step_dev(MVAE_ADAM_KEEP_COUNT | MVAE_ADAM_ZERO_GRAD) leaves the step count to a MVAE_PREP_ADD_I32 job of the
    next weight-preparation launch: three such steps (odd length: vector body + scalar tail; unaligned views: scalar path)
    equal the oracle's Keras Adam, the gradients come back zeroed and the count ends at 3."""
    rng = np.random.default_rng(18)
    for n, off in ((5003, 0), (4099, 1)):
        p0, m = rng.standard_normal(n), vo.OracleVAE(vo.make_cfg(lr=1e-3))
        p_o = {"w": p0.copy()}
        st = m.new_opt_state(p_o)
        buf = [torch.zeros(n + off, device=DEV) for _ in range(4)]
        p, g_d, mm, vv = [b[off:] for b in buf]
        p.copy_(dev(p0))
        t_done = torch.zeros(1, dtype=torch.int32, device=DEV)
        bump = ops.PrepBatch()
        bump.add_i32(t_done)
        for t in range(1, 4):
            g = rng.standard_normal(n)
            m.opt_step(p_o, {"w": g}, st)
            g_d.copy_(dev(g))
            ops.adam_step_dev(p, g_d, mm, vv, 1e-3, t_done, zero_grad=True, keep_count=True)
            assert int(t_done.item()) == t - 1
            bump.run()
            assert float(g_d.abs().max()) == 0.0
        close(host(p), p_o["w"], 1e-5)
        assert int(t_done.item()) == 3


def test_keras_adam_and_rmsprop_match_oracle():
    rng = np.random.default_rng(8)
    n = 5000
    p0, m = rng.standard_normal(n), vo.OracleVAE(vo.make_cfg(lr=1e-3))
    p_o = {"w": p0.copy()}
    st = m.new_opt_state(p_o)
    p = dev(p0)
    mm, vv = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t_done = torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in range(1, 4):
        g = rng.standard_normal(n)
        m.opt_step(p_o, {"w": g}, st)
        if t < 3:
            ops.adam_step(p, dev(g), mm, vv, 1e-3, t)
            t_done += 1
        else:
            ops.adam_step_dev(p, dev(g), mm, vv, 1e-3, t_done)
    torch.cuda.synchronize()
    close(host(p), p_o["w"], 1e-5)
    assert int(t_done.item()) == 3
    m2 = vo.OracleVAE(vo.make_cfg(lr=1e-3, optimizer="RMSprop"))
    p_o = {"w": p0.copy()}
    st = m2.new_opt_state(p_o)
    p, vv = dev(p0), torch.zeros(n, device=DEV)
    g = rng.standard_normal(n)
    m2.opt_step(p_o, {"w": g}, st)
    ops.rmsprop_step(p, dev(g), vv, 1e-3)
    torch.cuda.synchronize()
    close(host(p), p_o["w"], 1e-5)


def test_rejects_bad_arguments_without_launching():
    lib = hl.load()
    assert lib.mvae_rnn_fwd(None, None) == -1
    a = hl.RnnFwdArgs()
    assert lib.mvae_rnn_fwd(a, None) == -1
    with pytest.raises(RuntimeError):
        ops.rnn_fwd(hl.GRU, hl.F32, 4, 4, 96, torch.zeros(8, device=DEV), xp=torch.zeros(8, device=DEV))   # H=96 unsupported


@pytest.mark.gpu
def test_gemm_weight_gradient_with_fused_column_sums():
    """C += A^T B over a long K with split-K, plus colsum_b += column sums of B from the same pass (the bias gradient beside
    a recurrent-kernel gradient): against float64 on the bf16-rounded operands."""
    rng = np.random.default_rng(5)
    for (M, N, K, sk, ldb) in ((256, 1024, 4096, 16, None), (256, 512, 2048, 8, 768), (128, 256, 1024, 1, None)):
        ldb_ = N if ldb is None else ldb
        A = torch.tensor(rng.standard_normal((K, M)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
        Bf = torch.tensor(rng.standard_normal((K, ldb_)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
        C = torch.zeros((M, N), device=DEV)
        cs = torch.full((N,), 0.25, device=DEV)
        ops.gemm(A, Bf, C, M, N, K, trans_a=True, ldb=ldb_, accumulate=True, split_k=sk, colsum_b=cs)
        torch.cuda.synchronize()
        A64, B64 = A.double().cpu().numpy(), Bf.double().cpu().numpy()[:, :N]
        np.testing.assert_allclose(C.cpu().numpy(), A64.T @ B64, rtol=2e-3, atol=2e-3 * np.sqrt(K))
        np.testing.assert_allclose(cs.cpu().numpy(), 0.25 + B64.sum(0), rtol=2e-3, atol=2e-3 * np.sqrt(K))
        par.assert_product(host(C), A64.T @ B64, par.product_unit(A64.T, B64), "bf16", "C K=%d" % K)
        par.assert_product(host(cs), 0.25 + B64.sum(0), par.sum_unit(B64, extra=[0.25]), "sum", "colsum_b K=%d" % K)
        Ai, Bi = par.integer_operands(rng, (K, M)), par.integer_operands(rng, (K, ldb_))
        Ci, csi = dev(par.integer_operands(rng, (M, N))), dev(par.integer_operands(rng, (N,)))
        wC, wcs = host(Ci) + 0.25 * (Ai.T @ Bi[:, :N]), host(csi) + Bi[:, :N].sum(0)
        ops.gemm(dev(Ai, torch.bfloat16), dev(Bi, torch.bfloat16), Ci, M, N, K, trans_a=True, ldb=ldb_, accumulate=True, split_k=sk,
                 colsum_b=csi, alpha=0.25)
        torch.cuda.synchronize()
        par.assert_bits(host(Ci), wC, "f32", "C of integers K=%d" % K)
        par.assert_bits(host(csi), wcs, "f32", "colsum_b of integers K=%d" % K)


@pytest.mark.gpu
@pytest.mark.parametrize("onehot", [False, True])
@pytest.mark.parametrize("live", [False, True])
def test_gemm_k_streaming_follows_a_producer(onehot, live):
    """mvae_gemm k_wait: C += A^T B with the K rows arriving in chunks (last chunk first), P partitions per chunk, the accumulator
    kept in registers over all chunks.  ``live``: the GEMM is launched FIRST and waits; a second stream then writes B chunk by
    chunk (NaN before) and publishes each chunk's counter - a chunk read early would poison C.  Against float64 on the bf16-rounded
    operands, with the fused column sums (bias gradient) and the one-hot left operand (table gradient)."""
    rng = np.random.default_rng(11 + onehot)
    M, N, rows, nch, P = (61 if onehot else 256), 512, 1024, 8, 2
    K = rows * nch
    if onehot:
        idx = torch.tensor(rng.integers(0, M, (K,)), dtype=torch.uint8, device=DEV)
        A = idx
        A64 = np.zeros((K, M))
        A64[np.arange(K), idx.cpu().numpy()] = 1.0
    else:
        A = torch.tensor(rng.standard_normal((K, M)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
        A64 = A.double().cpu().numpy()
    Btrue = torch.tensor(rng.standard_normal((K, N)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
    Bf = torch.full_like(Btrue, float("nan")) if live else Btrue.clone()
    C = torch.full((M, N), 0.5, device=DEV)
    cs = torch.full((N,), 0.25, device=DEV)
    target = 7
    counters = torch.zeros(nch, dtype=torch.int32, device=DEV) if live else torch.full((nch,), target + 3, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s1, s2 = two_queues()
    with no_host_sync():
        with torch.cuda.stream(s1):
            ops.gemm(A, Bf, C, M, N, K, trans_a=True, accumulate=True, split_k=P, a_kind=hl.ONEHOT if onehot else None,
                     colsum_b=None if onehot else cs, k_wait=counters, k_wait_value=target, k_chunk_rows=rows, k_reverse=True,
                     chunk_status=status)
        if live:
            with torch.cuda.stream(s2):
                for c in range(nch - 1, -1, -1):
                    Bf[c * rows:(c + 1) * rows].copy_(Btrue[c * rows:(c + 1) * rows])
                    ops.stream_write_value32(counters[c:c + 1], target, stream=s2)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    B64 = Btrue.double().cpu().numpy()
    np.testing.assert_allclose(C.cpu().numpy(), 0.5 + A64.T @ B64, rtol=2e-3, atol=2e-3 * np.sqrt(K))
    if not onehot:
        np.testing.assert_allclose(cs.cpu().numpy(), 0.25 + B64.sum(0), rtol=2e-3, atol=2e-3 * np.sqrt(K))
        par.assert_product(host(cs), 0.25 + B64.sum(0), par.sum_unit(B64, extra=[0.25]), "sum", "colsum_b")
    par.assert_product(host(C), 0.5 + A64.T @ B64, par.product_unit(A64.T, B64, extra=[0.5]), "bf16", "C")
    if not live:            # small-integer operands, counters already at their value: bit-equal to float64
        Bi = par.integer_operands(rng, (K, N))
        Ai = A64 if onehot else par.integer_operands(rng, (K, M))
        Ci, csi = dev(par.integer_operands(rng, (M, N))), dev(par.integer_operands(rng, (N,)))
        wC, wcs = host(Ci) + 0.5 * (Ai.T @ Bi), host(csi) + Bi.sum(0)
        ops.gemm(A if onehot else dev(Ai, torch.bfloat16), dev(Bi, torch.bfloat16), Ci, M, N, K, trans_a=True, accumulate=True, split_k=P,
                 a_kind=hl.ONEHOT if onehot else None, colsum_b=None if onehot else csi, k_wait=counters, k_wait_value=target,
                 k_chunk_rows=rows, k_reverse=True, chunk_status=status, alpha=0.5)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        par.assert_bits(host(Ci), wC, "f32", "C of integers")
        if not onehot:
            par.assert_bits(host(csi), wcs, "f32", "colsum_b of integers")
    lib = hl.load()
    with pytest.raises(RuntimeError):
        ops.gemm(A, Bf, C, M, N, K, trans_a=True, accumulate=True, split_k=3, a_kind=hl.ONEHOT if onehot else None,
                 k_wait=counters, k_wait_value=target, k_chunk_rows=rows)
    with pytest.raises(RuntimeError):
        ops.gemm(A, Bf, C, M, N, K, trans_a=True, accumulate=True, split_k=P, max_blocks=8, a_kind=hl.ONEHOT if onehot else None,
                 k_wait=counters, k_wait_value=target, k_chunk_rows=rows)
    torch.cuda.synchronize()
    assert lib is not None


@pytest.mark.gpu
def test_gemm_k_streaming_multi_launch():
    """mvae_gemm_kstream_multi: three K-streaming problems of different kinds (dense + fused column sums, dense, one-hot) and
    different partition counts as ONE launch, released chunk by chunk by a second stream (B is NaN before its chunk is written)."""
    rng = np.random.default_rng(23)
    rows, nch, N = 1024, 6, 512
    K = rows * nch
    A1 = torch.tensor(rng.standard_normal((K, 256)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
    A2 = torch.tensor(rng.standard_normal((K, 128)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
    idx = torch.tensor(rng.integers(0, 61, (K,)), dtype=torch.uint8, device=DEV)
    Btrue = torch.tensor(rng.standard_normal((K, N)) * 0.5, dtype=torch.float32, device=DEV).to(torch.bfloat16)
    Bf = torch.full_like(Btrue, float("nan"))
    C1, C2, C3 = (torch.zeros((m, N), device=DEV) for m in (256, 128, 61))
    cs = torch.zeros((N,), device=DEV)
    counters = torch.zeros(nch, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(trans_a=True, accumulate=True, k_wait=counters, k_wait_value=3, k_chunk_rows=rows, k_reverse=True, chunk_status=status,
              build_only=True)
    problems = [ops.gemm(A1, Bf, C1, 256, N, K, split_k=4, colsum_b=cs, **kw), ops.gemm(A2, Bf, C2, 128, N, K, split_k=2, **kw),
                ops.gemm(idx, Bf, C3, 61, N, K, split_k=8, a_kind=hl.ONEHOT, **kw)]
    s1, s2 = two_queues()
    with no_host_sync():
        with torch.cuda.stream(s1):
            ops.gemm_kstream_multi(problems)
        with torch.cuda.stream(s2):
            for c in range(nch - 1, -1, -1):
                Bf[c * rows:(c + 1) * rows].copy_(Btrue[c * rows:(c + 1) * rows])
                ops.stream_write_value32(counters[c:c + 1], 3, stream=s2)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    B64 = Btrue.double().cpu().numpy()
    A3 = np.zeros((K, 61))
    A3[np.arange(K), idx.cpu().numpy()] = 1.0
    for C, A64 in ((C1, A1.double().cpu().numpy()), (C2, A2.double().cpu().numpy()), (C3, A3)):
        np.testing.assert_allclose(C.cpu().numpy(), A64.T @ B64, rtol=2e-3, atol=2e-3 * np.sqrt(K))
        par.assert_product(host(C), A64.T @ B64, par.product_unit(A64.T, B64), "bf16", "C (M = %d)" % A64.shape[1])
    np.testing.assert_allclose(cs.cpu().numpy(), B64.sum(0), rtol=2e-3, atol=2e-3 * np.sqrt(K))
    par.assert_product(host(cs), B64.sum(0), par.sum_unit(B64), "sum", "colsum_b")
    with pytest.raises(RuntimeError):       # more than 256 waiting workgroups in all
        ops.gemm_kstream_multi([ops.gemm(A1, Bf, C1, 256, N, K, split_k=16, **kw)] * 3)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gemm_multi_equals_the_single_launches():
    """mvae_gemm_multi: the weight-gradient GEMMs of a short-sequence step as ONE launch - dense A with and without fused column
    sums, a column block of a wider gradient (ldb / ldc), a narrow output (a head's Dense, N = 61 of 64 padded columns), a one-hot
    A (table gradient), different split-K counts (bases padded to multiples of 8) - against float64 on the bf16-rounded operands
    and against the same problems launched one by one; 20 problems = two launches; a problem the batched launch does not take
    is reported, not computed."""
    rng = np.random.default_rng(29)
    K, GH = 4096, 768
    bf = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).to(torch.bfloat16)
    A1, A2 = bf(rng.standard_normal((K, 256)) * 0.5), bf(rng.standard_normal((K, 256)) * 0.5)
    Bf = bf(rng.standard_normal((K, GH)) * 0.5)
    Bn = bf(rng.standard_normal((K, 64)) * 0.5)
    idx = torch.tensor(rng.integers(0, 61, (K,)), dtype=torch.uint8, device=DEV)
    def fresh():
        return dict(C1=torch.zeros((256, GH), device=DEV), C2=torch.zeros((256, GH), device=DEV), C3=torch.zeros((256, 61), device=DEV),
                    C4=torch.zeros((61, GH), device=DEV), cs=torch.zeros((GH,), device=DEV))
    def problems(o, build):
        kw = dict(trans_a=True, accumulate=True, build_only=build)
        return [ops.gemm(A1, Bf, o["C1"], 256, 512, K, ldb=GH, ldc=GH, split_k=16, colsum_b=o["cs"][:512], **kw),
                ops.gemm(A2, Bf[:, 512:], o["C1"][:, 512:], 256, 256, K, ldb=GH, ldc=GH, split_k=16, colsum_b=o["cs"][512:], **kw),
                ops.gemm(A2, Bf, o["C2"], 256, GH, K, split_k=4, **kw),
                ops.gemm(A1, Bn, o["C3"], 256, 61, K, ldb=64, split_k=16, **kw),
                ops.gemm(idx, Bf, o["C4"], 61, GH, K, a_kind=hl.ONEHOT, split_k=3, **kw)]
    multi, single = fresh(), fresh()
    assert ops.gemm_multi(problems(multi, True)) == 5
    problems(single, False)
    torch.cuda.synchronize()
    A164, A264, B64, Bn64 = (t.double().cpu().numpy() for t in (A1, A2, Bf, Bn))
    A3 = np.zeros((K, 61))
    A3[np.arange(K), idx.cpu().numpy()] = 1.0
    want = dict(C1=np.concatenate([A164.T @ B64[:, :512], A264.T @ B64[:, 512:]], 1), C2=A264.T @ B64, C3=A164.T @ Bn64[:, :61],
                C4=A3.T @ B64, cs=B64.sum(0))
    for k, w in want.items():
        np.testing.assert_allclose(multi[k].cpu().numpy(), w, rtol=2e-3, atol=2e-3 * np.sqrt(K), err_msg=k)
        np.testing.assert_allclose(multi[k].cpu().numpy(), single[k].cpu().numpy(), rtol=1e-4, atol=1e-3, err_msg=k)
    units = dict(C1=np.concatenate([par.product_unit(A164.T, B64[:, :512]), par.product_unit(A264.T, B64[:, 512:])], 1),
                 C2=par.product_unit(A264.T, B64), C3=par.product_unit(A164.T, Bn64[:, :61]), C4=par.product_unit(A3.T, B64),
                 cs=par.sum_unit(B64))
    for k, w in want.items():
        for name, o in (("multi", multi), ("single", single)):
            par.assert_product(host(o[k]), w, units[k], "sum" if k == "cs" else "bf16", "%s %s" % (name, k))
    # small-integer operands: every partition and arrival order gives the same bits as float64
    Ai1, Ai2, Bi, Bni = (par.integer_operands(rng, t.shape) for t in (A1, A2, Bf, Bn))
    keep = A1, A2, Bf, Bn
    A1, A2, Bf, Bn = bf(Ai1), bf(Ai2), bf(Bi), bf(Bni)     # (problems() reads these names)
    exact = fresh()
    assert ops.gemm_multi(problems(exact, True)) == 5
    torch.cuda.synchronize()
    A1, A2, Bf, Bn = keep
    wanti = dict(C1=np.concatenate([Ai1.T @ Bi[:, :512], Ai2.T @ Bi[:, 512:]], 1), C2=Ai2.T @ Bi, C3=Ai1.T @ Bni[:, :61], C4=A3.T @ Bi,
                 cs=Bi.sum(0))
    for k, w in wanti.items():
        par.assert_bits(host(exact[k]), w, "f32", "integers " + k)
    # more than 16 problems: two launches; every one accumulates into the same C
    C = torch.zeros((256, GH), device=DEV)
    assert ops.gemm_multi([ops.gemm(A2, Bf, C, 256, GH, K, trans_a=True, accumulate=True, split_k=2, build_only=True) for _ in range(20)]) == 20
    torch.cuda.synchronize()
    np.testing.assert_allclose(C.cpu().numpy(), 20 * want["C2"], rtol=2e-3, atol=20 * 2e-3 * np.sqrt(K))
    # not of the batched form (no accumulate / a transposed B): refused as a whole, nothing launched
    assert ops.gemm_multi([ops.gemm(A1, Bf, torch.zeros((256, GH), device=DEV), 256, GH, K, trans_a=True, build_only=True)]) == 0
    # ... in the SECOND part of a long list: the first 16 have been launched and are reported as such - the caller runs the rest
    # one by one and nothing is added twice (the engine used to re-launch all of them)
    C = torch.zeros((256, GH), device=DEV)
    mixed = [ops.gemm(A2, Bf, C, 256, GH, K, trans_a=True, accumulate=True, split_k=2, build_only=True) for _ in range(18)]
    mixed.append(ops.gemm(A2, Bf, C, 256, GH, K, trans_a=True, accumulate=True, split_k=2, max_blocks=7, build_only=True))
    done = ops.gemm_multi(mixed)
    assert done == 16
    for g in mixed[done:]:
        ops.gemm_args(g)
    torch.cuda.synchronize()
    np.testing.assert_allclose(C.cpu().numpy(), 19 * want["C2"], rtol=2e-3, atol=19 * 2e-3 * np.sqrt(K))
    arr = (hl.GemmArgs * 1)(ops.gemm(A2, Bf, C, 256, GH, K, trans_a=True, accumulate=True, build_only=True))
    assert hl.load().mvae_gemm_multi(arr, 17, torch.cuda.current_stream().cuda_stream) == hl.E_ARG
    assert hl.load().mvae_gemm_multi(None, 1, torch.cuda.current_stream().cuda_stream) == hl.E_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("kind,N", [(0, 61), (0, 16), (1, 1)])
def test_head_fused_input_gradient(dtype, tol, kind, N):
    """mvae_head with wc / dhs: the gradient w.r.t. the h sequence, d(logits) W^T, comes out of the head launch in TILE16 -
    against float64 on the d(logits) the same launch returned (and the zero / padded weight copies of mvae_prepare_batch)."""
    R, H = 320, 256 if dtype == hl.BF16 else 64
    hs_h, W, rw, bias, tgt = par.fused_head_problem(kind, N, H, R, seed=N + kind)
    td = ops.torch_dtype(dtype)
    hs = dev(hs_h, td)
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=td, device=DEV)
    wc = torch.full((H, NP), 7.0, dtype=td, device=DEV)
    sc_zero = torch.ones((3,), device=DEV)
    pb = ops.PrepBatch()
    pb.transpose_convert(dev(W), wt, n_pad=NP); pb.convert_pad(dev(W), wc, NP); pb.zero(sc_zero)
    pb.run()
    assert np.array_equal(host(wc)[:, :N], host(wt)[:N].T) and np.all(host(wc)[:, N:] == 0) and np.all(host(sc_zero) == 0)
    dl = torch.zeros((R, NP), dtype=td, device=DEV)
    dhs = torch.zeros((R, H), dtype=td, device=DEV)
    sc = torch.zeros((2,), device=DEV)
    if kind == 0:
        ops.head(0, dtype, R, H, N, hs, wt, dev(bias), target_idx=dev(tgt, torch.uint8),
                 row_weight=dev(rw), grad_scale=0.7, dlogits=dl, scalars=sc, wc=wc, dhs=dhs)
    else:
        ops.head(1, dtype, R, H, 1, hs, wt, dev(bias), target_val=dev(tgt), row_weight=dev(rw), grad_scale=1.0,
                 dlogits=dl, scalars=sc, wc=wc, dhs=dhs)
    torch.cuda.synchronize()
    want = host(dl) @ host(wc).T                                   # (R,NP) (NP,H)
    got = host(tile16(dhs, R, H, False))
    assert np.abs(want).max() > 0
    close(got, want, tol, "dhs")
    par.assert_parity(got, want, dtype, par.row_blocks, "dhs")
    # ... and the d(logits) it came from against the oracle's
    Wq = host(wt)[:N].T
    if kind == 0:
        want_dl = par.softmax_head_oracle(host(hs), Wq, bias, tgt, rw, 0.7)[2]
    else:
        p = vo.sigmoid(host(hs) @ Wq + bias)[:, 0]
        want_dl = (rw * 2 * (p - tgt) * p * (1 - p))[:, None]
    par.assert_parity(host(dl)[:, :N], want_dl, dtype, par.row_blocks, "dlogits")


@pytest.mark.parametrize("dtype", [hl.F32, hl.BF16])
def test_head_fused_input_gradient_refuses_h_above_256(dtype):
    """dhs needs H <= 256: at H = 320 mvae_head reports MVAE_E_UNSUPPORTED and launches nothing - dhs and dlogits keep what
    they held (the caller then runs the GEMM)"""
    rng = np.random.default_rng(41)
    R, H, N = 320, 320, 61
    td = ops.torch_dtype(dtype)
    NP = ops.head_np(N)
    wt = dev(rng.standard_normal((NP, H)) * 0.1, td)
    wc = dev(rng.standard_normal((H, NP)) * 0.1, td)
    dl = torch.full((R, NP), 3.0, dtype=td, device=DEV)
    dhs = torch.full((R, H), 5.0, dtype=td, device=DEV)
    with pytest.raises(RuntimeError, match="MVAE_E_UNSUPPORTED"):
        ops.head(0, dtype, R, H, N, dev(rng.standard_normal((R, H)), td), wt, dev(np.zeros(N)),
                 target_idx=dev(rng.integers(0, N, (R,)), torch.uint8), grad_scale=1.0, dlogits=dl, wc=wc, dhs=dhs)
    torch.cuda.synchronize()
    assert torch.all(dhs == 5.0) and torch.all(dl == 3.0)


# ---- heads at the clips of Keras' cross-entropy and at the ends of the sigmoid -----------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("N", [3, 61, 145])
@pytest.mark.parametrize("two_hot", [False, True])
@pytest.mark.parametrize("b_stride", [0, 8])
def test_softmax_head_clipped_rows(dtype, tol, N, two_hot, b_stride):
    """head_k's ``inside`` / ``inside2`` (par.softmax_head_clipped_problem): R = 40 rows - a fully clipped row in the last, partial
    16-row tile - at 1, 4 and 10 column tiles; b_stride = 8 / b_valid = 5 puts planted rows 6 and 7 at padding positions"""
    _softmax_head_clipped_case(dtype, tol, N, 64, 40, two_hot, b_stride, fused=False)


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("N", [3, 61, 145])
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("two_hot", [False, True])
def test_head_fused_input_gradient_clipped_rows(dtype, tol, N, H, two_hot):
    """... and through the fused dhs epilogue (R = 48: it takes whole 16-row tiles only): a fully clipped row has dhs exactly zero"""
    _softmax_head_clipped_case(dtype, tol, N, H, 48, two_hot, 0, fused=True)


def _softmax_head_clipped_case(dtype, tol, N, H, R, two_hot, b_stride, fused):
    td = ops.torch_dtype(dtype)
    rnd = lambda a: host(dev(a, td))
    rng, hs_h, W, bias, tgt, rw, tgt2, rows = par.softmax_head_clipped_problem(N, H, R, par.CLIPPED_HEAD_SEEDS[(N, H, R, two_hot)],
                                                                               two_hot, rnd)
    hs = dev(hs_h, td)
    NP = ops.head_np(N)
    wt = torch.zeros((NP, H), dtype=td, device=DEV)
    wc = torch.zeros((H, NP), dtype=td, device=DEV)
    pb = ops.PrepBatch()
    pb.transpose_convert(dev(W), wt, n_pad=NP); pb.convert_pad(dev(W), wc, NP)
    pb.run()
    Wq = host(wt)[:N].T
    assert np.array_equal(host(hs), hs_h) and np.array_equal(Wq, rnd(W))
    b_valid = 5 if b_stride else 0
    counted = (np.arange(R) % b_stride < b_valid) if b_stride else np.ones(R, bool)
    retargeted = par.retarget_padding_rows(host(hs), Wq, bias, tgt, tgt2, counted, [5] + list(rows.values()))    # hits, if they were counted
    low, high, inside = par.ce_bands(host(hs), Wq, bias, tgt, tgt2)         # (on exactly what the kernel is handed)
    clipped = par.fully_clipped_rows(low, high, inside)
    assert len(clipped) >= (6 if two_hot else 5) and R - 2 in clipped
    p, want_loss, want_dl, y = par.softmax_head_oracle(host(hs), Wq, bias, tgt, rw, 0.7, tgt2)
    probs = torch.zeros((R, N), device=DEV)
    am = torch.zeros((R,), dtype=torch.uint8, device=DEV)
    dl = torch.full((R, NP), 3.0, dtype=td, device=DEV)
    dhs = torch.full((R, H), 5.0, dtype=td, device=DEV) if fused else None
    sc = torch.zeros((2,), device=DEV)
    ops.head(0, dtype, R, H, N, hs, wt, dev(bias), target_idx=dev(tgt, torch.uint8), row_weight=dev(rw), grad_scale=0.7,
             probs=probs, argmax=am, dlogits=dl, scalars=sc, b_stride=b_stride, b_valid=b_valid,
             target_idx2=dev(tgt2, torch.uint8) if two_hot else None, wc=wc if fused else None, dhs=dhs)
    torch.cuda.synchronize()
    close(host(probs), p, tol, "probs")
    close(host(dl)[:, :N], want_dl, tol, "dlogits")
    assert np.all(host(dl)[:, N:] == 0)
    close(host(sc)[0], want_loss, tol * 5, "loss")
    assert np.array_equal(am.cpu().numpy(), np.argmax(probs.cpu().numpy(), axis=1).astype(np.uint8))
    match = np.argmax(probs.cpu().numpy(), 1) == np.argmax(y, 1)
    assert host(sc)[1] == np.sum(match & counted)
    assert match[rows["high"]] and all(am.cpu().numpy()[r] == N - 1 for k, r in rows.items() if "inside" not in k)
    if b_stride:            # rows 6 and 7 are planted AND padding: a one-hot "high" row 6 is its own argmax, and must not count
        assert len(retargeted) >= R // 4 and np.all(match[retargeted]) and not counted[6] and not counted[7]
        assert two_hot or (match[6] and not match[7])
    par.assert_parity(host(probs), p, dtype, par.row_blocks, "probs", values=True)
    par.assert_parity(host(dl)[:, :N], want_dl, dtype, par.row_blocks, "dlogits")
    # the loss: -log(1e-7) per low target.  (The high clip moves a row's loss by 1e-7 only: no loss check can see that branch; the
    # gradient check does - a row whose only target is above 1 - 1e-7 must come back exactly zero.)
    par.assert_rel(host(sc)[0], want_loss, par.LOSS_RTOL, "loss")
    assert np.all(want_dl[clipped] == 0) and np.all(host(dl)[clipped] == 0) and np.all(host(dl)[5] == 0)
    part = np.nonzero(inside.any(1) & (low | high).any(1))[0]                   # one target clipped, the other not
    assert len(part) == (3 if two_hot else 0) and np.all(np.abs(host(dl)[part]).max(1) > 0)
    if fused:
        want = host(dl) @ host(wc).T
        got = host(tile16(dhs, R, H, False))
        close(got, want, tol, "dhs")
        par.assert_parity(got, want, dtype, par.row_blocks, "dhs")
        assert np.all(got[clipped] == 0) and np.all(got[5] == 0) and np.all(np.abs(got[part]).max(1) > 0)


@pytest.mark.parametrize("dtype,tol", [(hl.F32, 2e-5), (hl.BF16, 2e-2)])
@pytest.mark.parametrize("fused", [False, True])
def test_sigmoid_head_at_its_extremes(dtype, tol, fused):
    """par.sigmoid_head_saturated_problem: logits of +-100 give pr exactly 1 / 0 and a gradient of exactly zero whatever the target
    (float64 has sigmoid(-100) = 3.7e-44 and a gradient of 1e-45: those four rows are asserted exactly, not by the bounds); a logit
    of exactly 0 gives pr = 1/2, which Keras' binary accuracy rounds half-to-even to 0: a hit only if the target is 0"""
    R, H = (48, 64) if fused else (40, 64)
    td = ops.torch_dtype(dtype)
    hs_h, W, bias, y, rw, rows = par.sigmoid_head_saturated_problem(R, H, 2, lambda a: host(dev(a, td)))
    hs = dev(hs_h, td)
    wt = torch.zeros((16, H), dtype=td, device=DEV)
    wc = torch.zeros((H, 16), dtype=td, device=DEV)
    pb = ops.PrepBatch()
    pb.transpose_convert(dev(W), wt, n_pad=16); pb.convert_pad(dev(W), wc, 16)
    pb.run()
    p = vo.sigmoid(host(hs) @ host(wt)[:1].T + bias)[:, 0]
    want_dl = rw * 2 * (p - y) * p * (1 - p)
    probs = torch.zeros((R,), device=DEV)
    am = torch.full((R,), 9, dtype=torch.uint8, device=DEV)
    dl = torch.zeros((R, 16), dtype=td, device=DEV)
    dhs = torch.full((R, H), 5.0, dtype=td, device=DEV) if fused else None
    sc = torch.zeros((2,), device=DEV)
    ops.head(1, dtype, R, H, 1, hs, wt, dev(bias), target_val=dev(y), row_weight=dev(rw), grad_scale=1.0, probs=probs, argmax=am,
             dlogits=dl, scalars=sc, wc=wc if fused else None, dhs=dhs)
    torch.cuda.synchronize()
    pr, g, a = host(probs), host(dl)[:, 0], am.cpu().numpy()
    ends = rows["plus"] + rows["minus"]
    rest = np.setdiff1d(np.arange(R), ends)
    assert np.all(pr[rows["plus"]] == 1.0) and np.all(pr[rows["minus"]] == 0.0) and np.all(g[ends] == 0.0)
    assert np.all(a[rows["plus"]] == 1) and np.all(a[rows["minus"]] == 0)
    assert np.all(pr[rows["half"]] == 0.5) and np.all(a[rows["half"]] == 0) and list(y[rows["half"]]) == [0.0, 1.0]
    close(pr, p, tol)
    close(g, want_dl, tol)
    close(host(sc)[0], np.sum(rw * (p - y) ** 2), tol * 5)
    hits = np.round(probs.cpu().numpy()) == y.astype(np.float32)
    assert host(sc)[1] == np.sum(hits) and list(hits[rows["half"]]) == [True, False] and list(hits[ends]) == [True, False, True, False]
    par.assert_parity(pr[rest, None], p[rest, None], dtype, par.row_blocks, "probs", values=True)
    par.assert_parity(g[rest, None], want_dl[rest, None], dtype, par.row_blocks, "dlogits")
    assert np.all(host(dl)[:, 1:] == 0)
    par.assert_rel(host(sc)[0], np.sum(rw * (p - y) ** 2), par.LOSS_RTOL, "loss")
    if fused:
        want = host(dl) @ host(wc).T
        got = host(tile16(dhs, R, H, False))
        close(got, want, tol, "dhs")
        par.assert_parity(got, want, dtype, par.row_blocks, "dhs")
        assert np.all(got[ends] == 0) and np.all(np.abs(got[rows["half"]]).max(1) > 0)


# ---- GEMM paths no other op test reaches (each against float64 on the rounded operands: tests/parity.py assert_product / assert_bits) ----
def _operand(rng, rows, cols, ld, dt, integer, scale=1.0):
    """a (rows, cols) operand inside rows of ``ld`` elements (the pad columns hold non-zero data too); device buffer, host values"""
    a = par.integer_operands(rng, (rows, ld)) if integer else rng.standard_normal((rows, ld)) * scale
    d = dev(a, dt)
    return d, host(d)[:, :cols]


def _gemm_case(M, N, K, a_dt, b_dt, c_dt=torch.float32, ta=False, tb=False, integer=False, alpha=1.0, bias=False, accumulate=False,
               split_k=1, lda=None, ldb=None, ldc=None, seed=0, what="", **kw):
    """one mvae_gemm call on random (unit bound) or small-integer operands (bit-equal); the columns of C beyond N must stay.
    Mixed operand kinds run on the bf16 matrix cores: the reference rounds the f32 operand to bf16 first.  Returns C."""
    rng = np.random.default_rng(seed + M + N + K)
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    lda, ldb, ldc = lda or ac, ldb or bc, ldc or N
    Ad, Ah = _operand(rng, ar, ac, lda, a_dt, integer)
    Bd, Bh = _operand(rng, br, bc, ldb, b_dt, integer)
    f32_path = a_dt == torch.float32 and b_dt == torch.float32
    if not f32_path:
        Ah, Bh = par.bf16_round(Ah), par.bf16_round(Bh)
    opA, opB = (Ah.T if ta else Ah), (Bh.T if tb else Bh)
    bias_h = host(dev(par.integer_operands(rng, (N,)) if integer else rng.standard_normal(N))) if bias else None
    c0 = host(dev(par.integer_operands(rng, (M, ldc)) if integer else rng.standard_normal((M, ldc)), c_dt))
    Cd = dev(c0, c_dt)
    ops.gemm(Ad, Bd, Cd, M, N, K, trans_a=ta, trans_b=tb, lda=lda, ldb=ldb, ldc=ldc, bias=dev(bias_h) if bias else None,
             accumulate=accumulate, split_k=split_k, alpha=alpha, **kw)
    torch.cuda.synchronize()
    al = np.float64(np.float32(alpha))
    extra = ([bias_h] if bias else []) + ([c0[:, :N]] if accumulate else [])
    want = al * (opA @ opB) + sum(extra)
    storage = "bf16" if c_dt == torch.bfloat16 else "f32"
    got = host(tile16(Cd, M, N, False)) if kw.get("c_layout") == hl.TILE16 else host(Cd)
    par.assert_bits(got[:, N:], c0[:, N:], storage, what + ": columns beyond N")
    if integer:
        par.assert_bits(got[:, :N], want, storage, what + " (integers)")
    else:
        par.assert_product(got[:, :N], want, par.product_unit(opA, opB, al, extra), "f32" if f32_path else "bf16", what,
                           out_bf16=storage == "bf16")
    return Cd


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("a_dt,b_dt", [(torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)])
def test_gemm_mixed_operand_kinds(ta, tb, a_dt, b_dt):
    """by_trans<bf16_t, MVAE_BF16, MVAE_F32> and its mirror: the f32 operand is rounded to bf16 on its way into LDS"""
    for M, N, K in ((50, 61, 33), (300, 192, 256)):
        _gemm_case(M, N, K, a_dt, b_dt, ta=ta, tb=tb, bias=True, what="mixed store")
        _gemm_case(M, N, K, a_dt, b_dt, ta=ta, tb=tb, accumulate=True, split_k=3, what="mixed split-k")
        _gemm_case(M, N, K, a_dt, b_dt, ta=ta, tb=tb, integer=True, alpha=0.5, bias=True, what="mixed store")
        _gemm_case(M, N, K, a_dt, b_dt, ta=ta, tb=tb, integer=True, alpha=0.25, accumulate=True, split_k=3, what="mixed split-k")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", [576, 2304])
def test_gemm_store_mode_splits_k_by_itself_only_into_a_packed_c(dt, K):
    """a store-mode f32 GEMM with K >= 512, at most 32 tiles and ldc == N zeroes C and runs split-K over atomics, the bias added by
    partition 0 alone; with ldc > N it must not (the memset would not fit the rows) - the same answer either way, and with
    integers the same bits"""
    M, N = 16, 64
    for integer, alpha in ((False, 1.0), (True, 0.5)):
        a = _gemm_case(M, N, K, dt, dt, bias=True, integer=integer, alpha=alpha, what="automatic split-K")
        b = _gemm_case(M, N, K, dt, dt, bias=True, integer=integer, alpha=alpha, ldc=N + 4, what="ldc > N")
        if integer:
            assert torch.equal(a, b[:, :N])


@pytest.mark.parametrize("accumulate", [False, True])
def test_gemm_persistent_tile_loop_under_max_blocks(accumulate):
    """max_blocks below the tile count: gemm_k (f32, 64 x 64 tiles) and gemm_fast_k (bf16, 128 x 128 tiles) walk the tiles in a
    loop - 1, 3 and tiles - 1 workgroups, store and split-K accumulate; sys_release on one case of each"""
    sk = 2 if accumulate else 1
    for (M, N, K, dt, tiles) in ((300, 192, 256, torch.float32, 15), (384, 256, 512, torch.bfloat16, 6)):
        for mb in (1, 3, tiles * sk - 1):
            for integer, alpha in ((False, 1.0), (True, 0.5)):
                _gemm_case(M, N, K, dt, dt, tb=True, bias=not accumulate, accumulate=accumulate, split_k=sk, integer=integer, alpha=alpha,
                           max_blocks=mb, sys_release=(mb == 3), what="max_blocks=%d" % mb)


@pytest.mark.parametrize("path", ["fast", "generic"])
def test_gemm_alpha_and_system_scope_release(path):
    """alpha = 0.37 with sys_release = 1 on the fast (bf16, 128-multiples) and on the generic kernel (f32 output and bf16 output)"""
    M, N, K = (256, 256, 512) if path == "fast" else (300, 192, 256)
    for c_dt in (torch.float32, torch.bfloat16):
        _gemm_case(M, N, K, torch.bfloat16, torch.bfloat16, c_dt=c_dt, tb=True, alpha=0.37, bias=True, sys_release=True, what=path)
    _gemm_case(M, N, K, torch.bfloat16, torch.bfloat16, ta=True, alpha=0.37, accumulate=True, split_k=4, sys_release=True, what=path)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gemm_tile16_output_with_bias_equals_the_row_major_run(dt):
    """the TILE16 epilogue (f32: generic kernel; bf16: fast kernel) with bias and alpha, bit for bit the row-major result"""
    M, N, K = 320 if dt == torch.float32 else 384, 192 if dt == torch.float32 else 256, 128
    for integer, alpha in ((False, 0.37), (True, 0.5)):
        rm = _gemm_case(M, N, K, dt, dt, c_dt=dt, tb=True, bias=True, alpha=alpha, integer=integer, what="row-major")
        tl = _gemm_case(M, N, K, dt, dt, c_dt=dt, tb=True, bias=True, alpha=alpha, integer=integer, c_layout=hl.TILE16, what="TILE16")
        assert torch.equal(tile16(tl, M, N, False), rm)


@pytest.mark.parametrize("N", [8, 24, 61, 77, 120])
def test_gemm_fast_narrow_n_pad_columns(N):
    """one narrow N tile on the fast path (accumulate, row-contiguous B): ldb = N rounded up to 8 and ldb = 128.  Columns N up
    to the next multiple of 8 belong to the last 16-byte load of a row and are zero, as the callers keep them; the columns beyond
    hold non-zero data here: whatever the kernel does with them must not reach C"""
    R, H = 1024, 256
    rng = np.random.default_rng(N)
    for ldb in ((N + 7) // 8 * 8, 128):
        for integer, alpha in ((False, 1.0), (True, 0.5)):
            Bm = par.integer_operands(rng, (R, ldb)) if integer else rng.standard_normal((R, ldb))
            Bm[:, N:(N + 7) // 8 * 8] = 0
            A = par.integer_operands(rng, (R, H)) if integer else rng.standard_normal((R, H))
            Ad, Bd = dev(A, torch.bfloat16), dev(Bm, torch.bfloat16)
            c0 = host(dev(par.integer_operands(rng, (H, N)) if integer else rng.standard_normal((H, N))))
            C = dev(c0)
            ops.gemm(Ad, Bd, C, H, N, R, trans_a=True, ldb=ldb, accumulate=True, split_k=4, alpha=alpha)
            torch.cuda.synchronize()
            want = c0 + alpha * (host(Ad).T @ host(Bd)[:, :N])
            if integer:
                par.assert_bits(host(C), want, "f32", "narrow N, ldb = %d" % ldb)
            else:
                par.assert_product(host(C), want, par.product_unit(host(Ad).T, host(Bd)[:, :N], extra=[c0]), "bf16", "narrow N, ldb = %d" % ldb)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gemm_generic_kernel_edges(dt):
    """gemm_k: a single element; K = 7 (under one 8-wide load); odd lda / ldb (the unaligned scalar-load branch of stage_tile), in
    both storage orders; M x N on both sides of the switch to 128 x 128 tiles (M * N >= 256 * 1024); more split-K partitions than
    k tiles (the empty ones are skipped)"""
    for integer, alpha in ((False, 1.0), (True, 0.5)):
        kw = dict(integer=integer, alpha=alpha)
        _gemm_case(1, 1, 1, dt, dt, bias=True, what="1 x 1 x 1", **kw)
        for ta, tb in ((False, False), (True, True)):
            _gemm_case(5, 9, 7, dt, dt, ta=ta, tb=tb, bias=True, what="K = 7", **kw)
            _gemm_case(50, 61, 33, dt, dt, ta=ta, tb=tb, lda=(50 if ta else 33) + 3, ldb=(33 if tb else 61) + 5, ldc=63, bias=True,
                       what="odd leading dimensions", **kw)
        _gemm_case(512, 512, 40, dt, dt, tb=True, bias=True, what="128-tiles", **kw)
        _gemm_case(504, 512, 40, dt, dt, tb=True, bias=True, what="64-tiles", **kw)
        _gemm_case(50, 61, 33, dt, dt, accumulate=True, split_k=8, what="empty split-K partitions", **kw)


@pytest.mark.parametrize("K", [1024, 768])
@pytest.mark.parametrize("lay", [hl.TILE16, hl.ROWMAJOR])
@pytest.mark.parametrize("reverse", [False, True])
def test_gemm_chunked_persistent_nt_equals_the_plain_gemm(K, lay, reverse):
    """the persistent chunked mode on gemm_fast_k (not the weights-stationary kernel: K != 256) - the dX GEMM between two pipelined
    layers, da (M, K) x W (256, K)^T: 1, 2 and 3 row blocks per workgroup and chunk on two workgroups, and the XCD-grouped order
    (8 workgroups, 8 row blocks per chunk).  The chunk counters are at their wait value beforehand; the result is BIT-equal to
    the same GEMM without chunking, every wave publishes every chunk, no wait times out."""
    N = 256
    rng = np.random.default_rng(K + lay)
    for blocks, rb, nchunks in ((2, 1, 3), (2, 2, 3), (2, 3, 3), (8, 8, 2)):
        rows = 128 * rb
        M = rows * nchunks
        A = dev(rng.standard_normal((M, K)) * 0.5, torch.bfloat16)
        W = dev(rng.standard_normal((N, K)) * 0.1, torch.bfloat16)
        want = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        ops.gemm(A, W, want, M, N, K, trans_b=True, c_layout=lay)
        ready = torch.full((nchunks,), 5, dtype=torch.int32, device=DEV)
        done = torch.zeros((nchunks,), dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.gemm(A, W, got, M, N, K, trans_b=True, c_layout=lay, max_blocks=blocks, chunk_rows=rows, chunk_reverse=reverse,
                 chunk_wait=ready, chunk_wait_value=5, chunk_done=done, chunk_status=status)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (blocks, rb)
        assert int(status.item()) == 0 and done.tolist() == [4 * blocks] * nchunks
        out = host(tile16(got, M, N, False) if lay == hl.TILE16 else got)
        par.assert_product(out, host(A) @ host(W).T, par.product_unit(host(A), host(W).T), "bf16", "dX", out_bf16=True)
        Ai, Wi = par.integer_operands(rng, (M, K)), par.integer_operands(rng, (N, K))            # integers: exact, then rounded once
        goti = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.gemm(dev(Ai, torch.bfloat16), dev(Wi, torch.bfloat16), goti, M, N, K, trans_b=True, c_layout=lay, alpha=0.5, max_blocks=blocks,
                 chunk_rows=rows, chunk_reverse=reverse, chunk_wait=ready, chunk_wait_value=5, chunk_status=status)
        torch.cuda.synchronize()
        par.assert_bits(host(tile16(goti, M, N, False) if lay == hl.TILE16 else goti), 0.5 * (Ai @ Wi.T), "bf16", "dX of integers")
        assert int(status.item()) == 0
