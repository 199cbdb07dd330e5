"""Per-row outputs of the head and latent kernels (GPU box only): mvae_head_args.row_out, and kl_rows / style_rows of
mvae_latent_fwd_args and mvae_latent_chain_fwd_args - the fields appended under ABI 9 - called through ``ops``, every output in
tests/footprint.py's sentinel-filled, guarded arena.

Heads.  For every row r < R of a launch, row_out[r] = (the addend to scalars[0], the addend to scalars[1]).  Checked:
  1. the hit column is exactly ``argmax == first hot column`` on counted rows and 0 elsewhere, and sums to scalars[1];
  2. the float64 sum of the loss column is within parity.LOSS_RTOL of the oracle's loss (the bound on scalars[0] elsewhere);
  3. each loss addend against rw x CE (kind 1: rw x (p - y)^2) computed in float64 from the probabilities THE SAME LAUNCH returned:
     the difference is one f32 logarithm and a multiply (kind 1: three multiplies), so it is measured in units of
     rw x (2^-23 x CE + 2^-23) and held to four times the largest ratio the first run on an MI355X showed (MEASURED below;
     profiles/r14_per_window_margins.txt) - anything beyond a few units there is a bug, not noise;
  4. exactly 8 R bytes are written: the buffer is (R, 2) f32, all of it is written, its guards are intact;
  5. probs, argmax, dlogits and dhs have the bits of the same launch with row_out = NULL;
  6. the launch cut into two row ranges, the pointer advanced as for dlogits, gives the bits of one launch.

On point 6: the kernel numbers the rows of a launch from 0 (b = row % b_stride), so a cut must fall on a multiple of b_stride for
the padding rows to stay the same rows.  The cut at row 48 does with b_stride = 16.  With b_stride = 32 it does not: there the
loss column and every other output still have the bits of the one launch, the hit column is checked against the rows each launch
counts by its own numbering, and a second cut at row 64 (a multiple of 32) is held to the bits of the one launch in full.

Latent.  kl_rows / style_rows against the float64 reference of tests/latent_ref.py evaluated row by row, with the bound
test_latent_ops_gpu.py puts on the slots (parity.LOSS_RTOL relative, zeros and hit counts exact); their float64 sums against
the launch's own scalars within parity.sum_unit of the addends (x PRODUCT["sum"]); rows >= B_valid exactly 0; style_rows
untouched where no style head runs."""
import os

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from tests import footprint as fp
from tests import latent_ref as lr
from tests import parity as par
from tests.gpu_util import DEV, dev, host
from test_footprint_gpu import _head_inputs, carve_in, tensor, zeros

pytestmark = pytest.mark.gpu

F32, BF16 = hl.F32, hl.BF16
ROWS = [(3, 32, 19), (5, 16, 16)]            # (T, Bp, b_valid): R = 96 (half-padded 16-row tiles) and 80 (a partial last pass)
CUT = 48
U23 = 2.0 ** -23
# the largest |row_out[r, 0] - rw x score| / (rw x (2^-23 x score + 2^-23)) of the first run on an MI355X, per head kind
# (profiles/r14_per_window_margins.txt); the tests assert four times these
MEASURED = {0: 1.6236, 1: 0.3572}
_RECORD = os.environ.get("MVAE_PER_WINDOW_RECORD")       # a file: every check appends its ratio


def _record(what, ratio):
    print("per-window margin %s: %.4f units" % (what, ratio))
    if _RECORD:
        with open(_RECORD, "a") as f:
            f.write("%s\t%.4f\n" % (what, ratio))


def _launch(d, out, r0=0, r1=None, grad_scale=0.7):
    """rows [r0, r1) of problem ``d`` as one launch: every per-row pointer advanced to the launch's first row"""
    r1 = d.R if r1 is None else r1
    cut = lambda t: None if t is None else t[r0:r1]
    ops.head(d.kind, d.dtype, r1 - r0, d.H, d.N, d.hs[r0:r1], d.wt, d.bias, target_idx=cut(d.tgt), target_val=cut(d.y),
             row_weight=cut(d.rw), grad_scale=grad_scale if d.kind == 0 else 1.0, probs=cut(out.get("probs")),
             argmax=cut(out.get("argmax")), dlogits=cut(out.get("dlogits")), scalars=out.get("scalars"), b_stride=d.b_stride,
             b_valid=d.b_valid, wc=d.wc if out.get("dhs") is not None else None, dhs=cut(out.get("dhs")), target_idx2=cut(d.tgt2),
             row_out=cut(out.get("row_out")))


def _tight(d, grad, fused, row_out):
    R, N, NP, H = d.R, d.N, d.NP, d.H
    return dict(probs=zeros((R, N) if d.kind == 0 else (R,)), argmax=zeros((R,), torch.uint8),
                dlogits=zeros((R, NP), d.td) if grad else None, dhs=zeros((R, H), d.td) if fused else None, scalars=zeros((2,)),
                row_out=zeros((R, 2)) if row_out else None)


def _arena(d, grad, fused, scalars=True):
    """the launch with row_out, every input and output in one arena"""
    ar = fp.Arena(DEV)
    ins = {k: carve_in(ar, k, d[k], "zero" if k in ("tgt", "tgt2") else "sentinel") for k in ("hs", "wt", "bias", "tgt", "tgt2", "y", "rw", "wc")}
    R, N, NP, H = d.R, d.N, d.NP, d.H
    bufs = dict(probs=ar.carve("probs", (R, N) if d.kind == 0 else (R,), torch.float32), argmax=ar.carve("argmax", (R,), torch.uint8),
                dlogits=ar.carve("dlogits", (R, NP), d.td) if grad else None, dhs=ar.carve("dhs", (R, H), d.td) if fused else None,
                row_out=ar.carve("row_out", (R, 2), torch.float32),
                scalars=ar.carve("scalars", (4,), torch.float32, prefill=np.zeros(2), region=np.s_[:2]) if scalars else None)
    ar.commit()
    di = d.copy()
    di.update({k: tensor(b) for k, b in ins.items()})
    _launch(type(d)(di), {k: tensor(b) for k, b in bufs.items()})
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(bufs["row_out"])               # point 4: (R, 2) f32 = 8 R bytes, all written, nothing around them
    assert bufs["row_out"].nbytes == 8 * R
    if scalars:
        ar.assert_untouched(bufs["scalars"], np.s_[2:])
    return ar, bufs


def _same_outputs(d, bufs, ref, what, rows=np.s_[:]):
    """point 5 / 6: probs, argmax, dlogits (kind 1: column 0), dhs of ``bufs`` (arena) have the bits of ``ref`` (tight tensors)"""
    for k in ("probs", "argmax", "dlogits", "dhs"):
        if bufs.get(k) is None:
            continue
        g, w = bufs[k].bits() if isinstance(bufs[k], fp.Buf) else fp.bits_of(bufs[k]), fp.bits_of(ref[k])
        if k == "dlogits" and d.kind == 1:
            g, w = g[:, :1], w[:, :1]
        if k != "dhs":                  # (dhs is tiled: compared whole)
            g, w = g[rows], w[rows]
        fp.assert_same_bits(g, w, "%s %s" % (k, what))


def _scores(d, probs):
    """float64 (score per row, prediction matches the target per row - counted or not) from the probabilities the launch returned"""
    R = d.R
    if d.kind == 0:
        lo, hi = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))
        tg = host(d.tgt).astype(np.int64)
        tg2 = host(d.tgt2).astype(np.int64) if d.tgt2 is not None else np.full(R, 255)
        ce = np.zeros(R)
        for t in (tg, tg2):
            ok = t < d.N
            ce[ok] += -np.log(np.clip(probs[np.nonzero(ok)[0], t[ok]], lo, hi))
        return ce, np.argmax(probs, 1) == np.argmax(d.target, 1)
    rounded = np.round(probs.astype(np.float32)).astype(np.float64)          # (NumPy rounds half to even, as rintf)
    return (probs - d.y_h) ** 2, rounded == d.y_h


def _check_rows(d, bufs, what, scalars=True):
    """points 1 - 3 on the arena run"""
    row = bufs["row_out"].values()
    probs = bufs["probs"].values()
    score, match = _scores(d, probs)
    hit = match & d.counted
    assert np.array_equal(row[:, 1], hit.astype(np.float64)), "hit column " + what
    assert hit.sum() > 0 and (d.counted.all() or (match & ~d.counted).any())      # (hits to count, and hits that must not be)
    if scalars:
        sc = bufs["scalars"].values()[:2]
        assert float(np.sum(row[:, 1])) == sc[1], ("hit column against scalars[1] " + what, np.sum(row[:, 1]), sc[1])
        par.assert_rel(sc[0], d.loss, par.LOSS_RTOL, "scalars[0] " + what)
    par.assert_rel(float(np.sum(row[:, 0])), d.loss, par.LOSS_RTOL, "sum of the loss column " + what)
    rw = host(d.rw)
    ratio = float(np.max(np.abs(row[:, 0] - rw * score) / (rw * (U23 * score + U23))))
    _record("kind %d %s" % (d.kind, what), ratio)
    assert ratio <= 4 * MEASURED[d.kind], "loss column %s: %.3f units of rw (2^-23 score + 2^-23), measured %.3f" % (
        what, ratio, MEASURED[d.kind])
    return row


def _check_slices(d, bufs, grad, fused, what):
    """point 6"""
    R, Bp = d.R, d.b_stride
    row = bufs["row_out"].bits()
    cuts = [CUT] + ([64] if CUT % Bp else [])
    for cut in cuts:
        out = _tight(d, grad, fused, True)
        _launch(d, out, 0, cut)
        _launch(d, out, cut, R)
        torch.cuda.synchronize()
        w = "%s cut at row %d" % (what, cut)
        _same_outputs(d, bufs, out, w)
        got = fp.bits_of(out["row_out"])
        fp.assert_same_bits(got[:, 0], row[:, 0], "loss column " + w)
        if cut % Bp == 0:
            fp.assert_same_bits(got[:, 1], row[:, 1], "hit column " + w)
        else:           # (the second launch numbers its rows from 0: it counts the rows with (row - cut) % b_stride < b_valid)
            local = np.concatenate([np.arange(cut), np.arange(R - cut)])
            _, match = _scores(d, bufs["probs"].values())
            want = match & (local % Bp < d.b_valid)
            assert np.array_equal(host(out["row_out"])[:, 1], want.astype(np.float64)), "hit column " + w


def _softmax_case(N, H, dtype, T, Bp, bv, two_hot, fused):
    """par.softmax_head_problem as test_footprint_gpu.py stages it (padding rows retargeted to what they predict: hits if they
    were counted) - and every seventh counted row retargeted the same way, so that there are hits to count at every width"""
    d = _head_inputs(0, dtype, N, H, T * Bp, two_hot, Bp, bv, fused, None)
    Wq, bias, rw = host(d.wt)[:N].T, host(d.bias), host(d.rw)
    tgt = host(d.tgt).astype(np.int64)
    tgt2 = host(d.tgt2).astype(np.int64) if two_hot else None
    sel = np.nonzero(d.counted)[0][::7]
    sel = sel[sel != 5]                         # (row 5 keeps its all-zero target)
    tgt[sel] = np.argmax(host(d.hs) @ Wq + bias, 1)[sel]
    d.tgt = dev(tgt, torch.uint8)
    if two_hot:
        tgt2[sel] = 255
        d.tgt2 = dev(tgt2, torch.uint8)
    d.p, d.loss, d.dl, d.target = par.softmax_head_oracle(host(d.hs), Wq, bias, tgt, rw, 0.7, tgt2)
    return d


@pytest.mark.parametrize("grad", [False, True], ids=["fwd", "grad"])
@pytest.mark.parametrize("two_hot", [False, True], ids=["onehot", "twohot"])
@pytest.mark.parametrize("T,Bp,bv", ROWS)
@pytest.mark.parametrize("N,H,dtype", [(61, 64, F32), (16, 64, F32), (145, 256, BF16), (61, 256, BF16)])
def test_softmax_head_rows(N, H, dtype, T, Bp, bv, two_hot, grad):
    what = "(N=%d H=%d %s T=%d Bp=%d valid=%d%s)" % (N, H, "bf16" if dtype == BF16 else "f32", T, Bp, bv, " two-hot" if two_hot else "")
    for fused in ([False, True] if grad else [False]):          # (with want_grad also with the fused dhs: H <= 256 here)
        w = what + (" fused dhs" if fused else "")
        d = _softmax_case(N, H, dtype, T, Bp, bv, two_hot, fused)
        assert int(host(d.tgt)[5]) == 255                       # the problem's all-zero target row
        ref = _tight(d, grad, fused, False)
        _launch(d, ref)
        torch.cuda.synchronize()
        ar, bufs = _arena(d, grad, fused)
        _same_outputs(d, bufs, ref, w + " with and without row_out")
        row = _check_rows(d, bufs, w)
        assert row[5, 0] == 0.0                                 # (no target: no loss)
        assert np.all(row[~d.counted, 1] == 0.0)
        _check_slices(d, bufs, grad, fused, w)


def test_softmax_head_rows_without_scalars():
    """row_out is written whether or not the launch accumulates: scalars = NULL, no probs either in a second launch"""
    T, Bp, bv = ROWS[0]
    d = _softmax_case(61, 64, F32, T, Bp, bv, False, False)
    ar, bufs = _arena(d, False, False, scalars=False)
    row = _check_rows(d, bufs, "(scalars = NULL)", scalars=False)
    out = dict(row_out=zeros((d.R, 2)))
    _launch(d, out)
    torch.cuda.synchronize()
    fp.assert_same_bits(fp.bits_of(out["row_out"]), bufs["row_out"].bits(), "row_out alone: no scalars, probs, argmax or gradient")
    assert np.array_equal(host(out["row_out"]), row)


@pytest.mark.parametrize("grad", [False, True], ids=["fwd", "grad"])
@pytest.mark.parametrize("T,Bp,bv", ROWS)
@pytest.mark.parametrize("H,dtype", [(64, F32), (256, BF16)])
def test_sigmoid_head_rows(H, dtype, T, Bp, bv, grad):
    what = "(sigmoid H=%d %s T=%d Bp=%d valid=%d)" % (H, "bf16" if dtype == BF16 else "f32", T, Bp, bv)
    for fused in ([False, True] if grad else [False]):
        w = what + (" fused dhs" if fused else "")
        d = _head_inputs(1, dtype, 1, H, T * Bp, False, Bp, bv, fused, None)
        # every third target is what the oracle's output rounds to (a hit wherever the row counts), the rest stay in (0, 1)
        y = d.y_h.copy()
        y[::3] = np.round(d.p)[::3]
        d.y_h, d.y = y, dev(y)
        d.loss = np.sum(host(d.rw) * (d.p - y) ** 2)
        ref = _tight(d, grad, fused, False)
        _launch(d, ref)
        torch.cuda.synchronize()
        ar, bufs = _arena(d, grad, fused)
        _same_outputs(d, bufs, ref, w + " with and without row_out")
        row = _check_rows(d, bufs, w)
        assert np.all(row[~d.counted, 1] == 0.0)
        _check_slices(d, bufs, grad, fused, w)


# ---- latent ------------------------------------------------------------------------------------------------------------------
LB, LBV, LZ, LC = 32, 19, 16, 2


def _row_reference(mu, lv, eps, C, tgt, rw, inv_batch):
    """float64 [KL, style CE, hit] of every row evaluated alone (tests/latent_ref.py)"""
    hy = {k: lr.HYPER[k] for k in ("beta", "prior_mean", "prior_std")}
    out = np.zeros((mu.shape[0], 3))
    for b in range(mu.shape[0]):
        s = np.s_[b:b + 1]
        out[b] = lr.latent_block_fwd(mu[s], lv[s], eps[s], C, None if tgt is None else tgt[s], None if rw is None else rw[s], 1,
                                     inv_batch=inv_batch, **hy)[2]
    return out


def _check_latent_rows(kl, st, want, sc, n_valid, styled, what, rw=None):
    for b in range(n_valid):
        par.assert_rel(kl[b], want[b, 0], par.LOSS_RTOL, "%s kl_rows[%d]" % (what, b))
        if styled:
            if want[b, 1] != 0:
                # (a row clipped at the upper end: the f32 kernel clips at 1 - 2^-23, the nearest f32 to 1 - 1e-7, so its
                #  cross-entropy is off by up to 2^-23 absolute - nothing in a slot, everything in a row that holds nothing else)
                assert abs(st[b, 0] - want[b, 1]) <= par.LOSS_RTOL * abs(want[b, 1]) + rw[b] * U23, (what, b, st[b, 0], want[b, 1])
            else:
                assert st[b, 0] == 0, (what, b, st[b, 0])
            assert st[b, 1] == want[b, 2], (what, b, st[b, 1], want[b, 2])
    # the sums against the launch's own scalars: both are f32 sums of these addends, in some order
    cols = [(kl[:n_valid], sc[0])] + ([(st[:n_valid, 0], sc[1])] if styled else [])
    for x, s in cols:
        unit = par.sum_unit(x[:, None])[0]
        assert abs(float(np.sum(x)) - s) <= par.PRODUCT["sum"]["c_acc"] * unit + par.U_ACC * abs(s), (what, np.sum(x), s, unit)
    if styled:
        assert float(np.sum(st[:n_valid, 1])) == sc[2], (what, np.sum(st[:, 1]), sc[2])


@pytest.mark.parametrize("styled", [True, False], ids=["style", "nostyle"])
def test_latent_chain_rows(styled):
    case = (64, 1, 0, 0, 0, LZ, 1, LC if styled else 0, 64, LB, LBV, 1)
    p = lr.chain_problem(case, 77)
    want = lr.chain_reference(p)
    hy = lr.HYPER
    t = {k: dev(p[k]) for k in ("cat", "w_mu", "b_mu", "w_lv", "b_lv", "w_init", "b_init", "eps", "style_row_weight") if p.get(k) is not None}
    if styled:
        t["style_target"] = dev(p["style_target"], torch.uint8)
        t["style_probs"] = torch.zeros((LB, LC), device=DEV)
    t["zh"] = dev(np.concatenate([np.zeros((LB, LZ)), p["hist"]], 1))
    for k, cols in (("mu", LZ), ("logvar", LZ), ("S", 64)):
        t[k] = torch.zeros((LB, cols), device=DEV)
    ar = fp.Arena(DEV)
    kl = ar.carve("kl_rows", (LB,), torch.float32)
    st = ar.carve("style_rows", (LB, 2), torch.float32)
    sc = ar.carve("scalars", (4,), torch.float32, prefill=np.zeros(3), region=np.s_[:3])
    ar.commit()
    assert ops.latent_chain_fwd(LB, LBV, 64, LZ, LC if styled else 0, 1, LZ, 64, 0, hy["beta"], hy["prior_mean"], hy["prior_std"],
                                p["inv_batch"], scalars=sc.t, kl_rows=kl.t, style_rows=st.t, **t)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(kl)
    ar.assert_untouched(sc, np.s_[3:])
    rows = _row_reference(want["mu"], want["logvar"], p["eps"], LC if styled else 0,
                          p["style_target"].astype(np.int64) if styled else None, p.get("style_row_weight"), p["inv_batch"])
    if styled:
        ar.assert_written(st)
        assert np.all(st.bits()[LBV:] == 0), "style_rows of the padding rows"
    else:
        ar.assert_untouched(st)                 # (used only where the style head runs)
    assert np.all(kl.bits()[LBV:] == 0), "kl_rows of the padding rows"
    _check_latent_rows(kl.values(), st.values(), rows, sc.values()[:3], LBV, styled, "chain", rw=p.get("style_row_weight"))
    for i in (0, 1):
        if want["scalars"][i] != 0:
            par.assert_rel(sc.values()[i], want["scalars"][i], par.LOSS_RTOL, "chain scalars[%d]" % i)


@pytest.mark.parametrize("styled", [True, False], ids=["style", "nostyle"])
def test_latent_block_rows(styled):
    """mvae_latent_fwd has no padding rows of its own: the engine launches it over the B_valid real windows of a padded batch, so the
    (32)-row outputs keep their sentinels behind row 19"""
    rng = np.random.default_rng(5)
    hy = lr.HYPER
    mu, lv, eps = (lr.f32(rng.standard_normal((LB, LZ)) * s) for s in (0.5, 0.3, 1.0))
    tgt = w = None
    C = LC if styled else 0
    if styled:
        tgt = rng.integers(0, LC, LB)
        tgt[1] = 255
        eps[2, 0], tgt[2] = 60.0, 0
        eps[3, 1], tgt[3] = 60.0, 0
        w = lr.f32(rng.random(LB) / LBV)
    inv_b = float(np.float32(1.0 / LBV))
    ar = fp.Arena(DEV)
    kl = ar.carve("kl_rows", (LB,), torch.float32)
    st = ar.carve("style_rows", (LB, 2), torch.float32)
    sc = ar.carve("scalars", (4,), torch.float32, prefill=np.zeros(3), region=np.s_[:3])
    ar.commit()
    kw = dict(style_target=dev(tgt, torch.uint8), style_row_weight=dev(w), style_probs=torch.zeros((LB, LC), device=DEV)) if styled else {}
    ops.latent_fwd(LBV, LZ, C, hy["beta"], hy["prior_mean"], hy["prior_std"], inv_b, dev(mu), dev(lv), dev(eps),
                   torch.zeros((LB, LZ), device=DEV), sc.t, kl_rows=kl.t, style_rows=st.t, **kw)
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(kl, np.s_[:LBV])
    ar.assert_untouched(kl, np.s_[LBV:])
    if styled:
        ar.assert_written(st, np.s_[:LBV])
        ar.assert_untouched(st, np.s_[LBV:])
    else:
        ar.assert_untouched(st)
    rows = _row_reference(mu, lv, eps, C, tgt, w, inv_b)
    _check_latent_rows(kl.values(), st.values(), rows, sc.values()[:3], LBV, styled, "latent_fwd", rw=w)
    _, _, sc_o = lr.latent_block_fwd(mu, lv, eps, C, tgt, w, LBV, hy["beta"], hy["prior_mean"], hy["prior_std"], inv_b)
    for i in (0, 1):
        if sc_o[i] != 0:
            par.assert_rel(sc.values()[i], sc_o[i], par.LOSS_RTOL, "latent_fwd scalars[%d]" % i)
