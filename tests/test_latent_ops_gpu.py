"""mvae_latent_fwd / _bwd and the fused Dense chain mvae_latent_chain_fwd / _bwd (csrc/latent.hip), called directly, every output
against the float64 numpy reference of tests/latent_ref.py (GPU box only).

The chain is f32 arithmetic in both engine modes; through the engine it is only ever compared at bf16 tolerances.  Here: the
covering set of shapes of latent_ref.CHAIN_CASES (H 64 .. 512, one to three column chunks of dense_rows, exactly 160 KB of LDS
in the backward kernel), padding rows, row weights, an all-zero target, rows whose target probability is clipped, the history
columns of zh, and the two refusals (return codes only).  Elementwise outputs are held to rtol |want| + floor RMS
(parity.ELEMWISE_F32, calibrated on the float32 evaluation of the same reference), the three scalars to a relative 1e-4 and
the hit count exactly; what must be zero or untouched is asserted exactly.
"""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from tests import latent_ref as lr
from tests import parity as par

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _scalars(got, want, n_valid, what):
    """[KL, style CE, hits] on top of what the accumulators held"""
    for i, name in ((0, "KL"), (1, "style CE")):
        if want[i] != 0:
            par.assert_rel(got[i], want[i], par.LOSS_RTOL, "%s %s" % (what, name))
        else:
            assert got[i] == 0, (what, name, got[i])
    assert got[2] == want[2], (what, "hits", got[2], want[2])


@pytest.mark.parametrize("ci", range(len(lr.CHAIN_CASES)))
def test_latent_chain_forward_and_backward(ci):
    case = lr.CHAIN_CASES[ci]
    p = lr.chain_problem(case, 100 + ci)
    want = lr.chain_reference(p)
    H, ncat, Z, zin, C, n_init, B, Bv = (p[k] for k in ("H", "ncat", "Z", "zin", "C", "n_init", "B", "B_valid"))
    if ci == 0:
        assert lr.bwd_lds_bytes(H, ncat, Z, zin, n_init) == 160 * 1024
    hy = lr.HYPER
    t = {k: dev(p[k]) for k in ("cat", "w_pack", "b_pack", "w_extra", "b_extra", "w_mu", "b_mu", "w_lv", "b_lv", "w_init", "b_init", "eps",
                                "style_row_weight") if p.get(k) is not None}
    if C:
        t["style_target"] = dev(p["style_target"], torch.uint8)
        t["style_probs"] = torch.full((B, C), 7.0, device=DEV)
    zh0 = np.concatenate([np.full((B, Z), 7.0), p["hist"]], 1)
    t["zh"] = dev(zh0)
    for k, cols in (("pack", H), ("extra", H), ("mu", Z), ("logvar", Z), ("S", n_init)):
        if k in want:
            t[k] = torch.full((B, cols), 7.0, device=DEV)
    sc0 = np.array([0.5, 0.25, 3.0])
    t["scalars"] = dev(sc0)
    assert ops.latent_chain_fwd(B, Bv, H, Z, C, ncat, zin, n_init, p["split"], hy["beta"], hy["prior_mean"], hy["prior_std"],
                                p["inv_batch"], **t)
    torch.cuda.synchronize()
    for k in ("pack", "extra", "mu", "logvar", "zh", "S"):
        if k in want:
            par.assert_elementwise(host(t[k]), want[k], "case %d %s" % (ci, k))
    par.assert_bits(host(t["zh"])[:, Z:], p["hist"], "f32", "history columns")
    got_sc = host(t["scalars"]) - sc0
    if C:
        # (rows >= B_valid are padding: the kernel leaves their probabilities unwritten)
        par.assert_elementwise(host(t["style_probs"])[:Bv], want["style_probs"][:Bv], "case %d style_probs" % ci)
        assert np.all(host(t["style_probs"])[Bv:] == 7.0)
    _scalars(got_sc, want["scalars"], Bv, "case %d" % ci)

    # backward, on the forward's own device outputs
    tr = lambda k: dev(np.ascontiguousarray(p[k].T))
    b = dict(wt_mu=tr("w_mu"), wt_lv=tr("w_lv"), wt_init=tr("w_init"), S=t["S"], mu=t["mu"], logvar=t["logvar"], eps=t["eps"],
             dS=dev(p["dS"]), dzh=torch.full((B, zin), 7.0, device=DEV), dmu=torch.full((B, Z), 7.0, device=DEV),
             dlogvar=torch.full((B, Z), 7.0, device=DEV), dcat=torch.full((B, ncat * H), 7.0, device=DEV))
    if "pack" in want:
        b.update(wt_pack=tr("w_pack"), pack=t["pack"], d_pack=torch.full((B, H), 7.0, device=DEV))
    if "extra" in want:
        b.update(wt_extra=tr("w_extra"), extra=t["extra"], d_extra=torch.full((B, H), 7.0, device=DEV))
    if C:
        b.update(style_probs=t["style_probs"], style_target=t["style_target"])
        if "style_row_weight" in t:
            b["style_row_weight"] = t["style_row_weight"]
    assert ops.latent_chain_bwd(B, Bv, H, Z, C, ncat, zin, n_init, p["split"], hy["beta"], hy["prior_mean"], hy["prior_std"],
                                hy["style_weight"], p["inv_batch"], **b)
    torch.cuda.synchronize()
    for k in ("dS", "dzh", "dmu", "dlogvar", "d_extra", "d_pack", "dcat"):
        if k in want:
            par.assert_elementwise(host(b[k]), want[k], "case %d %s" % (ci, k))
            if k not in ("dS", "dzh"):
                assert np.all(host(b[k])[Bv:] == 0), "%s of the padding rows" % k
    if C:                 # rows 1 (no target), 2 and 3 (clipped): d(mu) = dz + the KL term, no style term at all
        kl = hy["beta"] * (host(t["mu"]) - hy["prior_mean"]) / hy["prior_std"] ** 2 * p["inv_batch"]
        rows = [r for r in (1, 2, 3) if r < Bv]
        par.assert_elementwise(host(b["dmu"])[rows, :C], (host(b["dzh"])[:, :Z] + kl)[rows, :C], "dmu of the rows without a style gradient")


def test_latent_chain_refusals():
    """return codes only, nothing is launched: ncat = 3 without the pack Dense is MVAE_E_ARG; the 160 KB case with zin = 516 needs
    more LDS than a CU has: MVAE_E_UNSUPPORTED from _bwd"""
    B, H, Z = 4, 64, 4
    z = lambda *sh: torch.zeros(sh, device=DEV)
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.latent_chain_fwd(B, B, H, Z, 0, 3, Z, 4, 0, 0.1, 0.0, 1.0, 0.25, cat=z(B, 3 * H), w_mu=z(H, Z), b_mu=z(Z), w_lv=z(H, Z), b_lv=z(Z),
                             w_init=z(Z, 4), b_init=z(4), eps=z(B, Z), mu=z(B, Z), logvar=z(B, Z), zh=z(B, Z), scalars=z(3), S=z(B, 4))
    with pytest.raises(RuntimeError, match="MVAE_E_ARG"):
        ops.latent_chain_bwd(B, B, H, Z, 0, 3, Z, 4, 0, 0.1, 0.0, 1.0, 0.3, 0.25, wt_mu=z(Z, H), wt_lv=z(Z, H), wt_init=z(4, Z), S=z(B, 4),
                             mu=z(B, Z), logvar=z(B, Z), eps=z(B, Z), dS=z(B, 4), dzh=z(B, Z), dmu=z(B, Z), dlogvar=z(B, Z), dcat=z(B, 3 * H))
    B, H, Z, zin, n_init, ncat = 4, 512, 256, 516, 4608, 3
    assert lr.bwd_lds_bytes(H, ncat, Z, zin, n_init) > 160 * 1024 >= lr.bwd_lds_bytes(H, ncat, Z, 512, n_init)
    dmu = torch.full((B, Z), 7.0, device=DEV)
    ok = ops.latent_chain_bwd(B, B, H, Z, 0, ncat, zin, n_init, 1, 0.1, 0.0, 1.0, 0.3, 0.25, wt_pack=z(H, ncat * H), wt_extra=z(H, H),
                              wt_mu=z(Z, H // 2), wt_lv=z(Z, H // 2), wt_init=z(n_init, zin), S=z(B, n_init), pack=z(B, H), extra=z(B, H),
                              mu=z(B, Z), logvar=z(B, Z), eps=z(B, Z), dS=z(B, n_init), dzh=z(B, zin), dmu=dmu, dlogvar=z(B, Z),
                              d_extra=z(B, H), d_pack=z(B, H), dcat=z(B, ncat * H))
    torch.cuda.synchronize()
    assert ok is False and torch.all(dmu == 7.0)          # (ops maps MVAE_E_UNSUPPORTED to False)
    a = hl.LatentChainBwdArgs()
    assert hl.load().mvae_latent_chain_bwd(a, None) == hl.E_ARG


@pytest.mark.parametrize("B,Z,C,ldz,rw", [(37, 24, 4, 0, False), (37, 24, 4, 40, True), (6, 4, 2, 8, True), (13, 100, 4, 128, False),
                                          (21, 256, 4, 512, True), (9, 100, 0, 0, False)])
def test_latent_block_shapes_strides_weights_and_clipped_rows(B, Z, C, ldz, rw):
    """mvae_latent_fwd / _bwd: Z in {4, 24, 100, 256} (Z > 64: the one-wave-per-row loop takes further trips), ldz / lddz > Z with
    the columns beyond Z untouched, row weights given and NULL, a target of 255, rows whose target probability is clipped,
    B not a multiple of 4, eps at epsilon_std = 1"""
    rng = np.random.default_rng(B + Z)
    hy = lr.HYPER
    mu, lv, eps = (lr.f32(rng.standard_normal((B, Z)) * s) for s in (0.5, 0.3, 1.0))
    tgt = w = None
    if C:
        tgt = rng.integers(0, C, B)
        tgt[1] = 255
        eps[2, 0], tgt[2] = 60.0, 0
        eps[3, 1], tgt[3] = 60.0, 0
        w = lr.f32(rng.random(B) / B) if rw else None
    inv_b = float(np.float32(1.0 / B))
    z_o, p_o, sc_o = lr.latent_block_fwd(mu, lv, eps, C, tgt, w, B, hy["beta"], hy["prior_mean"], hy["prior_std"], inv_b)
    ld = ldz if ldz else Z
    zbuf = torch.full((B, ld), 7.0, device=DEV)
    sp = torch.zeros((B, C), device=DEV) if C else None
    sc0 = np.array([0.5, 0.25, 3.0])
    sc = dev(sc0)
    kw = dict(style_target=dev(tgt, torch.uint8), style_row_weight=dev(w) if rw else None, style_probs=sp) if C else {}
    ops.latent_fwd(B, Z, C, hy["beta"], hy["prior_mean"], hy["prior_std"], inv_b, dev(mu), dev(lv), dev(eps), zbuf[:, :Z] if ldz else zbuf,
                   sc, ldz=ldz, **kw)
    torch.cuda.synchronize()
    par.assert_elementwise(host(zbuf)[:, :Z], z_o, "z")
    assert np.all(host(zbuf)[:, Z:] == 7.0)
    if C:
        par.assert_elementwise(host(sp), p_o, "style_probs")
    _scalars(host(sc) - sc0, sc_o, B, "latent_fwd")
    dz = lr.f32(rng.standard_normal((B, ld)) * 0.1)
    dmu_o, dlv_o = lr.latent_block_bwd(dz[:, :Z], mu, lv, eps, p_o, C, tgt, w, B, hy["beta"], hy["prior_mean"], hy["prior_std"],
                                       hy["style_weight"], inv_b)
    dmu, dlv = torch.zeros((B, Z), device=DEV), torch.zeros((B, Z), device=DEV)
    kwb = dict(style_probs=sp, style_target=kw["style_target"], style_row_weight=kw["style_row_weight"]) if C else {}
    dz_d = dev(dz)
    ops.latent_bwd(B, Z, C, hy["beta"], hy["prior_mean"], hy["prior_std"], hy["style_weight"], inv_b, dev(mu), dev(lv), dev(eps),
                   dz_d[:, :Z] if ldz else dz_d, dmu, dlv, lddz=ldz, **kwb)
    torch.cuda.synchronize()
    par.assert_elementwise(host(dmu), dmu_o, "dmu")
    par.assert_elementwise(host(dlv), dlv_o, "dlogvar")
    if C:                 # rows 1 (no target), 2 and 3 (clipped): d(mu) carries no style term at all
        kl = hy["beta"] * (mu - hy["prior_mean"]) / hy["prior_std"] ** 2 * inv_b
        par.assert_elementwise(host(dmu)[1:4, :C], (dz[:, :Z] + kl)[1:4, :C], "dmu of the rows without a style gradient")
