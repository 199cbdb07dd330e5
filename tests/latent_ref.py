"""numpy reference of the latent block and of the fused Dense chain around it (mvae_latent_fwd / _bwd, mvae_latent_chain_fwd /
_bwd; formulas: reference vae_definition.py:29-37, 483-530, oracle/vae_oracle.py), and the problems the tests run it on.

One implementation in two precisions: float64 is the reference the GPU tests compare with (test_latent_ops_gpu.py), float32
(``ft=np.float32``: every operand and intermediate in float32) is the CPU model of a correct kernel that the elementwise bound
of tests/parity.py is calibrated on (test_parity_gemm_cpu.py).  No GPU needed to import.
"""
import numpy as np

CE_EPS = 1e-7

# the covering set of chain shapes: every value of every axis occurs - H in {64, 200, 256, 512}, ncat in {1, 3}, pack / extra
# present and absent, split 0 / 1, Z in {4, 24, 64, 256}, zin = Z and 2 Z, C in {0, 2, 4}, n_init in {4, 576, 2304, 4608} (the last
# two take 2 and 3 column chunks of dense_rows), row weights given and NULL - and every pair (pack) x (split), (B_valid < B) x
# (C > 0), (zin > Z) x (n_init > 2048).  The first case needs exactly 160 KB of LDS in the backward kernel.
#              H  ncat pack extra split  Z  zin/Z C  n_init  B  B_valid rw
CHAIN_CASES = [(512, 3, 1, 1, 1, 256, 2, 4, 4608, 8, 5, 1),
               (64, 1, 0, 0, 0, 4, 1, 0, 4, 4, 4, 0),
               (64, 1, 0, 1, 1, 4, 2, 2, 576, 8, 8, 1),
               (200, 3, 1, 0, 0, 24, 1, 4, 576, 12, 9, 0),
               (200, 1, 0, 0, 1, 24, 2, 0, 2304, 8, 6, 0),
               (256, 3, 1, 1, 0, 64, 1, 2, 2304, 16, 16, 1),
               (256, 1, 1, 1, 1, 64, 2, 4, 4, 8, 7, 1),
               (256, 3, 1, 1, 1, 24, 1, 4, 4608, 8, 8, 0),
               (512, 1, 0, 1, 0, 256, 1, 2, 576, 4, 3, 1),
               (64, 3, 1, 0, 1, 64, 2, 0, 2304, 8, 8, 0),
               (200, 1, 1, 0, 0, 4, 2, 2, 4608, 8, 8, 1),
               (512, 3, 1, 1, 0, 4, 1, 0, 2304, 4, 4, 0),
               (256, 1, 0, 0, 1, 256, 1, 4, 576, 20, 17, 0),
               (64, 1, 0, 0, 0, 24, 2, 4, 4, 8, 5, 1),
               (200, 3, 1, 1, 1, 64, 1, 2, 4, 8, 8, 1),
               (512, 1, 1, 1, 1, 24, 2, 2, 4608, 8, 6, 0),
               (256, 3, 1, 0, 0, 256, 2, 0, 576, 8, 8, 0),
               (64, 3, 1, 1, 0, 256, 1, 4, 2304, 12, 12, 1),
               (200, 1, 0, 1, 1, 256, 2, 4, 2304, 8, 4, 1),
               (512, 3, 1, 0, 1, 64, 2, 4, 576, 8, 8, 0)]

HYPER = dict(beta=0.1, prior_mean=0.2, prior_std=1.5, style_weight=0.3)


def bwd_lds_bytes(H, ncat, Z, zin, n_init):
    """what latent.hip's bwd_lds asks for (the launch is refused above 160 KB)"""
    return 16 * (n_init + zin + 2 * Z + 2 * H + ncat * H) + 32768


def f32(a):
    """float64 values that float32 holds exactly (what the device is handed)"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def chain_problem(case, seed):
    """the inputs of a chain case, as float64 arrays of float32-representable values"""
    H, ncat, pack, extra, split, Z, zmul, C, n_init, B, B_valid, rw = case
    rng = np.random.default_rng(seed)
    zin, h1w = Z * zmul, (H // 2 if split else H)
    p = dict(H=H, ncat=ncat, split=split, Z=Z, zin=zin, C=C, n_init=n_init, B=B, B_valid=B_valid, inv_batch=float(np.float32(1.0 / B_valid)))
    nrm = lambda *sh: rng.standard_normal(sh)
    p["cat"] = f32(nrm(B, ncat * H))
    if pack:
        p["w_pack"], p["b_pack"] = f32(nrm(ncat * H, H) / np.sqrt(ncat * H)), f32(nrm(H) * 0.1)
    if extra:
        p["w_extra"], p["b_extra"] = f32(nrm(H, H) / np.sqrt(H)), f32(nrm(H) * 0.1)
    p["w_mu"], p["b_mu"] = f32(nrm(h1w, Z) / np.sqrt(h1w)), f32(nrm(Z) * 0.1)
    p["w_lv"], p["b_lv"] = f32(nrm(H - h1w if split else H, Z) * 0.5 / np.sqrt(h1w)), f32(nrm(Z) * 0.1)
    p["w_init"], p["b_init"] = f32(nrm(zin, n_init) / np.sqrt(zin)), f32(nrm(n_init) * 0.1)
    p["eps"] = f32(nrm(B, Z))                             # epsilon_std = 1: the product's scale
    p["hist"] = f32(nrm(B, zin - Z))
    p["dS"] = f32(nrm(B, n_init) * 0.1)
    if C:
        tgt = rng.integers(0, C, B)
        tgt[1] = 255                                      # an all-zero target row
        p["eps"][2, 0], tgt[2] = 60.0, 0                  # p[target] > 1 - 1e-7: the clipped cross-entropy has no gradient
        p["eps"][3, 1], tgt[3] = 60.0, 0                  # p[target] < 1e-7: the same, and the loss is -log(1e-7)
        p["style_target"] = tgt.astype(np.uint8)
        if rw:
            p["style_row_weight"] = f32(rng.random(B) / B_valid)
    return p


def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def latent_block_fwd(mu, lv, eps, C, tgt, rw, n_valid, beta, prior_mean, prior_std, inv_batch, ft=np.float64):
    """z, style probabilities (or None), [KL, style CE, style hits] over rows < n_valid"""
    one, half = ft(1.0), ft(0.5)
    z = mu + np.exp(half * lv) * eps
    klr = np.sum(one + lv - ft(2.0) * np.log(ft(prior_std)) - ((mu - ft(prior_mean)) ** 2 + np.exp(lv)) / ft(prior_std) ** 2, 1)
    sc = [ft(inv_batch) * ft(beta) * ft(-0.5) * np.sum(klr[:n_valid], dtype=ft), ft(0.0), ft(0.0)]
    probs = None
    if tgt is not None and C > 0:
        probs = _softmax(z[:, :C])
        B = mu.shape[0]
        hot = tgt < C
        pt = np.where(hot, probs[np.arange(B), np.where(hot, tgt, 0)], one)
        ce = np.where(hot, -np.log(np.clip(pt, ft(CE_EPS), one - ft(CE_EPS))), ft(0.0))
        w = rw if rw is not None else np.full(B, inv_batch, ft)
        sc[1] = np.sum((w * ce)[:n_valid], dtype=ft)
        sc[2] = ft(np.sum((np.argmax(probs, 1) == np.where(hot, tgt, 0))[:n_valid]))
    return z, probs, np.array(sc, ft)


def latent_block_bwd(dz, mu, lv, eps, probs, C, tgt, rw, n_valid, beta, prior_mean, prior_std, style_weight, inv_batch, ft=np.float64):
    """dmu, dlogvar; rows >= n_valid zero"""
    B = mu.shape[0]
    dz = dz.copy()
    if probs is not None and tgt is not None:
        hot = tgt < C
        pt = probs[np.arange(B), np.where(hot, tgt, 0)]
        live = hot & (pt >= ft(CE_EPS)) & (pt <= ft(1.0) - ft(CE_EPS))
        y = np.zeros((B, C), ft)
        y[np.arange(B)[hot], tgt[hot]] = 1
        w = rw if rw is not None else np.full(B, inv_batch, ft)
        dz[:, :C] += np.where(live[:, None], ft(style_weight) * w[:, None] * (probs - y), ft(0.0))
    dmu = dz + ft(beta) * (mu - ft(prior_mean)) / ft(prior_std) ** 2 * ft(inv_batch)
    dlv = dz * eps * ft(0.5) * np.exp(ft(0.5) * lv) + ft(beta) * ft(-0.5) * (ft(1.0) - np.exp(lv) / ft(prior_std) ** 2) * ft(inv_batch)
    dmu[n_valid:], dlv[n_valid:] = 0, 0
    return dmu, dlv


def chain_reference(p, ft=np.float64, defect=None):
    """every output of mvae_latent_chain_fwd and, with p["dS"], of _bwd, as a dict.  ``defect`` plants what a broken kernel
    would do (test_parity_gemm_cpu.py): "kl_padding" counts the padding rows in the KL scalar, "split_swapped" reads z_mean /
    z_log_var from each other's half, "chunk2_bias" leaves the second chunk of 2048 columns of S at its bias"""
    g = lambda k: None if p.get(k) is None else np.asarray(p[k]).astype(ft)
    H, Z, zin, C, B, Bv, split = p["H"], p["Z"], p["zin"], p["C"], p["B"], p["B_valid"], p["split"]
    o = {}
    h = g("cat")
    if p.get("w_pack") is not None:
        o["pack"] = h = np.tanh(h @ g("w_pack") + g("b_pack"))
    if p.get("w_extra") is not None:
        o["extra"] = h = np.tanh(h @ g("w_extra") + g("b_extra"))
    h1w = H // 2 if split else H
    ha, hb = (h[:, :h1w], h[:, h1w:]) if split else (h, h)
    if defect == "split_swapped" and split:
        ha, hb = hb, ha
    o["mu"], o["logvar"] = ha @ g("w_mu") + g("b_mu"), hb @ g("w_lv") + g("b_lv")
    tgt = None if p.get("style_target") is None else p["style_target"].astype(np.int64)
    hy = {k: HYPER[k] for k in ("beta", "prior_mean", "prior_std")}
    z, probs, sc = latent_block_fwd(o["mu"], o["logvar"], g("eps"), C, tgt, g("style_row_weight"), B if defect == "kl_padding" else Bv,
                                    inv_batch=p["inv_batch"], ft=ft, **hy)
    if defect == "kl_padding":
        sc[1:] = latent_block_fwd(o["mu"], o["logvar"], g("eps"), C, tgt, g("style_row_weight"), Bv, inv_batch=p["inv_batch"], ft=ft, **hy)[2][1:]
    o["zh"] = np.concatenate([z, g("hist")], 1)
    o["style_probs"], o["scalars"] = probs, sc
    o["S"] = np.tanh(o["zh"] @ g("w_init") + g("b_init"))
    if defect == "chunk2_bias":
        o["S"][:, 2048:4096] = np.tanh(g("b_init")[2048:4096])
    if p.get("dS") is None:
        return o
    o["dS"] = g("dS") * (ft(1.0) - o["S"] ** 2)
    o["dzh"] = o["dS"] @ g("w_init").T
    o["dmu"], o["dlogvar"] = latent_block_bwd(o["dzh"][:, :Z], o["mu"], o["logvar"], g("eps"), probs, C, tgt, g("style_row_weight"), Bv,
                                              style_weight=HYPER["style_weight"], inv_batch=p["inv_batch"], ft=ft, **hy)
    if split:
        cur = np.concatenate([o["dmu"] @ g("w_mu").T, o["dlogvar"] @ g("w_lv").T], 1)
    else:
        cur = o["dmu"] @ g("w_mu").T + o["dlogvar"] @ g("w_lv").T
    if "extra" in o:
        o["d_extra"] = cur * (ft(1.0) - o["extra"] ** 2)
        cur = o["d_extra"] @ g("w_extra").T
    if "pack" in o:
        o["d_pack"] = cur * (ft(1.0) - o["pack"] ** 2)
        cur = o["d_pack"] @ g("w_pack").T
    o["dcat"] = cur
    return o


ELEMENTWISE_OUTPUTS = ("pack", "extra", "mu", "logvar", "zh", "style_probs", "S", "dS", "dzh", "dmu", "dlogvar", "d_extra", "d_pack", "dcat")
