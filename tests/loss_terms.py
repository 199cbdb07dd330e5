"""Engine-level problems in which ONE loss term carries the gradient (no GPU needed to import; no test lives here).

The whole-graph tests of the resident bf16 path (H = 256: resident recurrent kernels, time-pipelined stacks, fused latent chain,
phase launches, TILE16 layouts) compare every gradient tensor with the float64 oracle by relative L2 (< 6e-2; 8e-2 with the optional
heads) at the DEFAULT loss weights and epsilon_std = 0.01.  On the all-heads graph, HALF of what any
head but the KL and the signature head sends into the encoder changes the encoder's tensors by at most 1 % (style: 5 - 6 %), the WHOLE
reparameterisation path dz * eps * 0.5 * exp(logvar / 2) changes enc.zlogvar.{W,b} by 0.3 - 0.7 %: a contribution that is missing,
doubled or added into the wrong slot on its way through z stays inside the bound (test_loss_terms_cpu.py records which planted
defects do).

The gradient is linear in the loss weights, so the remedy is a choice of problems, not of tolerances: ``isolated(cell, term)`` is
the generator's problem (``problem``: what test_engine_gpu.py has always drawn, same seeds, same draws) with ``term`` at its
default weight and every other term scaled by OFF = 2^-10, a power of two, so the scaling itself is exact in every number format.
The term then dominates every tensor it reaches and the EXISTING bounds see half of it missing as an error of 0.24 or more.

TERMS says how a term's weight is set: a ModelSpec field, or - the notes loss has none - the ``w_notes`` row weights handed to
stage_targets and to the oracle's batch, scaled uniformly and never to zero (Keras' mean(score * w) / mean(w != 0) is 0 / 0 at
all-zero weights).  Three problems need the others further down than 2^-10, by what the oracle shows (test_loss_terms_cpu.py asserts
the outcome: half the term changes every tensor it reaches by 4 x the bound, enc.zlogvar.{W,b} excepted where the KL holds them):

  "reparam"   the notes problem with eps drawn at standard deviation 1 (the engine takes eps explicitly) and beta scaled by
              REPARAM_BETA = 2^-14, so that the eps path owns enc.zlogvar.{W,b}: at beta * 2^-10 the KL still holds 6 - 13 % of the
              two tensors, at 2^-14 0.4 - 0.8 % - below a quarter of the bound (1.5 %)
  "cinstr"    OFF_FOR = 2^-20: the classifier on the instrument OUTPUT sends its gradient through the softmax Jacobian of the head it
              reads and a 4-step decoder cell; at 2^-10 the other terms keep 50 - 70 % of the encoder tensors
  "cnotes"    OFF_FOR = 2^-40: the same through a 61-way softmax at near-uniform probabilities and two 32-step stacks - this
              term's share of the decoder's notes stack and of the encoder is about 3e-7 of the notes loss's at equal weights.  Its
              gradients are of the order of 1e-12: nothing here compares against an absolute threshold (``rel_l2``, exact zeros)

``planted(cell, term)``: the oracle's gradients with that term's weight halved = half of the term's contribution dropped; for
"reparam", enc.zlogvar.{W,b} of a backward pass whose d(logvar) omits the eps path.

``bf16_model``: a float64 model of a correct bf16 engine - the oracle with every parameter matrix rounded by parity.bf16_round and
every recurrence's projected inputs and stored hs rounded, each step reading back the h its predecessor stored (more rounding than
the engine does: its latent chain keeps f32 weights) - which test_loss_terms_cpu.py holds at a quarter of every bound the GPU
test uses (worst gradient tensor: 5.4e-3 on the default graph, 1.2e-2 with the optional heads, 5.1e-3 bidirectional).

Loss parts are compared RELATIVELY, |m - m_o| <= RTOL_LOSS[part] * |m_o|: the older tests' 3e-2 * (1 + |m_o|) is an absolute 3e-2,
33 - 75 % of a KL of 0.04 - 0.09.  RTOL_LOSS comes from ``bf16_model`` (the reference side, never the engine): its worst relative
error per loss part over every isolated problem of CASES and both cells, times 4, rounded up to one significant digit
(test_loss_terms_cpu.py prints the figures with -s and asserts the rule):

    part          model, worst   x 4, rounded up = RTOL_LOSS
    kl            1.08e-3        5e-3       (-0.5 sum(1 + lv - mu^2 - exp(lv)) cancels for small lv: 1 % in mu is 2 % in KL)
    notes_loss    2.02e-5        9e-5
    instr_loss    3.42e-5        2e-4
    vel_loss      7.00e-4        3e-3
    style_loss    3.90e-4        2e-3
    held_loss     3.78e-5        2e-4
    next_loss     1.01e-5        5e-5
    sig_loss      5.14e-4        3e-3
    cnotes_loss   4.97e-5        2e-4
    cinstr_loss   3.98e-5        2e-4

(The cross-entropies sit near ln(number of classes) at initialisation and hardly move with the logits, hence the small figures.)
No part needs more than the 3e-2 of the older tests, and none has an absolute floor.  ``loss``, the weighted total, is a sum of
the parts and is held to the largest of their bounds.  The margins measured on the MI355X against all of these:
profiles/r15_loss_term_margins.txt.
"""
import dataclasses
import functools

import numpy as np

from midi_vae_amd.layout import ModelSpec, init_params
from oracle import vae_oracle as vo
from oracle.vae_oracle import OracleVAE, make_cfg
from tests import parity as par

OFF = 2.0 ** -10
REPARAM_BETA = 2.0 ** -14                                   # "reparam": the factor of beta
OFF_FOR = {"cnotes": 2.0 ** -40, "cinstr": 2.0 ** -20}     # problems whose other terms go further down than OFF

# term -> how its weight is set: ("spec", ModelSpec field) or ("rows", key of the row weights in ``raw`` and in the oracle's batch)
TERMS = {"kl": ("spec", "beta"), "style": ("spec", "w_style"), "instr": ("spec", "w_instr"), "vel": ("spec", "w_vel"),
         "notes": ("rows", "w_notes"),
         "held": ("spec", "w_held"), "next": ("spec", "w_next"), "sig": ("spec", "w_sig"), "cnotes": ("spec", "w_cnotes"),
         "cinstr": ("spec", "w_cinstr")}
DEFAULT_TERMS = ("kl", "style", "instr", "vel", "notes", "reparam")
OPTIONAL_TERMS = ("held", "next", "sig", "cnotes", "cinstr")

# the shapes of the GPU test.  RESIDENT: the smallest at which Engine.tile16, fused_latent and _pipelined(...) all hold (and the
# default-weight problem of test_optional_heads_on_the_resident_bf16_path without its heads); OPTIONAL: that test's graph
RESIDENT = dict(B=16, seed=19, H=256, Z=32, T=32)
OPTIONAL = dict(RESIDENT, meta_held=True, meta_next=True, signature=True, SD=6, add_dim=4, comp_notes=True, comp_instr=True)
BIDIRECTIONAL = dict(RESIDENT, bidirectional=True, Le=3)
GENERIC = dict(B=7, seed=7, H=64, Z=32, T=12)
# (name, shape, terms, gradient bound) of the bf16 cases; GENERIC runs DEFAULT_TERMS at the f32 bound
CASES = (("default", RESIDENT, DEFAULT_TERMS, 6e-2), ("optional", OPTIONAL, OPTIONAL_TERMS, 8e-2),
         ("bidirectional", BIDIRECTIONAL, ("notes",), 6e-2))

RTOL_LOSS = dict(kl=5e-3, notes_loss=9e-5, instr_loss=2e-4, vel_loss=3e-3, style_loss=2e-3, held_loss=2e-4, next_loss=5e-5,
                 sig_loss=3e-3, cnotes_loss=2e-4, cinstr_loss=2e-4)


def rtol_loss(part):
    return max(RTOL_LOSS.values()) if part == "loss" else RTOL_LOSS[part]


def onehot(idx, n):
    out = np.zeros(idx.shape + (n,))
    np.put_along_axis(out, idx[..., None].astype(np.int64), 1, -1)
    return out


def problem(cell, B, seed=0, H=64, Z=32, T=12, V=4, C=2, **kw):
    """(spec, params, batch for the oracle, raw arrays for the engine) - the generator of test_engine_gpu.py"""
    spec = ModelSpec(cell=cell, H=H, Z=Z, T=T, V=V, C=C, lr=1e-3, **kw)
    rng = np.random.default_rng(seed)
    params = init_params(spec, seed)
    for k in params:                       # non-zero biases so every path carries signal
        if k.endswith(".b"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.1).astype(np.float32)
    x_idx = np.where(rng.random((B, T)) < 0.35, spec.Dout - 1, rng.integers(0, spec.Dout - 1, (B, T))).astype(np.uint8)
    i_idx = rng.integers(0, spec.ID, (B, V)).astype(np.uint8)
    vel = np.where((x_idx == spec.Dout - 1) | (rng.random((B, T)) < 0.5), 0.0, 0.5 + 0.5 * rng.random((B, T)))
    vel = vel.astype(np.float32)
    hist = (rng.standard_normal((B, Z)) * 0.1).astype(np.float32)
    eps = (rng.standard_normal((B, Z)) * spec.epsilon_std).astype(np.float32)
    c_idx = rng.integers(0, C, (B,)).astype(np.uint8)
    w_notes = np.where(x_idx == spec.Dout - 1, 0.5, 1.0)
    d_idx = (rng.random((B, T)) < 0.4).astype(np.uint8)                   # held-notes roll (reference import_midi.py:267-286)
    n_idx = rng.integers(0, spec.Dout, (B, T)).astype(np.uint8)          # the next window's notes
    sig = (rng.standard_normal((B, spec.SD)) * 0.5).astype(np.float32)        # signature vectors (reference data_class.py:96-221)
    add = rng.standard_normal((B, max(spec.add_dim, 1))).astype(np.float32)[:, :spec.add_dim]
    batch = dict(X=onehot(x_idx, spec.Din), I=onehot(i_idx, spec.ID), Vel=vel[..., None].astype(np.float64),
                 Hist=hist.astype(np.float64), Y=onehot(x_idx, spec.Dout), C=onehot(c_idx, C), w_notes=w_notes,
                 Held=onehot(d_idx, 2), Next=onehot(n_idx, spec.Dout), S=sig.astype(np.float64), Add=add.astype(np.float64))
    raw = dict(x_idx=x_idx, i_idx=i_idx, vel=vel, hist=hist, eps=eps, c_idx=c_idx, w_notes=w_notes, d_idx=d_idx, n_idx=n_idx,
               sig=sig, add=add)
    return spec, params, batch, raw


def stage(eng, raw, B):
    eng.stage_encoder_inputs(raw["x_idx"], raw["i_idx"], raw["vel"], raw["eps"], d_idx=raw["d_idx"])
    eng.stage_decoder_inputs(B, hist=raw["hist"], add=raw["add"])
    eng.stage_targets(B, raw["x_idx"], raw["c_idx"], w_notes=raw["w_notes"], n_idx=raw["n_idx"], sig=raw["sig"])


def weighted(cell, factors, unit_eps=False, **shape):
    """``problem(cell, **shape)`` with the default weight of every term t multiplied by factors[t] (default 1);
    ``unit_eps``: eps drawn anew at standard deviation 1 (from a generator of its own: the other draws stay)"""
    spec, params, batch, raw = problem(cell, **shape)
    fields = {}
    for term, f in factors.items():
        kind, name = TERMS[term]
        if kind == "spec":
            fields[name] = getattr(spec, name) * f
        else:
            assert f != 0
            raw[name] = raw[name] * f
            batch[name] = batch[name] * f
    spec = dataclasses.replace(spec, **fields)
    if unit_eps:
        raw["eps"] = np.random.default_rng(shape["seed"] + 7919).standard_normal(raw["eps"].shape).astype(np.float32)
    return spec, params, batch, raw


def isolated_factors(term):
    """the weight factors of the problem that isolates ``term``"""
    keep = "notes" if term == "reparam" else term
    f = {t: (1.0 if t == keep else OFF_FOR.get(term, OFF)) for t in TERMS}
    if term == "reparam":
        f["kl"] = REPARAM_BETA
    return f


def isolated(cell, term, **shape):
    return weighted(cell, isolated_factors(term), unit_eps=(term == "reparam"), **shape)


@functools.lru_cache(maxsize=None)
def _oracle_cached(cell, factors, unit_eps, shape, model, no_eps_path):
    spec, params, batch, raw = weighted(cell, dict(factors), unit_eps=unit_eps, **dict(shape))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    if model:
        p64 = {k: (par.bf16_round(v) if v.ndim == 2 else v) for k, v in p64.items()}
    orc = OracleVAE(make_cfg(**spec.oracle_cfg()))
    fwd = vo.rnn_forward

    def rounded_hs(cell_, xp, U, h0, c0=None, **kw):
        # step by step on the oracle's own arithmetic: every h is stored as bf16 and read back by the next step (c is not rounded)
        xp = par.bf16_round(xp)                       # (the projected inputs are a bf16 sequence too)
        hs, cs, acts, h, c = [par.bf16_round(h0)], [c0], [], par.bf16_round(h0), c0
        for t in range(xp.shape[0]):
            h1, c1, a1 = fwd(cell_, xp[t:t + 1], U, h, c, **kw)
            h, c = par.bf16_round(h1[1]), (c1[1] if c1 is not None else None)
            hs.append(h), cs.append(c), acts.append(a1[0])
        return np.stack(hs), (np.stack(cs) if c0 is not None else None), np.stack(acts)

    if model:
        vo.rnn_forward = rounded_hs
    try:
        m, cache = orc.forward(p64, batch, raw["eps"].astype(np.float64))
    finally:
        vo.rnn_forward = fwd
    if no_eps_path:
        cache = dict(cache, eps=np.zeros_like(cache["eps"]))           # (the backward pass reads eps in d(logvar) only)
    return dict(m), orc.backward(p64, cache)


def _freeze(d):
    return tuple(sorted(d.items()))


def oracle(cell, factors, unit_eps=False, model=False, no_eps_path=False, **shape):
    """(metrics, gradients) of the float64 oracle on ``weighted(cell, factors, unit_eps, **shape)`` - computed once per process and
    shared: treat the arrays as read-only.  ``model``: bf16_model instead."""
    return _oracle_cached(cell, _freeze(factors), bool(unit_eps), _freeze(shape), bool(model), bool(no_eps_path))


def isolated_oracle(cell, term, **shape):
    return oracle(cell, isolated_factors(term), unit_eps=(term == "reparam"), **shape)


def bf16_model(cell, term, **shape):
    return oracle(cell, isolated_factors(term), unit_eps=(term == "reparam"), model=True, **shape)


def planted(cell, term, factors=None, encoder_only=False, **shape):
    """the oracle's gradients with a defect in ``term``: its weight halved (= half of its contribution to every tensor dropped);
    "reparam": enc.zlogvar.{W,b} without the eps path of d(logvar).  ``factors``: the problem (default: the one isolating ``term``).
    ``encoder_only``: only the encoder's tensors (enc.*) carry the defect - half of what the term sends through z is lost on its way
    into the encoder, the head's own stack and the other decoder heads are right"""
    f = dict(isolated_factors(term) if factors is None else factors)
    unit_eps = factors is None and term == "reparam"
    good = oracle(cell, f, unit_eps=unit_eps, **shape)[1]
    if term == "reparam":
        bad = oracle(cell, f, unit_eps=unit_eps, no_eps_path=True, **shape)[1]
        return {k: (bad[k] if k in ("enc.zlogvar.W", "enc.zlogvar.b") else v) for k, v in good.items()}
    f[term] = 0.5 * f.get(term, 1.0)
    bad = oracle(cell, f, **shape)[1]
    return {k: (bad[k] if not encoder_only or k.startswith("enc.") else v) for k, v in good.items()}


def rel_l2(a, b):
    """||a - b|| / ||b|| (no absolute term: the gradients of the classifier problems are of the order of 1e-12); b != 0"""
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
