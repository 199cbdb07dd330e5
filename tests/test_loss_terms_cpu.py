"""tests/loss_terms.py on the float64 oracle alone (no GPU): what the default-weight engine tests of the resident bf16 path cannot
see, that the isolated problems of test_loss_terms_gpu.py do see it, and that a correct bf16 engine can pass them."""
import numpy as np
import pytest

from tests import loss_terms as lt

CELLS = ("LSTM", "GRU")
ZLOGVAR = ("enc.zlogvar.W", "enc.zlogvar.b")


def old_grads_pass(g, g_o, tol):
    """the gradient loop of test_optional_heads_on_the_resident_bf16_path (tol 8e-2) / _check_grads (6e-2)"""
    return all(lt.rel_l2(g[k], g_o[k]) < tol for k in g_o if np.linalg.norm(g_o[k]) > 1e-9)   # (the old tests' own threshold)


def old_losses_pass(m, m_o):
    return all(abs(m[k] - m_o[k]) <= 3e-2 * (1 + abs(m_o[k])) for k in m_o if not k.endswith("_acc"))


# Which planted defects the old checks let through on the DEFAULT-weight problem of test_optional_heads_on_the_resident_bf16_path
# (bi = False): (cell, term) -> (passes the gradient bound 6e-2 of _check_grads, passes the 8e-2 that test uses).  The defect sits where
# the terms share tensors - in the encoder, reached through z (``encoder_only``): a head's own stack belongs to its term alone and shows
# half of it missing as 0.5 at any weights.  The loss parts are not touched by a defect of the backward pass: they pass.
OLD_PASSES = {
    ("LSTM", "kl"): (False, False), ("LSTM", "style"): (True, True), ("LSTM", "instr"): (True, True), ("LSTM", "vel"): (True, True),
    ("LSTM", "notes"): (True, True), ("LSTM", "reparam"): (True, True), ("LSTM", "held"): (True, True), ("LSTM", "next"): (True, True),
    ("LSTM", "sig"): (False, False), ("LSTM", "cnotes"): (True, True), ("LSTM", "cinstr"): (True, True),
    ("GRU", "kl"): (False, False), ("GRU", "style"): (False, True), ("GRU", "instr"): (True, True), ("GRU", "vel"): (True, True),
    ("GRU", "notes"): (True, True), ("GRU", "reparam"): (True, True), ("GRU", "held"): (True, True), ("GRU", "next"): (True, True),
    ("GRU", "sig"): (False, False), ("GRU", "cnotes"): (True, True), ("GRU", "cinstr"): (True, True),
}


def test_the_defects_the_default_weight_checks_let_through():
    seen, worst = {}, {}
    for cell in CELLS:
        m_o, g_o = lt.oracle(cell, {}, **lt.OPTIONAL)
        assert old_losses_pass(m_o, m_o)
        for term in lt.DEFAULT_TERMS + lt.OPTIONAL_TERMS:
            g = lt.planted(cell, term, factors={}, encoder_only=True, **lt.OPTIONAL)
            changed = [lt.rel_l2(g[k], g_o[k]) for k in g_o if np.any(g[k] != g_o[k])]
            assert changed, (cell, term)                       # (the defect is one: some tensor differs)
            worst[cell, term] = max(changed)
            seen[cell, term] = (old_grads_pass(g, g_o, 6e-2), old_grads_pass(g, g_o, 8e-2))
    print("\nworst relative L2 change of a tensor under each planted defect, default weights:")
    for k, v in worst.items():
        print("  %-5s %-8s %.3e  passes at 6e-2: %s, at 8e-2: %s" % (k + (v,) + seen[k]))
    assert seen == OLD_PASSES, seen
    for cell in CELLS:                                         # the hole
        assert all(seen[cell, t][1] for t in ("style", "instr", "reparam"))


# Tensors of an isolated problem that another path dominates: (case, term) -> {tensor: the path}.  At most 4 per problem.
# A term other than the KL reaches d(logvar) only as dz * eps * 0.5 * exp(logvar / 2) with eps = 0.01 x N(0, 1); the KL writes to it
# directly, and 2^-10 of the KL is still of that size: halving the term changes these two tensors by 0.016 - 0.11.  The "reparam"
# problem is there for them.
_KL_HOLDS = {k: "the KL's own d(logvar), comparable at 2^-10 to dz * eps at epsilon_std = 0.01" for k in ZLOGVAR}
EXCEPTIONS = {(case, term): _KL_HOLDS for case, _, terms, _ in lt.CASES for term in terms if term not in ("kl", "reparam")}
MAX_EXCEPTIONS = 4


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", [c[0] for c in lt.CASES])
def test_isolated_problems_show_half_a_term_at_four_times_the_bound(cell, case):
    _, shape, terms, bound = [c for c in lt.CASES if c[0] == case][0]
    for term in terms:
        _, g_o = lt.isolated_oracle(cell, term, **shape)
        g = lt.planted(cell, term, **shape)
        reached = [k for k in g_o if np.any(g[k] != g_o[k])]
        assert set(ZLOGVAR) <= set(reached) and (term == "reparam" or len(reached) >= 4), (term, reached)
        exc = EXCEPTIONS.get((case, term), {})
        assert len(exc) <= MAX_EXCEPTIONS and set(exc) <= set(reached)
        change = {k: lt.rel_l2(g[k], g_o[k]) for k in reached}
        low = {k: v for k, v in change.items() if not v >= 4 * bound}
        print("\n%s %s %s: %d tensors reached, smallest change %.3f outside the exceptions %s" % (
            cell, case, term, len(reached), min(v for k, v in change.items() if k not in exc), {k: "%.3f" % change[k] for k in exc}))
        assert set(low) <= set(exc), (term, low)
        if term == "reparam":          # the KL's share of the two tensors the eps path owns: below a quarter of the bound
            f = lt.isolated_factors(term)
            half = lt.oracle(cell, dict(f, kl=0.5 * f["kl"]), unit_eps=True, **shape)[1]
            for k in ZLOGVAR:
                share = 2.0 * lt.rel_l2(half[k], g_o[k])
                assert share < bound / 4, (k, share)


def _round_up_1(x):
    """x rounded up to one significant digit"""
    e = 10.0 ** np.floor(np.log10(x))
    return float(np.ceil(x / e - 1e-9) * e)


def test_a_correct_bf16_engine_passes_with_a_factor_of_four():
    """the float64 model of the bf16 path against the oracle on every isolated problem: gradients within a quarter of the case's
    bound, loss parts within a quarter of RTOL_LOSS - and RTOL_LOSS is 4 x the model's worst, rounded up, no more."""
    worst_g, worst_m = {}, {}
    for case, shape, terms, bound in lt.CASES:
        for cell in CELLS:
            for term in terms:
                m_o, g_o = lt.isolated_oracle(cell, term, **shape)
                m, g = lt.bf16_model(cell, term, **shape)
                for k in g_o:
                    if not np.any(g_o[k]):
                        assert not np.any(g[k]), k
                    else:
                        e = lt.rel_l2(g[k], g_o[k])
                        worst_g[case] = max(worst_g.get(case, 0.0), e)
                        assert e <= bound / 4, (case, cell, term, k, e)
                for k in m_o:
                    if not k.endswith("_acc") and k != "loss":
                        worst_m[k] = max(worst_m.get(k, 0.0), abs(m[k] - m_o[k]) / abs(m_o[k]))
                assert abs(m["loss"] - m_o["loss"]) <= lt.rtol_loss("loss") / 4 * abs(m_o["loss"])
    print("\nbf16 model, worst relative L2 of a gradient tensor per case:", {k: "%.2e" % v for k, v in worst_g.items()})
    print("bf16 model, worst relative error per loss part -> 4 x, rounded up:")
    for k, v in worst_m.items():
        print("  %-12s %.2e -> %.0e   (RTOL_LOSS %.0e)" % (k, v, _round_up_1(4 * v), lt.RTOL_LOSS[k]))
    assert set(worst_m) == set(lt.RTOL_LOSS)
    for k, v in worst_m.items():
        assert lt.RTOL_LOSS[k] == pytest.approx(_round_up_1(4 * v), rel=1e-9), (k, v)
