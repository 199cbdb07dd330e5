"""The engine against the float64 oracle on problems in which ONE loss term carries the gradient (tests/loss_terms.py): a
contribution that is dropped, mis-scaled or added into the wrong slot is an error of tens of per cent there, where the default weights
hide it below the bound.  The gradient bounds are the existing ones (bf16: relative L2 per tensor < 6e-2, 8e-2 on the all-heads graph;
f32: 2e-6 + 2e-4 |g| + 2e-4 max|g|); the loss parts are compared relatively (loss_terms.RTOL_LOSS), without an absolute floor.
test_loss_terms_cpu.py holds a float64 model of a correct bf16 engine at a quarter of every bound used here.  Every figure goes
through parity._record (MVAE_PARITY_RECORD: profiles/r15_loss_term_margins.txt)."""
import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd.engine import Engine
from tests import loss_terms as lt
from tests import parity as par

pytestmark = pytest.mark.gpu

BF16_CASES = [(case, term) for case, _, terms, _ in lt.CASES for term in terms]


def _run(cell, term, shape, dtype, check_path):
    spec, params, batch, raw = lt.isolated(cell, term, **shape)
    m_o, g_o = lt.isolated_oracle(cell, term, **shape)
    B = shape["B"]
    eng = Engine(spec, max_batch=max(B, 16), dtype=dtype, seed=0)
    eng.set_params(params)
    lt.stage(eng, raw, B)
    eng.forward_backward(B)
    eng.check_pipeline()
    check_path(eng)
    return m_o, g_o, eng.metrics(B), eng.get_grads()


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
@pytest.mark.parametrize("case,term", BF16_CASES)
def test_isolated_term_on_the_resident_bf16_path(cell, case, term):
    _, shape, _, bound = [c for c in lt.CASES if c[0] == case][0]

    def resident(eng):
        assert eng.tile16 and eng.fused_latent
        assert eng._pipelined(eng.dec_notes), "time-pipelined stacks are off"
        if case != "bidirectional":          # (a bidirectional encoder of Le = 3: one Bidirectional layer + one on top, run layer by layer)
            assert eng._pipelined(eng.enc_notes), "time-pipelined stacks are off"
        # the fused latent chain ran both ways - except beside a signature head, which adds to d(z) inside the chain's span: that
        # graph takes the separate launches by design
        assert eng._chain_refused == (case == "optional")

    m_o, g_o, m, g = _run(cell, term, shape, "bf16", resident)
    what = "%s:%s:%s:" % (cell, case, term)
    bad = []
    for k in g_o:
        if not np.any(g_o[k]):
            n = float(np.linalg.norm(g[k]))
            par._record("loss_terms:bf16:zero", what + k, norm=n)
            if not n < 1e-6:
                bad.append((k, "expected zero", n))
        else:
            e = lt.rel_l2(g[k], g_o[k])
            par._record("loss_terms:bf16:gradient", what + k, rel_l2=e, ratio=e / bound)
            if not e < bound:
                bad.append((k, e))
    for k in m_o:
        if not k.endswith("_acc"):
            r = abs(m[k] - m_o[k]) / (lt.rtol_loss(k) * abs(m_o[k]))
            par._record("loss_terms:bf16:loss", what + k, rel=abs(m[k] - m_o[k]) / abs(m_o[k]), ratio=r)
            if not r <= 1.0:
                bad.append((k, m[k], m_o[k], "%.3g x the bound %.0e" % (r, lt.rtol_loss(k))))
    assert not bad, bad


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
@pytest.mark.parametrize("term", lt.DEFAULT_TERMS)
def test_isolated_term_on_the_generic_f32_path(cell, term):
    """H = 64 in f32 on a ragged batch (7 windows: padding rows): the isolated problems themselves against the oracle at the bound of
    test_forward_backward_matches_oracle, where nothing hides."""
    m_o, g_o, m, g = _run(cell, term, lt.GENERIC, "f32", lambda eng: None)
    what = "%s:generic:%s:" % (cell, term)
    bad = []
    for k in m_o:
        if not k.endswith("_acc"):
            r = abs(m[k] - m_o[k]) / (2e-4 * (1 + abs(m_o[k])))
            par._record("loss_terms:f32:loss", what + k, ratio=r)
            if not r <= 1.0:
                bad.append((k, m[k], m_o[k]))
    for k in g_o:
        err = np.abs(g[k] - g_o[k])
        r = float((err / (2e-6 + 2e-4 * np.abs(g_o[k]) + 2e-4 * np.abs(g_o[k]).max())).max())
        par._record("loss_terms:f32:gradient", what + k, ratio=r)
        if not r <= 1.0:
            bad.append((k, float(err.max()), r))
    assert not bad, bad
