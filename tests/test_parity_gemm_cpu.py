"""The bounds of tests/parity.py for matrix products, reductions and elementwise f32 kernels, checked on the CPU (no GPU).

Specificity: the CPU models of a CORRECT kernel - float32 accumulation of the products in three orders (sequential, 64-row k
tiles, the call's split-K partitions added in a random order), with float32 and with fused products on the f32-operand path;
the float32 evaluation of the latent chain's reference - pass the bounds at every shape the GPU tests use, and their worst
figures are the ones tests/parity.py quotes (run with -s to see them).  Small-integer operands give the same bits in every order.

Sensitivity: the float64 result, changed the way a broken kernel would change it, FAILS the new bounds; ``OLD_PASSES`` records
which of these defects the checks they replace (``close``: tol (1 + |want|); assert_allclose(rtol = 2e-3, atol = 2e-3 sqrt(K)))
let through.
"""
import numpy as np
import pytest

from tests import latent_ref as lr
from tests import parity as par

bf = par.bf16_round


def old_close(got, want, tol):
    """test_ops_gpu.close"""
    return bool(np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want))))


def old_allclose(got, want, K):
    """np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3 * sqrt(K)) of the weight-gradient / K-stream / multi tests"""
    return bool(np.all(np.abs(got - want) <= 2e-3 * np.sqrt(K) + 2e-3 * np.abs(want)))


def new_fails(got, want, unit, kind, **kw):
    with pytest.raises(AssertionError):
        par.assert_product(got, want, unit, kind, "defect", **kw)
    return True


def operands(kind, M, N, K, scale, seed=None):
    rng = np.random.default_rng(M + N + K if seed is None else seed)
    Nc = min(N, 128)                    # (wide outputs are sampled by their first 128 columns)
    return par.cast(rng.standard_normal((M, K)) * scale, kind), par.cast(rng.standard_normal((K, Nc)) * scale, kind), rng


# ---- specificity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_accumulation_models_pass_the_product_bounds(kind):
    worst_u = worst_n = 0.0
    for (M, N, K, sk, scale) in par.GEMM_SHAPES[kind]:
        A, B, rng = operands(kind, M, N, K, scale)
        c0 = 1.0 if sk > 1 else None
        want = A @ B + (c0 or 0.0)
        unit = par.product_unit(A, B, extra=[c0] if c0 else [])
        for fused in ((False, True) if kind == "f32" else (False,)):
            for name, got in par.product_models(A, B, sk, c0=c0, fused=fused).items():
                r = par.assert_product(got, want, unit, kind, "%s %s fused=%d" % ((M, N, K, sk), name, fused))
                worst_u, worst_n = max(worst_u, r["units"]), max(worst_n, r["norm_rel"])
                if kind == "bf16" and name == "tiles":
                    par.assert_product(bf(got), want, unit, kind, "bf16 output", out_bf16=True)
    print("\n%s operands: model worst %.1f units, %.2e normwise (bounds %g, %g)" % (kind, worst_u, worst_n, par.PRODUCT[kind]["c_acc"],
                                                                                     par.PRODUCT[kind]["nw"]))
    assert 4.0 * worst_u <= par.PRODUCT[kind]["c_acc"] * 1.02 and 4.0 * worst_n <= par.PRODUCT[kind]["nw"] * 1.02      # the x 4 margin


def test_summation_models_pass_the_sum_bounds():
    worst_u = worst_n = 0.0
    for (R, N, scale) in par.GEMM_SHAPES["sum"]:
        for storage in ("bf16", "f32"):
            for weighted in (False, True):
                rng = np.random.default_rng(R + N)
                X = par.cast(rng.standard_normal((R, N)) * scale, storage)
                w = par.cast(rng.random(R), "f32") if weighted else np.ones(R)
                want, unit = w @ X + 0.5, par.sum_unit(X, w, extra=[0.5])
                for fused in (False, True):
                    for name, got in par.product_models(w[None, :], X, 8, c0=0.5, fused=fused).items():
                        r = par.assert_product(got[0], want, unit, "sum", "%s %s" % ((R, N), name))
                        worst_u, worst_n = max(worst_u, r["units"]), max(worst_n, r["norm_rel"])
    print("\nsums: model worst %.1f units, %.2e normwise" % (worst_u, worst_n))
    assert 4.0 * worst_u <= par.PRODUCT["sum"]["c_acc"] * 1.02 and 4.0 * worst_n <= par.PRODUCT["sum"]["nw"] * 1.02


def test_integer_operands_give_the_same_bits_in_every_order():
    rng = np.random.default_rng(0)
    for (M, N, K, sk) in ((64, 32, 8192, 16), (50, 61, 33, 3), (16, 64, 2304, 16)):
        A, B = par.integer_operands(rng, (M, K)), par.integer_operands(rng, (K, N))
        bias, c0 = par.integer_operands(rng, (N,)), par.integer_operands(rng, (M, N))
        want = 0.25 * (A @ B) + bias + c0
        for name, got in par.product_models(A, B, sk, alpha=0.25, bias=bias, c0=c0).items():
            par.assert_bits(got, want, "f32", name)
        assert K < 8192 or np.mean(bf(want) != want) > 0.5           # a bf16 output shows its rounding on most elements


def test_float32_chain_and_tanh_models_pass_the_elementwise_bound():
    worst = 0.0
    for i, case in enumerate(lr.CHAIN_CASES):
        p = lr.chain_problem(case, 100 + i)
        o64, o32 = lr.chain_reference(p), lr.chain_reference(p, np.float32)
        for k in lr.ELEMENTWISE_OUTPUTS:
            if o64.get(k) is not None:
                worst = max(worst, par.assert_elementwise(o32[k], o64[k], "case %d %s" % (i, k))["elem"])
        for j in (0, 1):
            if o64["scalars"][j] != 0:
                par.assert_rel(o32["scalars"][j], o64["scalars"][j], par.LOSS_RTOL, "scalar %d" % j)
        assert o32["scalars"][2] == o64["scalars"][2]
    for kind in ("bf16", "f32"):
        for (M, N, K) in [(50, 61, 33), (300, 192, 256), (128, 128, 1000), (256, 384, 1024), (512, 128, 192)]:
            A, B, rng = operands(kind, M, N, K, 1.0)
            bias = par.cast(rng.standard_normal(B.shape[1]), "f32")
            want = np.tanh(np.float64(np.float32(0.05)) * (A @ B) + bias)
            for name, x in par.product_models(A, B, 1, alpha=0.05, bias=bias, fused=(kind == "f32")).items():
                worst = max(worst, par.assert_elementwise(np.tanh(x.astype(np.float32)), want, "tanh epilogue")["elem"])
    print("\nelementwise: model worst %.2f x the bound" % worst)
    assert 4.0 * worst <= 1.02


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def truncate_bf16(a):
    b = np.ascontiguousarray(a, np.float64).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


TEST_GEMM_SHAPES = [(50, 61, 33), (300, 192, 256), (128, 128, 1000), (256, 384, 1024), (512, 128, 192)]


def test_the_defects_the_old_gemm_tolerances_let_through_fail():
    """proportional and rounding-mode errors: each one passes the check that used to stand alone in test_ops_gpu.py and fails the
    new bounds (dropped terms were caught before: OLD_PASSES below)"""
    for (M, N, K) in TEST_GEMM_SHAPES:
        A, B, rng = operands("bf16", M, N, K, 1.0)
        want, unit = A @ B, par.product_unit(A, B)
        unit1 = par.product_unit(A, B, extra=[1.0])
        scales = [0.9] + ([0.5] if K >= 1000 else []) + ([0.75] if K >= 192 else [])
        for s in scales:
            assert old_close(1.0 + s * want, 1.0 + want, 2e-2 * np.sqrt(K)), (K, s)               # bf16 "split-k"
            new_fails(1.0 + s * want, 1.0 + want, unit1, "bf16")
            assert old_close(bf(s * want), want, 2e-2 * np.sqrt(K)), (K, s)                         # "bf16 out"
            new_fails(bf(s * want), want, unit, "bf16", out_bf16=True)
        assert old_close(truncate_bf16(want), want, 2e-2 * np.sqrt(K))                              # truncated, not rounded
        new_fails(truncate_bf16(want), want, unit, "bf16", out_bf16=True)
        par.assert_product(bf(want), want, unit, "bf16", "rounded", out_bf16=True)
        A, B, rng = operands("f32", M, N, K, 1.0)                                                   # f32 "split-k"
        want, unit1 = A @ B, par.product_unit(A, B, extra=[1.0])
        assert old_close(1.0 + 0.9999 * want, 1.0 + want, 2e-5 * np.sqrt(K))
        new_fails(1.0 + 0.9999 * want, 1.0 + want, unit1, "f32")
    # tanh epilogue, bf16 at (50, 61, 33): alpha 0.04 for 0.05; the bias scaled by 0.8
    A, B, rng = operands("bf16", 50, 61, 33, 1.0)
    bias = rng.standard_normal(61)
    want = np.tanh(0.05 * (A @ B) + bias)
    for bad in (np.tanh(0.04 * (A @ B) + bias), np.tanh(0.05 * (A @ B) + 0.8 * bias)):
        assert old_close(bad, want, 2e-2 * 10)
        with pytest.raises(AssertionError):
            par.assert_elementwise(bad, want, "tanh epilogue")
    # column sums scaled by 0.995, at every N of test_colsum_bf16_vector_path_plain_and_weighted
    for N in (1024, 256, 64, 8, 61, 1):
        X = bf(np.random.default_rng(N).standard_normal((4099, N)))
        want = 0.5 + X.sum(0)
        assert old_close(0.5 + 0.995 * X.sum(0), want, 2e-4 * np.sqrt(4099))
        new_fails(0.5 + 0.995 * X.sum(0), want, par.sum_unit(X, extra=[0.5]), "sum")
    # weight-gradient, K-stream and gemm_multi tests: the product scaled by 0.999
    for (M, N, K, scale) in ((256, 1024, 4096, 0.5), (256, 512, 8192, 0.5), (256, 768, 4096, 0.5)):
        A, B, rng = operands("bf16", M, N, K, scale)
        want = A @ B
        assert old_allclose(0.999 * want, want, K)
        new_fails(0.999 * want, want, par.product_unit(A, B), "bf16")


# which of the further defects the old checks let through (True = passes the old check); every one fails the new bounds
OLD_PASSES = {"dropped k row, K = 8192": False, "a split-K partition added twice": False, "bias added by every partition": False,
              "colsum_b without the last 64-row tile": False, "one-hot table gradient of bf16 rows scaled by 0.99": True}


def test_structural_defects_fail_and_which_of_them_passed_before():
    seen = {}
    M, N, K, sk = 256, 512, 8192, 16
    A, B, rng = operands("bf16", M, N, K, 0.5)
    want, unit = A @ B, par.product_unit(A, B)
    dropped = want - A[:, 4000, None] * B[None, 4000, :]
    seen["dropped k row, K = 8192"] = old_allclose(dropped, want, K)
    new_fails(dropped, want, unit, "bf16")
    k0, k1 = par.split_ranges(K, sk, 64)[3]
    twice = want + A[:, k0:k1] @ B[k0:k1]
    seen["a split-K partition added twice"] = old_allclose(twice, want, K)
    new_fails(twice, want, unit, "bf16")
    # the automatic split-K of a store-mode f32 GEMM (16 x 64 x 2304, 16 partitions) with the bias in every partition
    A, B, rng = operands("f32", 16, 64, 2304, 1.0)
    bias = rng.standard_normal(64)
    want, unit = A @ B + bias, par.product_unit(A, B, extra=[bias])
    seen["bias added by every partition"] = old_close(A @ B + 16 * bias, want, 2e-5 * np.sqrt(2304))
    new_fails(A @ B + 16 * bias, want, unit, "f32")
    Bc = bf(np.random.default_rng(5).standard_normal((4096, 128)) * 0.5)
    want = 0.25 + Bc.sum(0)
    seen["colsum_b without the last 64-row tile"] = old_allclose(0.25 + Bc[:-64].sum(0), want, 4096)
    new_fails(0.25 + Bc[:-64].sum(0), want, par.sum_unit(Bc, extra=[0.25]), "sum")
    rng = np.random.default_rng(9)                          # test_gemm_onehot_table_gradient, bf16: checked to 0.1 (1 + |want|)
    idx, da = rng.integers(0, 61, 1024), bf(rng.standard_normal((1024, 128)))
    A1 = np.zeros((1024, 61))
    A1[np.arange(1024), idx] = 1.0
    want = A1.T @ da
    seen["one-hot table gradient of bf16 rows scaled by 0.99"] = old_close(0.99 * want, want, 1e-2 * 10)
    new_fails(0.99 * want, want, par.product_unit(A1.T, da), "bf16")
    assert seen == OLD_PASSES, seen


@pytest.mark.parametrize("defect", ["kl_padding", "split_swapped", "chunk2_bias"])
def test_latent_chain_defects_fail(defect):
    """chain level, on the 160 KB case (B_valid 5 of 8, split, three column chunks of S): padding rows counted in the KL scalar,
    the split halves swapped, the second column chunk of dense_rows left at its bias"""
    p = lr.chain_problem(lr.CHAIN_CASES[0], 100)
    good, bad = lr.chain_reference(p), lr.chain_reference(p, defect=defect)

    def check(o):
        for k in lr.ELEMENTWISE_OUTPUTS:
            if good.get(k) is not None:
                par.assert_elementwise(o[k], good[k], k)
        par.assert_rel(o["scalars"][0], good["scalars"][0], par.LOSS_RTOL, "KL")
    check(lr.chain_reference(p, np.float32))
    with pytest.raises(AssertionError):
        check(bad)


# ---- the helpers themselves --------------------------------------------------------------------------------------------------
def test_half_ulp_and_zero_units():
    x = np.array([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 0.0])
    assert np.array_equal(par.half_ulp_bf16(x), [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -7, 0.0])
    r = np.random.default_rng(1).standard_normal(100000) * 37.0
    assert np.all(np.abs(bf(r) - r) <= par.half_ulp_bf16(r))                      # round to nearest: within half an ulp, always
    assert np.mean(np.abs(truncate_bf16(r) - r) > par.half_ulp_bf16(r)) > 0.4      # truncation: beyond it on half the elements
    assert np.max(np.abs(bf(r) - r) / np.abs(r)) > 2.0 ** -9                       # (a flat 2^-9 |want| does not hold for either)
    want, unit = np.zeros((4, 4)), np.zeros((4, 4))
    par.assert_product(want, want, unit, "bf16", "untouched block")
    bad = want.copy()
    bad[2, 1] = 1e-30
    with pytest.raises(AssertionError, match="untouched block"):
        par.assert_product(bad, want, unit, "bf16", "untouched block")
    with pytest.raises(AssertionError):
        par.assert_bits(np.array([1.0, -0.0]), np.array([1.0, 0.0]), "f32", "sign of zero")
    with pytest.raises(AssertionError):
        par.assert_product(np.full((2, 2), np.nan), np.ones((2, 2)), np.ones((2, 2)), "f32", "nan")
