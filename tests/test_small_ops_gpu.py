"""The reductions, conversions, optimizers and glue kernels of csrc/misc.hip, each called directly and compared with float64
numpy (GPU box only).

Exact operations (concatenation, copies, gathers, one f32 addition, conversions, sums of small integers) are asserted
BIT-equal to the float64 result cast to the storage type; sums of rounded operands are held to the per-element accumulation
unit, elementwise f32 functions to rtol |want| + floor RMS (tests/parity.py: assert_bits / assert_product / assert_elementwise).
The grid-stride kernels run under a cap of 2048 x 256 threads: one case of each is larger than that, so that the second
trip of the stride loop is looked at.
"""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops
from oracle import vae_oracle as vo
from tests import parity as par

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 2048 * 256              # threads of the largest grid-stride launch (misc.hip nblocks)
KINDS = [("f32", torch.float32), ("bf16", torch.bfloat16)]


def dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def rounded(a, dt):
    """the values the device holds after storing ``a`` as ``dt``"""
    return host(dev(a, dt))


# ---- column sums, weighted column sums, sums over time -----------------------------------------------------------------------
@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("R,N,ldx,offset", [(4099, 64, 64, 0), (4099, 61, 64, 0), (4099, 64, 72, 4), (1000, 24, 28, 0), (777, 2056, 2056, 0),
                                            (1, 64, 64, 0), (15, 61, 64, 0), (15, 61, 61, 1)])
def test_colsum_generic_and_vector_paths_accumulate_onto_out(storage, dt, R, N, ldx, offset):
    """mvae_colsum / mvae_colsum_weighted, f32 and bf16: the bf16 vector path (16-byte loads) and what leaves it for the generic
    kernel - a base pointer that is not 16-byte aligned (``offset`` elements), ldx % 8 != 0, N > 2048 - R = 1 and R = 15 (below
    one lane group), on an ``out`` that already holds data (both entry points add to it)."""
    rng = np.random.default_rng(R + N + ldx)
    buf = dev(rng.standard_normal(R * ldx + offset), dt)
    X = buf[offset:].view(R, ldx)
    Xh = host(X)[:, :N]
    wgt = rounded(rng.random(R), torch.float32)
    out0 = rounded(rng.standard_normal(N), torch.float32)
    out, outw = dev(out0), dev(out0)
    ops.colsum(X, R, N, out, ldx=ldx)
    ops.colsum_weighted(X, dev(wgt), R, N, outw, ldx=ldx)
    torch.cuda.synchronize()
    par.assert_product(host(out), out0 + Xh.sum(0), par.sum_unit(Xh, extra=[out0]), "sum", "colsum")
    par.assert_product(host(outw), out0 + wgt @ Xh, par.sum_unit(Xh, wgt, extra=[out0]), "sum", "colsum_weighted")


@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("R,N,ldx", [(4099, 64, 64), (4099, 61, 64), (1000, 24, 28), (15, 2056, 2056)])
def test_colsum_of_small_integers_is_exact(storage, dt, R, N, ldx):
    """integer operands: every order of the f32 partial sums and atomics gives the same bits"""
    rng = np.random.default_rng(R + N)
    X = par.integer_operands(rng, (R, ldx))
    wgt = par.integer_operands(rng, (R,), 4)
    out0 = par.integer_operands(rng, (N,))
    out, outw = dev(out0), dev(out0)
    ops.colsum(dev(X, dt), R, N, out, ldx=ldx)
    ops.colsum_weighted(dev(X, dt), dev(wgt), R, N, outw, ldx=ldx)
    torch.cuda.synchronize()
    par.assert_bits(host(out), out0 + X[:, :N].sum(0), "f32", "colsum")
    par.assert_bits(host(outw), out0 + wgt @ X[:, :N], "f32", "colsum_weighted")


@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("T,BN", [(96, 4096), (11, 500), (1, 64), (15, 8 * 300 + 4)])
def test_sum_over_time_against_float64_and_exact_on_integers(storage, dt, T, BN):
    """mvae_sum_over_time: the bf16 vector kernel (BN % 8 == 0), the generic one (BN % 8 != 0, f32), store and accumulate"""
    rng = np.random.default_rng(T + BN)
    Xh = rounded(rng.standard_normal((T, BN)), dt)
    out0 = rounded(rng.standard_normal(BN), torch.float32)
    out, acc = dev(out0), dev(out0)                       # (store mode overwrites what is there)
    ops.sum_over_time(dev(Xh, dt), T, BN, out)
    ops.sum_over_time(dev(Xh, dt), T, BN, acc, accumulate=True)
    Xi = par.integer_operands(rng, (T, BN))
    exact = dev(out0)
    ops.sum_over_time(dev(Xi, dt), T, BN, exact)
    torch.cuda.synchronize()
    par.assert_product(host(out), Xh.sum(0), par.sum_unit(Xh), "sum", "sum_over_time")
    par.assert_product(host(acc), out0 + Xh.sum(0), par.sum_unit(Xh, extra=[out0]), "sum", "sum_over_time accumulate")
    par.assert_bits(host(exact), Xi.sum(0), "f32", "sum_over_time of integers")


# ---- bidirectional glue --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("T,B,H", [(1, 5, 8), (2, 5, 24), (7, 3, 64)])
@pytest.mark.parametrize("rev", [True, False])
def test_bi_concat(storage, dt, T, B, H, rev):
    """mvae_bi_concat: cat[t] = [f[t] | r[T-1-t]], cat_rev[k] = cat[T-1-k] - a copy, bit for bit; with cat_rev NULL"""
    _bi_concat_case(storage, dt, T, B, H, rev)


def test_bi_concat_above_the_grid_cap():
    """T * B * H / 4 = 589824 16-byte chunks of f32 > 2048 x 256 threads: the stride loop takes a second trip"""
    assert 9 * 256 * 1024 // 4 > GRID_CAP
    _bi_concat_case("f32", torch.float32, 9, 256, 1024, True)


def _bi_concat_case(storage, dt, T, B, H, rev):
    rng = np.random.default_rng(T + B + H)
    f, r = rounded(rng.standard_normal((T, B, H)), dt), rounded(rng.standard_normal((T, B, H)), dt)
    cat = torch.full((T, B, 2 * H), 7.0, dtype=dt, device=DEV)
    cat_rev = torch.full((T, B, 2 * H), 7.0, dtype=dt, device=DEV) if rev else None
    ops.bi_concat(dev(f, dt), dev(r, dt), cat, cat_rev, T, B, H)
    torch.cuda.synchronize()
    want = np.concatenate([f, r[::-1]], axis=2)
    par.assert_bits(host(cat), want, storage, "cat")
    if rev:
        par.assert_bits(host(cat_rev), want[::-1], storage, "cat_rev")


@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("T,slab", [(1, 4), (3, 148), (8, 16 * 64)])
@pytest.mark.parametrize("with_a", [True, False])
def test_add_time_reversed(storage, dt, T, slab, with_a):
    """mvae_add_time_reversed: dst[t] = a[t] + b[T-1-t] (a NULL: 0) - ONE rounding of a two-term sum: f32 bit-equal to the
    float64 sum cast to f32, bf16 to bf16_round of it.  Distinct buffers only: the kernel's pointers are __restrict__ and the
    engine never calls it in place."""
    _add_time_reversed_case(storage, dt, T, slab, with_a)


def test_add_time_reversed_above_the_grid_cap():
    assert 3 * 720000 // 4 > GRID_CAP
    _add_time_reversed_case("bf16", torch.bfloat16, 3, 720000, True)


def _add_time_reversed_case(storage, dt, T, slab, with_a):
    rng = np.random.default_rng(T + slab)
    a, b = rounded(rng.standard_normal((T, slab)), dt), rounded(rng.standard_normal((T, slab)), dt)
    dst = torch.full((T, slab), 7.0, dtype=dt, device=DEV)
    ops.add_time_reversed(dst, dev(a, dt) if with_a else None, dev(b, dt), T, slab)
    torch.cuda.synchronize()
    par.assert_bits(host(dst), (a if with_a else 0.0) + b[::-1], storage, "dst")


# ---- a gradient arriving at softmax probabilities ---------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("N", [3, 61, 77, 128])
def test_softmax_bwd_add(storage, dt, N):
    _softmax_bwd_add_case(storage, dt, N, R=333)


def test_softmax_bwd_add_above_the_grid_cap():
    """R > 2048 x 256 rows (one thread per row), at N = 3 to keep the host reference small"""
    _softmax_bwd_add_case("f32", torch.float32, 3, R=GRID_CAP + 1000)


def _softmax_bwd_add_case(storage, dt, N, R):
    """mvae_softmax_bwd_add: dlogits += p (dp - sum_j p_j dp_j) with p a real softmax, so that dp - sum(p dp) cancels; the pad
    columns N .. NP-1 of dlogits stay as they were"""
    rng = np.random.default_rng(N + R)
    NP = ops.head_np(N)
    p = rounded(vo.softmax(rng.standard_normal((R, N)) * 2.0), torch.float32)
    dp = rounded(rng.standard_normal((R, N)), torch.float32)
    dl0 = rounded(rng.standard_normal((R, NP)) * 0.1, dt)
    dl = dev(dl0, dt)
    ops.softmax_bwd_add(dev(p), dev(dp), dl, R, N, NP)
    torch.cuda.synchronize()
    want = dl0[:, :N] + p * (dp - np.sum(p * dp, 1, keepdims=True))
    got = host(dl)
    par.assert_elementwise(got[:, :N], want, "dlogits", out_bf16=(storage == "bf16"))
    par.assert_bits(got[:, N:], dl0[:, N:], storage, "pad columns")


# ---- signature head ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("SD,off,ldz", [(1, 0, 4), (5, 3, 16), (32, 8, 40)])
def test_signature_head(SD, off, ldz):
    """mvae_signature_head_fwd / _bwd on columns [off, off + SD) of a wider zh: tanh, weighted mean squared error, argmax hits
    (first maximum on planted ties; rows of weight 0 are not hits), and the gradient ADDED onto dz with every column outside
    [off, off + SD) untouched.  (sig_head_bwd_k is launched under the grid cap but does not stride: B x SD is a minibatch
    times at most a few dozen columns, far below 2048 x 256.)"""
    rng = np.random.default_rng(SD + off)
    B = 203
    zh = rounded(rng.standard_normal((B, ldz)), torch.float32)
    tgt = rounded(np.tanh(rng.standard_normal((B, SD))), torch.float32)
    rw = rounded(rng.random(B) / B, torch.float32)
    rw[::7] = 0.0
    if SD >= 5:
        zh[1, off + 1] = zh[1, off + 3] = 4.0             # ties of the output's maximum: the first one counts
        tgt[1, :] = 0.0
        tgt[1, 1] = 0.9
        tgt[2, 0] = tgt[2, 4] = 0.99                      # ... and of the target's
        zh[2, off:off + SD] = -1.0
        zh[2, off] = 2.0
    out_o = np.tanh(zh[:, off:off + SD])
    out = torch.zeros((B, SD), device=DEV)
    sc = dev(np.array([0.25, 3.0]))
    ops.signature_head_fwd(dev(zh), off, SD, B, out, target=dev(tgt), row_weight=dev(rw), scalars=sc)
    torch.cuda.synchronize()
    par.assert_elementwise(host(out), out_o, "out")
    out_h = host(out)
    par.assert_rel(host(sc)[0] - 0.25, np.sum(rw * np.mean((out_h - tgt) ** 2, 1)), par.LOSS_RTOL, "loss")
    hits = (np.argmax(out.cpu().numpy(), 1) == np.argmax(tgt.astype(np.float32), 1)) & (rw != 0)
    assert host(sc)[1] == 3.0 + hits.sum()
    assert np.sum((np.argmax(out.cpu().numpy(), 1) == np.argmax(tgt.astype(np.float32), 1)) & (rw == 0)) > 0 or SD == 1
    # without a target: the activations only, scalars unchanged
    out2 = torch.zeros((B, SD), device=DEV)
    sc2 = dev(np.array([0.25, 3.0]))
    ops.signature_head_fwd(dev(zh), off, SD, B, out2, scalars=sc2)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and host(sc2).tolist() == [0.25, 3.0]
    # backward, onto existing content
    dz0 = rounded(rng.standard_normal((B, ldz)) * 1e-3, torch.float32)
    dz = dev(dz0)
    ops.signature_head_bwd(dz, off, SD, B, out, dev(tgt), dev(rw), 0.7)
    torch.cuda.synchronize()
    add = np.float64(np.float32(0.7)) * rw[:, None] * 2.0 * (out_h - tgt) / SD * (1.0 - out_h ** 2)
    got = host(dz)
    par.assert_elementwise(got[:, off:off + SD] - dz0[:, off:off + SD], add, "dz", floor_of=dz0[:, off:off + SD] + add)
    keep = np.ones(ldz, bool)
    keep[off:off + SD] = False
    par.assert_bits(got[:, keep], dz0[:, keep], "f32", "columns outside the head")


# ---- history, copies, scalars --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,B_pad,Z,ldh,ldo", [(5, 8, 4, 4, 4), (37, 48, 24, 48, 24), (16, 16, 64, 128, 72), (1, 4, 256, 512, 256)])
@pytest.mark.parametrize("with_prev", [True, False])
@pytest.mark.parametrize("with_z", [True, False])
def test_history_from_latent(B, B_pad, Z, ldh, ldo, with_prev, with_z):
    """mvae_history_from_latent: z' = mu + exp(logvar / 2) eps2; hist[0] = prev (or 0), hist[b] = z'[b-1], rows B .. B_pad-1
    zero, inside wider rows whose other columns stay; z_out BIT-equal to what mvae_latent_fwd writes for the same inputs"""
    rng = np.random.default_rng(B + Z)
    mu, lv, eps = (rounded(rng.standard_normal((B_pad, Z)) * s, torch.float32) for s in (0.5, 0.3, 1.0))
    prev = rounded(rng.standard_normal(Z), torch.float32)
    zh = torch.full((B_pad, ldh), 7.0, device=DEV)
    hist = zh[:, ldh - Z:]
    zo = torch.full((B_pad, ldo), 7.0, device=DEV)
    ops.history_from_latent(dev(mu), dev(lv), dev(eps), B, B_pad, Z, hist, z_out=zo[:, :Z] if with_z else None,
                            prev=dev(prev) if with_prev else None)
    z_lat = torch.zeros((B, Z), device=DEV)
    ops.latent_fwd(B, Z, 0, 0.1, 0.0, 1.0, 1.0 / B, dev(mu[:B]), dev(lv[:B]), dev(eps[:B]), z_lat, torch.zeros(3, device=DEV))
    torch.cuda.synchronize()
    z_o = mu + np.exp(lv / 2) * eps
    want = np.zeros((B_pad, Z))
    want[0] = prev if with_prev else 0.0
    want[1:B] = z_o[:B - 1]
    got = host(zh)
    par.assert_elementwise(got[:, ldh - Z:], want, "hist")
    assert np.all(got[B:, ldh - Z:] == 0) and np.all(got[:, :ldh - Z] == 7.0)
    par.assert_bits(got[0, ldh - Z:], want[0], "f32", "hist row 0")
    par.assert_bits(got[1:B, ldh - Z:], host(z_lat)[:B - 1], "f32", "hist rows = latent_fwd's z")
    if with_z:
        par.assert_bits(host(zo)[:B, :Z], host(z_lat), "f32", "z_out = latent_fwd's z")
        assert np.all(host(zo)[B:] == 7.0) and np.all(host(zo)[:, Z:] == 7.0)
    else:
        assert np.all(host(zo) == 7.0)


@pytest.mark.parametrize("rows,cols,ldd,lds,src_row0,zero_rows", [(9, 24, 24, 24, 0, 0), (9, 24, 40, 32, -1, 1), (16, 5, 8, 7, -3, 3),
                                                                   (6, 4, 4, 4, 2, 0), (0, 24, 24, 24, 0, 0), (3, 24, 24, 24, -3, 3)])
def test_copy2d(rows, cols, ldd, lds, src_row0, zero_rows):
    """mvae_copy2d_f32: dst[r] = src[src_row0 + r], the first zero_rows rows zero (their source index may be negative), row
    strides above cols with the columns beyond untouched, rows = 0 a no-op"""
    rng = np.random.default_rng(rows + cols)
    src = rounded(rng.standard_normal((rows + 8, lds)), torch.float32)
    dst = torch.full((max(rows, 1), ldd), 7.0, device=DEV)
    ops.copy2d(dst[:, :cols], dev(src)[:, :cols], rows, cols, src_row0=src_row0, zero_rows=zero_rows)
    torch.cuda.synchronize()
    want = np.full((max(rows, 1), ldd), 7.0)
    for r in range(rows):
        want[r, :cols] = 0.0 if r < zero_rows else src[src_row0 + r, :cols]
    par.assert_bits(host(dst), want, "f32", "dst")


def test_copy2d_above_the_grid_cap():
    rows, cols = 1100, 512
    assert rows * cols > GRID_CAP
    src = rounded(np.random.default_rng(1).standard_normal((rows, cols)), torch.float32)
    dst = torch.zeros((rows, cols), device=DEV)
    ops.copy2d(dst, dev(src), rows, cols, src_row0=-1, zero_rows=1)
    torch.cuda.synchronize()
    par.assert_bits(host(dst), np.concatenate([np.zeros((1, cols)), src[:-1]]), "f32", "dst")


@pytest.mark.parametrize("n,mask", [(0, 0), (1, 0), (1, 1), (7, 0b0100101), (32, 0xA5A5A5A5), (32, 0xFFFFFFFF)])
def test_scalars_accumulate(n, mask):
    """mvae_scalars_accumulate: acc[i] += (bit i of the mask ? 1 : alpha) x[i], one f32 multiply and one add each; n = 33 refused"""
    rng = np.random.default_rng(n)
    acc0, x = rounded(rng.standard_normal(32), torch.float32), rounded(rng.standard_normal(max(n, 1)), torch.float32)[:n]
    acc = dev(acc0)
    assert hl.load().mvae_scalars_accumulate(acc.data_ptr(), dev(x).data_ptr() if n else acc.data_ptr(), n, 0.37, mask,
                                             torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    al = np.float32(0.37)
    want = acc0.astype(np.float32)
    plain = np.array([(mask >> i) & 1 for i in range(n)], bool)
    fused = want.copy()                                    # (the compiler may contract acc + alpha * x into one fma)
    want[:n] += np.where(plain, x.astype(np.float32), al * x.astype(np.float32))
    fused[:n] = np.where(plain, want[:n], (acc0[:n] + np.float64(al) * x).astype(np.float32))
    got = host(acc)
    assert np.all((got == want) | (got == fused)), np.nonzero((got != want) & (got != fused))
    par.assert_bits(got[n:], acc0[n:], "f32", "beyond n")
    par.assert_bits(got[:n][plain], acc0[:n][plain] + x[plain], "f32", "plain entries")
    assert hl.load().mvae_scalars_accumulate(acc.data_ptr(), acc.data_ptr(), 33, 1.0, 0, torch.cuda.current_stream().cuda_stream) == hl.E_ARG


# ---- written-out input projections -----------------------------------------------------------------------------------------
def _tile16_offsets(R, N):
    m, n = np.meshgrid(np.arange(R), np.arange(N), indexing="ij")
    return ((((m // 16) * (N // 16) + n // 16) * 64 + ((n % 16) // 4) * 16 + m % 16) * 4 + n % 4).ravel()


@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("layout", [hl.TILE16, hl.ROWMAJOR])
@pytest.mark.parametrize("R,N", [(16, 16), (48, 768), (1024, 1024)])
def test_gather2_tile16(storage, dt, layout, R, N):
    """mvae_gather2_tile16: out[r] = table[idx[r]] + table2[idx2[r]] - one f32 addition, then the store: f32 bit-equal to the
    float64 sum cast to f32, bf16 to bf16_round of it; the TILE16 image against the header's offset formula.  (1024 x 1024 / 4
    = 2048 x 128 threads: the largest shape below the grid cap the engine uses per chunk.)"""
    rng = np.random.default_rng(R + N)
    K1, K2 = 61, 16
    t1, t2 = rounded(rng.standard_normal((K1, N)), dt), rounded(rng.standard_normal((K2, N)), dt)
    i1, i2 = rng.integers(0, K1, R), rng.integers(0, K2, R)
    out = torch.full((R, N), 7.0, dtype=dt, device=DEV)
    ops.gather2_tile16(dev(i1, torch.uint8), dev(i2, torch.uint8), dev(t1, dt), dev(t2, dt), out, R, N, layout=layout)
    torch.cuda.synchronize()
    want = t1[i1] + t2[i2]
    got = host(out)
    if layout == hl.TILE16:
        got = got.ravel()[_tile16_offsets(R, N)].reshape(R, N)
    par.assert_bits(got, want, storage, "out")


def test_gather2_tile16_above_the_grid_cap():
    R, N = 2064, 1024
    assert R * N // 4 > GRID_CAP
    rng = np.random.default_rng(3)
    t1, t2 = rounded(rng.standard_normal((61, N)), torch.bfloat16), rounded(rng.standard_normal((16, N)), torch.bfloat16)
    i1, i2 = rng.integers(0, 61, R), rng.integers(0, 16, R)
    out = torch.zeros((R, N), dtype=torch.bfloat16, device=DEV)
    ops.gather2_tile16(dev(i1, torch.uint8), dev(i2, torch.uint8), dev(t1, torch.bfloat16), dev(t2, torch.bfloat16), out, R, N)
    torch.cuda.synchronize()
    par.assert_bits(host(out).ravel()[_tile16_offsets(R, N)].reshape(R, N), t1[i1] + t2[i2], "bf16", "out")


@pytest.mark.parametrize("storage,dt", KINDS)
@pytest.mark.parametrize("R,N", [(48, 1024), (16, 16), (2064, 1024)])
def test_outer_bias_tile16(storage, dt, R, N):
    """mvae_outer_bias_tile16: xs[r] w[n] + bias[n] in f32 (a multiply and an add, or one fma), stored as f32 or rounded to
    bf16: within half an ulp of bf16 of float64 plus two f32 units; (2064, 1024) is above the grid cap"""
    rng = np.random.default_rng(R + N)
    xs, w, b = (rounded(a, torch.float32) for a in (rng.random(R), rng.standard_normal(N), rng.standard_normal(N)))
    out = torch.zeros((R, N), dtype=dt, device=DEV)
    ops.outer_bias_tile16(dev(xs), dev(w), dev(b), out, R, N)
    torch.cuda.synchronize()
    got = host(out).ravel()[_tile16_offsets(R, N)].reshape(R, N)
    want = xs[:, None] * w[None] + b[None]
    unit = par.product_unit(xs[:, None], w[None], extra=[b[None]])
    err = np.abs(got - want)
    bound = 2.0 * unit + (par.half_ulp_bf16(want) if storage == "bf16" else 0.0)
    par._record("outer_bias:" + storage, "out", elem=float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())


def test_convert_rounds_to_nearest_even():
    """mvae_convert f32 -> bf16 against parity.bf16_round, on random values, exact ties (round to even) and values one f32 ulp
    either side of a tie; bf16 -> f32 is exact"""
    rng = np.random.default_rng(17)
    x = rng.standard_normal(4096).astype(np.float32)
    ties = (x.view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    allx = np.concatenate([x, ties.view(np.float32), (ties + np.uint32(1)).view(np.float32), (ties - np.uint32(1)).view(np.float32),
                           np.array([0.0, -0.0, 1.0, 255.0, 257.0, 3.0e38], np.float32)])
    src = dev(allx)
    dst = torch.zeros(allx.size, dtype=torch.bfloat16, device=DEV)
    ops.convert(src, dst)
    back = torch.zeros(allx.size, device=DEV)
    ops.convert(dst, back)
    torch.cuda.synchronize()
    par.assert_bits(host(dst), allx.astype(np.float64), "bf16", "f32 -> bf16")
    assert torch.equal(back, dst.float())


# ---- optimizers ----------------------------------------------------------------------------------------------------------
def _check_update(p, p0, want_update, what):
    """the UPDATE p - p0 (about lr in size, a thousandth of p) at its own scale: the elementwise f32 bound on the update (Adam's
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) evaluated in float32 is 3.4e-6 off relatively at t = 2, 3: inside its rtol), plus the
    rounding of p itself (half an ulp of p, at most 2^-24 |p| x 2)"""
    got = host(p) - p0
    err = np.abs(got - want_update)
    rms = np.sqrt(np.mean(want_update ** 2))
    bound = par.ELEMWISE_F32["rtol"] * np.abs(want_update) + par.ELEMWISE_F32["floor"] * rms + 2.0 * par.U_ACC * np.abs(p0)
    par._record("update", what, elem=float((err / bound).max()))
    assert np.all(err <= bound), "%s: update off by %.3g x its bound" % (what, (err / bound).max())


@pytest.mark.parametrize("n,off", [(5003, 0), (4099, 1), (GRID_CAP * 4 + 1027, 0)])
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_adam_update_at_its_own_scale_and_guard(n, off, grad_scale):
    """three mvae_adam_step_dev steps against float64 Keras Adam, the update itself held to a relative bound (the 1e-5 (1 + |p|)
    of test_ops_gpu is 1 % of an update); grad_scale != 1; vector body + tail, an unaligned view (scalar path) and one length
    above the grid cap; then a step with the guard word non-zero: parameters, moments and count stay, the gradient is zeroed"""
    rng = np.random.default_rng(n % 1000 + off)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p0 = rounded(rng.standard_normal(n), torch.float32)
    buf = [torch.zeros(n + off, device=DEV) for _ in range(4)]
    p, g_d, mm, vv = [b[off:] for b in buf]
    p.copy_(dev(p0))
    t_done = torch.zeros(1, dtype=torch.int32, device=DEV)
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    p_o, m_o, v_o = p0.copy(), np.zeros(n), np.zeros(n)
    gs = np.float64(np.float32(grad_scale))
    for t in range(1, 4):
        g = rounded(rng.standard_normal(n), torch.float32)
        before = host(p)
        m_o = b1 * m_o + (1 - np.float64(np.float32(b1))) * g * gs
        v_o = np.float64(np.float32(b2)) * v_o + (1 - np.float64(np.float32(b2))) * (g * gs) ** 2
        lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        upd = -lr_t * m_o / (np.sqrt(v_o) + eps)
        g_d.copy_(dev(g))
        ops.adam_step_dev(p, g_d, mm, vv, lr, t_done, grad_scale=grad_scale, zero_grad=True, guard=guard)
        torch.cuda.synchronize()
        _check_update(p, before, upd, "adam step %d" % t)
        assert float(g_d.abs().max()) == 0.0 and int(t_done.item()) == t
    par.assert_elementwise(host(mm), m_o, "m")
    par.assert_elementwise(host(vv), v_o, "v")
    keep = [x.clone() for x in (p, mm, vv)]
    guard.fill_(4)
    g_d.copy_(dev(rng.standard_normal(n)))
    ops.adam_step_dev(p, g_d, mm, vv, lr, t_done, grad_scale=grad_scale, zero_grad=True, guard=guard)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, mm, vv))) and int(t_done.item()) == 3
    assert float(g_d.abs().max()) == 0.0


@pytest.mark.parametrize("n,off", [(5003, 0), (4099, 1)])
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_rmsprop_update_at_its_own_scale_and_guard(n, off, grad_scale):
    rng = np.random.default_rng(n + off)
    lr, rho, eps = 1e-3, 0.9, 1e-8
    p0 = rounded(rng.standard_normal(n), torch.float32)
    buf = [torch.zeros(n + off, device=DEV) for _ in range(3)]
    p, g_d, vv = [b[off:] for b in buf]
    p.copy_(dev(p0))
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    v_o = np.zeros(n)
    gs = np.float64(np.float32(grad_scale))
    for t in range(1, 4):
        g = rounded(rng.standard_normal(n), torch.float32)
        before = host(p)
        v_o = np.float64(np.float32(rho)) * v_o + (1 - np.float64(np.float32(rho))) * (g * gs) ** 2
        upd = -lr * g * gs / (np.sqrt(v_o) + eps)
        g_d.copy_(dev(g))
        ops.rmsprop_step(p, g_d, vv, lr, grad_scale=grad_scale, zero_grad=True, guard=guard)
        torch.cuda.synchronize()
        _check_update(p, before, upd, "rmsprop step %d" % t)
        assert float(g_d.abs().max()) == 0.0
    par.assert_elementwise(host(vv), v_o, "v")
    keep = [x.clone() for x in (p, vv)]
    guard.fill_(1)
    g_d.copy_(dev(rng.standard_normal(n)))
    ops.rmsprop_step(p, g_d, vv, lr, grad_scale=grad_scale, zero_grad=True, guard=guard)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, vv))) and float(g_d.abs().max()) == 0.0
