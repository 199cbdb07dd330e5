"""The C ABI's contract on the device: the baselines of tests/abi_contract.py run, and what the library refuses leaves no trace.

Run this file on the MI355X only after tests/test_abi_contract_cpu.py passes on the same source: that file proves, with no device in
reach, that every violation is refused before anything is enqueued; this one runs only the rows flagged ``safe`` - a bad enum, a
refused combination of valid extents, a bad job among good ones - which even wrongly accepted stay inside the baseline's buffers.
Nothing here hands a device a NULL, a misaligned pointer, a negative or undersized extent or an out-of-range index.

  * every baseline, on buffers carved from the footprint arena (guards, sentinel-filled outputs): returns 0, the guards hold,
    the outputs are written, and the values are within the bounds tests/parity.py already holds (BOUNDS through assert_parity,
    assert_product / assert_bits / assert_elementwise, LOSS_RTOL - no new tolerance) of the float64 reference the operator tests
    use: the oracle's recurrence on a matrix packed by mvae_pack_recurrent, softmax_head_oracle, tests/latent_ref.py, NumPy.
    Not compared with a reference of their own: mvae_pack_recurrent and the PACK_RECURRENT job (no test holds a NumPy model of the
    fragment order: the forward and the backward recurrent baselines run on what mvae_pack_recurrent packed at the same shape, and
    the job is bit-compared with the call below), mvae_stream_wait_value32, mvae_streams_alias and mvae_occupancy (no output);
  * every safe refusal: the promised code, and after a synchronise the whole arena - inputs, outputs, counters, guards - is
    bit-identical to what was planted;
  * the accepting side of the caps no other test sits on: mvae_prepare_batch with 64, 65 and 130 jobs (bit-equal to the single
    calls), mvae_gemm_multi with n = 16, mvae_gemm_kstream_multi with n = 8 and exactly 256 workgroups, the phase launches with
    n = 8, mvae_latent_fwd with C = Z = 64 and C = Z = 4.  (mvae_scalars_accumulate at n = 32: test_small_ops_gpu.py; heads at
    N = 192: test_wide_onehot_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from tests import abi_contract as ac
from tests import footprint as fp
from tests import latent_ref as lref
from tests import parity as par
from oracle import vae_oracle as vo
from tests.gpu_util import DEV, _paired_columns

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8, "i32": torch.int32}


def _values(name, shape, dt, data):
    if data is None:
        return ac.default_data(name, shape, dt)
    if isinstance(data, str):
        rng = np.random.default_rng(len(name))
        return {"unit": 0.1 + 0.8 * rng.random(shape), "half": np.full(shape, 0.5)}[data]
    return np.asarray(data).reshape(shape)


class Carver:
    """first pass of a builder: carve every buffer it asks for; ``resolve`` (second pass) hands out the committed addresses"""

    def __init__(self):
        self.ar, self.bufs = fp.Arena(DEV), {}

    def __call__(self, name, shape, dt, data=None, out=False, acc=False):
        assert name not in self.bufs, name
        shape = tuple(shape)
        if out:
            b = self.ar.carve(name, shape, DT[dt])
        elif acc:
            b = self.ar.carve(name, shape, DT[dt], prefill=np.zeros(shape))
        else:
            b = self.ar.carve(name, shape, DT[dt], data=_values(name, shape, dt, data), guard="zero" if dt == "u8" else "sentinel")
        self.bufs[name] = b
        return 0x1000

    def resolve(self, name, shape, dt, data=None, out=False, acc=False):
        return self.bufs[name].t.data_ptr()


def _arena(entry):
    cv = Carver()
    entry.build(cv)
    cv.ar.commit()
    return cv


def _t(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _unchanged(ar):
    same = ar.fetched == ar.planted
    if same.all():
        return None
    at = int(np.argmin(same))
    owner = next((b.name for b in ar.bufs if b.start <= at < b.end), "?")
    return "%d bytes of the arena changed, first at byte %d (buffer '%s')" % (int((~same).sum()), at, owner)


# ---- references of the baselines whose definition is a line of NumPy: {label: f(values by buffer name) -> None (asserts)} ------------
def _ref_gemm(tag, ta, tb, kind, out_bf16=False):
    def check(v):
        A, B = v[tag + ".A"], v[tag + ".B"]
        A, B = (A.T if ta else A), (B.T if tb else B)
        par.assert_product(v[tag + ".C"], A @ B, par.product_unit(A, B), kind, "C", out_bf16=out_bf16)
    return check


def _ref_prep(v):
    par.assert_bits(v["pb.tab"], v["pb.W"] + v["pb.b"], "f32", "MAKE_TABLE")
    want = np.zeros((8, 3))
    want[:5] = v["pb.Wt"].T
    par.assert_bits(v["pb.wt"], want, "bf16", "TRANSPOSE_CONVERT")
    par.assert_bits(v["pb.cd"], v["pb.cs"], "bf16", "CONVERT")
    assert np.all(v["pb.z"] == 0), "ZERO"
    pad = np.zeros((3, 8))
    pad[:, :5] = v["pb.ps"]
    par.assert_bits(v["pb.pd"], pad, "f32", "CONVERT_PAD")
    assert v["pb.cnt"][0] == 1, "ADD_I32"
    par.assert_bits(v["pb.br"], np.tile(v["pb.row"], (3, 1)), "bf16", "BROADCAST_ROWS")


def _ref_latent(tag):
    def check(v):
        mu, lv, eps = v[tag + ".mu"], v[tag + ".lv"], v[tag + ".eps"]
        B, Cn = mu.shape[0], v[tag + ".sp"].shape[1]
        z, probs, sc = lref.latent_block_fwd(mu, lv, eps, Cn, v[tag + ".st"].astype(np.int64), None, B, 1.0, 0.0, 1.0, float(np.float32(1.0 / B)))
        par.assert_elementwise(v[tag + ".z"], z, "z")
        par.assert_elementwise(v[tag + ".sp"], probs, "style_probs")
        for i, what in enumerate(("KL", "style CE")):
            par.assert_rel(v[tag + ".sc"][i], sc[i], par.LOSS_RTOL, what)
        assert v[tag + ".sc"][2] == sc[2], "style hits"
    return check


def _ref_copy2d(v):
    want = v["c2.s"].copy()
    want[0] = 0
    par.assert_bits(v["c2.d"], want, "f32", "dst")


def _ref_history(v):
    z = v["hf.mu"] + np.exp(v["hf.lv"] / 2) * v["hf.e"]
    par.assert_elementwise(v["hf.z"], z, "z_out")
    par.assert_elementwise(v["hf.h"], np.vstack([np.zeros((1, 4)), z[:3]]), "hist")


def _equal(got, want, what):
    assert got == want, (what, got, want)


# ---- the recurrent baselines: a real recurrent matrix packed by the library, tiled inputs, the float64 recurrence ------------------
F32, BF16 = hl.F32, hl.BF16


def _tile16_offsets(rows, cols):
    """MVAE_TILE16 (include/midivae_hip.h): where element (m, n) of a (rows, cols) array lives"""
    m, n = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return ((m // 16 * (cols // 16) + n // 16) * 64 + ((n % 16) // 4) * 16 + m % 16) * 4 + n % 4


def _from_tile16(a):
    """the row-major reading of a buffer that holds TILE16 data (leading axes folded into the rows)"""
    flat = np.asarray(a).reshape(-1, a.shape[-1])
    return flat.reshape(-1)[_tile16_offsets(*flat.shape)].reshape(a.shape)


def _device_relayout(t, mode):
    """mvae_relayout of a whole tensor (rows = all leading axes); modes as in the header (1 / 3: row-major -> TILE16 / TILE16P)"""
    out = torch.empty_like(t)
    kind = BF16 if t.dtype == torch.bfloat16 else F32
    assert hl.load().mvae_relayout(t.data_ptr(), out.data_ptr(), kind, t.numel() // t.shape[-1], t.shape[-1], mode, _stream()) == 0
    return out


def _tile_in_place(buf, mode):
    """the buffer's values become its LOGICAL content: returns them (float64) and leaves the tiled image in the buffer"""
    logical = fp.host(buf.t)
    buf.t.copy_(_device_relayout(buf.t.clone(), mode))
    return logical


def _pack(buf, cellname, H, kind, direction):
    """a recurrent matrix of the usual scale, packed into ``buf`` by mvae_pack_recurrent; returns what the kernel was handed"""
    G = vo.GATES[cellname]
    U = _t(np.random.default_rng(H + direction).standard_normal((H, G * H)) / np.sqrt(H))
    assert hl.load().mvae_pack_recurrent(U.data_ptr(), buf.t.data_ptr(), hl.CELL_CODE[cellname], H, kind, direction, _stream()) == 0
    torch.cuda.synchronize()
    return par.bf16_round(fp.host(U)) if kind == BF16 else fp.host(U)


def _pre_fwd(cv):
    return dict(U=_pack(cv.bufs["rf.u"], "GRU", 64, F32, 0))


def _ref_fwd(v):
    hs, _, acts = vo.rnn_forward("GRU", v["rf.xp"], v["ctx"]["U"], v["rf.h0"])
    par.assert_parity(v["rf.hs"], hs, F32, par.step_blocks, "hs", values=True)
    par.assert_parity(v["rf.acts"], acts, F32, par.gate_blocks("GRU"), "acts", values=True)
    par.assert_parity(v["rf.hl"], hs[-1], F32, par.whole, "h_last", values=True)


def _pre_bwd(cv):
    return dict(U=_pack(cv.bufs["rb.ut"], "GRU", 64, F32, 1))


def _ref_bwd(v):
    hs, acts, H = v["rb.hs"], v["rb.acts"], 64
    da, _, dh0, _ = vo.rnn_backward("GRU", hs, None, acts, v["ctx"]["U"], v["rb.dhs"], v["rb.dhl"])
    par.assert_parity(v["rb.da"], da, F32, par.gate_blocks("GRU"), "da")
    par.assert_parity(v["rb.dh0"], dh0, F32, par.whole, "dh0")
    par.assert_parity(v["rb.rh"], acts[:, :, H:2 * H] * hs[:-1], F32, par.step_blocks, "rh", values=True)


def _pre_fwd_il(cv):
    return dict(U=_pack(cv.bufs["ril.u"], "LSTM", ac.RH, BF16, 0), xp=_tile_in_place(cv.bufs["ril.xp"], 1))


def _ref_fwd_il(v):
    c, cv = v["ctx"], v["cv"]
    zero = np.zeros((16, ac.RH))
    hs, cs, acts = vo.rnn_forward("LSTM", c["xp"], c["U"], zero, zero)
    par.assert_parity(v["ril.hs"], hs, BF16, par.step_blocks, "hs", values=True)
    par.assert_parity(fp.host(_device_relayout(cv.bufs["ril.acts"].t, 2)), acts, BF16, par.gate_blocks("LSTM"), "acts", values=True)
    par.assert_parity(fp.host(_device_relayout(cv.bufs["ril.cs"].t, 2)), cs, BF16, par.step_blocks, "cs", values=True)
    par.assert_parity(v["ril.hl"], hs[-1], BF16, par.whole, "h_last", values=True)
    par.assert_parity(v["ril.cl"], cs[-1], BF16, par.whole, "c_last", values=True)


def _ref_fwd_multi(v):
    _ref_fwd_il(v)
    name = "mvae_rnn_fwd_multi"          # the expansion that runs inside the launch: out = xs w + bias in TILE16, chunk by chunk
    want = v[name + ".xs"][:, None] * v[name + ".w"][None] + v[name + ".b"][None]
    par.assert_elementwise(_from_tile16(v[name + ".xout"]), want, "xpand out", out_bf16=True)
    assert list(v[name + ".xdone"]) == [4, 4], "one increment per publishing wave and chunk"


def _pre_bwd_il(cv):
    b = cv.bufs
    return dict(U=_pack(b["rbil.ut"], "LSTM", ac.RH, BF16, 1), acts=_tile_in_place(b["rbil.acts"], 3), cs=_tile_in_place(b["rbil.cs"], 3),
                dhs=_tile_in_place(b["rbil.dhs"], 1))


def _ref_bwd_il(v):
    c = v["ctx"]
    da, _, dh0, dc0 = vo.rnn_backward("LSTM", v["rbil.hs"], c["cs"], c["acts"], c["U"], c["dhs"], v["rbil.dhl"])
    par.assert_parity(v["rbil.da"], da, BF16, par.gate_blocks("LSTM"), "da")
    par.assert_parity(v["rbil.dh0"], dh0, BF16, par.whole, "dh0")
    par.assert_parity(v["rbil.dc0"], dc0, BF16, par.whole, "dc0")


# ---- heads, sampler, latent chain, optimizers, the small operators ---------------------------------------------------------------
def _ref_head_probs(v):
    p = vo.softmax(v["hd.hs"] @ v["hd.wt"].T + v["hd.b"])
    par.assert_parity(v["hd.p"], p, F32, par.row_blocks, "probs", values=True)
    assert np.array_equal(v["hd.am"], np.argmax(p, 1)), "argmax"
    return p


def _ref_head(v):
    R = 16
    tgt = v["hd.t"].astype(np.int64)
    p, loss, dl, _ = par.softmax_head_oracle(v["hd.hs"], v["hd.wt"].T, v["hd.b"], tgt, np.ones(R), 1.0)
    _ref_head_probs(v)
    par.assert_parity(v["hd.dl"], dl, F32, par.row_blocks, "dlogits")
    par.assert_rel(v["hd.sc"][0], loss, par.LOSS_RTOL, "loss")
    assert v["hd.sc"][1] == np.sum(np.argmax(p, 1) == tgt), "accuracy count"


def _ref_latent_bwd(v):
    dmu, dlv = lref.latent_block_bwd(v["lb.dz"], v["lb.mu"], v["lb.lv"], v["lb.eps"], None, 0, None, None, 4, 1.0, 0.0, 1.0, 1.0,
                                     float(np.float32(0.25)))
    par.assert_elementwise(v["lb.dmu"], dmu, "dmu")
    par.assert_elementwise(v["lb.dlv"], dlv, "dlogvar")


def _ref_chain_fwd(v):
    mu, lv = v["cf.cat"] @ v["cf.wmu"] + v["cf.bmu"], v["cf.cat"] @ v["cf.wlv"] + v["cf.blv"]
    z, _, sc = lref.latent_block_fwd(mu, lv, v["cf.eps"], 0, None, None, 4, 1.0, 0.0, 1.0, float(np.float32(0.25)))
    for name, want in (("cf.mu", mu), ("cf.lv", lv), ("cf.zh", z), ("cf.S", np.tanh(z @ v["cf.wi"] + v["cf.bi"]))):
        par.assert_elementwise(v[name], want, name)
    par.assert_rel(v["cf.sc"][0], sc[0], par.LOSS_RTOL, "KL")
    assert v["cf.sc"][1] == 0 and v["cf.sc"][2] == 0, "no style head"


def _ref_chain_bwd(v):
    """the chain's backward on the inputs it is handed (transposed matrices; dS comes in as d/dS and leaves as d/d(pre-activation))"""
    dS = v["ctx"]["dS"] * (1 - v["cb.S"] ** 2)
    dzh = dS @ v["cb.wi"]
    dmu, dlv = lref.latent_block_bwd(dzh, v["cb.mu"], v["cb.lv"], v["cb.eps"], None, 0, None, None, 4, 1.0, 0.0, 1.0, 1.0,
                                     float(np.float32(0.25)))
    for name, want in (("cb.dS", dS), ("cb.dzh", dzh), ("cb.dmu", dmu), ("cb.dlv", dlv), ("cb.dcat", dmu @ v["cb.wmu"] + dlv @ v["cb.wlv"])):
        par.assert_elementwise(v[name], want, name)


def _f(x):
    return float(np.float32(x))        # the f32 value the entry point is handed


def _ref_adam(tag, t_word=None):
    def check(v):
        g, b1, b2 = v[tag + ".g"], _f(0.9), _f(0.999)
        m, vv = (1 - b1) * g, (1 - b2) * g * g
        lr_t = _f(1e-3) * np.sqrt(1 - b2) / (1 - b1)
        par.assert_elementwise(v[tag + ".m"], m, "m")
        par.assert_elementwise(v[tag + ".v"], vv, "v")
        par.assert_elementwise(v[tag + ".p"], -lr_t * m / (np.sqrt(vv) + _f(1e-8)), "p")
        if t_word:
            assert v[t_word][0] == 1, "the count of completed steps"
    return check


def _ref_rmsprop(v):
    g = v["rp.g"]
    vv = (1 - _f(0.9)) * g * g
    par.assert_elementwise(v["rp.v"], vv, "v")
    par.assert_elementwise(v["rp.p"], -_f(1e-3) * g / (np.sqrt(vv) + _f(1e-7)), "p")


def _ref_sig_bwd(v):
    out = v["sb.o"]
    want = np.zeros((4, 8))
    want[:, 4:] = v["sb.rw"][:, None] * 2 * (out - v["sb.t"]) / 4 * (1 - out ** 2)
    par.assert_elementwise(v["sb.dz"], want, "dz")
    assert np.all(v["sb.dz"][:, :4] == 0)


def _ref_softmax_bwd(v):
    p, dp = v["sm.p"], v["sm.dp"]
    want = np.zeros((4, 16))
    want[:, :5] = p * (dp - np.sum(p * dp, 1, keepdims=True))
    par.assert_elementwise(v["sm.dl"], want, "dlogits")
    assert np.all(v["sm.dl"][:, 5:] == 0)


PRE = {"mvae_rnn_fwd": _pre_fwd, "mvae_rnn_bwd": _pre_bwd, "mvae_rnn_fwd[TILE16P]": _pre_fwd_il, "mvae_rnn_fwd_multi": _pre_fwd_il,
       "mvae_rnn_bwd[TILE16P]": _pre_bwd_il, "mvae_rnn_bwd_multi": _pre_bwd_il,
       "mvae_latent_chain_bwd": lambda cv: dict(dS=fp.host(cv.bufs["cb.dS"].t))}

REFS = {
    "mvae_rnn_fwd": _ref_fwd, "mvae_rnn_bwd": _ref_bwd, "mvae_rnn_fwd[TILE16P]": _ref_fwd_il, "mvae_rnn_fwd_multi": _ref_fwd_multi,
    "mvae_rnn_bwd[TILE16P]": _ref_bwd_il, "mvae_rnn_bwd_multi": _ref_bwd_il,
    "mvae_head": _ref_head,
    "mvae_head_sample": lambda v: _equal(list(v["hs.out"]), [r % 16 for r in range(16)], "the bin each designed uniform lies in"),
    "mvae_latent_bwd": _ref_latent_bwd, "mvae_latent_chain_fwd": _ref_chain_fwd, "mvae_latent_chain_bwd": _ref_chain_bwd,
    "mvae_adam_step": _ref_adam("ad"), "mvae_adam_step_dev": _ref_adam("dd", "dd.t"), "mvae_rmsprop_step": _ref_rmsprop,
    "mvae_outer_bias_tile16": lambda v: par.assert_elementwise(_from_tile16(v["ob.out"]), v["ob.xs"][:, None] * v["ob.w"][None] + v["ob.b"][None], "out"),
    "mvae_gather2_tile16": lambda v: par.assert_bits(_from_tile16(v["g2.out"]), np.tile(v["g2.t"] + v["g2.u"], (16, 1)), "f32", "out"),
    "mvae_relayout": lambda v: par.assert_bits(_from_tile16(v["rl.d"]), v["rl.s"], "f32", "dst"),
    "mvae_signature_head_fwd": lambda v: par.assert_elementwise(v["sf.o"], np.tanh(v["sf.zh"][:, 4:]), "out"),
    "mvae_signature_head_bwd": _ref_sig_bwd,
    "mvae_softmax_bwd_add": _ref_softmax_bwd,
    "mvae_gemm": _ref_gemm("g", 0, 0, "f32"),
    "mvae_gemm[self-splitting store]": _ref_gemm("gs", 0, 0, "f32"),
    "mvae_gemm[K-streaming]": _ref_gemm("gk", 1, 0, "bf16"),
    "mvae_gemm[persistent chunks]": _ref_gemm("gc", 0, 1, "bf16", out_bf16=True),
    "mvae_gemm_kstream_multi": _ref_gemm("gkm", 1, 0, "bf16"),
    "mvae_gemm_multi": _ref_gemm("gm", 1, 0, "bf16"),
    "mvae_colsum": lambda v: par.assert_product(v["cs.out"], v["cs.X"].sum(0), par.sum_unit(v["cs.X"]), "sum", "out"),
    "mvae_colsum_weighted": lambda v: par.assert_product(v["cw.out"], v["cw.w"] @ v["cw.X"], par.sum_unit(v["cw.X"], v["cw.w"]), "sum", "out"),
    "mvae_sum_over_time": lambda v: par.assert_product(v["st.out"], v["st.X"].sum(0), par.sum_unit(v["st.X"]), "sum", "out"),
    "mvae_prepare_batch": _ref_prep,
    "mvae_latent_fwd": _ref_latent("lf"),
    "mvae_tanh_bwd": lambda v: par.assert_elementwise(v["tb.dx"], v["tb.dy"] * (1 - v["tb.y"] ** 2), "dx"),
    "mvae_convert": lambda v: par.assert_bits(v["cv.d"], v["cv.s"], "bf16", "dst"),
    "mvae_make_table": lambda v: par.assert_bits(v["mt.t"], v["mt.W"] + v["mt.b"], "f32", "table"),
    "mvae_transpose_convert": lambda v: par.assert_bits(v["tc.o"], np.vstack([v["tc.W"].T, np.zeros((3, 3))]), "f32", "out"),
    "mvae_copy2d_f32": _ref_copy2d,
    "mvae_history_from_latent": _ref_history,
    "mvae_bi_concat": lambda v: (par.assert_bits(v["bc.c"], np.concatenate([v["bc.f"], v["bc.r"][::-1]], 2), "f32", "cat"),
                                 par.assert_bits(v["bc.cr"], np.concatenate([v["bc.f"], v["bc.r"][::-1]], 2)[::-1], "f32", "cat_rev")),
    "mvae_add_time_reversed": lambda v: par.assert_bits(v["tr.d"], v["tr.a"] + v["tr.b"][::-1], "f32", "dst"),
    "mvae_scalars_accumulate": lambda v: par.assert_elementwise(v["sc.a"][:4], v["sc.x"][:4] * np.array([1.0, 0.5, 0.5, 0.5]), "acc"),
    "mvae_stream_write_value32": lambda v: _equal(v["sv.w"][0], 5, "the word"),
}


@pytest.mark.parametrize("entry", ac.ENTRIES, ids=[e.label for e in ac.ENTRIES])
def test_baseline_is_accepted_and_stays_inside_its_buffers(entry):
    lib = hl.load()
    cv = _arena(entry)
    ctx = PRE[entry.label](cv) if entry.label in PRE else None
    call = entry.build(cv.resolve)
    rc = call.invoke(lib, _stream())
    cv.ar.fetch()
    assert rc == 0 or (entry.fn in ("mvae_streams_alias", "mvae_occupancy") and rc > 0), (entry.label, rc)
    cv.ar.assert_guards_intact()
    for b in cv.ar.bufs:
        if b.is_output and b.prefill is None and b.t.data_ptr() in _passed(call):
            cv.ar.assert_written(b)
    if entry.label in REFS:
        REFS[entry.label](dict({n: b.values() for n, b in cv.bufs.items()}, ctx=ctx, cv=cv))
    for name, mutate, does in entry.accepted:         # the forms the product relies on: accepted, inside the same buffers
        cv = _arena(entry)
        call = entry.build(cv.resolve)
        mutate(call)
        assert call.invoke(lib, _stream()) == 0, (entry.label, name)
        cv.ar.fetch().assert_guards_intact()
        if does is ac.NOTHING:
            assert _unchanged(cv.ar) is None, (entry.label, name)
        if entry.fn == "mvae_head":              # (with or without targets: the probabilities and the argmax of the same rows)
            _ref_head_probs({n: b.values() for n, b in cv.bufs.items()})


def _passed(call):
    """the addresses a call hands to the library (a spare buffer is not one of them)"""
    seen = {v for _, v in call.args if isinstance(v, int)}
    items = list(call.host) if isinstance(call.host, C.Array) else ([call.host] if call.host is not None else [])
    for x in items + list(getattr(call, "xpand", []) or []):
        seen |= {getattr(x, f) for f, t in x._fields_ if t is hl._vp and getattr(x, f)}
    return seen


SAFE = [e for e in ac.ENTRIES if any(v.safe for v in e.violations)]


@pytest.mark.parametrize("entry", SAFE, ids=[e.label for e in SAFE])
def test_a_refused_call_enqueues_nothing(entry):
    """the device-side reading of "nothing enqueued": the promised code, and every byte of the arena as planted"""
    lib = hl.load()
    cv = _arena(entry)
    failures = []
    for v in entry.violations:
        if not v.safe:
            continue
        call = entry.build(cv.resolve)
        v.mutate(call)
        rc = call.invoke(lib, _stream())
        cv.ar.fetch()
        changed = _unchanged(cv.ar)
        if rc != v.code or changed:
            failures.append("%s, %s: returned %d (promised %d); %s.  Header: \"%s\"" % (entry.label, v.name, rc, v.code, changed or "arena intact", v.why))
            if changed:
                break           # (the arena no longer holds what was planted)
    assert not failures, "\n".join(failures)


def test_the_three_late_refusals_of_the_parent_are_among_the_device_rows():
    rows = {(e.label, v.name) for e in SAFE for v in e.violations if v.safe}
    assert {("mvae_sum_over_time", "kind = 7, accumulate = 0"), ("mvae_gemm[self-splitting store]", "a_kind = 7"),
            ("mvae_prepare_batch", "job 64 of 65: op = 99")} <= rows


# ---- the accepting side of the caps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_jobs", [64, 65, 130])
def test_prepare_batch_at_and_past_one_launch_of_jobs(n_jobs):
    """64 jobs are one launch, 65 two, 130 three (the job offset j0 of the second and third): mixed ops and kinds, every job its own
    destination, bit-equal to the single calls (NumPy for the ops that have none)"""
    lib, s, rng = hl.load(), _stream(), np.random.default_rng(n_jobs)
    J, jobs, keep, checks = hl.PrepJob, [], [], []
    bf, f32 = torch.bfloat16, torch.float32
    U, W, b = _t(rng.standard_normal((64, 192))), _t(rng.standard_normal((5, 64))), _t(rng.standard_normal(64))
    Wn, bn = fp.host(W), fp.host(b)
    keep += [U, W, b]
    counters = torch.zeros(n_jobs, dtype=torch.int32, device=DEV)      # (a word per job: the jobs of a launch run side by side)
    for j in range(n_jobs):
        kind, dt = (hl.BF16, bf) if (j // 8 + j) % 2 else (hl.F32, f32)        # (every op in both kinds)
        op = j % 8
        if op == hl.PREP_PACK_RECURRENT:
            d = (j // 16) % 2
            dst, one = torch.zeros(192 * 64, dtype=dt, device=DEV), torch.zeros(192 * 64, dtype=dt, device=DEV)
            assert lib.mvae_pack_recurrent(U.data_ptr(), one.data_ptr(), hl.GRU, 64, kind, d, s) == 0
            jobs.append(J(op, kind, 64, 192, d, 0, U.data_ptr(), None, dst.data_ptr()))
            checks.append((j, dst, fp.bits_of(one)))
            keep.append(one)
        elif op == hl.PREP_MAKE_TABLE:
            lay = (j // 16) % 2
            dst, one = torch.zeros((5, 64), dtype=dt, device=DEV), torch.zeros((5, 64), dtype=dt, device=DEV)
            assert lib.mvae_make_table(W.data_ptr(), b.data_ptr(), one.data_ptr(), 5, 64, kind, s) == 0
            torch.cuda.synchronize()
            want = fp.bits_of(one)
            jobs.append(J(op, kind, 5, 64, lay, 0, W.data_ptr(), b.data_ptr(), dst.data_ptr()))
            checks.append((j, dst, _paired_columns(want) if lay else want))
            keep.append(one)
        elif op == hl.PREP_TRANSPOSE_CONVERT:
            dst, one = torch.zeros((80, 5), dtype=dt, device=DEV), torch.zeros((80, 5), dtype=dt, device=DEV)
            assert lib.mvae_transpose_convert(W.data_ptr(), one.data_ptr(), 5, 64, 80, kind, s) == 0
            jobs.append(J(op, kind, 5, 64, 80, 0, W.data_ptr(), None, dst.data_ptr()))
            checks.append((j, dst, one))
        elif op == hl.PREP_CONVERT:
            dst, one = torch.zeros(320, dtype=dt, device=DEV), torch.zeros(320, dtype=dt, device=DEV)
            assert lib.mvae_convert(W.data_ptr(), hl.F32, one.data_ptr(), kind, 320, s) == 0
            jobs.append(J(op, kind, 320, 1, 0, 0, W.data_ptr(), None, dst.data_ptr()))
            checks.append((j, dst, one))
        elif op == hl.PREP_ZERO:
            dst = torch.full((6 + 2 * j,), 3.0, dtype=dt, device=DEV)
            jobs.append(J(op, kind, 6 + 2 * j, 1, 0, 0, None, None, dst.data_ptr()))
            checks.append((j, dst, torch.zeros_like(dst)))
        elif op == hl.PREP_CONVERT_PAD:
            dst = torch.full((5, 72), 3.0, dtype=dt, device=DEV)
            want = np.zeros((5, 72))
            want[:, :64] = Wn
            jobs.append(J(op, kind, 5, 64, 72, 0, W.data_ptr(), None, dst.data_ptr()))
            checks.append((j, dst, _t(want, dt)))
        elif op == hl.PREP_ADD_I32:
            jobs.append(J(op, hl.F32, j, 0, 0, 0, None, None, counters.data_ptr() + 4 * j))
            continue
        else:
            dst = torch.full((3 + j % 5, 64), 3.0, dtype=dt, device=DEV)
            jobs.append(J(op, kind, 3 + j % 5, 64, 0, 0, b.data_ptr(), None, dst.data_ptr()))
            checks.append((j, dst, _t(np.tile(bn, (3 + j % 5, 1)), dt)))
        keep.append(dst)
    arr = (J * n_jobs)(*jobs)
    assert lib.mvae_prepare_batch(C.addressof(arr), n_jobs, s) == 0
    torch.cuda.synchronize()
    assert counters.tolist() == [j if j % 8 == hl.PREP_ADD_I32 else 0 for j in range(n_jobs)]
    for j, dst, want in checks:
        fp.assert_same_bits(fp.bits_of(dst), want, "job %d of %d (op %d)" % (j, n_jobs, j % 8))


def _problem_arena(make, n, tag):
    """n problems of one builder, each with buffers of its own, in one arena"""
    cv = Carver()
    for i in range(n):
        make(cv, "%s%d" % (tag, i))
    cv.ar.commit()
    return cv, [make(cv.resolve, "%s%d" % (tag, i)) for i in range(n)]


def test_gemm_multi_takes_sixteen_problems():
    cv, probs = _problem_arena(lambda al, tag: ac._gemm_wgrad(al, tag), 16, "m")
    arr = (hl.GemmArgs * 16)(*probs)
    assert hl.load().mvae_gemm_multi(arr, 16, _stream()) == 0
    cv.ar.fetch().assert_guards_intact()
    for i in range(16):
        A, B = cv.bufs["m%d.A" % i].values().T, cv.bufs["m%d.B" % i].values()
        par.assert_product(cv.bufs["m%d.C" % i].values(), A @ B, par.product_unit(A, B), "bf16", "problem %d" % i)


def _kstream_256(al, tag):
    """32 workgroups: C (512, 1024) += A^T B over one chunk of 64 rows whose counter is at its target"""
    M_, N_, K = 512, 1024, 64
    return hl.GemmArgs(M=M_, N=N_, K=K, trans_a=1, a_kind=hl.BF16, b_kind=hl.BF16, c_kind=hl.F32, lda=M_, ldb=N_, ldc=N_, accumulate=1,
                       split_k=1, alpha=1.0, A=al(tag + ".A", (K, M_), "bf16"), B=al(tag + ".B", (K, N_), "bf16"),
                       C=al(tag + ".C", (M_, N_), "f32", acc=True), k_wait=al(tag + ".kw", (1,), "i32", data=np.ones(1)), k_wait_value=1,
                       k_chunk_rows=K, chunk_status=al(tag + ".st", (1,), "i32", acc=True))


def test_gemm_kstream_multi_takes_eight_problems_and_256_workgroups():
    cv, probs = _problem_arena(_kstream_256, 8, "k")
    arr = (hl.GemmArgs * 8)(*probs)
    assert hl.load().mvae_gemm_kstream_multi(arr, 8, _stream()) == 0
    cv.ar.fetch().assert_guards_intact()
    for i in range(8):
        assert cv.bufs["k%d.st" % i].values()[0] == 0, "a wait timed out"
        A, B = cv.bufs["k%d.A" % i].values().T, cv.bufs["k%d.B" % i].values()
        par.assert_product(cv.bufs["k%d.C" % i].values(), A @ B, par.product_unit(A, B), "bf16", "problem %d" % i)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_phase_launches_take_eight_problems(direction):
    """n = 8 at B = 16, T = 2: "workgroups [base[i], base[i+1]) run problem i with the SAME code as the single launches" - every
    output of the phase launch is bit-equal to the single launch of the same problem (whose values test_ops_gpu.py and
    test_rnn_handover_gpu.py compare with the float64 recurrence)"""
    lib = hl.load()
    make, cls, single, multi = ((ac._fwd_il, hl.RnnFwdArgs, lib.mvae_rnn_fwd, lambda a: lib.mvae_rnn_fwd_multi(a, 8, None, 0, _stream()))
                                if direction == "fwd" else
                                (ac._bwd_il, hl.RnnBwdArgs, lib.mvae_rnn_bwd, lambda a: lib.mvae_rnn_bwd_multi(a, 8, _stream())))
    cv, probs = _problem_arena(lambda al, tag: make(al, tag), 8, "p")
    assert multi((cls * 8)(*probs)) == 0
    cv.ar.fetch().assert_guards_intact()
    outs = [b for b in cv.ar.bufs if b.is_output]
    got = {b.name: b.bits().copy() for b in outs}
    cv2, probs2 = _problem_arena(lambda al, tag: make(al, tag), 8, "p")       # (the same names: the same inputs)
    for p in probs2:
        assert single(C.byref(p), _stream()) == 0
    cv2.ar.fetch().assert_guards_intact()
    for b in cv2.ar.bufs:
        if b.is_output:
            cv2.ar.assert_written(b)
            fp.assert_same_bits(got[b.name], b.bits(), b.name)


@pytest.mark.parametrize("Z", [64, 4])
def test_latent_fwd_with_as_many_classes_as_it_takes(Z):
    """C = Z = 64: both caps of the style classifier at once; C = Z = 4: every latent column is a class"""
    entry = ac.Entry("mvae_latent_fwd", lambda al: ac._latent_fwd(al, Z, Z, "lz"), [])
    cv = _arena(entry)
    assert entry.build(cv.resolve).invoke(hl.load(), _stream()) == 0
    cv.ar.fetch().assert_guards_intact()
    for n in ("lz.z", "lz.sp"):
        cv.ar.assert_written(cv.bufs[n])
    _ref_latent("lz")({n: b.values() for n, b in cv.bufs.items()})
