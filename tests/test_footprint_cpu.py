"""The footprint checker (tests/footprint.py) checked without a GPU: NumPy and torch-CPU "kernels" with planted faults stand in for
the device.  The fake kernel computes out[:, :N] = 2 x, out[:, N:NP] = 0 into rows of ``ld`` > NP elements (columns [NP, ld) are a
gap no kernel may touch) and an argmax byte per row beside it - the shape of a head's outputs.  A correct one passes every check;
one element a row past the end, one before the start, a pad column left unwritten and a gap column overwritten each fail the
matching check with a message that names the buffer (and the offset)."""
import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import parity as par

R, N, NP, LD = 21, 7, 16, 20
TYPES = [torch.float32, torch.bfloat16]


def _arena(dtype):
    x = np.random.default_rng(3).standard_normal((R, N))
    ar = fp.Arena("cpu")
    b = dict(x=ar.carve("x", (R, N), dtype, data=x), out=ar.carve("out", (R, LD), dtype), am=ar.carve("am", (R,), torch.uint8),
             idx=ar.carve("idx", (R,), torch.uint8, data=np.arange(R) % N, guard="zero"),
             words=ar.carve("words", (4,), torch.int32))
    ar.commit()
    return ar, b, x


def _kernel_numpy(ar, b, fault=None):
    """writes through the raw bytes of the arena, as a device kernel would through its pointers"""
    raw = ar.flat.numpy()
    out, item = b["out"], b["out"].t.element_size()
    view = raw[out.body - 64 * item:out.body + out.nbytes + 64 * item].view(np.uint16 if item == 2 else np.uint32)
    lead, view = view[:64], view[64:]                # 64 elements in front of the buffer; the buffer and 64 behind it
    x = fp.host(b["x"].t)
    val = torch.as_tensor(2.0 * x).to(out.dtype).view(torch.int16 if item == 2 else torch.int32).numpy().view(view.dtype)
    npad = NP - 1 if fault == "pad column unwritten" else NP
    for r in range(R):
        view[r * LD:r * LD + N] = val[r]
        view[r * LD + N:r * LD + npad] = 0
    if fault == "row past the end":
        view[R * LD + 3] = val[0, 3]
    if fault == "before the start":
        lead[-1] = val[0, 0]
    if fault == "gap column overwritten":
        view[5 * LD + NP] = 0
    raw[b["am"].body:b["am"].body + R] = np.argmax(x, 1)
    raw[b["words"].body:b["words"].body + 8].view(np.uint32)[:] = (3, 4)


def _kernel_torch(ar, b, fault=None):
    out = b["out"].t
    out[:, :N] = (2.0 * b["x"].t.float()).to(out.dtype)
    out[:, N:NP - 1 if fault == "pad column unwritten" else NP] = 0
    flat = ar.flat[b["out"].body - 256:b["out"].body + b["out"].nbytes + 256].view(out.dtype)
    lead = 256 // out.element_size()
    if fault == "row past the end":
        flat[lead + R * LD + 3] = 1.5
    if fault == "before the start":
        flat[lead - 1] = 1.5
    if fault == "gap column overwritten":
        out[5, NP] = 0.0
    b["am"].t.copy_(torch.argmax(b["x"].t.float(), 1).to(torch.uint8))
    b["words"].t[:2] = torch.tensor([3, 4], dtype=torch.int32)


def _check(ar, b, x):
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(b["out"], np.s_[:, :N])
    ar.assert_zero(b["out"], np.s_[:, N:NP])
    ar.assert_untouched(b["out"], np.s_[:, NP:])
    ar.assert_written(b["am"])
    ar.assert_written(b["words"], np.s_[:2])
    ar.assert_untouched(b["words"], np.s_[2:])
    storage = "bf16" if b["out"].dtype == torch.bfloat16 else "f32"
    par.assert_bits(b["out"].values()[:, :N], 2.0 * fp.host(b["x"].t), storage, "out")
    assert np.array_equal(b["am"].bits(), np.argmax(x, 1))


KERNELS = [_kernel_numpy, _kernel_torch]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", TYPES)
def test_a_correct_kernel_passes_every_check(kernel, dtype):
    ar, b, x = _arena(dtype)
    kernel(ar, b)
    _check(ar, b, x)
    # ... and the run is bit-identical to one into a tight zero-filled buffer
    tight = torch.zeros((R, LD), dtype=dtype)
    tight[:, :N] = (2.0 * b["x"].t.float()).to(dtype)
    fp.assert_same_bits(b["out"].bits()[:, :NP], tight[:, :NP].contiguous(), "out")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("fault,message", [
    ("row past the end", r"guard of 'out' overwritten: \d+ bytes after the buffer, first at byte offset \+%d past its end"),
    ("before the start", r"guard of 'out' overwritten: \d+ bytes before the buffer, first at byte offset -%d from its start"),
    ("pad column unwritten", r"'out': 21 of \d+ pad elements are not zero, first at \(0, 15\)"),
    ("gap column overwritten", r"'out': 1 of \d+ elements of a region no kernel may touch were overwritten, first at \(5, 16\)"),
])
def test_every_planted_fault_is_caught_and_named(kernel, dtype, fault, message):
    ar, b, x = _arena(dtype)
    kernel(ar, b, fault)
    item = b["out"].t.element_size()
    if "%d" in message:
        message = message % (3 * item if fault == "row past the end" else item)
    with pytest.raises(AssertionError, match=message):
        _check(ar, b, x)


def test_an_unwritten_element_and_a_stale_sentinel_are_told_apart():
    ar, b, x = _arena(torch.float32)
    _kernel_numpy(ar, b)
    b["am"].t[R - 1] = fp.BYTE_SENTINEL                   # "argmax" of the last row never stored
    with pytest.raises(AssertionError, match=r"'am': 1 of 21 elements of the region were never written, first at \(20,\)"):
        _check(ar, b, x)
    with pytest.raises(AssertionError, match="fetch"):
        fp.Arena("cpu").carve("a", (4,), torch.float32).arena.commit().assert_guards_intact()


def test_guards_of_index_inputs_hold_a_valid_index_and_are_watched_too():
    ar, b, x = _arena(torch.float32)
    raw = ar.flat.numpy()
    i = b["idx"]
    assert not raw[i.start:i.body].any() and not raw[i.body + R:i.end].any()
    assert np.array_equal(raw[i.body:i.body + R], np.arange(R) % N)
    _kernel_numpy(ar, b)
    raw[i.body + R + 40] = 9
    with pytest.raises(AssertionError, match=r"guard of 'idx' overwritten: 1 bytes after the buffer, first at byte offset \+40"):
        _check(ar, b, x)


def test_layout_alignment_and_band_sizes():
    ar = fp.Arena("cpu")
    small = ar.carve("small", (3,), torch.uint8)
    wide = ar.carve("wide", (5, 4096), torch.float32)
    ar.commit()
    assert ar.flat.data_ptr() % 256 == 0
    for b in (small, wide):
        assert b.t.data_ptr() % 256 == 0 and b.t.is_contiguous()
        row = b.shape[-1] * b.t.element_size()
        assert b.body - b.start >= max(64 * 1024, 16 * row) and b.end - (b.body + b.nbytes) >= max(64 * 1024, 16 * row)
    assert wide.body - wide.start == 16 * 4096 * 4 and small.end <= wide.start


def test_sentinels_are_not_the_canonical_nans_and_survive_the_round_trip_as_bits():
    assert fp.F32_SENTINEL != fp.F32_CANONICAL_NAN and fp.BF16_SENTINEL != fp.BF16_CANONICAL_NAN
    assert np.isnan(np.array([fp.F32_SENTINEL], np.uint32).view(np.float32)[0])
    assert np.array([float("nan")], np.float32).view(np.uint32)[0] & 0x7FFFFFFF == fp.F32_CANONICAL_NAN
    ar = fp.Arena("cpu")
    f, h, w, u = (ar.carve(n, (5, 3), dt) for n, dt in (("f", torch.float32), ("h", torch.bfloat16), ("w", torch.int32), ("u", torch.uint8)))
    ar.commit().fetch()
    for b, sent in ((f, fp.F32_SENTINEL), (h, fp.BF16_SENTINEL), (w, par.WORD_SENTINEL), (u, 0xFF)):
        assert np.all(b.bits() == sent) and fp.sentinel_of(b.dtype) == sent
        ar.assert_untouched(b)
    # host(): device -> float64 keeps the payload (bf16 -> f32 is a shift)
    assert np.all(fp.f32_bits(fp.host(f.t)) == fp.F32_SENTINEL)
    assert np.all(fp.f32_bits(fp.host(h.t)) == fp.BF16_SENTINEL << 16)
    assert np.all(fp.f32_bits(f.values()) == fp.F32_SENTINEL) and np.all(fp.f32_bits(h.values()) == fp.BF16_SENTINEL << 16)
    # dev(): float64 -> f32 keeps it as well; float -> bf16 does NOT keep a NaN's payload, which is why sentinels go in through integer views
    back = torch.as_tensor(fp.host(f.t)).to(torch.float32)
    assert np.all(back.view(torch.int32).numpy().view(np.uint32) == fp.F32_SENTINEL)
    assert np.all(torch.as_tensor(fp.host(h.t)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16) != fp.BF16_SENTINEL)
