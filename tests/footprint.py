"""Which memory a kernel touches: guarded, sentinel-filled buffers carved from one allocation (no test lives here; runs on the CPU
and on the GPU alike - test_footprint_cpu.py checks the checker on planted faults, test_footprint_gpu.py uses it on the kernels).

``Arena(device)`` is ONE flat uint8 allocation.  ``carve(name, shape, dtype)`` reserves a buffer at a 256-byte-aligned offset - the
alignment of a fresh allocation, so misalignment is not a variable - with a guard band in front of it and one behind it: at least
16 rows of the buffer's widest row and at least 64 KiB each, so that every overrun a one-tile masking error can make (a pad row of a
16-row tile, a 128-column tile, a 16-byte vector) lands in memory the test owns.  ``commit()`` allocates and fills.  Buffers carved
one after the other are neighbours: the outputs of one launch guard each other as well.

Before the launch every byte of an OUTPUT and of its guards carries a sentinel no kernel produces:

    f32             bits 0x7FC5A5A5   a quiet NaN with a payload (the canonical NaN is 0x7FC00000)
    bf16            bits 0x7FC5       (canonical: 0x7FC0)
    32-bit words    parity.WORD_SENTINEL
    uint8           0xFF              (no valid column: N <= 192)

They are planted through integer views and compared as integers: NaN != NaN as a float, and a float conversion may canonicalise
the payload (torch's f32 -> bf16 does not keep it).  An INPUT (``data=``) is carved at its exact size with the same sentinel NaNs around it: an
over-read that is USED poisons the result and fails the value check of the test; an over-read that is not used cannot be seen.
Guards around INDEX inputs (``guard="zero"``: idx, target_idx) hold the valid index 0, so that an over-read can never become an
out-of-range gather - which also means over-reads of index arrays are NOT detectable here.  Nothing in this module can make a kernel
fault: no buffer is smaller than its documented size and no index is out of range.

After the launch ``fetch()`` synchronises and copies the arena to the host once; the checks read that copy:

    assert_guards_intact()          every guard byte of every buffer is as planted; names the buffer, the side, the first byte offset
    assert_written(buf, region)     no element of the region still carries the sentinel bits
    assert_untouched(buf, region)   every element of the region still does
    assert_zero(buf, region)        every element of the region is a zero (documented pad)

A region is an index expression on the row-major view of the buffer (default: all of it).  For the tiled layouts the whole buffer
is the region; convert with gpu_util.tile16 only after the check."""
import numpy as np
import torch

from tests import parity as par

F32_SENTINEL, BF16_SENTINEL, BYTE_SENTINEL = 0x7FC5A5A5, 0x7FC5, 0xFF
F32_CANONICAL_NAN, BF16_CANONICAL_NAN = 0x7FC00000, 0x7FC0
ALIGN, MIN_BAND, BAND_ROWS = 256, 64 * 1024, 16

# element type -> (integer view of the same width, NumPy's name for it, sentinel)
_INT_VIEW = {
    torch.float32: (torch.int32, np.uint32, F32_SENTINEL),
    torch.bfloat16: (torch.int16, np.uint16, BF16_SENTINEL),
    torch.int32: (torch.int32, np.uint32, par.WORD_SENTINEL),
    torch.uint8: (torch.uint8, np.uint8, BYTE_SENTINEL),
}


def sentinel_of(dtype):
    return _INT_VIEW[dtype][2]


def _signed(value, np_unsigned):
    """the bit pattern as the integer torch's fill_ takes for the (signed, except uint8) view type"""
    bits = 8 * np.dtype(np_unsigned).itemsize
    return value - (1 << bits) if bits > 8 and value >= 1 << (bits - 1) else value


def host(t):
    """gpu_util.host: a tensor as float64 on the host (NaN payloads survive: bf16 -> f32 is a shift, f32 -> f64 keeps the payload)"""
    return t.detach().float().cpu().numpy().astype(np.float64)


def f32_bits(a):
    """float64 values (as ``host`` returns them) -> the bits of their f32 form"""
    return np.ascontiguousarray(a, np.float64).astype(np.float32).view(np.uint32)


def _round_up(n, m):
    return -(-n // m) * m


class Buf:
    """one carved buffer: ``t`` is the live tensor (after commit), ``bits()`` / ``values()`` read the fetched host copy"""

    def __init__(self, arena, name, shape, dtype, data, guard, start, body, end):
        self.arena, self.name, self.shape, self.dtype, self.data, self.guard = arena, name, tuple(shape), dtype, data, guard
        self.start, self.body, self.end = start, body, end           # byte offsets: region start, first body byte, region end
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        self.t = None

    @property
    def is_output(self):
        return self.data is None

    def bits(self):
        """the body as unsigned integers of the element width, in the buffer's shape, from the fetched copy"""
        raw = self.arena._fetched()
        return raw[self.body:self.body + self.nbytes].view(_INT_VIEW[self.dtype][1]).reshape(self.shape)

    def values(self):
        """the body as float64 from the fetched copy (integers for the integer types)"""
        b = self.bits()
        if self.dtype == torch.float32:
            return b.view(np.float32).astype(np.float64)
        if self.dtype == torch.bfloat16:
            return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return b.astype(np.float64)


class Arena:
    def __init__(self, device="cpu"):
        self.device, self.bufs, self.size, self.flat, self.planted, self.fetched = device, [], 0, None, None, None

    def carve(self, name, shape, dtype, data=None, guard="sentinel", prefill=None, region=None):
        """reserve a buffer.  ``data`` (the buffer's shape): an input - a NumPy array is converted as gpu_util.dev does, a tensor of the
        buffer's type is copied bit for bit; ``prefill``: an OUTPUT whose ``region`` (an index expression; default: all of it) starts
        from these values - what an accumulating kernel adds to - the rest of it sentinels; neither: an output full of sentinels.
        ``guard``: "sentinel", or "zero" for index inputs."""
        assert self.flat is None, "carve before commit"
        assert dtype in _INT_VIEW, dtype
        assert guard in ("sentinel", "zero") and not (guard == "zero" and data is None)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        item = torch.empty(0, dtype=dtype).element_size()
        band = _round_up(max(MIN_BAND, BAND_ROWS * shape[-1] * item), ALIGN)
        start = _round_up(self.size, ALIGN)
        buf = Buf(self, name, shape, dtype, data, guard, start, start + band, 0)
        buf.prefill, buf.region = prefill, region
        buf.end = _round_up(buf.body + buf.nbytes + band, ALIGN)
        self.size = buf.end
        self.bufs.append(buf)
        return buf

    def commit(self):
        """allocate, plant the sentinels, write the inputs; returns self"""
        assert self.flat is None
        raw = torch.zeros(self.size + ALIGN, dtype=torch.uint8, device=self.device)
        skip = -raw.data_ptr() % ALIGN                  # (0 on the device; the host allocator aligns to less)
        self.flat = raw[skip:skip + self.size]
        for b in self.bufs:
            it, npt, sent = _INT_VIEW[b.dtype]
            if b.guard == "sentinel":
                self.flat[b.start:b.end].view(it).fill_(_signed(sent, npt))
            body = self.flat[b.body:b.body + b.nbytes]
            b.t = body.view(b.dtype).reshape(b.shape)
            src = b.data if b.data is not None else b.prefill
            if src is not None:
                dst = b.t if b.data is not None or b.region is None else b.t[b.region]
                if isinstance(src, torch.Tensor):
                    assert src.dtype == b.dtype, (b.name, src.dtype)
                else:
                    src = torch.as_tensor(np.ascontiguousarray(src)).to(b.dtype)
                assert tuple(src.shape) == tuple(dst.shape), (b.name, tuple(src.shape), tuple(dst.shape))
                dst.copy_(src)
        assert self.flat.data_ptr() % ALIGN == 0
        self.planted = self.flat.cpu().numpy().copy()
        return self

    def fetch(self):
        """after the launch: wait for the device, copy the arena to the host; the checks read this copy"""
        if self.flat.is_cuda:
            torch.cuda.synchronize()
        self.fetched = self.flat.cpu().numpy().copy()
        return self

    def _fetched(self):
        assert self.fetched is not None, "fetch() after the launch, before the checks"
        return self.fetched

    # ---- checks ------------------------------------------------------------------------------------------------------------
    def assert_guards_intact(self):
        raw = self._fetched()
        for b in self.bufs:
            for side, lo, hi in (("before", b.start, b.body), ("after", b.body + b.nbytes, b.end)):
                bad = np.nonzero(raw[lo:hi] != self.planted[lo:hi])[0]
                if bad.size:
                    at = int(bad[0]) - (hi - lo) if side == "before" else int(bad[0])
                    raise AssertionError("guard of '%s' overwritten: %d bytes %s the buffer, first at byte offset %+d %s (value 0x%02X)"
                                         % (b.name, bad.size, side, at,
                                            "from its start" if side == "before" else "past its end", int(raw[lo + bad[0]])))

    def _region(self, buf, region):
        bits = buf.bits()
        sel = bits if region is None else bits[region]
        return bits, np.asarray(sel), sentinel_of(buf.dtype)

    def _first(self, buf, bits, region, mask_sel):
        """index, in the whole buffer, of the first element of the region where mask_sel holds"""
        where = np.zeros(bits.shape, bool)
        if region is None:
            where[...] = mask_sel
        else:
            where[region] = mask_sel
        return tuple(int(i) for i in np.argwhere(where)[0])

    def assert_written(self, buf, region=None):
        assert buf.is_output and buf.prefill is None, "%s was not sentinel-filled" % buf.name
        bits, sel, sent = self._region(buf, region)
        assert sel.size, "empty region of '%s'" % buf.name
        left = sel == sent
        if left.any():
            raise AssertionError("'%s': %d of %d elements of the region were never written, first at %s"
                                 % (buf.name, int(left.sum()), left.size, self._first(buf, bits, region, left)))

    def assert_untouched(self, buf, region=None):
        assert buf.is_output, "%s was not sentinel-filled" % buf.name
        bits, sel, sent = self._region(buf, region)
        hit = sel != sent
        if hit.any():
            raise AssertionError("'%s': %d of %d elements of a region no kernel may touch were overwritten, first at %s (bits 0x%X)"
                                 % (buf.name, int(hit.sum()), hit.size, self._first(buf, bits, region, hit), int(sel[hit][0])))

    def assert_zero(self, buf, region=None):
        """documented pad: written, and a zero of the element type"""
        bits, sel, sent = self._region(buf, region)
        assert sel.size, "empty region of '%s'" % buf.name
        magnitude = {torch.float32: 0x7FFFFFFF, torch.bfloat16: 0x7FFF}.get(buf.dtype, int(np.iinfo(sel.dtype).max))
        bad = (sel & sel.dtype.type(magnitude)) != 0          # (-0.0 is a zero)
        if bad.any():
            raise AssertionError("'%s': %d of %d pad elements are not zero, first at %s (bits 0x%X)"
                                 % (buf.name, int(bad.sum()), bad.size, self._first(buf, bits, region, bad), int(sel[bad][0])))


def bits_of(t):
    """a tensor as unsigned integers of its element width, on the host"""
    return t.detach().contiguous().view(_INT_VIEW[t.dtype][0]).cpu().numpy().view(_INT_VIEW[t.dtype][1])


def assert_same_bits(got, want, what):
    """two runs of one kernel: ``got`` (a Buf or an integer array) and ``want`` (a tensor or an integer array) hold the same bits"""
    g = got.bits() if isinstance(got, Buf) else np.asarray(got)
    w = bits_of(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    diff = g != w
    assert not diff.any(), "%s: %d of %d elements differ between the arena run and the tight zero-filled run, first at %s: 0x%X vs 0x%X" % (
        what, int(diff.sum()), diff.size, tuple(int(i) for i in np.argwhere(diff)[0]), int(g[diff][0]), int(w[diff][0]))
