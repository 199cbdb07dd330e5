"""NumPy mirror of the device 'choice' decode (csrc/sample.hip, ``mvae_head_sample``).

Reference counterpart: ``sample_vector(v, 'choice')`` (reference vae_definition.py:1048-1067) - normalise, log(p) / temperature,
softmax, ``np.random.choice`` up to ``number_of_tries`` times until a draw's probability exceeds ``cutoff_sample_threshold``.
``np.random.choice(N, p=q)`` is ``cdf = cumsum(q); cdf /= cdf[-1]; searchsorted(cdf, u, side='right')`` for one uniform ``u``
of the generator; ``choice_index_rows`` applies exactly that rule to whole arrays of rows with the uniforms handed in, in float64.
It is the oracle of the device kernel's tests and a fast host path for probabilities that are on the host already (the per-row
Python loop of ``packers._choice_rows`` stays what it is: it consumes NumPy's global stream draw by draw).

``philox4x32_10`` / ``uniforms`` reproduce the uniforms the kernel generates: key = the 64-bit seed, counter = (global row low
word, global row high word, head id, 0), global row = window * T + t in the CALLER's order, output word i = try i,
u = (word >> 8) * 2^-24 (24-bit uniforms in [0, 1)).
"""
from __future__ import annotations

import numpy as np

MAX_TRIES = 4
# head ids of the Philox counter (word 2): one stream per softmax decoder head
HEAD_IDS = {"notes": 0, "instr": 1, "held": 2, "next": 3}

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter (..., 4), key (..., 2) of 32-bit words (broadcast against each other)
    -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _LO
    k = np.asarray(key, dtype=np.uint64) & _LO
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + np.uint64(_W0)) & _LO
        k1 = (k1 + np.uint64(_W1)) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(seed, head_id, n_windows, T, tries=1, first_window=0):
    """the f32 uniforms the kernel generates for windows first_window .. first_window + n_windows - 1 of ``T`` rows each, in the
    caller's (n, T, tries) order"""
    if not 1 <= int(tries) <= MAX_TRIES:
        raise NotImplementedError("number_of_tries = %r: the device sampler draws 1..%d times per row" % (tries, MAX_TRIES))
    seed = int(seed) & ((1 << 64) - 1)
    rows = (int(first_window) * int(T) + np.arange(int(n_windows) * int(T), dtype=np.uint64))
    ctr = np.stack([rows & _LO, rows >> _S32, np.full(rows.shape, int(head_id), np.uint64), np.zeros(rows.shape, np.uint64)], axis=-1)
    words = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    u = (words[:, :int(tries)] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u.reshape(int(n_windows), int(T), int(tries))


def as_f32_uniforms(u):
    """uniforms in [0, 1) of any float type as float32 in [0, 1): a float64 value within 2^-25 of 1 (np.random.random_sample
    yields one per 2^25 draws) would round to 1.0 - it becomes the largest float32 below 1, the bin it falls into either way.
    Values outside [0, 1) are the caller's error."""
    a = np.asarray(u)
    if not (np.all(a >= 0) and np.all(a < 1)):
        raise ValueError("uniforms must lie in [0, 1)")
    return np.minimum(a.astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))


def tempered(P_or_logits, temperature, from_logits=False):
    """float64 terms e (rows, N) >= 0 and their row sums S: e / S is the distribution ``sample_vector`` draws from -
    softmax(log(p / sum p) / temperature), i.e. softmax(logits / temperature) on softmax outputs.  Zero probabilities stay 0."""
    X = np.asarray(P_or_logits, dtype=np.float64)
    X = X.reshape(-1, X.shape[-1])
    tau = float(temperature)
    if not tau > 0:
        raise ValueError("temperature must be > 0")
    if from_logits:
        e = np.exp((X - X.max(axis=-1, keepdims=True)) / tau)
    else:
        with np.errstate(divide="ignore"):          # (operation by operation what sample_vector does: log(p) <= 0, nothing overflows)
            e = np.exp(np.log(X / (X.sum(axis=-1, keepdims=True) * 1.0)) / tau)
    return e, e.sum(axis=-1)


def choice_index_rows(P_or_logits, u, temperature, tries=1, cutoff=0.0, from_logits=False):
    """Row-wise ``np.random.choice`` draws with the uniforms handed in.  P_or_logits (..., N); u one value per row and try,
    (...,) or (..., tries).  Try i of a row uses u[..., i]; the first draw k whose probability exceeds ``cutoff`` is kept, else the
    last.  Rows of probabilities whose sum is not > 0 give 0 (as the reference).  Returns int64 (...)."""
    X = np.asarray(P_or_logits, dtype=np.float64)
    lead = X.shape[:-1]
    if not 1 <= int(tries) <= MAX_TRIES:
        raise NotImplementedError("number_of_tries = %r: 1..%d draws per row are supported" % (tries, MAX_TRIES))
    flat = X.reshape(-1, X.shape[-1])
    R, N = flat.shape
    U = np.asarray(u, dtype=np.float64).reshape(R, -1)
    if U.shape[1] < tries:
        raise ValueError("%d uniforms per row for %d tries" % (U.shape[1], tries))
    empty = np.zeros(R, bool) if from_logits else ~(flat.sum(axis=-1) > 0)
    if empty.any():
        flat = flat.copy()
        flat[empty] = 1.0
    e, _ = tempered(flat, temperature, from_logits)
    q = e / e.sum(axis=-1, keepdims=True)          # the p np.random.choice is handed
    cdf = np.cumsum(q, axis=-1)
    cdf /= cdf[:, -1:]
    idx = np.zeros(R, np.int64)
    done = np.zeros(R, bool)
    for t in range(int(tries)):
        k = np.minimum((cdf <= U[:, t:t + 1]).sum(axis=-1), N - 1)        # searchsorted(cdf, u, side='right')
        idx = np.where(done, idx, k)
        done |= q[np.arange(R), k] > cutoff
    idx[empty] = 0
    return idx.reshape(lead)


def cdf_bins(P_or_logits, temperature, from_logits=False):
    """normalised float64 CDF (rows, N) of the tempered distribution: bin k is (cdf[k-1], cdf[k]]"""
    e, S = tempered(P_or_logits, temperature, from_logits)
    return np.cumsum(e, axis=-1) / S[:, None]


def control_words(seed, first_window, temperature, cutoff, tries):
    """the 8 32-bit words of the device control block (mvae_sample_ctl) as an int32 array"""
    seed, w0 = int(seed) & ((1 << 64) - 1), int(first_window) & ((1 << 64) - 1)
    out = np.zeros(8, np.uint32)
    out[0], out[1], out[2], out[3] = seed & 0xFFFFFFFF, seed >> 32, w0 & 0xFFFFFFFF, w0 >> 32
    out[4:6] = np.array([temperature, cutoff], np.float32).view(np.uint32)
    out[6] = int(tries)
    return out.view(np.int32)
