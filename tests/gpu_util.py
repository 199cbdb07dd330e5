"""What the operator-level GPU test files share (test_ops_gpu.py, test_rnn_handover_gpu.py): host <-> device copies, the device
relayouts, the NumPy definitions of the paired lookup-table layouts, two streams on different hardware queues, a region without
host synchronisation, and the ``close`` check.  No test lives here: importing ``test_*`` functions across test modules would
collect them twice."""
import contextlib
import gc

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import ops

DEV = "cuda:0"

_KEEP_STREAMS = []


def two_queues():
    """two streams on DIFFERENT hardware queues.  The runtime deals streams onto GPU_MAX_HW_QUEUES queues as they are first used, and
    two pool streams taken one after the other can land on one queue: a kernel that WAITS on the first for work enqueued on the second
    then waits until its time-out (status 4).  That is what made the live-producer tests fail in one full-suite run of three in
    round 6 - never alone: it depends on how many streams the process has used before.  Asked of the runtime by experiment, as the
    engine does for its own streams (Engine._own_queue_stream, mvae_streams_alias)."""
    s1 = torch.cuda.Stream()
    scratch = torch.zeros(2, dtype=torch.int32, device=DEV)
    for attempt in range(1, 17):
        s2 = torch.cuda.Stream()
        rc = hl.load().mvae_streams_alias(s1.cuda_stream, s2.cuda_stream, scratch.data_ptr(), attempt)
        if rc == 0:
            return s1, s2
        hl.check(min(rc, 0), "mvae_streams_alias")
        _KEEP_STREAMS.append(s2)                 # (kept alive: a released stream's queue slot would be dealt again)
    pytest.skip("no two streams of this process run beside each other (kernels are being run one at a time)")


@contextlib.contextmanager
def no_host_sync():
    """Between the launch of a WAITING kernel and the last chunk its producer publishes the host must not synchronise with the device:
    a garbage collection that releases an earlier test's engine (pinned staging mirrors: hipHostFree waits for the device) would block
    until the waiter gives up (status 4).  (A precaution; what DID fail these tests in round 6 was two_queues()'s subject.)"""
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


def dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def tile16(t, rows, cols, to_tile, paired=False):
    """device relayout of a (rows, cols) view between row-major and TILE16 / TILE16P (returns a new tensor, same shape)"""
    out = torch.empty_like(t)
    ops.relayout(t.contiguous(), out, rows, cols, to_tile, paired=paired)
    return out


def pairing(lay):
    """the ``paired`` argument of tile16() / ops.relayout for a sequence layout's saved activations"""
    return "q" if lay == hl.TILE16Q else lay == hl.TILE16P


def close(got, want, tol, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bound = tol * (1.0 + np.abs(want))
    assert np.all(err <= bound), "%s: max err %.3e (tol %.1e) at %s" % (
        what, err.max(), tol, np.unravel_index(np.argmax(err - bound), err.shape))


def _paired8_columns(table):
    """MVAE_TABLE_PAIRED8: inside every block of 256 columns, column 128 h + 16 j + 4 q + e moves to 32 j + 8 q + 4 h + e"""
    K, N = table.shape
    c = np.arange(N)
    dst = (c & ~255) + ((c >> 4) & 7) * 32 + ((c & 15) >> 2) * 8 + ((c >> 7) & 1) * 4 + (c & 3)
    out = np.empty_like(table)
    out[:, dst] = table
    return out


def _paired_columns(table):
    """MVAE_TABLE_PAIRED: inside every block of 32 columns, column 16 h + 4 q + e moves to 8 q + 4 h + e"""
    K, N = table.shape
    c = np.arange(N)
    dst = (c & ~31) + ((c & 15) >> 2) * 8 + ((c >> 4) & 1) * 4 + (c & 3)
    out = np.empty_like(table)
    out[:, dst] = table
    return out
