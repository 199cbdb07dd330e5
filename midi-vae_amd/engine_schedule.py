"""The schedule state of ONE engine call, in one place (no torch, no GPU).

``CallState`` lives for a whole ``Engine.backward``; ``PhaseState`` for one recurrence phase of a call (the encoder recurrences
of ``encoder_forward``, the decoder recurrences of ``decoder_forward``, each of the two BPTT phases of ``backward``).  The engine
creates one where the call / phase starts (``Engine._scheduling``) and puts a fresh default instance back in a ``finally`` where
it ends, so nothing armed for a call outlives it - not after an exception either (a raised status word, a refused multi launch).
Outside a call the engine holds default instances: every reader finds "nothing armed".

What is NOT here, because it is an argument: the padded batch of the call and the number of recurrences beside a stack are
parameters of the decision functions (_pipelined, _resident_cus, _phase_ok, _kstream_ok, _decoder_kstream_ok,
_fork_with_stack), and "the side heads' queues stay forked" is the ``stay_forked`` argument of decoder_forward / backward.
Persistent engine state (cumulative counters, join sequence numbers, verified call kinds, plan state) stays on the engine."""
from __future__ import annotations


class CallState(object):
    __slots__ = ("deferred_gemms", "deferred_small", "deferred_side", "after_chain", "tail_streams")

    def __init__(self):
        self.deferred_gemms = None      # list: the step collects its weight-gradient GEMMs (armed: backward, _defers_grads; filled: _wgemm; consumed: _flush_deferred_gemms)
        self.deferred_small = []        # ... and the small reductions that go with them (filled: _small; consumed: _flush_deferred_gemms)
        self.deferred_side = None       # list: side-queue work released by a device counter, not an event (armed: backward around the latent block; filled: _side; consumed: _encoder_backward_multi)
        self.after_chain = None         # list: decoder gradient work held back behind the latent chain (armed: backward; filled: _notes_backward_multi, _stack_backward; consumed: _encoder_backward_multi)
        self.tail_streams = []          # queues besides the two gradient queues that carry gradient work (filled: _encoder_backward_multi; consumed: backward's last joins)


class PhaseState(object):
    __slots__ = ("n_side", "grad_streams", "prefork", "hold_side", "kstream_extra", "grad_portion_jobs", "single_slot",
                 "single_slot_end", "top_publish", "last_stack_gate")

    def __init__(self, n_side=0):
        self.n_side = n_side            # recurrences running beside the stack being scheduled (armed: the phase's start; read: callers of _kstream_ok / _decoder_kstream_ok)
        self.grad_streams = None        # (queue, queue) in place of (s_grad, s_grad2) (armed: backward, _encoder_backward_multi beside a K-streaming launch; read: _rec_param_grads_rows)
        self.prefork = None             # (stream, streams already forked from it) (armed: _fork_with_stack; consumed: _fork, once per stream)
        self.hold_side = False          # the side heads' gradient GEMMs wait behind the latent chain (armed: backward; read: _stack_backward)
        self.kstream_extra = None       # list of (problems, gate word, value) of single-layer branches (armed: backward; filled: _stack_backward; consumed: _stack_backward_pipe)
        self.grad_portion_jobs = None   # list of (portion, job) (armed: backward, per-queue schedule; filled: _rec_param_grads; consumed: _flush_grad_portions behind the phase)
        self.single_slot = 0            # next sync slot (11 + it) of a single-layer branch in time portions ...
        self.single_slot_end = 3        # ... and the end of the phase's range (armed: backward - decoder 0..3, encoder 3..5; advanced: _stack_backward)
        self.top_publish = None         # (counters, target, chunk steps) of a top layer that publishes (armed: _pipe_stack_forward; consumed: _head_forward)
        self.last_stack_gate = None     # (word, value): first published chunk of the phase launch's bottom layer (armed: _pipe_stack_forward; consumed: decoder_forward)
