"""What becomes of a decode: one sink per public method of model.Decoder.  ``Decoder._run`` hands every engine batch to
``sink.batch(eng, lo, hi, views)`` - ``views`` is ``Engine.decoded(...)``, the first ``hi - lo`` columns are the caller's windows
``lo .. hi`` - and returns ``sink.result()``; ``want_probs`` / ``want_velocity`` are what the sink asks of ``Engine.decode``.  What a
sink enqueues runs behind the decode on its stream, outside the step plans.  Every sink owns its result for no windows at all.
"""
from __future__ import annotations

import numpy as np

from . import descriptors
from . import sweep


def _joined(parts, keys):
    return {k: np.concatenate([d[k] for d in parts], 0) for k in keys}


class Sink(object):
    want_probs = want_velocity = False

    def __init__(self, **own):
        self.parts = []
        self.__dict__.update(own)


class Probabilities(Sink):
    """predict: per engine batch the dict head -> probabilities of Engine.outputs"""
    want_probs = True

    def batch(self, eng, lo, hi, views):
        self.parts.append(eng.outputs(hi - lo))

    def result(self):
        return self.parts


class NoteIndices(Sink):
    """predict_note_indices (``T``): (n, T) uint8"""

    def batch(self, eng, lo, hi, views):
        self.parts.append(eng.rows_to_host(views["notes"], hi - lo))

    def result(self):
        return np.concatenate(self.parts, 0) if self.parts else np.zeros((0, self.T), np.uint8)


class AllIndices(Sink):
    """predict_indices: dict head -> indices of every softmax head, plus 'velocity' where the model has the head"""
    want_velocity = True

    def batch(self, eng, lo, hi, views):
        self.parts.append({k: eng.rows_to_host(v, hi - lo) for k, v in views.items()})

    def result(self):
        return _joined(self.parts, self.parts[0]) if self.parts else {}


class Descriptors(Sink):
    """predict_descriptors (``p``, ``T``): the descriptor kernels read the decode's own note buffer; one read per engine batch"""

    def batch(self, eng, lo, hi, views):
        self.parts.append(descriptors.decoded_batch(views["notes"], hi - lo, self.p))

    def result(self):
        if self.parts:
            return _joined(self.parts, ("notes", "signature", "harmonicity"))
        V = self.p["voices"]
        return dict(notes=np.zeros((0, self.T), np.uint8), signature=np.zeros((0, descriptors.SIGNATURE_LENGTH)),
                    harmonicity=np.zeros((0, V, V)))


class SweepStatistics(Sink):
    """latent_sweep (``p``, ``T``, ``return_rolls``): the statistics kernel reads the decode's note, velocity and instrument buffers.
    dict ``table`` (n, 22), ``instr`` (n, V) or None for a model without the head and, with ``return_rolls``, ``notes`` (n, T) uint8
    and ``velocity`` (n, T) float32 after the rules"""
    want_velocity = True

    def batch(self, eng, lo, hi, views):
        self.parts.append(sweep.decoded_batch(views["notes"], views.get("velocity"), views.get("instr"), hi - lo, self.p,
                                              self.return_rolls))

    def result(self):
        res = dict(table=np.zeros((0, sweep.N_COLUMNS)), instr=None)
        if self.return_rolls:
            res.update(notes=np.zeros((0, self.T), np.uint8), velocity=np.zeros((0, self.T), np.float32))
        if self.parts:
            res.update(_joined(self.parts, [k for k, v in self.parts[0].items() if v is not None]))
        return res


class JudgedSweepStatistics(SweepStatistics):
    """latent_sweep with ``judges`` (style.Judges): SweepStatistics, and behind every engine batch the three style classifiers read
    the decode's note and instrument buffers and the velocities after the rules (a second launch of the statistics kernel that
    only writes them) on the device; the class-0 probabilities of the whole run stay there until ``result`` reads them once.
    ``style`` (n, 3) float32, a NaN column where the model lacks the head or the judge is absent"""

    def batch(self, eng, lo, hi, views):
        import torch
        SweepStatistics.batch(self, eng, lo, hi, views)
        B, rows, vel = hi - lo, views["notes"], views.get("velocity")
        after = None
        with torch.cuda.device(rows.device):
            if vel is not None:
                after = torch.empty((B, rows.shape[0]), dtype=torch.float32, device=rows.device)
                sweep.enqueue(rows[:, :B].t(), vel[:, :B].t(), self.p, None, after, torch.cuda.current_stream().cuda_stream)
            instr = views["instr"][:, :B].t() if "instr" in views else None
            tables = self.judges.probabilities(rows[:, :B].t(), after, instr, self.batch_size)
            col = torch.full((B, 3), float("nan"), dtype=torch.float32, device=rows.device)
            for j, t in enumerate(tables):
                if t is not None:
                    col[:, j].copy_(t[:, 0])
        self.style.append(col)

    def result(self):
        import torch
        res = SweepStatistics.result(self)
        res["style"] = torch.cat(self.style, 0).cpu().numpy() if self.style else np.zeros((0, 3), np.float32)
        return res


class SongRolls(Sink):
    """predict_songs: every engine batch's buffers are copied - transposed, on the device - into window-major rolls of the
    whole run (a song may straddle engine batches); nothing is read back.  dict of device tensors ``notes`` (n, T) uint8 and, as far as
    the model has the heads, ``velocity`` (n, T) float32, ``held`` (n, T) uint8 and ``instr`` (n, V) uint8."""
    want_velocity = True

    def __init__(self, n):
        Sink.__init__(self, n=n, rolls={})

    def _copy(self, eng, views, count, rows):
        """the first ``count`` columns of every buffer of ``views`` to the rows ``rows`` of its roll, allocated on first sight"""
        import torch
        for k in ("notes", "velocity", "held", "instr"):
            if k in views:
                if k not in self.rolls:
                    self.rolls[k] = torch.empty((self.n, views[k].shape[0]), dtype=views[k].dtype, device=eng.device)
                self.rolls[k][rows].copy_(views[k][:, :count].t())

    def batch(self, eng, lo, hi, views):
        self._copy(eng, views, hi - lo, slice(lo, hi))

    def result(self):
        return self.rolls


class LockstepRolls(SongRolls):
    """long_songs: S songs of ``length`` windows decode in lockstep, one window of every song per engine batch; the rolls of the run
    stay song-contiguous - window ``it`` of song ``s`` is row ``s * length + it`` - so a batch's columns go to every length-th row"""

    def __init__(self, songs, length):
        SongRolls.__init__(self, songs * length)
        self.length = length

    def batch_at(self, eng, it, first_song, count, views):
        self._copy(eng, views, count, slice(first_song * self.length + it, (first_song + count) * self.length, self.length))
