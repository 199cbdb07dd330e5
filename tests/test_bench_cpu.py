"""bench.py --dump-outputs without a GPU: the files dump_outputs writes for a train and a decode step, their dtypes, and the
seeded sample that keeps a large dump within the limit."""
import os

import numpy as np

import bench


class _FakeEngine:
    def __init__(self, params, notes=None):
        self._params, self._notes = params, notes

    def get_params(self):
        return self._params

    def note_indices(self, B):
        return self._notes[:B]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_train_step_dump_holds_the_losses_of_the_last_step(tmp_path):
    metrics = {"kl": 0.25, "notes_loss": 4.5, "notes_acc": 0.375, "style_loss": 0.5, "style_acc": 0.75, "loss": 5.25}
    bench.dump_outputs(str(tmp_path), _FakeEngine({"enc.notes.0.W": np.ones((4, 4), np.float32)}), 16, False, metrics)
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(["metric.kl", "metric.notes_loss", "metric.style_loss", "metric.loss"])
    for k in ("kl", "notes_loss", "style_loss", "loss"):
        assert got["metric." + k].dtype == np.float64 and got["metric." + k].tolist() == [metrics[k]]


def test_decode_dump_holds_the_note_indices_as_float32(tmp_path):
    notes = np.random.default_rng(1).integers(0, 61, (32, 64)).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), _FakeEngine({}, notes), 20, True, None)
    got = _load(str(tmp_path))
    assert list(got) == ["note_indices"]
    assert got["note_indices"].dtype == np.float32 and np.array_equal(got["note_indices"], notes[:20])


def test_a_dump_over_the_limit_is_a_fixed_sample_within_it(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    notes = np.random.default_rng(2).integers(0, 61, (64, 64)).astype(np.uint8)
    first = None
    for run in ("one", "two"):
        d = str(tmp_path / run)
        bench.dump_outputs(d, _FakeEngine({}, notes), 64, True, None)
        got = _load(d)["note_indices"]
        assert got.dtype == np.float32 and got.nbytes <= 4096 and 0 < got.size < notes.size
        assert np.isin(got, notes).all()
        if first is not None:
            assert np.array_equal(got, first)
        first = got
