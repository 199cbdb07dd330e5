"""midi_vae_amd.rolls without a device: what descriptors, sweep and reconstruction share - the one-copy read-back pack, the closed form
of the velocity post-rule, and the common refusals.

Bounds (derived, not measured).  HostPack moves bytes.  A velocity after the rule is an input float32 or a zero, so the closed form
has the BITS of the reference's outputs in tests/golden/sweep_stats.npz (every window its own song) and tests/golden/recon.npz (the
state carried through a song): no tolerance anywhere."""
import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import descriptors as de
from midi_vae_amd import reconstruction as rec
from midi_vae_amd import rolls
from midi_vae_amd import sweep as sw
from tests import recon_contract, sweep_contract


def test_host_pack_on_the_cpu_device():
    blocks = [("bytes", torch.uint8, (5, 2)), ("table", torch.float64, (5, 22)), ("roll", torch.float32, (5, 16))]
    pack = rolls.HostPack("cpu", blocks)
    lo, hi = pack.pack.data_ptr(), pack.pack.data_ptr() + pack.pack.numel()
    assert pack.pack.dtype == torch.uint8 and pack.pack.numel() == 5 * 22 * 8 + 5 * 16 * 4 + 5 * 2
    spans = []
    for name, dtype, shape in blocks:
        v = pack.views[name]
        assert v.dtype == dtype and tuple(v.shape) == shape and v.is_contiguous()
        assert v.data_ptr() % v.element_size() == 0                                  # aligned to its element
        spans.append((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()))
        assert lo <= spans[-1][0] and spans[-1][1] <= hi                              # one allocation
    spans.sort()
    assert spans[0][0] == lo and spans[-1][1] == hi and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))     # no overlap, no gap
    assert spans[0][1] - spans[0][0] == 5 * 22 * 8 and spans[2][1] - spans[2][0] == 5 * 2      # descending element size
    rng = np.random.default_rng(3)
    want = dict(table=rng.standard_normal((5, 22)), roll=rng.standard_normal((5, 16)).astype(np.float32),
                bytes=rng.integers(0, 256, (5, 2)).astype(np.uint8))
    for name in ("bytes", "roll", "table"):                                           # written in any order, nothing is clobbered
        pack.views[name].copy_(torch.from_numpy(want[name]))
    got = pack.to_host()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    pack.views["table"].zero_()                                                       # the host arrays are copies
    assert np.array_equal(got["table"], want["table"]) and np.all(pack.to_host()["table"] == 0)
    assert np.array_equal(pack.to_host()["roll"], want["roll"]) and np.array_equal(pack.to_host()["bytes"], want["bytes"])


def test_host_pack_takes_a_block_without_rows():
    pack = rolls.HostPack("cpu", [("table", torch.float64, (0, 22)), ("bytes", torch.uint8, (3, 2)), ("roll", torch.float32, (0, 16))])
    assert tuple(pack.views["table"].shape) == (0, 22) and tuple(pack.views["roll"].shape) == (0, 16) and pack.pack.numel() == 6
    pack.views["bytes"].fill_(7)
    got = pack.to_host()
    assert got["table"].shape == (0, 22) and got["table"].dtype == np.float64 and got["roll"].shape == (0, 16)
    assert got["roll"].dtype == np.float32 and np.all(got["bytes"] == 7)
    empty = rolls.HostPack("cpu", [("table", torch.float64, (0, 22))])
    assert empty.pack.numel() == 0 and empty.to_host()["table"].shape == (0, 22)


def _v0(idx, vel, p):
    on = rolls.sounding(idx, p)
    return on, np.where(on, vel, np.float32(0)).astype(np.float32)


def test_carried_velocity_rule_with_every_window_its_own_song():
    fx = sweep_contract.load_fixture()
    p = sw.params(fx["s"])
    on, v0 = _v0(fx["idx"], fx["vel"], p)
    got = rolls.carried_velocity_rule(fx["idx"], on, v0, np.arange(len(fx["idx"])), p)
    assert got.dtype == np.float32 and got.shape == fx["velocity_rules_on"].shape
    assert np.array_equal(got.view(np.uint32), fx["velocity_rules_on"].view(np.uint32))
    assert np.array_equal(v0.view(np.uint32), fx["velocity_rules_off"].view(np.uint32))          # the rule's input is the rule switched off
    assert np.any(got != v0)


def test_carried_velocity_rule_over_songs():
    fx = recon_contract.load_fixture()
    p = rec.params(fx["s"])
    on, v0 = _v0(fx["idx"], fx["vel"], p)
    n = len(fx["idx"])
    got = rolls.carried_velocity_rule(fx["idx"], on, v0, rec.first_windows(fx["lengths"], n), p)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fx["velocity"].view(np.uint32))
    alone = rolls.carried_velocity_rule(fx["idx"], on, v0, np.arange(n), p)
    assert np.any(alone != got)                                                       # the fixture needs the state carried
    assert rolls.carried_velocity_rule(fx["idx"][:0], on[:0], v0[:0], np.arange(0), p).shape == (0, 64)


def test_base_params_are_the_modules_first_keys():
    s = recon_contract.load_fixture()["s"]
    base = rolls.base_params(s)
    assert base == dict(voices=4, n_pitch=60, silent=60)
    assert rolls.base_params(dict(s, include_silent_note=False))["silent"] == -1
    for params in (de.params(dict(s, SMALLEST_NOTE=16)), sw.params(s), rec.params(s)):
        assert list(params)[:3] == list(base) and all(params[k] == base[k] for k in base)


def test_check_rows_and_device_roll_refusals():
    p = dict(voices=4, n_pitch=60, silent=60, threshold=0.5)
    rolls.check_rows(64, p)
    rolls.check_rows(64, dict(voices=4, n_pitch=60, silent=60))                       # the descriptors have no threshold
    rolls.check_rows(64, p, 64, "statistics")
    for T, q, max_T in ((63, p, None), (64, dict(p, voices=1), None), (72, dict(p, voices=9), None), (68, p, 64),
                        (64, dict(p, threshold=float("nan")), None), (64, dict(p, threshold=float("inf")), None)):
        with pytest.raises(ValueError):
            rolls.check_rows(T, q, max_T, "statistics")
    with pytest.raises(ValueError, match=r"rows per window \(63\) must be a multiple of max_voices \(4, 2..8\)"):
        rolls.check_rows(63, p)
    with pytest.raises(ValueError, match=r"rows per window \(68\) above the limit of the song-level decode \(64\)"):
        rolls.check_rows(68, p, 64, "song-level decode")
    with pytest.raises(ValueError, match="the velocity threshold must be finite"):
        rolls.check_rows(64, dict(p, threshold=float("nan")))
    # the intake: every refusal comes before anything touches a device
    two_hot = np.zeros((3, 8, 61))
    two_hot[:, :, 5] = two_hot[:, :, 7] = 1
    with pytest.raises(NotImplementedError):                                          # a host (n, T, K) array that is not one-hot
        rolls.device_roll(two_hot, torch.uint8, "notes")
    with pytest.raises(ValueError):                                                   # a wrong ndim
        rolls.device_roll(np.zeros(8, np.uint8), torch.uint8, "notes")
    with pytest.raises(ValueError):                                                   # indices that do not fit one byte
        rolls.device_roll(np.full((3, 8), 256), torch.uint8, "notes")
    with pytest.raises(ValueError):                                                   # a wrong dtype
        rolls.device_roll(torch.zeros((3, 8), dtype=torch.float32), torch.uint8, "notes")
    with pytest.raises(ValueError):                                                   # a tensor that is not on a device
        rolls.device_roll(torch.zeros((3, 8), dtype=torch.uint8), torch.uint8, "notes")
    with pytest.raises(ValueError):
        rolls.device_roll(torch.zeros((3, 8, 2), dtype=torch.uint8), torch.uint8, "notes")
    with pytest.raises(ValueError, match="velocities have shape"):                    # a host array of another shape than the notes
        rolls.device_roll(np.zeros((3, 7)), torch.float32, "velocities", shape=(3, 8))
    # ... and through the public functions, as before
    fx = sweep_contract.load_fixture()
    with pytest.raises(NotImplementedError):
        sw.window_statistics(two_hot, None, fx["s"])
    with pytest.raises(ValueError):
        de.signature_vectors(np.zeros(8, np.uint8), dict(fx["s"], SMALLEST_NOTE=16))
