"""'choice' decode, the parts that need no GPU: the NumPy mirror of the device sampler (midi_vae_amd/sampling.py) against
published Philox vectors and against np.random.choice itself, process_decoder_indices against process_decoder_outputs, the
ctypes mirror of the new argument struct against the header, argument validation, and the seeds the GPU tests use (the
mirror alone must satisfy their caps: tests/test_choice_decode_gpu.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from midi_vae_amd import packers, sampling
from midi_vae_amd.config import build_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- shared with the GPU tests: the generated-uniform cases and the exclusion rule ---------------------------------------


def boundary_delta(N):
    """|u - cdf_j| below this (normalised CDF) = the f32 path may land in the neighbouring bin: one f32 rounding of every term's
    exponent argument (x e^-x <= 0.37), v_exp_f32's ~1e-6 relative error, one rounding per addition of the scan"""
    return (2 * N + 16) * 2.0 ** -23


def excluded_rows(cdf, u, N):
    """rows whose uniform lies within boundary_delta of a float64 CDF boundary - named by the oracle alone"""
    return (np.abs(cdf - np.asarray(u, np.float64).reshape(-1, 1)) <= boundary_delta(N)).any(axis=-1)


def integer_problem(R, H, N, seed):
    """small-integer hs / W / bias: logits exact in f32 and bf16 (|values| <= 4, sums far below 2^8 ... 2^24)"""
    rng = np.random.default_rng(seed)
    hs = rng.integers(-2, 3, (R, H)).astype(np.float32)
    W = np.zeros((H, N), np.float32)
    for j in range(N):          # a few non-zero weights per column: logits of a handful of units, a spread of probabilities
        W[rng.integers(0, H, 3), j] = rng.integers(-1, 2, 3)
    bias = rng.integers(-2, 3, N).astype(np.float32)
    return hs, W, bias, hs.astype(np.float64) @ W.astype(np.float64) + bias


GENERATED_CASES = [(61, 4100, 64, 20240917, 1, 5), (192, 1500, 64, 77, 3, 0), (17, 700, 256, 5, 0, 123456789)]     # N, R, H, seed, head, window0
DISTRIBUTION_SEED = 424242


def distribution_row():
    rng = np.random.default_rng(3)
    return rng.integers(-4, 5, 61).astype(np.float64)


# ---- Philox ---------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in sampling.philox4x32_10(np.array(ctr), np.array(key))) == want
    # vectorised over rows: the same values row by row
    ctrs = np.array([k[0] for k in kat])
    keys = np.array([k[1] for k in kat])
    assert np.array_equal(sampling.philox4x32_10(ctrs, keys), np.array([k[2] for k in kat], np.uint32))


def test_uniforms_layout_and_range():
    u = sampling.uniforms(seed=(7 << 40) + 3, head_id=2, n_windows=5, T=8, tries=3, first_window=2)
    assert u.shape == (5, 8, 3) and u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    # a window's values depend on its index only, try i is output word i, 24 bits
    whole = sampling.uniforms((7 << 40) + 3, 2, 7, 8, 4)
    assert np.array_equal(whole[2:, :, :3], u)
    w = sampling.philox4x32_10(np.array([3 * 8 + 5, 0, 2, 0]), np.array([3, 7 << 8]))
    assert np.array_equal(whole[3, 5], (w >> 8).astype(np.float32) * np.float32(2.0 ** -24))
    assert np.all(whole * 2.0 ** 24 == np.round(whole * 2.0 ** 24))
    assert not np.array_equal(sampling.uniforms(1, 0, 2, 8), sampling.uniforms(1, 1, 2, 8))
    with pytest.raises(NotImplementedError, match="number_of_tries"):
        sampling.uniforms(1, 0, 2, 8, tries=5)


# ---- the draw rule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_choice_index_rows_is_np_random_choice(tau):
    """the reference's call chain row by row (np.random.seed; np.random.choice(N, p=tempered(P[i]))) against ONE
    random_sample(R) after the same seed: every row equal"""
    N, R = 61, 2000
    rng = np.random.default_rng(5)
    P = rng.dirichlet(np.full(N, 0.3), R).astype(np.float32).astype(np.float64)
    np.random.seed(11)
    want = []
    for row in P:
        p = row / (np.sum(row) * 1.0)
        p = np.log(p) / tau
        p = np.exp(p) / np.sum(np.exp(p))
        want.append(np.random.choice(N, p=p))
    np.random.seed(11)
    u = np.random.random_sample(R)
    got = sampling.choice_index_rows(P, u, tau)
    assert np.array_equal(got, np.array(want))


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_choice_index_rows_is_sample_notes_prediction(tau):
    N, R = 61, 2000
    s = build_settings(temperature=tau, number_of_tries=1, cutoff_sample_threshold=0.0)
    rng = np.random.default_rng(6)
    Y = rng.dirichlet(np.full(N, 0.3), R).astype(np.float32).astype(np.float64).reshape(R // 50, 50, N)
    np.random.seed(11)
    want = packers.sample_notes_prediction(s, Y, "choice")
    np.random.seed(11)
    u = np.random.random_sample(R)
    got = packers.notes_from_indices(s, sampling.choice_index_rows(Y, u.reshape(R // 50, 50), tau), N)
    assert np.array_equal(got, want)


def test_edge_uniforms_and_zero_probability_columns():
    one_below = float(np.nextafter(np.float32(1), np.float32(0)))
    P = np.array([[0.0, 0.0, 0.25, 0.0, 0.5, 0.25, 0.0, 0.0]])
    for tau in (0.5, 1.0, 2.0):
        assert sampling.choice_index_rows(P, [0.0], tau) == 2             # u = 0: the first column that has probability
        assert sampling.choice_index_rows(P, [one_below], tau) == 5       # the last one that has: never a trailing zero column
    assert sampling.choice_index_rows(P, [0.25], 1.0) == 4                # a boundary belongs to the bin above (side='right'),
    assert sampling.choice_index_rows(P, [0.2499999], 1.0) == 2           # ... and the zero column 3 is skipped
    assert sampling.choice_index_rows(P, [0.75], 1.0) == 5
    lg = np.log(np.array([[0.25, 0.5, 0.25]]))
    assert sampling.choice_index_rows(lg, [0.3], 1.0, from_logits=True) == 1
    assert sampling.choice_index_rows(np.zeros((1, 4)), [0.7], 1.0) == 0      # a row without mass: 0, as the reference
    u = np.array([[0.1, 0.9], [0.5, 0.2]])
    assert sampling.choice_index_rows(np.array([[0.5, 0.5]] * 4).reshape(2, 2, 2), u, 1.0).shape == (2, 2)


def test_tries_and_cutoff():
    P = np.array([[0.1, 0.6, 0.3]])
    # first draw lands on column 0 (0.1 <= cutoff 0.2), the second on column 1 (0.6 > 0.2): the second is kept
    assert sampling.choice_index_rows(P, [[0.05, 0.5, 0.05]], 1.0, tries=3, cutoff=0.2) == 1
    # the first draw already passes: later uniforms are not looked at
    assert sampling.choice_index_rows(P, [[0.5, 0.05, 0.8]], 1.0, tries=3, cutoff=0.2) == 1
    # every try below the cutoff: the last draw is kept
    assert sampling.choice_index_rows(P, [[0.05, 0.8]], 1.0, tries=2, cutoff=0.7) == 2
    assert sampling.choice_index_rows(P, [[0.8, 0.05]], 1.0, tries=2, cutoff=0.7) == 0
    # tries = 1 ignores the cutoff
    assert sampling.choice_index_rows(P, [0.05], 1.0, tries=1, cutoff=0.7) == 0
    with pytest.raises(NotImplementedError, match="number_of_tries"):
        sampling.choice_index_rows(P, [[0.1] * 5], 1.0, tries=5)
    # the reference's loop, fed the same uniforms through NumPy's global stream
    s = build_settings(temperature=1.0, number_of_tries=3, cutoff_sample_threshold=0.2)
    rng = np.random.default_rng(8)
    Pm = rng.dirichlet(np.full(7, 0.5), 300)
    for i, row in enumerate(Pm):
        np.random.seed(i)
        want = packers.sample_vector(s, row, "choice")
        np.random.seed(i)
        u = np.random.random_sample(3)
        assert sampling.choice_index_rows(row[None], u[None], 1.0, tries=3, cutoff=0.2)[0] == want


# ---- process_decoder_indices --------------------------------------------------------------------------------------------------

def _onehot(idx, width):
    out = np.zeros(idx.shape + (width,))
    np.put_along_axis(out, idx[..., None], 1, axis=-1)
    return out


@pytest.mark.parametrize("vel,held,nxt,instr", [(False, False, False, False), (False, False, False, True), (True, False, False, True),
                                                (True, True, True, True), (False, True, False, True), (False, False, True, True)])
def test_process_decoder_indices_is_process_decoder_outputs_of_onehots(vel, held, nxt, instr):
    s = build_settings(meta_instrument=instr, meta_velocity=vel, meta_held_notes=held, meta_next_notes=nxt)
    n, T, D, V, ID = 6, s["output_length"], s["output_dim"], s["max_voices"], s["meta_instrument_dim"]
    rng = np.random.default_rng(12)
    idx = {"notes": rng.integers(0, D, (n, T)).astype(np.uint8)}
    idx["notes"][0, :5] = D - 1                   # silent rows
    outs = [_onehot(idx["notes"].astype(np.int64), D)]
    if instr:
        idx["instr"] = rng.integers(0, ID, (n, V)).astype(np.uint8)
        outs.append(_onehot(idx["instr"].astype(np.int64), ID))
    if vel:
        idx["velocity"] = rng.random((n, T)).astype(np.float32)
        outs.append(idx["velocity"][:, :, None])
    if held:
        idx["held"] = rng.integers(0, 2, (n, T)).astype(np.uint8)
        outs.append(_onehot(idx["held"].astype(np.int64), 2))
    if nxt:
        idx["next"] = rng.integers(0, D, (n, T)).astype(np.uint8)
        outs.append(_onehot(idx["next"].astype(np.int64), D))
    want = packers.process_decoder_outputs(s, outs if len(outs) > 1 else outs[0], "argmax")
    got = packers.process_decoder_indices(s, idx)
    assert len(got) == 5
    for g, w in zip(got, want):
        assert np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w)


def test_process_decoder_indices_refuses_a_meta_head_without_the_instrument_head():
    """the reference would read that head as the instrument head (element 1 of the list): refused by name, not decoded wrongly"""
    for flag in ("meta_velocity", "meta_held_notes", "meta_next_notes"):
        s = build_settings(**dict(dict(meta_instrument=False, meta_velocity=False, meta_held_notes=False, meta_next_notes=False), **{flag: True}))
        with pytest.raises(NotImplementedError, match=flag):
            packers.process_decoder_indices(s, {"notes": np.zeros((2, s["output_length"]), np.uint8)})


def test_float64_uniforms_just_below_one_stay_below_one():
    """np.random.random_sample yields float64: a value within 2^-25 of 1 rounds to 1.0 as float32 - it must become the largest
    float32 below 1 (the same bin), on the way through the public surface and through the engine's own range check"""
    from midi_vae_amd.model import Decoder

    class _S(object):
        seed = 0
    one_below = np.nextafter(np.float32(1), np.float32(0))
    u = np.full((4, 8), 1 - 2.0 ** -30)
    u[0, 0] = 0.0
    assert np.float32(u[1, 1]) == 1.0
    got = sampling.as_f32_uniforms(u)
    assert got.dtype == np.float32 and got.max() == one_below and got[0, 0] == 0
    d = Decoder(_S())
    spec = d._sample_spec(4, "choice", None, 1, u, {"notes": 8})
    un = spec["uniforms"]["notes"]
    assert un.shape == (4, 8, 1) and un.dtype == np.float32 and un.max() == one_below and np.all(un >= 0)
    assert sampling.as_f32_uniforms(un).max() == one_below          # (what Engine._stage_sample applies once more)
    P = np.array([[0.25, 0.5, 0.25, 0.0]])
    assert sampling.choice_index_rows(P, sampling.as_f32_uniforms([1 - 2.0 ** -30]), 1.0) == 2
    for bad in (1.0, -1e-9, 1.5):
        with pytest.raises(ValueError):
            sampling.as_f32_uniforms([0.5, bad])
        with pytest.raises(ValueError):
            d._sample_spec(1, "choice", None, 1, np.full((1, 8), bad), {"notes": 8})


def test_root_module_binds_the_decoder_to_settings():
    import settings
    import vae_definition
    from midi_vae_amd.model import VAE as EngineVAE
    assert issubclass(vae_definition.VAE, EngineVAE)
    src = open(os.path.join(ROOT, "vae_definition.py")).read()
    assert "self.decoder.sample_settings = _settings" in src
    from midi_vae_amd.model import Decoder

    class _S(object):
        seed = 0
    d = Decoder(_S())
    d.sample_settings = settings            # a module is read like a namespace, at call time
    spec = d._sample_spec(2, "choice", None, 3, None, {"notes": 8})
    assert spec["temperature"] == settings.temperature and spec["tries"] == settings.number_of_tries
    assert spec["cutoff"] == settings.cutoff_sample_threshold


def test_root_module_exposes_process_decoder_indices():
    import vae_definition
    import settings
    idx = {"notes": np.zeros((2, settings.output_length), np.uint8)}
    for flag, key, shape in (("meta_instrument", "instr", (2, settings.max_voices)), ("meta_velocity", "velocity", (2, settings.output_length)),
                             ("meta_held_notes", "held", (2, settings.output_length)), ("meta_next_notes", "next", (2, settings.output_length))):
        if getattr(settings, flag):
            idx[key] = np.zeros(shape, np.float32 if key == "velocity" else np.uint8)
    got = vae_definition.process_decoder_indices(idx)
    want = packers.process_decoder_indices(vars(settings), idx)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_sample_structs_match_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"mvae_head_sample_args": hl.HeadSampleArgs, "mvae_sample_ctl": hl.SampleCtl}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "midivae_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    for cname, cls in pairs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(hl.SampleCtl) == 32 == sampling.control_words(1, 2, 1.0, 0.0, 1).nbytes
    assert ctypes.sizeof(hl.HeadSampleArgs) % 8 == 0


def test_control_words_are_the_struct():
    w = sampling.control_words((5 << 32) | 9, (1 << 33) | 4, 0.5, 0.125, 3)
    c = hl.SampleCtl.from_buffer_copy(w.tobytes())
    assert (c.seed_lo, c.seed_hi, c.window0_lo, c.window0_hi, c.temperature, c.cutoff, c.tries) == (9, 5, 4, 2, 0.5, 0.125, 3)


def test_sample_argument_validation_needs_no_gpu():
    lib = hl.load()
    assert lib.mvae_abi_version() == 9
    assert lib.mvae_head_sample(None, None) == hl.E_ARG
    from midi_vae_amd import plan
    assert "mvae_head_sample" in plan.RECORDABLE and "mvae_head_sample" in hl.SIGNATURES

    def args(**kw):
        a = hl.HeadSampleArgs(hl.F32, 16, 64, 61, 0x1000, 0x1000, 0x1000, None, None, 0x1000, 0, 0, 0, 0, 0, 0,
                              hl.SampleCtl(0, 0, 0, 0, 1.0, 0.0, 1, 0))
        for k, v in kw.items():
            if k in ("temperature", "cutoff", "tries"):
                setattr(a.host, k, v)
            else:
                setattr(a, k, v)
        return a
    # every one of these is refused before anything is enqueued (the pointers are not real)
    assert lib.mvae_head_sample(args(temperature=0.0), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(temperature=-1.0), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(temperature=float("nan")), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(tries=0), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(tries=5), None) == hl.E_UNSUPPORTED
    assert lib.mvae_head_sample(args(N=193), None) == hl.E_UNSUPPORTED
    assert lib.mvae_head_sample(args(out=None), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(R=0), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(uniforms=0x1000, u_stride=1, tries=2), None) == hl.E_ARG      # fewer uniforms than tries
    assert lib.mvae_head_sample(args(b_stride=16, T=0), None) == hl.E_ARG
    assert lib.mvae_head_sample(args(dtype=hl.BF16, H=48), None) == hl.E_UNSUPPORTED


def test_public_surface_refuses_more_than_four_tries():
    from midi_vae_amd.model import Decoder

    class _S(object):
        seed = 0
    d = Decoder(_S())
    d.sample_settings = build_settings(number_of_tries=5)
    with pytest.raises(NotImplementedError, match="number_of_tries"):
        d._sample_spec(4, "choice", None, 1, None, {"notes": 8})
    with pytest.raises(ValueError):
        d._sample_spec(4, "multinomial", None, None, None, {"notes": 8})
    d.sample_settings = build_settings(number_of_tries=2, temperature=0.7, cutoff_sample_threshold=0.1)
    spec = d._sample_spec(4, "choice", None, None, np.zeros((4, 8, 2)), {"notes": 8})
    assert spec["tries"] == 2 and spec["temperature"] == 0.7 and spec["cutoff"] == 0.1 and spec["uniforms"]["notes"].shape == (4, 8, 2)
    assert d._sample_spec(4, "choice", 2.0, None, None, {"notes": 8})["seed"] != spec["seed"]      # the model's own key stream moves on
    assert d._sample_spec(4, "argmax", None, None, None, {"notes": 8}) is None


# ---- the GPU tests' seeds, checked on the mirror alone ----------------------------------------------------------------------

@pytest.mark.parametrize("N,R,H,seed,head,window0", GENERATED_CASES)
def test_generated_cases_keep_the_exclusion_cap(N, R, H, seed, head, window0):
    _, _, _, logits = integer_problem(R, H, N, seed=N)
    for tau in (0.5, 1.0, 2.0):
        u = sampling.uniforms(seed, head, R // 4, 4, 1, first_window=window0).reshape(-1)
        cdf = sampling.cdf_bins(logits[:u.size], tau, from_logits=True)
        share = excluded_rows(cdf, u, N).mean()
        assert share <= 0.03, (tau, share)


def test_distribution_seed_meets_the_bound_on_the_mirror():
    R, N = 65536, 61
    lg = distribution_row()
    u = sampling.uniforms(DISTRIBUTION_SEED, 0, R // 16, 16, 1).reshape(-1)
    idx = sampling.choice_index_rows(np.broadcast_to(lg, (R, N)), u, 1.0, from_logits=True)
    e, S = sampling.tempered(lg[None], 1.0, from_logits=True)
    q = e[0] / S[0]
    cnt = np.bincount(idx, minlength=N)
    assert np.all(np.abs(cnt - R * q) <= 6 * np.sqrt(R * q * (1 - q)) + 1)
