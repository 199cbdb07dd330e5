"""Long songs on the device (csrc/longsong.hip: mvae_nearest_walk, mvae_feedback_rows) against tests/golden/long_songs.npz - the
reference's restated search loop and its own process_decoder_outputs / prepare_encoder_input_list - and the public surface that joins
them to the engine: decoder.long_songs against the same lockstep loop run through the host (longsongs.nearest_walk(device=False),
decoder.predict_indices, packers.process_decoder_indices, packers.prepare_encoder_input_list, encoder.predict).

Bounds (derived, not measured).  A picked index is an integer.  The pull is one float32 product, one sum, one quotient and at most one
cast, each rounded on its own in the type NumPy uses: BIT-EQUAL.  The squared distance is a double sum in ascending column order on
device and mirror alike and sqrt is correctly rounded or one ulp off: distances within 1 ulp of the mirror's double.  The feedback's
bytes are copies and its floats input values or zeros: EQUAL.  Both routes of the whole loop hand the engine the same batches of the
same bytes: every key EQUAL.

Outputs live in guarded, sentinel-filled arenas (tests/footprint.py) with row pitches wider than the rows: what a kernel must not
touch is checked with what it must write.  Doubles are carved as pairs of float32 words."""

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import events as ev
from midi_vae_amd import generation as gen
from midi_vae_amd import hiplib as hl
from midi_vae_amd import longsongs as ls
from midi_vae_amd import packers, sampling
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import Decoder, VAE
from tests import footprint as fp
from tests import longsong_contract as lc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
WALKS, FEEDBACK = lc.load_fixture()
PAD = 3          # floats a row of an output is wider than Z


def stream():
    return torch.cuda.current_stream().cuda_stream


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- mvae_nearest_walk ---------------------------------------------------------------------------------------------------------------
def device_walk(all_z_dev, R, hist, picked, e, den, cap):
    """one call on guarded outputs: ``all_z_dev`` an (N, Z) device view of any row pitch, ``R`` (S, Z) host codes, ``hist`` host rows or
    None, ``picked`` (S, k) host.  dict best, dist, z, r, hist, picked - after the sentinel checks"""
    S, Z = R.shape
    k = picked.shape[1]
    wide = 2 if R.dtype == np.float64 else 1
    ar = fp.Arena(DEV)
    z = ar.carve("z_out", (S + 1, Z + PAD), torch.float32)                    # (a row more than the songs: nothing past row S-1)
    r = ar.carve("r_out", (S + 1, wide * (Z + PAD)), torch.float32)
    h = ar.carve("hist_out", (S + 1, Z + PAD), torch.float32)
    pk = ar.carve("picked", (S + 1, cap), torch.int32, prefill=picked.astype(np.int32), region=np.s_[:S, :k]) if k else \
        ar.carve("picked", (S + 1, cap), torch.int32)
    best = ar.carve("best_out", (1, S + 1), torch.int32)
    dist = ar.carve("dist_out", (1, 2 * (S + 1)), torch.float32)
    ar.commit()
    r_view = r.t.view(torch.float64) if wide == 2 else r.t
    ws = torch.empty(ls.workspace_bytes(all_z_dev.shape[0], S, Z), dtype=torch.uint8, device=DEV)
    ls.enqueue_walk(all_z_dev, up(R), None if hist is None else up(hist), pk.t[:S], k, float(e), float(den), ws, best.t[0, :S],
                    dist.t.view(torch.float64)[0, :S], z.t[:S, :Z], r_view[:S, :Z], h.t[:S, :Z], stream())
    ar.fetch()
    ar.assert_guards_intact()
    for buf, cols in ((z, Z), (r, wide * Z), (h, Z)):
        ar.assert_written(buf, np.s_[:S, :cols])
        ar.assert_untouched(buf, np.s_[:S, cols:])
        ar.assert_untouched(buf, np.s_[S:])
    ar.assert_untouched(pk, np.s_[:S, k + 1:])
    ar.assert_untouched(pk, np.s_[S:])
    ar.assert_untouched(best, np.s_[:, S:])
    ar.assert_untouched(dist, np.s_[:, 2 * S:])
    got_picked = pk.bits()[:S, :k + 1].astype(np.int64)
    assert np.array_equal(got_picked[:, :k], picked), "the entries picked before were changed"
    rr = np.ascontiguousarray(r.bits()[:S, :wide * Z])
    return dict(best=best.bits()[0, :S].astype(np.int32), dist=np.ascontiguousarray(dist.bits()[0, :2 * S]).view(np.float64),
                z=np.ascontiguousarray(z.bits()[:S, :Z]).view(np.float32), r=rr.view(np.float64 if wide == 2 else np.float32),
                hist=np.ascontiguousarray(h.bits()[:S, :Z]).view(np.float32), picked=got_picked)


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((got == want) | (np.abs(got - want) <= np.spacing(np.abs(want))) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("name", sorted(WALKS))
def test_nearest_walk_is_the_reference(name):
    """every iteration of every walk case, all its songs in one call: the fixture's indices, its pulled codes bit for bit in both
    precisions, the mirror's distances; the history is the code pulled one iteration earlier, as a float32"""
    fx = WALKS[name]
    S, L = fx["picked"].shape
    Z = fx["all_z"].shape[1]
    A = up(fx["all_z"])
    picked, previous = np.zeros((S, 0), np.int64), None
    for it in range(L):
        R = lc.walk_inputs(fx, it)
        got = device_walk(A, R, previous, picked, fx["e"], fx["den"], L)
        mirror = ls.nearest_walk(fx["all_z"], R, picked, fx["e"], device=False)
        assert np.array_equal(got["best"], fx["picked"][:, it]) and np.array_equal(got["picked"][:, it], fx["picked"][:, it]), (name, it)
        assert lc.same_bits(got["z"], fx["z"][:, it]), (name, it)
        assert lc.same_bits(got["r"], fx["r0"] if it == 0 else fx["z"][:, it]), (name, it)
        assert within_one_ulp(got["dist"], mirror["distances"]), (name, it, got["dist"], mirror["distances"])
        want_hist = np.zeros((S, Z), np.float32) if previous is None else previous.astype(np.float32)
        assert lc.same_bits(got["hist"], want_hist), (name, it)
        picked, previous = got["picked"], got["r"]
    # the public function, tight rows
    pub = ls.nearest_walk(fx["all_z"], lc.walk_inputs(fx, L - 1), fx["picked"][:, :L - 1], fx["e"])
    assert np.array_equal(pub["picked"], fx["picked"]) and lc.same_bits(pub["z"], fx["z"][:, L - 1])


@pytest.mark.parametrize("name", ["dups", "z257", "n257", "s9", "n3000"])
def test_the_result_does_not_depend_on_row_pitch_or_on_how_songs_are_grouped(name):
    fx = WALKS[name]
    S, L = fx["picked"].shape
    N, Z = fx["all_z"].shape
    A = up(fx["all_z"])
    wide = torch.full((N, Z + 5), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :Z].copy_(A)
    it = L - 1
    R, picked = lc.walk_inputs(fx, it), fx["picked"][:, :it].astype(np.int64)
    one = device_walk(A, R, None, picked, fx["e"], fx["den"], L)
    other = device_walk(wide[:, :Z], R, None, picked, fx["e"], fx["den"], L)
    for k in ("best", "dist", "z", "r", "picked"):
        assert np.array_equal(one[k], other[k]), (name, k)
    for s in range(S):
        alone = device_walk(A, R[s:s + 1], None, picked[s:s + 1], fx["e"], fx["den"], L)
        for k in ("best", "dist", "z", "r", "picked"):
            assert np.array_equal(alone[k], one[k][s:s + 1]), (name, s, k)


def test_nan_and_infinite_distances_on_the_device():
    all_z = np.array([[0, 0], [1, 1], [np.nan, 0], [0.5, 0.5]], np.float32)
    R = np.array([[0.9, 0.9]], np.float32)
    for rows, picked, want in ((all_z, np.zeros((1, 0), np.int64), 1), (all_z, np.array([[1, 3]]), 0), (all_z[[2, 1, 0, 3]], np.zeros((1, 0), np.int64), 0),
                               (np.array([[np.inf, 0], [np.inf, -np.inf]], np.float32), np.zeros((1, 0), np.int64), 0)):
        got = ls.nearest_walk(rows, R, picked, 0.5)
        mirror = ls.nearest_walk(rows, R, picked, 0.5, device=False)
        assert got["best"][0] == want == mirror["best"][0]
        assert lc.same_bits(got["r"], mirror["r"]) and within_one_ulp(got["distances"], mirror["distances"])


# ---- mvae_feedback_rows --------------------------------------------------------------------------------------------------------------
def rolls_on_device(c, layout, n=None):
    """idx, vel, held as (n, T) device tensors and instr as (n, V): window-major, or views of time-major (T, Bp) buffers as a decode
    leaves them; ``n`` windows by tiling the case's"""
    reps = 1 if n is None else -(-n // c["n"])
    tile = lambda a: np.tile(a, (reps, 1))[:n]
    host = dict(idx=tile(c["idx"]), vel=tile(c["vel"]) if c["has_vel"] else None, held=tile(c["held"]) if c["has_held"] else None,
                instr=tile(c["instr"]), X=tile(c["X"]), V=tile(c["V"]), D=tile(c["D"]), I=tile(c["I"]))
    dev = {}
    for k, fill in (("idx", 255), ("vel", float("nan")), ("held", 255), ("instr", 255)):
        a = host[k]
        if a is None:
            dev[k] = None
        elif layout == "window-major":
            dev[k] = up(a)
        else:
            Bp = (a.shape[0] + 15) // 16 * 16
            t = torch.full((a.shape[1], Bp), fill, dtype=torch.float32 if k == "vel" else torch.uint8, device=DEV)
            t[:, :a.shape[0]].copy_(up(a).t())
            dev[k] = t[:, :a.shape[0]].t()
    return host, dev


def check_feedback(c, layout, n=None, skip=()):
    host, dev = rolls_on_device(c, layout, n)
    n, T = host["idx"].shape
    V, ld = c["voices"], n + 5
    ar = fp.Arena(DEV)
    out = {k: ar.carve(k, (T if k != "instr_out" else V, ld), torch.float32 if k == "vel_out" else torch.uint8)
           for k in ("x_out", "x_rev_out", "vel_out", "held_out", "instr_out")}
    ar.commit()
    t = {k: (None if k in skip else b.t) for k, b in out.items()}
    ls.enqueue_feedback(dev["idx"], dev["vel"], dev["held"], dev["instr"], ls.params(lc.feedback_settings(c)), ld, t["x_out"], t["x_rev_out"],
                        t["vel_out"], t["held_out"], t["instr_out"], stream())
    ar.fetch()
    ar.assert_guards_intact()
    want = dict(x_out=host["X"].T, x_rev_out=host["X"][:, ::-1].T, vel_out=host["V"].T, held_out=host["D"].T, instr_out=host["I"].T)
    for k, b in out.items():
        if k in skip:
            ar.assert_untouched(b)
            continue
        ar.assert_written(b)
        ar.assert_zero(b, np.s_[:, n:])          # the padding columns: the host staging's fill
        got = np.ascontiguousarray(b.bits()[:, :n])
        if k == "vel_out":
            assert lc.same_bits(got.view(np.float32), np.ascontiguousarray(want[k])), (lc.feedback_id(c), layout, k)
        else:
            assert np.array_equal(got, want[k]), (lc.feedback_id(c), layout, k)


@pytest.mark.parametrize("layout", ["window-major", "time-major"])
def test_feedback_rows_are_the_reference(layout):
    """all 63 cases of the fixture in either layout (four windows each)"""
    for c in FEEDBACK:
        check_feedback(c, layout)


def _case(voices, ticks, flags):
    return next(c for c in FEEDBACK if (c["voices"], c["T"] // c["voices"]) == (voices, ticks) and
                (c["silent"], c["has_vel"], c["has_held"], c["override"]) == flags)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("voices", [2, 4, 8])
def test_feedback_rows_across_workgroups(voices, n):
    """256 lanes hold 128, 64 or 32 windows: one window, a workgroup less one, a full one, one more, several; both layouts"""
    c = _case(voices, 3, (True, True, False, True))
    check_feedback(c, "time-major", n)
    check_feedback(_case(voices, 16, (True, True, True, True)), "window-major", n)


def test_outputs_passed_as_null_are_not_written():
    c = _case(4, 3, (True, True, False, True))
    check_feedback(c, "time-major", 20, skip=("x_rev_out", "instr_out"))
    check_feedback(c, "window-major", 20, skip=("x_out", "vel_out", "held_out"))
    check_feedback(c, "time-major", 20, skip=("x_out", "x_rev_out", "vel_out", "instr_out"))
    got = ls.feedback_rows(c["idx"], c["vel"], None, c["instr"], lc.feedback_settings(c))          # the public function
    assert np.array_equal(got["x"], c["X"]) and lc.same_bits(got["vel"], c["V"]) and np.array_equal(got["held"], c["D"])
    assert np.array_equal(got["x_rev"], c["X"][:, ::-1]) and np.array_equal(got["instr"], c["I"])


# ---- refusals on real buffers --------------------------------------------------------------------------------------------------------
def _contract_arena(baseline, contents, prefilled):
    """a contract's baseline on real buffers: outputs guarded and sentinel-filled, inputs filled by ``contents(name, shape)``"""
    ar, bufs, inputs = fp.Arena(DEV), {}, {}

    def carve(name, shape, kind, out=False):
        if out:
            dtype = {"f32": torch.float32, "f64": torch.float32, "i32": torch.int32, "u8": torch.uint8}[kind]
            shape = (shape[0], shape[1] * (2 if kind == "f64" else 1))
            if name in prefilled:
                bufs[name] = ar.carve(name, shape, dtype, prefill=prefilled[name][0], region=prefilled[name][1])
            else:
                bufs[name] = ar.carve(name, shape, dtype)
        else:
            inputs[name] = up(contents(name, shape))
        return 0x1000

    baseline(carve)
    ar.commit()
    return ar, bufs, (lambda name, shape, kind, out=False: (bufs[name].t if name in bufs else inputs[name]).data_ptr()), inputs


def _walk_contents(name, shape):
    rng = np.random.default_rng(5)
    return rng.standard_normal(shape).astype(np.float32)


def _feedback_contents(name, shape):
    rng = np.random.default_rng(6)
    return {"idx": lambda: rng.integers(0, lc.F_PITCH + 1, shape).astype(np.uint8), "vel": lambda: rng.random(shape).astype(np.float32),
            "held_idx": lambda: rng.integers(0, 2, shape).astype(np.uint8), "instr": lambda: rng.integers(0, 16, shape).astype(np.uint8)}[name]()


@pytest.mark.parametrize("which", ["walk", "feedback"])
def test_refused_calls_enqueue_nothing(which):
    """the safe rows of tests/longsong_contract.py on real buffers: the promised code, and every byte of the arena - sentinel-filled
    outputs and guards - as planted; the baseline itself then runs inside its buffers and agrees with the mirror"""
    before = np.array([[3, 7], [7, 0], [39, 38]], np.int32)
    entry, baseline, rows, contents, prefilled = {
        "walk": ("mvae_nearest_walk", lc.walk_baseline, lc.WALK_ROWS, _walk_contents, {"picked": (before, np.s_[:, :lc.W_PICKED])}),
        "feedback": ("mvae_feedback_rows", lc.feedback_baseline, lc.FEEDBACK_ROWS, _feedback_contents, {})}[which]
    ar, bufs, resolve, inputs = _contract_arena(baseline, contents, prefilled)
    lib = hl.load()
    safe = [r for r in rows if r[3]]
    assert len(safe) >= 12
    for name, mutate, code, _ in safe:
        rc = lc.invoke(lib, entry, mutate(baseline(resolve)), stream())
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert lc.invoke(lib, entry, baseline(resolve), stream()) == 0
    ar.fetch()
    ar.assert_guards_intact()
    host = {k: v.cpu().numpy() for k, v in inputs.items()}
    if which == "walk":
        Z = lc.W_Z
        want = ls.nearest_walk(host["all_z"][:, :Z].copy(), host["r_in"][:, :Z].copy(), before, 0.75, device=False, den=1.75)
        assert np.array_equal(bufs["picked"].bits()[:, :lc.W_PICKED + 1].astype(np.int64), want["picked"])
        ar.assert_untouched(bufs["picked"], np.s_[:, lc.W_PICKED + 1:])
        assert np.array_equal(bufs["best_out"].bits()[0], want["best"])
        assert within_one_ulp(np.ascontiguousarray(bufs["dist_out"].bits()).view(np.float64)[0], want["distances"])
        for name, rows_want in (("z_out", want["z"]), ("r_out", want["r"]), ("hist_out", host["hist_in"][:, :Z])):
            ar.assert_written(bufs[name], np.s_[:, :Z])
            ar.assert_untouched(bufs[name], np.s_[:, Z:])
            assert lc.same_bits(np.ascontiguousarray(bufs[name].bits()[:, :Z]).view(np.float32), np.ascontiguousarray(rows_want))
    else:
        s = dict(max_voices=lc.F_V, low_crop=0, high_crop=lc.F_PITCH, include_silent_note=True,
                 velocity_threshold_such_that_it_is_a_played_note=0.5, override_sampled_pitches_based_on_velocity_info=True)
        want = ls.feedback_rows(host["idx"], host["vel"], host["held_idx"], host["instr"], s, device=False)
        n = lc.F_N
        for name, key in (("x_out", "x"), ("x_rev_out", "x_rev"), ("held_out", "held"), ("instr_out", "instr")):
            ar.assert_zero(bufs[name], np.s_[:, n:])
            assert np.array_equal(bufs[name].bits()[:, :n], want[key].T), name
        ar.assert_zero(bufs["vel_out"], np.s_[:, n:])
        assert lc.same_bits(np.ascontiguousarray(bufs["vel_out"].bits()[:, :n]).view(np.float32), np.ascontiguousarray(want["vel"].T))


# ---- the whole loop ------------------------------------------------------------------------------------------------------------------
SONGS, LENGTH, N_CODES = 3, 4, 50
MODELS = {"gru64": dict(cell_type="GRU", lstm_size=64, dtype="f32"),
          "lstm64-held": dict(cell_type="LSTM", lstm_size=64, dtype="f32", meta_held_notes=True),
          "gru64-bidirectional": dict(cell_type="GRU", lstm_size=64, dtype="f32", bidirectional=True),
          "gru256-bf16": dict(cell_type="GRU", lstm_size=256, dtype="bf16"),
          "lstm256-bf16-held": dict(cell_type="LSTM", lstm_size=256, dtype="bf16", meta_held_notes=True)}
_models = {}


def model(tag):
    """Z = 8, T = 16 rows of 4 voices, velocity and instrument heads; made once per tag"""
    if tag not in _models:
        kw = dict(MODELS[tag])
        dtype = kw.pop("dtype")
        s = build_settings(latent_dim=8, input_length=4, output_length=4, max_voices=4, batch_size=8, epsilon_std=0.5, **kw)
        m = VAE().create(compute_dtype=dtype, seed=11, **create_kwargs(s))
        m.decoder.sample_settings = s
        assert (m.spec.T, m.spec.V, m.spec.Z) == (16, 4, 8) and s["meta_velocity"] and s["meta_instrument"]
        rng = np.random.default_rng(77)
        all_z = (rng.standard_normal((N_CODES, 8)) * 0.8).astype(np.float32)
        codes = rng.normal(0.0, float(np.std(all_z)), (SONGS, 8))
        _models[tag] = (s, m, all_z, codes)
    return _models[tag]


def host_route(s, m, all_z, codes, length, method, seed):
    """the same lockstep loop through the host, at batch S: one dict per song"""
    S, Z = codes.shape
    T, V = m.spec.T, m.spec.V
    e = np.std(all_z)
    heads = m.decoder._softmax_heads()
    R, previous, picked = codes, np.zeros((S, Z)), np.zeros((S, 0), np.int64)
    per_song = [dict(notes=[], velocity=[], starts=[], instr=[], z=[], distances=[]) for _ in range(S)]
    A64 = all_z.astype(np.float64)
    for it in range(length):
        # every search is decisive: the two smallest candidate distances are a relative 1e-9 apart
        for k in range(S):
            d2 = np.cumsum((A64 - R[k].astype(np.float64)) ** 2, axis=1)[:, -1]
            cand = np.ones(len(d2), bool)
            cand[picked[k]] = False
            cand[0] = True
            two = np.sort(d2[cand])[:2]
            assert len(two) < 2 or two[1] - two[0] > 1e-9 * two[1], "song %d, iteration %d: the search is not decisive" % (k, it)
        got = ls.nearest_walk(all_z, R, picked, e, device=False)
        picked, pulled = got["picked"], got["r"]
        x = packers.prepare_decoder_input(s, pulled, 0, np.zeros((S, s["signature_vector_length"])), previous)
        kw = {}
        if method == "choice":          # the uniforms the device generates for the windows it * S .. it * S + S - 1 of the run
            kw = dict(seed=seed, uniforms={h: sampling.uniforms(seed, sampling.HEAD_IDS[h], S, Th, 1, first_window=it * S) for h, Th in heads.items()})
        ind = m.decoder.predict_indices(x, batch_size=S, sample_method=method, **kw)
        lists = []
        for k in range(S):          # one window a call, as the reference post-processes here
            Y, I, Vp, Dp, _ = packers.process_decoder_indices(s, {h: a[k:k + 1] for h, a in ind.items()})
            X = np.copy(Y)
            X = np.append(X, np.zeros((X.shape[0], 1)), axis=1)
            X[np.sum(X, axis=1) == 0, -1] = 1
            lists.append(packers.prepare_encoder_input_list(s, np.asarray([X]), I[0], np.expand_dims(Vp, 0), np.expand_dims(Dp, 0)))
            d = per_song[k]
            d["notes"].append(ind["notes"][k])
            d["velocity"].append(Vp.astype(np.float32))
            d["starts"].append(np.asarray(Dp).astype(np.uint8))
            d["instr"].append(ind["instr"][k])
            d["z"].append(got["z"][k])
            d["distances"].append(got["distances"][k])
        previous = pulled
        if it + 1 < length:
            R = m.encoder.predict([np.concatenate([l[j] for l in lists], 0) for j in range(len(lists[0]))], batch_size=S)
            assert R.dtype == np.float32 and R.shape == (S, Z)
    out = []
    for k, d in enumerate(per_song):
        notes, vel, starts = np.stack(d["notes"]), np.stack(d["velocity"]), np.stack(d["starts"])
        instr = np.stack(d["instr"])
        out.append(dict(notes=notes, velocity=vel, starts=starts, instr=instr, picked=picked[k], z=np.stack(d["z"]),
                        distances=np.asarray(d["distances"]), events=ev.note_events(notes, vel, starts, [length], s, device=False)[0],
                        programs=ev.vote_for_programs(instr, [length], s)[0]))
    return out


@pytest.mark.parametrize("method", ["argmax", "choice"])
@pytest.mark.parametrize("tag", sorted(MODELS))
def test_long_songs_are_the_host_loop(tag, method):
    s, m, all_z, codes = model(tag)
    seed = 9 if method == "choice" else None
    m._shared.rng = np.random.default_rng(123)
    kw = dict(seed=seed) if method == "choice" else {}
    got = m.decoder.long_songs(all_z, codes, length=LENGTH, sample_method=method, note_events=True, batch_size=SONGS, **kw)
    m._shared.rng = np.random.default_rng(123)          # the same epsilons
    want = host_route(s, m, all_z, codes, LENGTH, method, seed)
    assert len(got) == len(want) == SONGS
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["picked"], w["picked"]), (tag, k, g["picked"], w["picked"])
        assert lc.same_bits(g["z"], w["z"]), (tag, k)
        assert within_one_ulp(g["distances"], w["distances"])
        for key in ("notes", "velocity", "starts", "instr", "events"):
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape and np.array_equal(g[key], w[key]), (tag, k, key)
        assert list(g["programs"]) == list(w["programs"])
    assert sum(len(g["events"]) for g in got) > 0, "the model decodes no note: the comparison shows little"
    assert len({tuple(g["picked"].tolist()) for g in got}) > 1


def test_long_songs_in_groups_and_its_refusals():
    """an engine of 16 windows takes 20 songs in two groups; songs do not depend on their neighbours under 'argmax'"""
    s, m, all_z, codes = model("gru64")
    rng = np.random.default_rng(5)
    many = rng.normal(0.0, float(np.std(all_z)), (20, 8))
    zero = build_settings(latent_dim=8, input_length=4, output_length=4, max_voices=4, batch_size=8, epsilon_std=0.0, cell_type="GRU", lstm_size=64)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MVAE_INFER_BATCH", "16")
        m0 = VAE().create(compute_dtype="f32", seed=11, **create_kwargs(zero))
    m0.decoder.sample_settings = zero
    whole = m0.decoder.long_songs(all_z, many, length=3, pianoroll=True)
    assert m0._shared.infer.maxB == 16 and len(whole) == 20
    part = m0.decoder.long_songs(all_z, many[14:19], length=3)
    for a, b in zip(whole[14:19], part):
        assert all(np.array_equal(a[k], b[k]) for k in b if k != "programs") and list(a["programs"]) == list(b["programs"])
    assert whole[0]["pianoroll"].shape == (zero["high_crop"] - zero["low_crop"], 3 * 4) and whole[0]["z"].shape == (3, 8)
    assert sorted(part[0]) == ["counts", "distances", "instr", "notes", "picked", "programs", "starts", "velocity", "z"]
    # float32 start codes walk in float32 from the first iteration on
    f32 = m0.decoder.long_songs(all_z, many[:2].astype(np.float32), length=2, e=0.5)
    first = ls.nearest_walk(all_z, many[:2].astype(np.float32), np.zeros((2, 0)), 0.5, device=False)
    assert np.array_equal(np.stack([d["picked"][0] for d in f32]), first["best"]) and lc.same_bits(np.stack([d["z"][0] for d in f32]), first["z"])
    for bad in (dict(all_z=all_z.astype(np.float64)), dict(all_z=all_z[:, :4]), dict(codes=many[:, :4]), dict(length=0), dict(e=float("nan")),
                dict(seed=3)):
        a = dict(dict(all_z=all_z, codes=many[:2], length=2), **bad)
        with pytest.raises(ValueError):
            m0.decoder.long_songs(a.pop("all_z"), a.pop("codes"), **a)
    for knob in ("combine_velocity_and_held_notes", "attach_instruments"):
        m0.decoder.sample_settings = dict(zero, **{knob: True})
        with pytest.raises(NotImplementedError):
            m0.decoder.long_songs(all_z, many[:2], length=2)
    m0.decoder.sample_settings = zero


# ---- the siblings ----------------------------------------------------------------------------------------------------------------------
def test_random_songs_and_class_knob_songs():
    s, m, all_z, codes = model("gru64")
    dec = m.decoder
    got = dec.random_songs(codes, note_events=True, pianoroll=True)
    want = dec.decode_paths([dict(anchors=c.reshape(1, -1), a0=np.zeros(1, np.int32), a1=np.full(1, -1, np.int32), c0=np.ones(1), c1=np.zeros(1))
                             for c in codes], note_events=True, pianoroll=True)
    assert len(got) == SONGS
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w) and g["notes"].shape == (1, 16)
        assert all(np.array_equal(g[k], w[k]) for k in g if k != "programs") and list(g["programs"]) == list(w["programs"])
        assert lc.same_bits(g["z"], g["z"]) and not np.isnan(g["z"]).any()
    assert lc.same_bits(np.concatenate([g["z"] for g in got], 0), codes.astype(np.float32))
    # a one-window song has a zero history: the same windows through the host's packer
    x = packers.prepare_decoder_input(s, codes.astype(np.float32).astype(np.float64), 0, np.zeros((SONGS, s["signature_vector_length"])), np.zeros((SONGS, 8)))
    ind = dec.predict_indices(x, batch_size=SONGS)
    assert np.array_equal(np.concatenate([g["notes"] for g in got], 0), ind["notes"])
    knobs = dec.class_knob_songs(codes[0], 2, pianoroll=True)
    documented = Decoder.class_knob_codes(codes[0], 2)
    assert len(knobs) == 2 and documented[0, :2].tolist() == [1, -1] and documented[1, :2].tolist() == [-1, 1]
    assert np.array_equal(documented[:, 2:], np.repeat(codes[:1, 2:], 2, 0))
    assert lc.same_bits(np.concatenate([k["z"] for k in knobs], 0), documented.astype(np.float32))
    direct = dec.random_songs(documented, pianoroll=True)
    for a, b in zip(knobs, direct):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    from midi_vae_amd import pianoroll as pr
    assert pr.difference_image(knobs[1]["pianoroll"], knobs[0]["pianoroll"]).shape[:2] == knobs[0]["pianoroll"].shape[:2]
    with pytest.raises(ValueError):
        dec.random_songs(codes[0])
    assert gen.code_path(codes[0])["anchors"].shape == (1, 8)
