"""Generated songs on the device (csrc/generate.hip: mvae_latent_paths, mvae_pianoroll) against tests/golden/generation.npz - the
reference's own blends, its restated generation loops and its own prepare_for_drawing - and the public surface that joins them to a
decode: decoder.decode_paths against decoder.predict_songs on host-built inputs from the NumPy mirror.

Bounds (derived, not measured).  A latent row is two products and a sum, each rounded on its own in the anchors' type, and one cast;
an image cell one subtraction, one multiplication and at most max_voices - 1 additions in double in voice order: the device does
the same operations on the same bits as NumPy: BIT-EQUAL, signed zeros included.  decode_paths stages the very float32 rows the host
route uploads, so both routes decode the same bytes: every key EQUAL.  Nothing here has a tolerance.

Outputs live in guarded, sentinel-filled arenas (tests/footprint.py) with row pitches wider than the rows: what a kernel must not
touch is checked with what it must write.  Doubles are carved as pairs of float32 words."""

import numpy as np
import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import generation as gen
from midi_vae_amd import hiplib as hl
from midi_vae_amd import packers
from midi_vae_amd import pianoroll as pr
from midi_vae_amd.config import build_settings, create_kwargs
from midi_vae_amd.model import VAE
from midi_vae_amd.reconstruction import first_windows
from tests import footprint as fp
from tests import generate_contract as gc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
Z, N, LD_Z, LD_HIST = 32, 75, 40, 36


@pytest.fixture(scope="module")
def cases():
    return gc.load_fixture()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32_of(buf, cols=None):
    a = np.ascontiguousarray(buf.bits() if cols is None else buf.bits()[:, :cols])
    return a.view(np.float32)


def f64_of(buf, cols):
    """the first ``cols`` doubles of every row of a buffer carved as pairs of float32 words"""
    return np.ascontiguousarray(buf.bits()[:, :2 * cols]).view(np.float64)


# ---- mvae_latent_paths ---------------------------------------------------------------------------------------------------------------
def device_run(fx, **changed):
    run = dict(anchors=fx["anchors"], first_window=first_windows(fx["lengths"], N), **{k: fx[k] for k in ("a0", "a1", "c0", "c1")})
    run.update(changed)
    return gen.upload(run, DEV)


def paths_arena():
    ar = fp.Arena(DEV)
    z = ar.carve("z_out", (N, LD_Z), torch.float32)
    hist = ar.carve("hist_out", (N, LD_HIST), torch.float32)
    ar.commit()
    return ar, z, hist


def check_paths(ar, z, hist, want_z, want_hist, what):
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(z, np.s_[:, :Z])
    ar.assert_untouched(z, np.s_[:, Z:])
    assert gc.same_bits(f32_of(z, Z), want_z), "%s: z" % what
    if want_hist is None:
        ar.assert_untouched(hist)
    else:
        ar.assert_written(hist, np.s_[:, :Z])
        ar.assert_untouched(hist, np.s_[:, Z:])
        assert gc.same_bits(f32_of(hist, Z), want_hist), "%s: history" % what


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("calls", [((0, 75),), ((0, 32), (32, 32), (64, 11))], ids=["one call", "three calls"])
def test_latent_paths_are_the_reference(cases, tag, calls):
    """the run of 75 windows in songs of 1, 11, 32 and 31, row pitches of 40 and 36 floats: the second and third call start in the
    middle of a song, so their first history row is a window the call does not fill"""
    fx = cases["paths_" + tag]
    run = device_run(fx)
    assert run["anchors"].dtype == (torch.float32 if tag == "f32" else torch.float64)
    ar, z, hist = paths_arena()
    for lo, count in calls:
        gen.enqueue(run, lo, count, z.t[lo:lo + count, :Z], hist.t[lo:lo + count, :Z], stream())
    check_paths(ar, z, hist, fx["z"], fx["hist"], "%s %r" % (tag, calls))
    assert ((fx["z"] == 0) & np.signbit(fx["z"])).any()          # (-0.0 is among what was compared)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_latent_paths_without_history_and_without_songs(cases, tag):
    fx = cases["paths_" + tag]
    ar, z, hist = paths_arena()
    gen.enqueue(device_run(fx), 0, N, z.t[:, :Z], None, stream())
    check_paths(ar, z, hist, fx["z"], None, tag + " hist_out NULL")
    ar, z, hist = paths_arena()
    gen.enqueue(device_run(fx, first_window=None), 0, N, z.t[:, :Z], hist.t[:, :Z], stream())
    check_paths(ar, z, hist, fx["z"], np.zeros((N, Z), np.float32), tag + " first_window NULL")
    # the public function, tight rows
    got_z, got_hist = gen.latent_rows(fx["anchors"], fx, first_windows(fx["lengths"], N), lo=30, count=40)
    assert gc.same_bits(got_z, fx["z"][30:70]) and gc.same_bits(got_hist, fx["hist"][30:70])


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_an_anchor_out_of_range_is_one_nan_row(cases, tag):
    """window 5 names anchor 48 of 48, window 20 a negative one: their rows are NaN, and so is the history of the windows after them
    (5 and 6 share a song, 20 and 21 too); every other row is the fixture's"""
    fx = cases["paths_" + tag]
    a0, a1 = fx["a0"].copy(), fx["a1"].copy()
    a0[20] = -1
    assert a1[5] >= 0
    a1[5] = 48
    ar, z, hist = paths_arena()
    gen.enqueue(device_run(fx, a0=a0, a1=a1), 0, N, z.t[:, :Z], hist.t[:, :Z], stream())
    want_z, want_hist = fx["z"].copy(), fx["hist"].copy()
    want_z[[5, 20]] = np.nan
    want_hist[[6, 21]] = np.nan
    check_paths(ar, z, hist, want_z, want_hist, tag)
    mz, mh = gen.latent_rows(fx["anchors"], dict(fx, a0=a0, a1=a1), first_windows(fx["lengths"], N), device=False)
    assert gc.same_bits(mz, want_z) and gc.same_bits(mh, want_hist)


# ---- mvae_pianoroll ------------------------------------------------------------------------------------------------------------------
def rolls_on_device(fx, layout):
    """idx and vel as (n, T) device tensors: window-major, or views of time-major (T, Bp) buffers as a decode leaves them"""
    n, T = fx["idx"].shape
    idx, vel = torch.from_numpy(fx["idx"]).to(DEV), torch.from_numpy(fx["vel"]).to(DEV)
    if layout == "window-major":
        return idx, vel
    Bp = (n + 15) // 16 * 16
    ti = torch.full((T, Bp), 255, dtype=torch.uint8, device=DEV)
    tv = torch.full((T, Bp), float("nan"), dtype=torch.float32, device=DEV)
    ti[:, :n].copy_(idx.t())
    tv[:, :n].copy_(vel.t())
    return ti[:, :n].t(), tv[:, :n].t()


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("layout", ["window-major", "time-major"])
@pytest.mark.parametrize("drawn", [True, False], ids=["vel", "vel NULL"])
def test_pianoroll_is_the_reference(cases, case, layout, drawn):
    """case a: T = 16 / 2 voices with the song of 40 windows whose voices hold one note throughout (the longest look-back);
    case b: T = 12 / 3 voices.  ld_img = n_pitch + 3"""
    fx = cases["image_" + case]
    p = pr.params(gc.image_settings(fx))
    K, V = int(fx["n_pitch"]), int(fx["voices"])
    n, T = fx["idx"].shape
    idx, vel = rolls_on_device(fx, layout)
    assert idx.stride() == ((T, 1) if layout == "window-major" else (1, (n + 15) // 16 * 16))
    first = torch.from_numpy(first_windows(fx["lengths"], n)).to(DEV)
    ar = fp.Arena(DEV)
    img = ar.carve("img_out", (n * T // V, 2 * (K + 3)), torch.float32)
    ar.commit()
    pr.enqueue(idx, vel if drawn else None, first, p, img.t.view(torch.float64), stream())
    ar.fetch()
    ar.assert_guards_intact()
    ar.assert_written(img, np.s_[:, :2 * K])
    ar.assert_untouched(img, np.s_[:, 2 * K:])
    assert gc.same_bits(f64_of(img, K), fx["image"] if drawn else fx["binary"])
    if case == "a" and drawn and layout == "window-major":          # the public function; and the held song really is held
        songs = pr.images(fx["idx"], fx["vel"], fx["lengths"], gc.image_settings(fx))
        assert gc.same_bits(np.concatenate(songs, 1).T, fx["image"])
        assert songs[2].shape == (K, 40 * T // V) and (songs[2][4, 2:] > 0).all()
        alone = pr.images(idx[4:44], vel[4:44], [40], gc.image_settings(fx))[0]
        assert gc.same_bits(alone, songs[2])


# ---- refusals on real buffers --------------------------------------------------------------------------------------------------------
def _contract_arena(baseline, contents):
    """a contract's baseline on real buffers: outputs guarded and sentinel-filled, inputs filled by ``contents(name, shape)``"""
    ar, bufs, inputs = fp.Arena(DEV), {}, {}

    def carve(name, shape, kind, out=False):
        if out:
            bufs[name] = ar.carve(name, (shape[0], shape[1] * (2 if kind == "f64" else 1)), torch.float32)
        else:
            inputs[name] = torch.from_numpy(np.ascontiguousarray(contents(name, shape))).to(DEV)
        return 0x1000

    baseline(carve)
    ar.commit()
    return ar, bufs, (lambda name, shape, kind, out=False: (bufs[name].t if name in bufs else inputs[name]).data_ptr()), inputs


def _paths_contents(name, shape):
    rng = np.random.default_rng(3)
    return {"anchors": lambda: rng.standard_normal(shape).astype(np.float32), "a0": lambda: rng.integers(0, gc.P_ANCHORS, shape).astype(np.int32),
            "a1": lambda: rng.integers(-1, gc.P_ANCHORS, shape).astype(np.int32), "c0": lambda: rng.random(shape), "c1": lambda: rng.random(shape),
            "first_window": lambda: (np.arange(gc.P_N) // 5 * 5).astype(np.int32)}[name]()


def _pianoroll_contents(name, shape):
    rng = np.random.default_rng(4)
    return {"idx": lambda: rng.integers(0, gc.R_PITCH + 1, shape).astype(np.uint8), "vel": lambda: rng.random(shape).astype(np.float32),
            "first_window": lambda: (np.arange(gc.R_N) // 4 * 4).astype(np.int32)}[name]()


@pytest.mark.parametrize("which", ["paths", "pianoroll"])
def test_refused_calls_enqueue_nothing(which):
    """the safe rows of tests/generate_contract.py on real buffers: the promised code, and every byte of the arena - sentinel-filled
    outputs and guards - as planted; the baseline itself then runs inside its buffers and agrees with the mirror"""
    entry, baseline, rows, contents = {"paths": ("mvae_latent_paths", gc.paths_baseline, gc.PATHS_ROWS, _paths_contents),
                                       "pianoroll": ("mvae_pianoroll", gc.pianoroll_baseline, gc.PIANOROLL_ROWS, _pianoroll_contents)}[which]
    ar, bufs, resolve, inputs = _contract_arena(baseline, contents)
    lib = hl.load()
    safe = [r for r in rows if r[3]]
    assert len(safe) >= 10
    for name, mutate, code, _ in safe:
        rc = gc.invoke(lib, entry, mutate(baseline(resolve)), stream())
        ar.fetch()
        assert rc == code, "%s: returned %d, promised %d" % (name, rc, code)
        assert np.array_equal(ar.fetched, ar.planted), "%s: %d bytes of the arena changed" % (name, int((ar.fetched != ar.planted).sum()))
    assert gc.invoke(lib, entry, baseline(resolve), stream()) == 0
    ar.fetch()
    ar.assert_guards_intact()
    host = {k: v.cpu().numpy() for k, v in inputs.items()}
    if which == "paths":
        want_z, want_hist = gen.latent_rows(host["anchors"][:, :gc.P_Z], host, host["first_window"], device=False)
        for buf, want in ((bufs["z_out"], want_z), (bufs["hist_out"], want_hist)):
            ar.assert_written(buf, np.s_[:, :gc.P_Z])
            ar.assert_untouched(buf, np.s_[:, gc.P_Z:])
            assert gc.same_bits(f32_of(buf, gc.P_Z), want)
    else:
        s = dict(max_voices=gc.R_V, low_crop=0, high_crop=gc.R_PITCH, include_silent_note=True,
                 velocity_threshold_such_that_it_is_a_played_note=0.5, MAX_VELOCITY=127.0)
        want = pr._mirror(host["idx"], host["vel"], host["first_window"], pr.params(s))
        ar.assert_written(bufs["img_out"], np.s_[:, :2 * gc.R_PITCH])
        ar.assert_untouched(bufs["img_out"], np.s_[:, 2 * gc.R_PITCH:])
        assert gc.same_bits(f64_of(bufs["img_out"], gc.R_PITCH), want)


# ---- the model's surface ---------------------------------------------------------------------------------------------------------------
LENGTHS = [32, 11, 107, 100, 49, 1]          # 300 windows on an engine of 128: songs 2 and 4 straddle the batch edges at 128 and 256


@pytest.fixture(scope="module")
def small_model():
    """the small model of test_decode_paths_gpu.py; its forward-only engine holds 128 windows.  Six songs from float32 codes: a
    medley at the reference's defaults, an interpolation song of length 10, a medley of 40 + 30 + 25 windows with bridges of 6, an
    interpolation song of length 99, a slerp medley of 20 + 20 with a bridge of 9, a medley of one window"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MVAE_INFER_BATCH", "128")
        s = build_settings(cell_type="GRU", lstm_size=64, latent_dim=32, input_length=8, output_length=8, max_voices=2, batch_size=8)
        m = VAE().create(compute_dtype="f32", seed=4, **create_kwargs(s))
    m.decoder.sample_settings = s
    assert (m.spec.T, m.spec.V, m.spec.Z) == (16, 2, 32) and m._shared.infer_cap == 128
    assert s["meta_velocity"] and s["meta_instrument"]
    rng = np.random.default_rng(41)
    code = lambda rows: (rng.standard_normal((rows, 32)) * 2.0).astype(np.float32)
    paths = [gen.medley_path([code(8), code(8), code(8)], 4), gen.interpolation_path(code(1), code(1), 10),
             gen.medley_path([code(40), code(30), code(25)], 6), gen.interpolation_path(code(1), code(1), 99),
             gen.medley_path([code(20), code(20)], 9, mode="slerp"), gen.medley_path([code(1)], 4)]
    run = gen.concat_paths(paths)
    assert run["lengths"] == LENGTHS and sum(LENGTHS) == 300
    z, hist = gen.latent_rows(run["anchors"], run, run["first_window"], device=False)
    xs, lo = [], 0
    for n in LENGTHS:          # the host route's inputs: the mirror's rows through the reference's packer
        xs.append(packers.prepare_decoder_input(s, z[lo:lo + n].astype(np.float64), 0, np.zeros((n, s["signature_vector_length"])),
                                                hist[lo:lo + n].astype(np.float64)))
        lo += n
    return s, m, paths, xs, z


def assert_same_songs(got, want, what):
    assert len(got) == len(want) == len(LENGTHS)
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(set(g) - {"z"}) == sorted(w), (what, i, sorted(g), sorted(w))
        for k, v in w.items():
            if k == "programs":
                assert list(g[k]) == list(v), (what, i, k)
            else:
                assert g[k].dtype == v.dtype and g[k].shape == v.shape and np.array_equal(g[k], v), (what, i, k)


@pytest.mark.parametrize("method,kw", [("argmax", {}), ("choice", dict(seed=5))], ids=["argmax", "choice"])
def test_decode_paths_is_predict_songs_on_the_mirrors_rows(small_model, method, kw):
    s, m, paths, xs, z = small_model
    dec = m.decoder
    got = dec.decode_paths(paths, 8, sample_method=method, note_events=True, pianoroll=True, **kw)
    assert m._shared.infer.maxB == 128          # two full engine batches and one of 44
    want = dec.predict_songs(xs, 8, sample_method=method, note_events=True, pianoroll=True, **kw)
    assert sorted(want[0]) == ["counts", "events", "instr", "notes", "pianoroll", "programs", "starts", "velocity"]
    assert_same_songs(got, want, method)
    assert gc.same_bits(np.concatenate([d["z"] for d in got], 0), z)
    assert sum(len(d["events"]) for d in got) > 0, "the model decodes no note: the comparison shows little"
    # the image is the mirror's on what came back; without the flags the keys are gone and the rest is unchanged
    n_pitch = s["high_crop"] - s["low_crop"]
    for d, n in zip(got, LENGTHS):
        image = pr.images(d["notes"], d["velocity"], [n], s, device=False)[0]
        assert d["pianoroll"].shape == (n_pitch, n * 8) and gc.same_bits(d["pianoroll"], image)
    assert sum(float(d["pianoroll"].sum()) for d in got) > 0
    plain = dec.decode_paths(paths, 8, sample_method=method, **kw)
    assert sorted(plain[0]) == ["counts", "instr", "notes", "starts", "velocity", "z"]
    assert_same_songs(plain, dec.predict_songs(xs, 8, sample_method=method, **kw), method + " plain")
    for a, b in zip(plain, got):
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_device_anchors_and_the_wrappers(small_model):
    s, m, paths, xs, z = small_model
    dec = m.decoder
    want = dec.decode_paths(paths, 8)
    on_device = [dict(p, anchors=torch.from_numpy(p["anchors"]).to(DEV)) for p in paths]
    got = dec.decode_paths(on_device, 8)
    for a, b in zip(got, want):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # the two thin wrappers make the same paths: songs 0 and 1 of the run, decoded alone, are the same songs
    A0, A1 = paths[0]["anchors"], paths[1]["anchors"]
    med = dec.medleys([[A0[0:8], A0[8:16], A0[16:24]]], 4, batch_size=8)
    itp = dec.interpolation_songs([(A1[0], A1[1])], 10, batch_size=8)
    for a, b in ((med[0], want[0]), (itp[0], want[1])):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # device latents of encoded songs make a medley too
    dev_path = gen.medley_path([torch.from_numpy(A0[0:8]).to(DEV), torch.from_numpy(A0[8:16]).to(DEV), torch.from_numpy(A0[16:24]).to(DEV)], 4)
    again = dec.decode_paths([dev_path], 8)[0]
    assert all(np.array_equal(again[k], want[0][k]) for k in again)
    assert dec.decode_paths([]) == []
    with pytest.raises(ValueError):
        dec.decode_paths([gen.interpolation_path(np.zeros(16, np.float32), np.ones(16, np.float32), 3)])
    with pytest.raises(ValueError):
        dec.decode_paths(paths, seed=3)
    with pytest.raises(ValueError):
        gen.medley_path([torch.from_numpy(A0[0:8]).to(DEV), torch.from_numpy(A0[8:16]).to(DEV)], 4, mode="slerp")
