#!/usr/bin/env python3
"""The launch list of the engine's calls, as text: the check that a schedule refactor moved nothing.

For every case below: build an engine, run a call three times from Python (``use_plans = False``), record the fourth under
``plan.Recorder`` and print one line per recorded C-ABI call - entry point, every argument, every field of every argument struct -
and a SHA-256 of the case.  Arguments and fields whose DECLARED ctypes type is a pointer (streams, events, buffers) print as the
index of that address's first appearance in the case: which of them coincide stays, the addresses go.  Everything else prints
verbatim.  Two checkouts that enqueue the same schedule print the same text:
    python tools/launch_trace.py > a.txt        (in each checkout, this file copied in)        diff a.txt b.txt
``--hashes``: only the per-case lines; ``--only TEXT``: only the cases whose name contains TEXT.  The run ends at the first failing case and is killed after ``--timeout`` seconds."""
import argparse, ctypes as C, hashlib, os, signal, struct, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_vae_amd  # noqa
from midi_vae_amd import hiplib as hl, plan
from midi_vae_amd.classifier import ClassifierEngine
from midi_vae_amd.engine import Engine
from midi_vae_amd.layout import ClassifierSpec, ModelSpec

B, T, Z = 32, 32, 16
BLOB_TYPES = {("mvae_prepare_batch", 0): hl.PrepJob}        # (struct arrays the signature declares as void *)


def _is_ptr(t):
    return t is C.c_void_p or t is C.c_char_p or issubclass(t, C._Pointer)


def _fields(st, canon):
    for name, t in st._fields_:
        v = getattr(st, name)
        if _is_ptr(t):
            yield "%s=%s" % (name, canon(v))
        elif issubclass(t, C.Structure):
            yield "%s={%s}" % (name, " ".join(_fields(v, canon)))
        elif t is C.c_float:
            yield "%s=f%s" % (name, struct.pack("<f", v).hex())
        else:
            yield "%s=%d" % (name, v)


def trace_lines(rec):
    """the recorded calls (and host marks) of ``rec`` as lines, pointers canonicalised by first appearance"""
    seen = {}
    canon = lambda v: "0" if not v else "p%d" % seen.setdefault(int(v), len(seen))
    marks = {}
    for idx, tag, st in rec.marks:
        marks.setdefault(idx, []).append("host %s stream=%s" % (tag, canon(st)))
    lines = []
    for i, (name, slots, blobs) in enumerate(rec.calls):
        lines += marks.pop(i, [])
        out = [name]
        for j, (t, v) in enumerate(zip(hl.SIGNATURES[name][1], slots)):
            if j in blobs:
                st = BLOB_TYPES.get((name, j)) or t._type_
                n, size = divmod(len(blobs[j]), C.sizeof(st))
                assert size == 0 and issubclass(st, C.Structure), (name, j)
                out.append("[%s]" % " | ".join(" ".join(_fields(st.from_buffer_copy(blobs[j], k * C.sizeof(st)), canon)) for k in range(n)))
            else:
                out.append(canon(v) if _is_ptr(t) else "%d" % v)
        lines.append(" ".join(out))
    for rest in marks.values():
        lines += rest
    return lines


def inputs(spec, B=B, seed=1):
    rng = np.random.default_rng(seed)
    u8 = lambda hi, *shape: rng.integers(0, hi, shape).astype(np.uint8)
    return dict(x_idx=u8(spec.Dout, B, spec.T), i_idx=u8(spec.ID, B, spec.V), vel=rng.random((B, spec.T)).astype(np.float32),
                eps=(rng.standard_normal((B, spec.Z)) * spec.epsilon_std).astype(np.float32), d_idx=u8(2, B, spec.T),
                hist=(rng.standard_normal((B, spec.Z)) * 0.1).astype(np.float32), c_idx=u8(spec.C, B), n_idx=u8(spec.Dout, B, spec.T),
                sig=rng.standard_normal((B, spec.SD)).astype(np.float32), add=rng.standard_normal((B, spec.add_dim)).astype(np.float32))


class _Hook(object):
    """an in-process gradient hook that takes the early decoder bucket (dp.BucketedAllReduce's surface) and reduces nothing"""
    overlap = True

    def early(self, grads):
        return None

    def __call__(self, grads):
        return None


def vae_case(kinds, dtype="bf16", knobs=None, training=True, hook=None, batch=B, **spec_kw):
    """``batch``: windows of the engines' max_batch and of every call but "train96" (a train step of 96 windows on the same engine:
    with a larger ``batch`` the call's padded batch differs from the engine's)"""
    B = batch
    spec = ModelSpec(**dict(dict(cell="GRU", H=256, Z=Z, T=T, V=4, C=2, Le=2, Ld=2, lr=1e-3), **spec_kw))
    raw = inputs(spec, B)
    train = Engine(spec, max_batch=B, dtype=dtype, seed=0) if training else None
    infer = Engine(spec, max_batch=B, dtype=dtype, seed=0, training=False, share=train)

    def stage(eng, n):
        sub = {k: v[:n] for k, v in raw.items()}
        eng.stage_encoder_inputs(sub["x_idx"], sub["i_idx"], sub["vel"], sub["eps"], d_idx=sub["d_idx"])
        eng.stage_decoder_inputs(n, hist=sub["hist"], add=sub["add"])
        eng.stage_targets(n, sub["x_idx"], sub["c_idx"], n_idx=sub["n_idx"], sig=sub["sig"])
    for eng in (train, infer):
        if eng is None:
            continue
        eng.use_plans = False
        for k, v in (knobs or {}).items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        stage(eng, B)

    def decode(**kw):
        infer.stage_decoder_inputs(B, hist=raw["hist"], z=raw["hist"], add=raw["add"])
        infer.decode(B, **kw)
    calls = {"train": lambda: train.train_step(B, allreduce=hook), "train96": lambda: train.train_step(96, allreduce=hook), "eval": lambda: infer.eval_step(B), "encode": lambda: infer.encode(B),
             "decode": decode, "decode_argmax": lambda: decode(want_probs=False)}
    for kind in kinds:
        if kind == "train96":       # (restaged here, outside the recorded call: the generator runs on as the case gets to this kind)
            stage(train, 96)
        yield kind, calls[kind], (train if kind.startswith("train") else infer)


def classifier_case():
    spec = ClassifierSpec(K=61, T=T, C=2, H=256, L=2, lr=1e-3)
    eng = ClassifierEngine(spec, max_batch=B, dtype="bf16", seed=0)
    eng.use_plans = False
    rng = np.random.default_rng(2)
    eng.stage(rng.integers(0, 61, (B, T)).astype(np.uint8), rng.integers(0, 2, (B,)).astype(np.uint8))
    yield "train", lambda: eng.train_step(B), eng


ALL = ("train", "eval", "encode", "decode")
CASES = [("%s %s" % (cell, tag), lambda cell=cell, knobs=knobs: vae_case(ALL, cell=cell, knobs=knobs))
         for cell in ("LSTM", "GRU")
         for tag, knobs in (("default", {}), ("defer_grads_rows=0", dict(defer_grads_rows=0)), ("phase_multi=False", dict(phase_multi=False)),
                            ("pipeline=False", dict(pipeline=False)), ("phase_max_B=16", dict(phase_max_B=16)),
                            ("fused_latent=False", dict(fused_latent=False)),
                            # (defer_grads_rows = 0: the gradient GEMMs run beside the recurrences, K-streaming may be on)
                            ("phase_multi=False defer_grads_rows=0", dict(phase_multi=False, defer_grads_rows=0)),
                            ("phase_multi=False defer_grads_rows=0 grad_portions=2", dict(phase_multi=False, defer_grads_rows=0, grad_portions=2)),
                            ("kstream_grads=False defer_grads_rows=0", dict(kstream_grads=False, defer_grads_rows=0)))]
# an engine larger than the call: 512 windows (per-queue schedule, ordinary gradient GEMMs), then 96 on the same engine
CASES += [("%s max_batch=512 defer_grads_rows=0" % cell,
           lambda cell=cell: vae_case(("train", "train96"), cell=cell, batch=512, knobs=dict(defer_grads_rows=0))) for cell in ("LSTM", "GRU")]
CASES += [
    ("GRU H=64 f32", lambda: vae_case(ALL, dtype="f32", H=64)),
    ("LSTM comp_notes", lambda: vae_case(ALL, cell="LSTM", comp_notes=True)),
    ("GRU meta_held meta_next", lambda: vae_case(ALL, meta_held=True, meta_next=True)),
    ("LSTM bidirectional Le=3", lambda: vae_case(ALL, cell="LSTM", bidirectional=True, Le=3)),
    ("GRU signature SD=5", lambda: vae_case(ALL, signature=True, SD=5)),
    ("LSTM Le=1", lambda: vae_case(ALL, cell="LSTM", Le=1)),
    ("LSTM forward-only head_slices=2 phase_multi=False",
     lambda: vae_case(("eval", "encode", "decode_argmax"), cell="LSTM", training=False, knobs=dict(head_slices=2, phase_multi=False))),
    ("GRU classifier", classifier_case),
    ("GRU early-bucket hook defer_grads_rows=0", lambda: vae_case(("train",), knobs=dict(defer_grads_rows=0), hook=_Hook())),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", action="store_true", help="print the per-case SHA-256 lines only")
    ap.add_argument("--timeout", type=int, default=120, help="seconds after which the process is killed (SIGALRM)")
    ap.add_argument("--only", default="", help="run only the cases whose name contains this text")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    for name, make in CASES:
        if a.only and a.only not in name:
            continue
        lines = []
        for kind, call, eng in make():
            for _ in range(3):
                call()
            with plan.Recorder() as rec:
                call()
            torch.cuda.synchronize()
            eng.check_pipeline()        # (raises: a kernel gave up waiting - the run ends at this case)
            assert rec.calls, (name, kind)
            lines += ["%s | %s | %s" % (name, kind, ln) for ln in trace_lines(rec)]
        if not a.hashes:
            print("\n".join(lines))
        print("sha256 %s  %s (%d calls)" % (hashlib.sha256("\n".join(lines).encode()).hexdigest(), name, len(lines)), flush=True)
