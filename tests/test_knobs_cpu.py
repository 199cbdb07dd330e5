"""The engine's schedule knobs (midi-vae_amd/knobs.py): the defaults the engine used to compute inside ``Engine.__init__``, the
four environment overrides, and the names - which are the step plans' key (engine_plan._plan_state iterates them).  No GPU."""
import types

import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd.knobs import schedule_knobs

GATES = {"GRU": 3, "LSTM": 4}


def _spec(cell="GRU", H=256, T=64):
    return types.SimpleNamespace(cell=cell, H=H, T=T, GH=GATES[cell] * H)


@pytest.mark.parametrize("maxB,T,want", [(256, 64, 16), (512, 64, 32), (2048, 96, 32), (2048, 48, 16), (2048, 128, 64)])
def test_pipe_chunk_grows_with_the_batch_and_divides_the_sequence(maxB, T, want):
    assert schedule_knobs(_spec(T=T), maxB, env={})["pipe_chunk"] == want


def test_defaults_that_depend_on_the_model():
    gru, lstm = schedule_knobs(_spec("GRU"), 256, env={}), schedule_knobs(_spec("LSTM"), 256, env={})
    assert (gru["kstream_wgs"], lstm["kstream_wgs"]) == (16, 32)
    assert (lstm["head_slices"], gru["head_slices"]) == (2, 4)
    assert (lstm["pipe_proj_blocks"], gru["pipe_proj_blocks"]) == (64, 48)
    assert schedule_knobs(_spec("GRU", H=64), 256, env={})["pipe_proj_blocks"] == 8


def test_fixed_defaults():
    k = schedule_knobs(_spec(), 256, env={})
    want = dict(defer_grads_rows=32768, kstream_rows=2048, phase_max_B=256, kstream_max_B=256, pace_mask=6, pace_mask_split=2)
    assert {n: k[n] for n in want} == want
    assert (k["kstream_grads"], k["_diag_no_param_grads"], k["use_plans"]) == (True, False, True)


@pytest.mark.parametrize("var,value,name,want", [("MVAE_KSTREAM_GRADS", "0", "kstream_grads", False),
                                                 ("MVAE_DEFER_GRADS_ROWS", "4096", "defer_grads_rows", 4096),
                                                 ("MVAE_DIAG_NO_PARAM_GRADS", "1", "_diag_no_param_grads", True),
                                                 ("MVAE_PLANS", "0", "use_plans", False)])
def test_an_environment_override_changes_exactly_its_own_entry(var, value, name, want):
    base, got = schedule_knobs(_spec(), 256, env={}), schedule_knobs(_spec(), 256, env={var: value})
    assert got[name] == want != base[name]
    assert {n: v for n, v in got.items() if n != name} == {n: v for n, v in base.items() if n != name}


# what engine_plan._PLAN_CONFIG held before the key was derived from the knob dict, minus the switches folded into constants
# (multi_stream, lean_sync, fuse_head_bwd, fuse_bias_grad, gate_pipe_gemms, gate_side_heads, hold_side_heads, _hold_dec_grads,
# kstream_singles, dec_kstream, pace_early)
PLAN_CONFIG_BEFORE = ("head_slices", "grad_portions", "index_dense", "index_dense_blocks", "xpand_blocks", "pipe_chunk", "phase_max_B",
                      "kstream_grads", "kstream_wgs", "kstream_rows", "kstream_max_B", "flush_before_join", "pipe_gemm_blocks",
                      "pipe_proj_blocks", "time_chunks", "fused_latent", "_diag_no_param_grads", "use_plans", "defer_grads_rows",
                      "defer_early", "defer_early_rows", "defer_split_wgs", "pace_mask", "pace_mask_split", "_pace_mask_now")


def test_every_name_that_keyed_the_plans_is_a_knob():
    for cell in ("GRU", "LSTM"):
        names = set(schedule_knobs(_spec(cell), 256, env={}))
        assert names >= set(PLAN_CONFIG_BEFORE), set(PLAN_CONFIG_BEFORE) - names


def test_the_environment_is_only_read_through_the_argument(monkeypatch):
    monkeypatch.setenv("MVAE_DEFER_GRADS_ROWS", "1")
    assert schedule_knobs(_spec(), 256, env={})["defer_grads_rows"] == 32768
    assert schedule_knobs(_spec(), 256)["defer_grads_rows"] == 1


def test_a_default_schedule_state_has_nothing_armed():
    """engine_schedule.py: what the engine holds outside a call - the values Engine.__init__ used to give the loose attributes"""
    from midi_vae_amd.engine_schedule import CallState, PhaseState
    call, ph = CallState(), PhaseState()
    assert {n: getattr(call, n) for n in CallState.__slots__} == dict(
        deferred_gemms=None, deferred_small=[], deferred_side=None, after_chain=None, tail_streams=[])
    assert {n: getattr(ph, n) for n in PhaseState.__slots__} == dict(
        n_side=0, grad_streams=None, prefork=None, hold_side=False, kstream_extra=None, grad_portion_jobs=None, single_slot=0,
        single_slot_end=3, top_publish=None, last_stack_gate=None)
    assert CallState().tail_streams is not call.tail_streams      # (no list is shared between instances)
    assert PhaseState(n_side=2).n_side == 2
    with pytest.raises(AttributeError):
        ph.no_such_field = 1
