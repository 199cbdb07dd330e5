"""Every schedule knob keys the step plans: Engine.knobs (knobs.py) is the dict the engine's attributes were set from, and
engine_plan._plan_state iterates its names - a knob changed on a live engine must select other plans, never replay the launch list
recorded under the old value.  Nothing is launched here beyond building one small engine."""
import pytest

import midi_vae_amd  # noqa: F401
from midi_vae_amd.engine import Engine
from midi_vae_amd.layout import ModelSpec

pytestmark = pytest.mark.gpu


def test_changing_any_knob_changes_the_plan_key_and_restoring_it_restores_the_key():
    eng = Engine(ModelSpec(cell="GRU", H=64, Z=16, T=8, V=4, C=2), max_batch=16, dtype="f32")
    assert len(eng.knobs) >= 25
    base = eng._plan_state()
    for name in eng.knobs:
        old = getattr(eng, name)
        assert type(old) in (bool, int), (name, old)
        new = (not old) if isinstance(old, bool) else old + 1
        setattr(eng, name, new)
        assert eng._plan_state() != base, name
        setattr(eng, name, old)
        assert eng._plan_state() == base, name
