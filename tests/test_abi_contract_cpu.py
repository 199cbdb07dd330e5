"""The C ABI's refusals, without a device: every row of tests/abi_contract.py against the library in the tree.

With no device a call that passes validation fails at its first launch (MVAE_E_LAUNCH, -3) and no host code reads a device pointer,
so the baselines run on addresses nothing maps: -3 is "well-formed", and a violation must come back with its promised code instead -
-3 there means the call got past validation, whether the refusal is missing or merely comes after a fill or an earlier launch.

The whole module is skipped wherever a device is visible: there a missing refusal would launch a kernel on the fake addresses."""
import ctypes as C
import os
import re

import pytest
import torch

import midi_vae_amd  # noqa: F401
from midi_vae_amd import hiplib as hl
from tests import abi_contract as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_count():
    """hipGetDeviceCount of the HIP runtime the library has linked (found among the objects mapped into this process)"""
    hl.load()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert paths, "libmidivae_hip.so links no HIP runtime?"
    n = C.c_int(0)
    rc = C.CDLL(sorted(paths)[0]).hipGetDeviceCount(C.byref(n))
    return 0 if rc != 0 else n.value


if torch.cuda.is_available() or _device_count() > 0:
    pytest.skip("a device is visible: the fake addresses of this module must never reach a kernel", allow_module_level=True)

ROWS = ac.rows()


@pytest.mark.parametrize("entry", ac.ENTRIES, ids=[e.label for e in ac.ENTRIES])
def test_baseline_is_well_formed(entry):
    """... so that each violation is the only thing wrong with its call; the forms the product relies on stay accepted"""
    if not entry.cpu_baseline:
        return          # (mvae_streams_alias synchronises, mvae_occupancy asks the device: refusals only)
    lib = hl.load()
    assert ac.run_baseline(lib, entry) == hl.E_LAUNCH, entry.label
    for name, mutate, does in entry.accepted:
        c = entry.build(ac.FakeAlloc())
        mutate(c)
        assert c.invoke(lib) == (hl.E_LAUNCH if does is ac.LAUNCH else 0), "%s: '%s' must stay accepted (%s)" % (entry.label, name, does)


@pytest.mark.parametrize("entry,v", ROWS, ids=["%s: %s" % (e.label, v.name) for e, v in ROWS])
def test_violation_is_refused_with_its_code(entry, v):
    rc = ac.run_violation(hl.load(), entry, v)
    how = "got past validation: it would have enqueued" if rc in (hl.E_LAUNCH, 0) else "the wrong code"
    assert rc == v.code, "%s, %s: returned %d, promised %d - %s.  Header: \"%s\"" % (entry.label, v.name, rc, v.code, how, v.why)


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "midivae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mvae_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_entry_point_is_in_the_table_or_exempt():
    declared, table = set(_declared_symbols()), {e.fn for e in ac.ENTRIES}
    assert len(declared) >= 60
    assert not table & set(ac.EXEMPT), "both in the table and exempt: %s" % sorted(table & set(ac.EXEMPT))
    assert table | set(ac.EXEMPT) == declared, ("neither in the table nor exempt: %s; not declared: %s"
                                                % (sorted(declared - table - set(ac.EXEMPT)), sorted((table | set(ac.EXEMPT)) - declared)))
    assert all(reason for reason in ac.EXEMPT.values())
    # every stream-taking entry point is in the table: an exemption is for what launches nothing
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midivae_hip.h")).read(), flags=re.S)
    for name in ac.EXEMPT:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert "stream" not in proto or name.startswith(("mvae_event_", "mvae_stream_wait_event")), name
    for e in ac.ENTRIES:
        names = [v.name for v in e.violations]
        assert len(set(names)) == len(names), (e.label, sorted(n for n in names if names.count(n) > 1))
        for v in e.violations:
            assert v.code in (hl.E_ARG, hl.E_UNSUPPORTED) and v.why, (e.label, v.name)


def test_every_pointer_and_integer_a_baseline_passes_is_the_subject_of_a_row():
    """derived from hiplib.SIGNATURES and the ctypes structs, not from what the table says of itself: per entry point (its baselines
    taken together) every pointer handed over is NULLed by some row and every integer changed by some row, unless the header leaves
    it optional / unlimited (abi_contract.OPTIONAL / UNLIMITED, each with the header's words).  And what a row flagged ``safe`` does
    is looked at, not its name: it NULLs no pointer and moves none."""
    nulled, changed, passed = {}, {}, {}
    for e in ac.ENTRIES:
        base = ac.slots(e.build(ac.FakeAlloc()))
        for k, (kind, val) in base.items():
            if val:
                passed.setdefault(e.fn, {})[k[1]] = kind
        for v in e.violations:
            c = e.build(ac.FakeAlloc())
            v.mutate(c)
            for k, (kind, val) in ac.slots(c).items():
                if k not in base or base[k][1] == val:
                    continue
                changed.setdefault(e.fn, set()).add(k[1])
                if kind == "ptr" and base[k][1]:          # (a NULL slot given a buffer the baseline owns is no such thing)
                    assert not v.safe, "a row that runs on a device NULLs or moves %s: %s, %s" % (k[1], e.label, v.name)
                if kind == "ptr" and not val:
                    nulled.setdefault(e.fn, set()).add(k[1])
    for fn, fields in passed.items():
        for f, kind in fields.items():
            if kind == "ptr":
                assert f in nulled.get(fn, ()) or f in ac.OPTIONAL.get(fn, {}), "%s: no row passes %s = NULL, and it is not optional" % (fn, f)
            else:
                assert f in changed.get(fn, ()) or f in ac.UNLIMITED.get(fn, {}), "%s: no row changes %s, and it is not unlimited" % (fn, f)
    for table in (ac.OPTIONAL, ac.UNLIMITED):
        for fn, fields in table.items():
            assert fn in passed and set(fields) <= set(passed[fn]) and all(fields.values()), fn


def test_the_three_findings_of_the_probe_are_rows_that_may_run_on_a_device():
    safe = {(e.label, v.name) for e, v in ROWS if v.safe}
    assert ("mvae_sum_over_time", "kind = 7, accumulate = 0") in safe
    assert ("mvae_gemm[self-splitting store]", "a_kind = 7") in safe
    assert ("mvae_prepare_batch", "job 64 of 65: op = 99") in safe


class _Stub:
    """a "library" whose every entry point returns one code"""

    def __init__(self, code):
        self.code = code

    def __getattr__(self, name):
        assert name in hl.SIGNATURES, name
        return lambda *args: self.code


def test_a_library_that_accepts_everything_fails_every_row():
    """the checker on a planted fault: no refusal anywhere (every call "gets past validation")"""
    bad = ac.check_library(_Stub(hl.E_LAUNCH))
    rows = {(e.label, v.name) for e, v in ROWS}
    assert {(lab, what) for lab, what, _ in bad} & rows == rows
    assert all("got past validation" in msg and "Header" in msg for lab, what, msg in bad if (lab, what) in rows)
    # ... and every form that must return MVAE_OK without a launch
    assert {(lab, what) for lab, what, _ in bad} - rows == {(e.label, n) for e in ac.ENTRIES for n, _, does in e.accepted if does is ac.NOTHING}
    bad = ac.check_library(_Stub(0))
    assert {(lab, what) for lab, what, _ in bad if what != "baseline" and (lab, what) in {(e.label, v.name) for e, v in ROWS}} == \
        {(e.label, v.name) for e, v in ROWS}


def test_a_library_that_refuses_everything_fails_every_baseline():
    bad = ac.check_library(_Stub(hl.E_ARG))
    assert {lab for lab, what, _ in bad if what == "baseline"} == {e.label for e in ac.ENTRIES if e.cpu_baseline}
    # ... and every row that promises the other code, and every accepted form
    assert {(lab, what) for lab, what, _ in bad} >= {(e.label, v.name) for e, v in ROWS if v.code != hl.E_ARG}
    assert {(lab, what) for lab, what, _ in bad} >= {(e.label, n) for e in ac.ENTRIES if e.cpu_baseline for n, _, does in e.accepted if does is ac.LAUNCH}
