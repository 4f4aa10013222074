"""A live context takes the path on record.  For the small edge cases of tests/_plan_cases.py, fwi_create + fwi_destroy of
this build report the return code, error text, path line, kernel name and placed offsets that
tests/golden/plan_paths.json holds (tools/plan_table.py); tests/test_plan_host.py holds csrc/fwi_plan.cpp to the same
record without a GPU.  Only creation and destruction run: no kernel is launched."""
import json
import os
import sys

import pytest

import _plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_table  # noqa: E402

pytestmark = pytest.mark.gpu


def test_live_contexts_report_the_recorded_paths(gpu):
    from full_waveform_inversion_amd import _lib
    lib = _lib.load()
    with open(plan_table.GOLDEN) as f:
        entries = json.load(f)["entries"]
    cases = [c for c in pc.CASES if pc.small(c)]
    assert 36 <= len(cases) <= 120, len(cases)
    wrong = {c["id"]: (got, entries[c["id"]]) for c in cases for got in [plan_table.record(c, lib)] if got != entries[c["id"]]}
    assert not wrong, wrong
