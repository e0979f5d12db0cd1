"""Every tw_stage_* entry point (and tw_debug_png_kernel_time) over the tour of tools/stage_calls.py, call by call, against
tests/golden/stage_calls_parent.json: what the library returned, launched and refused at every step of the same tour before
the entry points moved onto one stage scaffold (csrc/twflow_stage.hip.h) and the span-grid chain's arguments into one place
each (profiles/stage_scaffold.md).  A step holds the status, the tw_last_error text of a refused call, the launches per
family with the grid z of each family's last one, and a SHA-256 of everything the call returned, guard regions included.
The recorded library repeated every step of the tour from run to run, so every step keeps its hash.  Integers, texts and
hashes: no tolerance."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stage_calls as SC  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_stage_call_equals_the_parents(twflow):
    with open(os.path.join(ROOT, "tests", "golden", "stage_calls_parent.json")) as f:
        want = json.load(f)
    got = SC.tour(twflow)
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, mine), (_, parents) in zip(got, want):
        assert mine == parents, name
