"""What the tests of the host layer's per-pair extras (tests/test_host_{regions,residual,shift,shift_bands,overlay}.py) share:
one consumer on the stub backend, fed by tools/consumer_probe.cpp and recorded call for call (TW_STUB_TRACE), through the
cases of tools/consumer_trace.py — and the rule they all begin with, that an extra that is off leaves the calls of the commit
before the ignore regions (tests/golden/consumer_trace_parent.json).  Not a conftest: each test module says what it uses.
"""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
ADDON = os.path.join(HOST, "build", "Release", "tidalwave.node")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import consumer_trace as CT  # noqa: E402

needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                                reason="node or the built addon is not available")
PARENT_CASES = ("fast_ten_rgb", "raw_mixed_with_files", "narrower3_png_reconcile1", "device_jpeg1", "three_sizes_interleaved",
                "resident_twelve_share_expected", "busy_at_third_submit")


def make_world(tmp_path_factory, name):
    """the probe built as host/build/consumer_probe_<name>, and the cases' files in a directory of this module's own"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    d = str(tmp_path_factory.mktemp("host_" + name))
    exe = CT.build(os.path.join(HOST, "build", "consumer_probe_" + name))
    f = CT.write_files(d)
    return {"exe": exe, "dir": d, "files": f, "cases": CT.cases(f)}


def run(world, case, threads=1):
    """(response lines without the closing counter line, the trace's lines)"""
    out, trace = CT.run_case(world["exe"], case, threads, world["dir"])
    return out.strip().splitlines()[:-1], trace.strip().splitlines()


def name_of(t):
    return t.split(" ", 2)[1]


def calls(trace, name):
    return [t for t in trace if name_of(t) == name]


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def row(out, text):
    """what the goldens hold of a run"""
    return {"responses": CT.sha(out), "trace": CT.sha(text), "lines": text.count("\n")}


def assert_off_is_the_parent(world, not_in_trace, not_in_out, also_off=()):
    """PARENT_CASES as they stand make the parent's calls, with nothing of the extra in the trace or in the responses; and so
    does fast_ten_rgb under each of `also_off`, functions that switch the extra on with a value that means off"""
    parent = golden("consumer_trace_parent.json")
    for name in PARENT_CASES:
        out, text = CT.run_case(world["exe"], world["cases"][name], 1, world["dir"])
        assert not any(n in text for n in not_in_trace) and not_in_out not in out
        assert row(out, text) == parent[name], name
    for turn in also_off:
        out, text = CT.run_case(world["exe"], turn(world["cases"]["fast_ten_rgb"]), 1, world["dir"])
        assert row(out, text) == parent["fast_ten_rgb"]
