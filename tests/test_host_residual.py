"""The residual in the host layer (Parameter::extras.residual / ::residualMin, Response::changes, new TidalWave({residual: tol,
residualMin: n}), the CLI's -residual / -residualMin), asserted from the engine's side as tests/test_host_regions.py does:
the stub backend records every call of the C ABI (TW_STUB_TRACE) and tools/consumer_probe.cpp feeds one consumer.  CPU only.

With the setting off a consumer makes exactly the calls it made before: tests/golden/consumer_trace_parent.json holds the
hashes of the commit before the ignore regions, and the probe's existing cases must still produce them.
"""
import json
import os
import subprocess

import pytest

import host_probe as HP
from host_probe import CT, HOST, ROOT, calls, needs_node, run


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return HP.make_world(tmp_path_factory, "residual")


def test_residual_off_makes_the_calls_of_the_parent_cases(world):
    # ... and "D 0 0" is off too; residualMin without the residual changes nothing
    HP.assert_off_is_the_parent(world, ("tw_ticket_changes", "tw_set_option"), " changes ",
                                [lambda c: CT.with_residual(c, 0, 0), lambda c: CT.with_residual(c, 0, 5)])


@pytest.mark.parametrize("name", ["fast_ten_rgb", "raw_mixed_with_files", "resident_twelve_share_expected", "damaged_both"])
def test_residual_on_sets_the_option_once_and_asks_before_each_collecting_wait(world, name):
    case = world["cases"][name]
    lines_off, trace_off = run(world, case)
    lines_on, trace_on = run(world, CT.with_residual(case, 12))
    opt = calls(trace_on, "tw_set_option")
    assert len(opt) == 1 and "option=4 value=12 -> OK" in opt[0]
    created = [i for i, t in enumerate(trace_on) if t.split(" ", 2)[1] == "tw_engine_create"]
    assert len(created) == 1 and trace_on.index(opt[0]) == created[0] + 1  # directly after the engine exists
    waits = calls(trace_on, "tw_wait")
    asks = calls(trace_on, "tw_ticket_changes")
    assert len(asks) == len(waits) == len(calls(trace_off, "tw_wait")) > 0
    # one tw_ticket_changes directly in front of each collecting wait, for the wait's ticket
    for w in waits:
        i = trace_on.index(w)
        prev = trace_on[i - 1].split(" ")
        assert prev[1] == "tw_ticket_changes" and prev[2] == w.split(" ")[2], (trace_on[i - 1], w)
    # every other call is what it was, in the order it was
    rest = lambda tr: [t for t in tr if t.split(" ", 2)[1] not in ("tw_ticket_changes", "tw_set_option")]  # noqa: E731
    assert rest(trace_on) == rest(trace_off)
    # the responses: what they were, plus the stub's one echo record (n_diff = n_unexplained = the tolerance)
    assert len(lines_on) == len(lines_off)
    for on, off in zip(lines_on, lines_off):
        if off.startswith("ERROR"):
            assert on == off
            continue
        head, _, tail = on.partition(" changes ")
        assert head == off
        assert tail.startswith("1: [") and " diff=12 unexplained=12 " in tail
    if name == "damaged_both":
        assert any(ln.startswith("ERROR") for ln in lines_on) and any(" changes 1:" in ln for ln in lines_on)


def test_regions_and_residual_together(world):
    env, budget, script = world["cases"]["fast_ten_rgb"]
    lines, trace = run(world, (env, budget, ["G", 2, "D", 7, 0] + list(script)))
    opts = calls(trace, "tw_set_option")
    assert len(opts) == 2 and "option=3 value=2" in opts[0] and "option=4 value=7" in opts[1]
    waits = calls(trace, "tw_wait_regions")
    assert len(waits) == 10 and not calls(trace, "tw_wait") and len(calls(trace, "tw_ticket_changes")) == 10
    for w in waits:
        assert trace[trace.index(w) - 1].split(" ")[1] == "tw_ticket_changes"
    assert all(" regions " in ln and " changes 1:" in ln and ln.index(" regions ") < ln.index(" changes ") for ln in lines)


def test_the_status_rule_of_residual_min(world):
    """The stub answers a vector only for a pair whose first bytes differ, and one change record with `tol` unexplained pixels
    for every pair: an equal pair is OK without residualMin and above the record's count, SUSPICIOUS from the count down."""
    env, budget, _ = world["cases"]["fast_ten_rgb"]
    script = ["M", CT.W, CT.H, 10, 10, "M", CT.W, CT.H, 10, 99]  # an equal pair, a differing one
    for tol, minimum, want in ((12, 0, "OK"), (12, 13, "OK"), (12, 12, "SUSPICIOUS"), (12, 1, "SUSPICIOUS")):
        lines, _ = run(world, (env, budget, ["D", tol, minimum] + script))
        status = sorted(ln.split("|")[0] for ln in lines)
        assert status == sorted([want, "SUSPICIOUS"]), (tol, minimum, lines)
        assert all(" changes 1:" in ln for ln in lines)


def test_a_tolerance_the_engine_refuses_leaves_the_consumer_without_an_engine(world):
    lines, trace = run(world, CT.with_residual(world["cases"]["fast_ten_rgb"], 255))
    assert all(ln.startswith("ERROR|engine: residual: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_ticket_changes")


def node(script, *args, timeout=120):
    return subprocess.run(["node", "-e", script, *args], cwd=HOST, capture_output=True, text=True, timeout=timeout)


@needs_node
def test_cli_parsing_and_pass_through():
    r = node("""
var C=require('./commandline');
console.log(JSON.stringify([C.getArgs(['-residual','16','-residualMin','50','a','b']), C.getArgs(['--residual=8','a','b']),
  C.getArgs(['a','b'])]));
""")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got[0] == {"expect_path": "a", "target_path": "b", "options": {"residual": 16, "residualMin": 50}}
    assert got[1]["options"] == {"residual": 8} and got[2]["options"] == {}
    # through the whole CLI: an unreadable pair answers as without the option
    r = subprocess.run(["node", "commandline.js", "-residual", "16", "/nonexistent/a.png", "/nonexistent/b.png"],
                       cwd=HOST, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
    assert docs[0] == {"status": "ERROR", "reason": "Can't open /nonexistent/a.png"}
    assert docs[-1] == {"request": 1, "data": 0, "error": 1}


@needs_node
def test_index_js_hands_the_options_to_the_addon(tmp_path):
    (tmp_path / "a.png").write_bytes(b"x")
    r = node("""
var seen=[], P=require('path');
function Fake(o){ seen.push([o && o.residual, o && o.residualMin]); }
Fake.prototype.calc=function(){ var s=this; setImmediate(function(){s.emit('error',{})}); };
Fake.prototype.dispose=function(){ var s=this; setImmediate(function(){s.emit('finish',{})}); };
var id=require.resolve('./build/Release/tidalwave');
require.cache[id]={id:id, filename:id, loaded:true, exports:{TidalWave:Fake}};
var T=require('./index');
var t=T.create(process.argv[1], {expectDir: process.argv[1], residual: 16, residualMin: 40});
t.on('finish',function(){ var u=T.create(process.argv[1], {expectDir: process.argv[1]});
  u.on('finish',function(){ console.log(JSON.stringify(seen)); }); });
""", str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [[16, 40], [None, None]]


REFERENCE_KEYS = ["status", "span", "threshold", "expect_image", "target_image", "time", "height", "width", "vector"]


@needs_node
@pytest.mark.gpu
def test_result_object_of_the_golden_pair_through_the_cli():
    """commandline.js -> index.js -> the addon -> a consumer -> the engine: with -residual the result carries `change` behind
    the reference's keys; without it the keys and their order are the reference's."""
    tree = os.path.join(ROOT, "tests", "golden", "tree")
    pair = [os.path.join(tree, "expected", "scenario2", "capture2.png"), os.path.join(tree, "revision2", "scenario2", "capture2.png")]
    with open(os.path.join(ROOT, "tests", "golden", "expected_responses.json")) as f:
        gold = json.load(f)["revision2_capture2"]

    def cli(*more):
        r = subprocess.run(["node", "commandline.js", *more, "-threshold", "5", "-span", "10", "-pyrLevels", "3"] + pair,
                           cwd=HOST, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
        assert docs[-1] == {"request": 1, "data": 1, "error": 0}
        return docs[0]

    on = cli("-residual", "16")
    assert list(on.keys()) == REFERENCE_KEYS + ["change"]
    assert on["vector"] == gold["vector"] and len(on["change"]) > 0
    assert all(list(c.keys()) == ["x", "y", "diff", "unexplained", "maxDiff", "maxUnexplained"] for c in on["change"])
    assert all(c["x"] % 10 == 0 and c["y"] % 10 == 0 and 1 <= c["diff"] <= 100 and c["unexplained"] <= c["diff"] for c in on["change"])
    both = cli("-residual", "16", "-regions", "1")
    assert list(both.keys()) == REFERENCE_KEYS + ["regions", "change"] and both["change"] == on["change"]
    off = cli()
    assert list(off.keys()) == REFERENCE_KEYS and off["vector"] == gold["vector"]
