"""Hit regions in the host layer (Parameter::extras.regions, Response::regions / regionOf, new TidalWave({regions: gap}), the CLI's
-regions), asserted from the engine's side as tests/test_host_ignore.py does: the stub backend records every call of the C
ABI (TW_STUB_TRACE) and tools/consumer_probe.cpp feeds one consumer.  CPU only, except for the last test: the result object of
the real addon, through the CLI on the golden pair, needs the GPU.

With the setting off a consumer makes exactly the calls it made before: tests/golden/consumer_trace_parent.json holds the
hashes of the commit before the ignore regions, and the probe's existing cases must still produce them.
"""
import json
import os
import subprocess

import pytest

import host_probe as HP
from host_probe import CT, HOST, ROOT, calls, needs_node, run

W, H = CT.W, CT.H


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return HP.make_world(tmp_path_factory, "regions")


def test_regions_off_makes_the_calls_of_the_parent_cases(world):
    # ... and "G 0" is off too
    HP.assert_off_is_the_parent(world, ("tw_wait_regions", "tw_set_option"), " regions ", [lambda c: CT.with_regions(c, 0)])


@pytest.mark.parametrize("name", ["fast_ten_rgb", "raw_mixed_with_files", "resident_twelve_share_expected", "damaged_both"])
def test_regions_on_sets_the_option_once_and_collects_with_wait_regions(world, name):
    env, budget, script = world["cases"][name]
    lines_off, trace_off = run(world, (env, budget, script))
    lines_on, trace_on = run(world, (env, budget, ["G", 2] + list(script)))
    opt = calls(trace_on, "tw_set_option")
    assert len(opt) == 1 and "option=3 value=2 -> OK" in opt[0]
    created = [i for i, t in enumerate(trace_on) if t.split(" ", 2)[1] == "tw_engine_create"]
    assert len(created) == 1 and trace_on.index(opt[0]) == created[0] + 1  # directly after the engine exists
    assert not calls(trace_on, "tw_wait") and not calls(trace_off, "tw_wait_regions")
    waits_on, waits_off = calls(trace_on, "tw_wait_regions"), calls(trace_off, "tw_wait")
    assert len(waits_on) == len(waits_off) > 0
    # every other call is what it was, in the order it was
    rest = lambda tr: [t for t in tr if t.split(" ", 2)[1] not in ("tw_wait", "tw_wait_regions", "tw_set_option")]  # noqa: E731
    assert rest(trace_on) == rest(trace_off)
    # the responses: what they were, plus the regions of the pairs that were answered
    assert len(lines_on) == len(lines_off)
    seen = 0
    for on, off in zip(lines_on, lines_off):
        if off.startswith("ERROR"):
            assert on == off
            continue
        head, _, tail = on.partition(" regions ")
        assert head == off
        nvec = off.count("(")
        if nvec:
            # the stub reports one vector (x = the width, y = the device): one region of one 1 x 1 cell, its own peak
            assert nvec == 1 and tail.startswith("1: [") and tail.endswith(" of: 0") and " n=1 peak=(" in tail
            seen += 1
        else:
            assert tail == "0: of:"
    assert seen > 0 or name == "damaged_both"  # (that case's readable pairs are all equal: errors and empty answers)
    if name == "damaged_both":
        assert any(ln.startswith("ERROR") for ln in lines_on) and any(ln.endswith(" regions 0: of:") for ln in lines_on)


def test_a_gap_the_engine_refuses_leaves_the_consumer_without_an_engine(world):
    env, budget, script = world["cases"]["fast_ten_rgb"]
    lines, trace = run(world, (env, budget, ["G", 9] + list(script)))
    assert all(ln.startswith("ERROR|engine: regions: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_wait_regions")


def node(script, *args, timeout=120):
    return subprocess.run(["node", "-e", script, *args], cwd=HOST, capture_output=True, text=True, timeout=timeout)


@needs_node
def test_cli_regions_parsing_and_pass_through():
    r = node("""
var C=require('./commandline');
console.log(JSON.stringify([C.getArgs(['-regions','2','a','b']), C.getArgs(['--regions=1','-span','4','a','b']),
  C.getArgs(['a','b'])]));
""")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got[0] == {"expect_path": "a", "target_path": "b", "options": {"regions": 2}}
    assert got[1]["options"] == {"regions": 1, "span": 4} and got[2]["options"] == {}
    # through the whole CLI: an unreadable pair answers as without the option
    r = subprocess.run(["node", "commandline.js", "-regions", "1", "/nonexistent/a.png", "/nonexistent/b.png"],
                       cwd=HOST, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
    assert docs[0] == {"status": "ERROR", "reason": "Can't open /nonexistent/a.png"}
    assert docs[-1] == {"request": 1, "data": 0, "error": 1}


@needs_node
def test_index_js_hands_the_option_to_the_addon(tmp_path):
    (tmp_path / "a.png").write_bytes(b"x")
    r = node("""
var seen=[], P=require('path');
function Fake(o){ seen.push(o && o.regions); }
Fake.prototype.calc=function(){ var s=this; setImmediate(function(){s.emit('error',{})}); };
Fake.prototype.dispose=function(){ var s=this; setImmediate(function(){s.emit('finish',{})}); };
var id=require.resolve('./build/Release/tidalwave');
require.cache[id]={id:id, filename:id, loaded:true, exports:{TidalWave:Fake}};
var T=require('./index');
var t=T.create(process.argv[1], {expectDir: process.argv[1], regions: 3});
t.on('finish',function(){ var u=T.create(process.argv[1], {expectDir: process.argv[1]});
  u.on('finish',function(){ console.log(JSON.stringify(seen)); }); });
""", str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [3, None]


REFERENCE_KEYS = ["status", "span", "threshold", "expect_image", "target_image", "time", "height", "width", "vector"]


@needs_node
@pytest.mark.gpu
def test_result_object_of_the_golden_pair_through_the_cli():
    """commandline.js -> index.js -> the addon -> a consumer -> the engine: with -regions the result carries `regions` behind
    `vector` — the records of tests/golden/regions_golden.json, key for key — and every vector its `region`; without it the
    keys and their order are the reference's."""
    tree = os.path.join(ROOT, "tests", "golden", "tree")
    pair = [os.path.join(tree, "expected", "scenario2", "capture2.png"), os.path.join(tree, "revision2", "scenario2", "capture2.png")]
    with open(os.path.join(ROOT, "tests", "golden", "expected_responses.json")) as f:
        gold = json.load(f)["revision2_capture2"]
    with open(os.path.join(ROOT, "tests", "golden", "regions_golden.json")) as f:
        fix = json.load(f)

    def cli(*more):
        r = subprocess.run(["node", "commandline.js", *more, "-threshold", "5", "-span", "10", "-pyrLevels", "3"] + pair,
                           cwd=HOST, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
        assert docs[-1] == {"request": 1, "data": 1, "error": 0}
        return docs[0]

    on = cli("-regions", str(fix["gap"]))
    assert list(on.keys()) == REFERENCE_KEYS + ["regions"]
    assert on["status"] == "SUSPICIOUS"
    assert [{k: v[k] for k in ("x", "y", "dx", "dy")} for v in on["vector"]] == gold["vector"]
    assert all(list(v.keys()) == ["x", "y", "dx", "dy", "region"] for v in on["vector"])
    assert [v["region"] for v in on["vector"]] == fix["region_of"]
    assert on["regions"] == fix["regions"]
    assert all(list(g.keys()) == ["x", "y", "width", "height", "count", "peak"] and list(g["peak"].keys()) == ["x", "y", "dx", "dy"]
               for g in on["regions"])
    assert sum(g["count"] for g in on["regions"]) == len(on["vector"]) == 24
    off = cli()
    assert list(off.keys()) == REFERENCE_KEYS and off["vector"] == gold["vector"]
    assert all(list(v.keys()) == ["x", "y", "dx", "dy"] for v in off["vector"])
    assert {k: on[k] for k in REFERENCE_KEYS if k not in ("time", "vector")} == {k: off[k] for k in REFERENCE_KEYS if k not in ("time", "vector")}
