"""The shift in the host layer (Parameter::extras.shift, Response::shift, new TidalWave({shift: R}), the CLI's -shift), asserted from
the engine's side as tests/test_host_residual.py does: the stub backend records every call of the C ABI (TW_STUB_TRACE) and
tools/consumer_probe.cpp feeds one consumer.  CPU only.

With the setting off a consumer makes exactly the calls it made before: tests/golden/consumer_trace_parent.json holds the
hashes of the commit before the ignore regions, and the probe's existing cases must still produce them.
"""
import json
import os
import re
import subprocess

import pytest

import host_probe as HP
from host_probe import CT, HOST, ROOT, calls, needs_node, run


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return HP.make_world(tmp_path_factory, "shift")


def test_shift_off_makes_the_calls_of_the_parent_cases(world):
    # ... and "S 0" is off too
    HP.assert_off_is_the_parent(world, ("tw_ticket_shift", "tw_set_option"), " shift ", [lambda c: CT.with_shift(c, 0)])


@pytest.mark.parametrize("name", ["fast_ten_rgb", "raw_mixed_with_files", "resident_twelve_share_expected", "damaged_both"])
def test_shift_on_sets_the_option_once_and_asks_before_each_collecting_wait(world, name):
    case = world["cases"][name]
    lines_off, trace_off = run(world, case)
    lines_on, trace_on = run(world, CT.with_shift(case, 64))
    opt = calls(trace_on, "tw_set_option")
    assert len(opt) == 1 and "option=5 value=64 -> OK" in opt[0]
    created = [i for i, t in enumerate(trace_on) if t.split(" ", 2)[1] == "tw_engine_create"]
    assert len(created) == 1 and trace_on.index(opt[0]) == created[0] + 1  # directly after the engine exists
    waits = calls(trace_on, "tw_wait")
    asks = calls(trace_on, "tw_ticket_shift")
    assert len(asks) == len(waits) == len(calls(trace_off, "tw_wait")) > 0
    # one tw_ticket_shift directly in front of each collecting wait, for the wait's ticket
    for w in waits:
        i = trace_on.index(w)
        prev = trace_on[i - 1].split(" ")
        assert prev[1] == "tw_ticket_shift" and prev[2] == w.split(" ")[2], (trace_on[i - 1], w)
    # every other call is what it was, in the order it was
    rest = lambda tr: [t for t in tr if t.split(" ", 2)[1] not in ("tw_ticket_shift", "tw_set_option")]  # noqa: E731
    assert rest(trace_on) == rest(trace_off)
    # the responses: what they were (the status too), plus the stub's shift
    assert len(lines_on) == len(lines_off)
    for on, off in zip(lines_on, lines_off):
        if off.startswith("ERROR"):
            assert on == off
            continue
        head, _, tail = on.partition(" shift ")
        assert head == off
        assert re.fullmatch(r"-?\d+,-?\d+ applied=[01]", tail), on
    if name == "damaged_both":
        assert any(ln.startswith("ERROR") for ln in lines_on) and any(" shift " in ln for ln in lines_on)


def test_responses_carry_the_stubs_shift_of_an_in_memory_pair(world):
    """The stub computes the definition on the whole images tw_submit_u8 hands it.  The probe's in-memory pairs are filled with
    7 except for pixel 0 (10 against 10, or 10 against 99): an equal pair has every cost 0 (0, 0, not applied); in a differing
    one the profiles differ at index 0 alone.  A positive d compares the expected profile's entry 0 (3 above the rest) with the
    target's flat part and leaves the target's entry 0 (92 above) out: cost 3 over L - d elements, least at d = +1 on both axes
    (d = 0 costs 89, a negative d 92).  At (1, 1) the overlap's only difference is 10 against 7: applied.  tests/shift_ref.py
    says the same."""
    import numpy as np
    import shift_ref as S
    E = np.full((CT.H, CT.W), 7, np.uint8)
    T = E.copy()
    E[0, 0], T[0, 0] = 10, 99
    assert S.estimate(E, T, 8)[:3] == (1, 1, 1) and S.estimate(E, E, 8)[:3] == (0, 0, 0)
    env, budget, _ = world["cases"]["fast_ten_rgb"]
    lines, _ = run(world, (env, budget, ["S", 8, "M", CT.W, CT.H, 10, 10, "M", CT.W, CT.H, 10, 99]))
    tails = sorted(ln.partition(" shift ")[2] for ln in lines)
    assert tails == ["0,0 applied=0", "1,1 applied=1"], lines
    assert sorted(ln.split("|")[0] for ln in lines) == ["OK", "SUSPICIOUS"]  # (the status rule is untouched)


def test_shift_with_regions_and_residual(world):
    env, budget, script = world["cases"]["fast_ten_rgb"]
    lines, trace = run(world, (env, budget, ["G", 2, "D", 7, 0, "S", 32] + list(script)))
    opts = calls(trace, "tw_set_option")
    assert len(opts) == 3 and "option=3 value=2" in opts[0] and "option=4 value=7" in opts[1] and "option=5 value=32" in opts[2]
    waits = calls(trace, "tw_wait_regions")
    assert len(waits) == 10 and len(calls(trace, "tw_ticket_shift")) == 10 and len(calls(trace, "tw_ticket_changes")) == 10
    for w in waits:
        i = trace.index(w)
        assert [trace[i - 2].split(" ")[1], trace[i - 1].split(" ")[1]] == ["tw_ticket_changes", "tw_ticket_shift"]
    assert all(ln.index(" regions ") < ln.index(" changes ") < ln.index(" shift ") for ln in lines)


def test_a_radius_the_engine_refuses_leaves_the_consumer_without_an_engine(world):
    lines, trace = run(world, CT.with_shift(world["cases"]["fast_ten_rgb"], 1025))
    assert all(ln.startswith("ERROR|engine: shift: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_ticket_shift")


def node(script, *args, timeout=120):
    return subprocess.run(["node", "-e", script, *args], cwd=HOST, capture_output=True, text=True, timeout=timeout)


@needs_node
def test_cli_parsing_and_pass_through():
    r = node("""
var C=require('./commandline');
console.log(JSON.stringify([C.getArgs(['-shift','64','a','b']), C.getArgs(['--shift=8','a','b']), C.getArgs(['a','b'])]));
""")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got[0] == {"expect_path": "a", "target_path": "b", "options": {"shift": 64}}
    assert got[1]["options"] == {"shift": 8} and got[2]["options"] == {}
    # through the whole CLI: an unreadable pair answers as without the option
    r = subprocess.run(["node", "commandline.js", "-shift", "64", "/nonexistent/a.png", "/nonexistent/b.png"],
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
function Fake(o){ seen.push(o && o.shift); }
Fake.prototype.calc=function(){ var s=this; setImmediate(function(){s.emit('error',{})}); };
Fake.prototype.dispose=function(){ var s=this; setImmediate(function(){s.emit('finish',{})}); };
var id=require.resolve('./build/Release/tidalwave');
require.cache[id]={id:id, filename:id, loaded:true, exports:{TidalWave:Fake}};
var T=require('./index');
var t=T.create(process.argv[1], {expectDir: process.argv[1], shift: 64});
t.on('finish',function(){ var u=T.create(process.argv[1], {expectDir: process.argv[1]});
  u.on('finish',function(){ console.log(JSON.stringify(seen)); }); });
""", str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [64, None]


REFERENCE_KEYS = ["status", "span", "threshold", "expect_image", "target_image", "time", "height", "width", "vector"]


@needs_node
@pytest.mark.gpu
def test_result_object_of_the_golden_pair_through_the_cli():
    """commandline.js -> index.js -> the addon -> a consumer -> the engine: with -shift the result carries `shift` behind every
    other key; without it the keys and their order are the reference's.  The golden pair has not moved as a whole: whatever the
    searches answer is not applied, and the vectors are the golden ones."""
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

    on = cli("-shift", "64")
    assert list(on.keys()) == REFERENCE_KEYS + ["shift"]
    assert list(on["shift"].keys()) == ["x", "y", "applied"]
    assert on["shift"] == {"x": 0, "y": 0, "applied": False}  # (tests/shift_ref.py on the golden pair at radius 64)
    assert on["vector"] == gold["vector"] and on["status"] == "SUSPICIOUS"
    both = cli("-shift", "64", "-residual", "16", "-regions", "1")
    assert list(both.keys()) == REFERENCE_KEYS + ["regions", "change", "shift"] and both["shift"] == on["shift"]
    off = cli()
    assert list(off.keys()) == REFERENCE_KEYS and off["vector"] == gold["vector"]
