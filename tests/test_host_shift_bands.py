"""The shift bands in the host layer (Parameter::extras.shiftBands, Response::bands, new TidalWave({shift: R, shiftBands: B}), the CLI's
-shiftBands), asserted from the engine's side as tests/test_host_shift.py does: the stub backend records every call of the C ABI
(TW_STUB_TRACE) and tools/consumer_probe.cpp feeds one consumer.  CPU only.

With the setting off a consumer makes exactly the calls it made before: tests/golden/consumer_trace_parent.json holds the
hashes of the commit before the ignore regions, and the probe's existing cases must still produce them.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import band_ref as BR
import host_probe as HP
from host_probe import CT, HOST, ROOT, calls, needs_node, run

BANDS = re.compile(r" bands (\d+):((?: \[\d+,\d+ dy=-?\d+ applied=[01]\])*)$")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return HP.make_world(tmp_path_factory, "shift_bands")


def parse_bands(line):
    """[(y, rows, dy, applied)] of a response line, and the line in front of the key."""
    m = BANDS.search(line)
    assert m, line
    recs = [tuple(int(v) for v in g) for g in re.findall(r"\[(\d+),(\d+) dy=(-?\d+) applied=([01])\]", m.group(2))]
    assert len(recs) == int(m.group(1))
    return recs, line[:m.start()]


def test_bands_off_makes_the_calls_of_the_parent_cases(world):
    # "S 0 B 64" is off too: the bands need the shift
    HP.assert_off_is_the_parent(world, ("tw_ticket_shift", "tw_set_option"), " bands ", [lambda c: CT.with_shift_bands(c, 0, 64)])
    # ... and with the shift alone a consumer makes the calls of the shift: no band call, no `bands`
    out, text = CT.run_case(world["exe"], CT.with_shift(world["cases"]["fast_ten_rgb"], 64), 1, world["dir"])
    out0, text0 = CT.run_case(world["exe"], CT.with_shift_bands(world["cases"]["fast_ten_rgb"], 64, 0), 1, world["dir"])
    assert "tw_ticket_shift_bands" not in text and " bands " not in out and "option=6" not in text
    assert (out0, text0) == (out, text)


@pytest.mark.parametrize("name", ["fast_ten_rgb", "raw_mixed_with_files", "resident_twelve_share_expected", "damaged_both"])
def test_bands_on_sets_the_option_once_and_asks_behind_the_shift(world, name):
    case = world["cases"][name]
    lines_off, trace_off = run(world, CT.with_shift(case, 64))
    lines_on, trace_on = run(world, CT.with_shift_bands(case, 64, 48))
    opt = calls(trace_on, "tw_set_option")
    assert len(opt) == 2 and "option=5 value=64 -> OK" in opt[0] and "option=6 value=48 -> OK" in opt[1]
    assert trace_on.index(opt[1]) == trace_on.index(opt[0]) + 1  # directly behind TW_OPT_SHIFT
    waits = calls(trace_on, "tw_wait")
    asks = calls(trace_on, "tw_ticket_shift_bands")
    assert len(asks) == len(waits) == len(calls(trace_off, "tw_wait")) > 0
    # one tw_ticket_shift and behind it one tw_ticket_shift_bands directly in front of each collecting wait, for its ticket
    for w in waits:
        i = trace_on.index(w)
        a, b = trace_on[i - 2].split(" "), trace_on[i - 1].split(" ")
        assert (a[1], b[1]) == ("tw_ticket_shift", "tw_ticket_shift_bands") and a[2] == b[2] == w.split(" ")[2]
    # every other call is what it was with the shift alone, in the order it was
    rest = lambda tr: [t for t in tr if t.split(" ", 2)[1] != "tw_ticket_shift_bands" and "option=6" not in t]  # noqa: E731
    assert rest(trace_on) == rest(trace_off)
    assert len(lines_on) == len(lines_off)
    for on, off in zip(lines_on, lines_off):
        if off.startswith("ERROR"):
            assert on == off
            continue
        recs, head = parse_bands(on)
        assert head == off and len(recs) >= 1
    if name == "damaged_both":
        assert any(ln.startswith("ERROR") for ln in lines_on) and any(" bands " in ln for ln in lines_on)


def test_responses_carry_band_ref_on_an_in_memory_pair(world):
    """The stub computes the definition on the whole images tw_submit_u8 hands it; the probe's in-memory pairs are filled with 7
    except for pixel 0.  40 x 70 at B = 32: three bands (32, 32 and 6 rows)."""
    h = 70
    E = np.full((h, CT.W), 7, np.uint8)
    T = E.copy()
    E[0, 0], T[0, 0] = 10, 99
    env, budget, _ = world["cases"]["fast_ten_rgb"]
    lines, _ = run(world, (env, budget, ["S", 8, "B", 32, "M", CT.W, h, 10, 10, "M", CT.W, h, 10, 99]))
    want = {}
    for name, pair in (("same", (E, E)), ("differ", (E, T))):
        g, bands = BR.estimate(pair[0], pair[1], 8, 32)
        want[name] = (g, [(b.y, b.rows, b.dy, b.applied) for b in bands])
    assert [b[:2] for b in want["same"][1]] == [(0, 32), (32, 32), (64, 6)]
    got = {}
    for ln in lines:
        recs, head = parse_bands(ln)
        got["same" if ln.startswith("OK") else "differ"] = (recs, head)
    for name in ("same", "differ"):
        g, bands = want[name]
        assert got[name][0] == bands, (name, got[name], bands)
        assert got[name][1].endswith(" shift %d,%d applied=%d" % (g.dx, g.dy, g.applied))
    assert want["same"][1] == [(0, 32, 0, 0), (32, 32, 0, 0), (64, 6, 0, 0)]


def test_a_band_height_the_engine_refuses_leaves_the_consumer_without_an_engine(world):
    lines, trace = run(world, CT.with_shift_bands(world["cases"]["fast_ten_rgb"], 64, 33))
    assert all(ln.startswith("ERROR|engine: shiftBands: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_ticket_shift_bands")


def node(script, *args, timeout=120):
    return subprocess.run(["node", "-e", script, *args], cwd=HOST, capture_output=True, text=True, timeout=timeout)


@needs_node
def test_cli_parsing_and_pass_through():
    r = node("""
var C=require('./commandline');
console.log(JSON.stringify([C.getArgs(['-shift','64','-shiftBands','48','a','b']), C.getArgs(['--shiftBands=32','a','b']),
  C.getArgs(['a','b'])]));
""")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got[0] == {"expect_path": "a", "target_path": "b", "options": {"shift": 64, "shiftBands": 48}}
    assert got[1]["options"] == {"shiftBands": 32} and got[2]["options"] == {}
    r = subprocess.run(["node", "commandline.js", "-shift", "64", "-shiftBands", "64", "/nonexistent/a.png", "/nonexistent/b.png"],
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
function Fake(o){ seen.push([o && o.shift, o && o.shiftBands]); }
Fake.prototype.calc=function(){ var s=this; setImmediate(function(){s.emit('error',{})}); };
Fake.prototype.dispose=function(){ var s=this; setImmediate(function(){s.emit('finish',{})}); };
var id=require.resolve('./build/Release/tidalwave');
require.cache[id]={id:id, filename:id, loaded:true, exports:{TidalWave:Fake}};
var T=require('./index');
var t=T.create(process.argv[1], {expectDir: process.argv[1], shift: 64, shiftBands: 48});
t.on('finish',function(){ var u=T.create(process.argv[1], {expectDir: process.argv[1]});
  u.on('finish',function(){ console.log(JSON.stringify(seen)); }); });
""", str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [[64, 48], [None, None]]


REFERENCE_KEYS = ["status", "span", "threshold", "expect_image", "target_image", "time", "height", "width", "vector"]


@needs_node
@pytest.mark.gpu
def test_result_object_of_the_golden_pair_through_the_cli():
    """commandline.js -> index.js -> the addon -> a consumer -> the engine: with -shift and -shiftBands the result carries
    `bands` behind `shift`; without -shiftBands it has no such key.  The bands equal tests/band_ref.py on the decoded pair."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    tree = os.path.join(ROOT, "tests", "golden", "tree")
    pair = [os.path.join(tree, "expected", "scenario2", "capture2.png"), os.path.join(tree, "revision2", "scenario2", "capture2.png")]
    with open(os.path.join(ROOT, "tests", "golden", "expected_responses.json")) as f:
        case = json.load(f)["revision2_capture2"]

    def cli(*more):
        r = subprocess.run(["node", "commandline.js", *more, "-threshold", "5", "-span", "10", "-pyrLevels", "3"] + pair,
                           cwd=HOST, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
        assert docs[-1] == {"request": 1, "data": 1, "error": 0}
        return docs[0]

    on = cli("-shift", "64", "-shiftBands", "64")
    assert list(on.keys()) == REFERENCE_KEYS + ["shift", "bands"]
    assert all(list(b.keys()) == ["y", "rows", "dy", "applied"] for b in on["bands"])
    g = os.path.join(ROOT, "tests", "golden")
    E, T = O.read_pgm(os.path.join(g, case["expect"])), O.read_pgm(os.path.join(g, case["target"]))
    _, want = BR.estimate(E, T, 64, 64)
    assert [(b["y"], b["rows"], b["dy"], int(b["applied"])) for b in on["bands"]] == [(b.y, b.rows, b.dy, b.applied) for b in want]
    off = cli("-shift", "64")
    assert list(off.keys()) == REFERENCE_KEYS + ["shift"]
