"""Diff images in the host layer (Parameter::extras.overlayDir / overlayTol, Response::overlay, new TidalWave({overlay: dir}), the
CLI's -overlay / -overlayTol), asserted from the engine's side as tests/test_host_shift.py does: the stub backend records
every call of the C ABI (TW_STUB_TRACE) and tools/consumer_probe.cpp feeds one consumer.  CPU only, but for the last test.

With the setting off a consumer makes exactly the calls it made before: tests/golden/consumer_trace_parent.json holds the
hashes of the commit before the ignore regions, and the probe's existing cases must still produce them.
"""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import host_probe as HP
from host_probe import CT, HOST, ROOT, calls, name_of, needs_node, run

NEW = ("tw_ticket_hits", "tw_ticket_overlay")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return HP.make_world(tmp_path_factory, "overlay")


def fnv1a64(s):
    h = 14695981039346656037
    for c in s.encode():
        h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return "%016x" % h


def test_overlay_off_makes_the_calls_of_the_parent_cases(world):
    HP.assert_off_is_the_parent(world, NEW, " overlay ")


def check_on(world, case, sub, tol, more=()):
    """the case with overlays into <dir>/<sub>: the trace's and the responses' shape; returns (lines, trace)"""
    from PIL import Image
    odir = os.path.join(world["dir"], sub)
    os.makedirs(odir, exist_ok=True)
    env, budget, script = case
    lines_off, trace_off = run(world, (env, budget, list(more) + list(script)))
    lines_on, trace_on = run(world, CT.with_overlay((env, budget, list(more) + list(script)), odir, tol))
    wait_name = "tw_wait_regions" if "G" in more else "tw_wait"
    waits = calls(trace_on, wait_name)
    asks, draws = calls(trace_on, "tw_ticket_hits"), calls(trace_on, "tw_ticket_overlay")
    assert len(asks) == len(waits) == len(calls(trace_off, wait_name)) > 0
    # every other call is what it was, in the order it was
    rest = lambda tr: [t for t in tr if name_of(t) not in NEW]  # noqa: E731
    assert rest(trace_on) == rest(trace_off)
    # in front of each collecting wait, for its ticket: tw_ticket_hits, then tw_ticket_overlay when the pair will be SUSPICIOUS
    drawn = set()
    for w in waits:
        i = trace_on.index(w)
        tk = w.split(" ")[2]
        k = i - 1
        if name_of(trace_on[k]) == "tw_ticket_overlay":
            assert trace_on[k].split(" ")[2] == tk and "tol=%d -> OK" % tol in trace_on[k]
            drawn.add(tk)
            k -= 1
        assert name_of(trace_on[k]) == "tw_ticket_hits" and trace_on[k].split(" ")[2] == tk, (trace_on[k], w)
        if "D" in more:  # (the status is known before the picture is asked for)
            assert name_of(trace_on[k - (2 if "S" in more else 1)]) == "tw_ticket_changes"
    assert len(drawn) == len(draws)
    # the responses: what they were, plus the path — exactly for the SUSPICIOUS ones
    assert len(lines_on) == len(lines_off)
    n_pictures = 0
    for on, off in zip(lines_on, lines_off):
        head, sep, path = on.partition(" overlay ")
        assert head == off
        assert bool(sep) == off.startswith("SUSPICIOUS"), on
        if not sep:
            continue
        n_pictures += 1
        target = off.split("|")[3]
        full_target = target.replace("<dir>", world["dir"]).replace("<root>", ROOT)
        base = os.path.splitext(os.path.basename(target))[0]
        assert path == "<dir>/%s/%s-%s.png" % (sub, fnv1a64(full_target), base), on
        w, h = (int(v) for v in off.split("|")[4].split("x"))
        with Image.open(path.replace("<dir>", world["dir"])) as im:
            px = np.asarray(im)
        assert px.shape == (h, w, 3)
        yy, xx = np.mgrid[0:h, 0:w]
        assert np.array_equal(px, np.stack([xx & 255, yy & 255, np.full_like(xx, tol)], -1).astype(np.uint8))
    assert n_pictures == sum(1 for ln in lines_off if ln.startswith("SUSPICIOUS"))
    assert len(draws) >= n_pictures  # (a target asked twice is drawn twice, into one file)
    return lines_on, trace_on, n_pictures


@pytest.mark.parametrize("name", ["fast_ten_rgb", "raw_mixed_with_files", "resident_twelve_share_expected", "damaged_both",
                                  "palette_gray2_kinds1"])
def test_overlay_on_asks_before_each_collecting_wait_and_draws_the_suspicious_pairs(world, name):
    lines, trace, n = check_on(world, world["cases"][name], "o_" + name, 16)
    statuses = [ln.split("|")[0] for ln in lines]
    if name == "fast_ten_rgb":
        assert n > 0 and "OK" in statuses, statuses  # both kinds of pair: some get a picture, some get nothing
    if name == "damaged_both":
        assert "ERROR" in statuses  # ERROR pairs get nothing (check_on: no path on a line that is not SUSPICIOUS)


def test_a_pair_made_suspicious_by_residual_min_alone_gets_its_picture(world):
    case = world["cases"]["fast_ten_rgb"]
    plain, _ = run(world, case)
    ok_before = sum(1 for ln in plain if ln.startswith("OK"))
    assert ok_before > 0
    # the stub's change record has n_unexplained = the tolerance: 7 >= 5 makes every answered pair SUSPICIOUS
    lines, trace, n = check_on(world, case, "o_residual", 200, more=("D", 7, 5))
    assert n == len(lines) == 10 and all(ln.startswith("SUSPICIOUS") for ln in lines)
    # ... and below the minimum the rule is the reference's again
    lines, trace, n = check_on(world, case, "o_residual_off", 0, more=("D", 7, 8))
    assert n == 10 - ok_before
    # with regions and the shift as well: changes, shift, hits, (overlay), the wait
    lines, trace, n = check_on(world, case, "o_all", 16, more=("G", 2, "D", 7, 0, "S", 32))
    for w in calls(trace, "tw_wait_regions"):
        i = trace.index(w)
        k = i
        while k > 0 and name_of(trace[k - 1]).startswith("tw_ticket_"):
            k -= 1
        before = [name_of(t) for t in trace[k:i]]
        assert before in (["tw_ticket_changes", "tw_ticket_shift", "tw_ticket_hits"],
                          ["tw_ticket_changes", "tw_ticket_shift", "tw_ticket_hits", "tw_ticket_overlay"]), before
    assert all(ln.index(" shift ") < ln.index(" overlay ") for ln in lines if " overlay " in ln)


def test_a_tolerance_outside_0_to_255_leaves_the_consumer_without_an_engine(world):
    odir = os.path.join(world["dir"], "o_bad")
    os.makedirs(odir, exist_ok=True)
    lines, trace = run(world, CT.with_overlay(world["cases"]["fast_ten_rgb"], odir, 256))
    assert all(ln.startswith("ERROR|engine: overlay: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_ticket_hits") and os.listdir(odir) == []


def test_a_directory_that_is_missing_or_not_writable_leaves_the_consumer_without_an_engine(world):
    missing = os.path.join(world["dir"], "o_missing", "deeper")
    lines, trace = run(world, CT.with_overlay(world["cases"]["fast_ten_rgb"], missing, 16))
    assert all(ln.startswith("ERROR|engine: overlay: not a writable directory: ") for ln in lines) and len(lines) == 10
    assert not calls(trace, "tw_wait") and not calls(trace, "tw_ticket_hits") and not os.path.exists(missing)
    a_file = os.path.join(world["dir"], "o_is_a_file")
    open(a_file, "w").close()
    lines, trace = run(world, CT.with_overlay(world["cases"]["fast_ten_rgb"], a_file, 16))
    assert all(ln.startswith("ERROR|engine: overlay: not a writable directory: ") for ln in lines) and len(lines) == 10


def test_a_picture_that_cannot_be_written_is_logged_and_its_pair_answered_without_the_key(world):
    env, budget, script = world["cases"]["fast_ten_rgb"]
    plain, _ = run(world, (env, budget, script))
    victim = next(ln for ln in plain if ln.startswith("SUSPICIOUS"))
    target = victim.split("|")[3].replace("<dir>", world["dir"]).replace("<root>", ROOT)
    odir = os.path.join(world["dir"], "o_blocked")
    blocked = os.path.join(odir, "%s-%s.png" % (fnv1a64(target), os.path.splitext(os.path.basename(target))[0]))
    os.makedirs(blocked)  # a directory where the file should go: the writer cannot open it
    logged = dict(env, TW_LOG="1")  # (the reference's progress lines, on stdout)
    out, trace = CT.run_case(world["exe"], CT.with_overlay((logged, budget, script), odir, 16), 1, world["dir"])
    out = out.strip().splitlines()
    said = [ln for ln in out if ln.startswith("overlay: ")]
    assert said == ["overlay: %s: cannot write the file" % blocked.replace(world["dir"], "<dir>")]
    answers = [ln for ln in out if ln.split("|")[0] in ("OK", "SUSPICIOUS", "ERROR")]
    assert len(answers) == 10
    for ln in answers:
        if ln.startswith(victim):
            assert ln == victim  # its answer is what it was: no key
        else:
            assert (" overlay " in ln) == ln.startswith("SUSPICIOUS")
    assert len(calls(trace.strip().splitlines(), "tw_wait")) == 10  # every ticket was still collected


def test_overlay_path(tmp_path):
    """<dir>/<16 hex digits of FNV-1a-64 of the target_image string>-<the target's base name without extension>.png"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    assert fnv1a64("") == "cbf29ce484222325" and fnv1a64("a") == "af63dc4c8601ec8c"  # the published test vectors
    names = ["/a/b/capture2.png", "capture2.png", "/x/.hidden", "/x/archive.tar.gz", "noext", "dir.d/file", "raw_target_3"]
    src = tmp_path / "p.cpp"
    src.write_text('#include <stdio.h>\n#include "twhost.h"\n'
                   'int main(int argc, char** argv) { for (int i = 1; i < argc; i++) puts(twhost::overlay_path("out", argv[i]).c_str()); }\n')
    exe = str(tmp_path / "p")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe, str(src)])
    got = subprocess.check_output([exe] + names, text=True).splitlines()
    bases = ["capture2", "capture2", ".hidden", "archive.tar", "noext", "file", "raw_target_3"]
    assert got == ["out/%s-%s.png" % (fnv1a64(n), b) for n, b in zip(names, bases)]
    assert got[0] != got[1]  # one base name in two directories: two files


def node(script, *args, timeout=120):
    return subprocess.run(["node", "-e", script, *args], cwd=HOST, capture_output=True, text=True, timeout=timeout)


@needs_node
def test_cli_parsing_and_the_addon_on_the_stub(tmp_path):
    r = node("""
var C=require('./commandline'), P=require('path');
console.log(JSON.stringify([C.getArgs(['-overlay','out','-overlayTol','3','a','b']), C.getArgs(['--overlay=x/y','a','b']),
  C.getArgs(['a','b']), P.resolve('out'), P.resolve('x/y')]));
""")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got[0] == {"expect_path": "a", "target_path": "b", "options": {"overlay": got[3], "overlayTol": 3}}
    assert got[1]["options"] == {"overlay": got[4]} and got[2]["options"] == {}
    # through the whole CLI: an unreadable pair answers as without the option, and the directory is made
    out = tmp_path / "pictures"
    r = subprocess.run(["node", "commandline.js", "-overlay", str(out), "/nonexistent/a.png", "/nonexistent/b.png"],
                       cwd=HOST, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
    assert docs[0] == {"status": "ERROR", "reason": "Can't open /nonexistent/a.png"}
    assert docs[-1] == {"request": 1, "data": 0, "error": 1}
    assert out.is_dir() and list(out.iterdir()) == []


REFERENCE_KEYS = ["status", "span", "threshold", "expect_image", "target_image", "time", "height", "width", "vector"]


@needs_node
@pytest.mark.gpu
def test_the_golden_pair_through_the_cli_leaves_one_png_that_equals_the_reference(tmp_path, golden):
    """commandline.js -> index.js -> the addon -> a consumer -> the engine -> the PNG writer: one file, which PIL opens and
    which equals tests/overlay_ref.py on the oracle's 24 vectors; `overlay` is the result's last key"""
    from PIL import Image
    import overlay_ref as R
    tree = os.path.join(ROOT, "tests", "golden", "tree")
    pair = [os.path.join(tree, "expected", "scenario2", "capture2.png"), os.path.join(tree, "revision2", "scenario2", "capture2.png")]
    case = golden["revision2_capture2"]
    out = tmp_path / "out"

    def cli(*more):
        r = subprocess.run(["node", "commandline.js", *more, "-threshold", "5", "-span", "10", "-pyrLevels", "3"] + pair,
                           cwd=HOST, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
        assert docs[-1] == {"request": 1, "data": 1, "error": 0}
        return docs[0]

    on = cli("-overlay", str(out))
    assert list(on.keys()) == REFERENCE_KEYS + ["overlay"] and on["vector"] == case["vector"] and on["status"] == "SUSPICIOUS"
    files = sorted(os.listdir(out))
    assert files == ["%s-capture2.png" % fnv1a64(pair[1])] and on["overlay"] == str(out / files[0])
    vec = [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    assert len(vec) == 24
    with Image.open(on["overlay"]) as im:
        assert np.array_equal(np.asarray(im), R.overlay_ref(case["expect_img"], case["target_img"], [], vec, [], 16))
    every = cli("-overlay", str(out), "-overlayTol", "0", "-shift", "64", "-residual", "16", "-regions", "1")
    assert list(every.keys()) == REFERENCE_KEYS + ["regions", "change", "shift", "overlay"]
    with Image.open(every["overlay"]) as im:
        boxes = [(g["x"], g["y"], g["width"], g["height"]) for g in every["regions"]]
        assert np.array_equal(np.asarray(im), R.overlay_ref(case["expect_img"], case["target_img"], [], vec, boxes, 0))
    off = cli()
    assert list(off.keys()) == REFERENCE_KEYS and off["vector"] == case["vector"]
    # a pair that is not SUSPICIOUS: no file, no key
    same = tmp_path / "same"
    r = subprocess.run(["node", "commandline.js", "-overlay", str(same), pair[0], pair[0]], cwd=HOST, capture_output=True, text=True,
                       timeout=120)
    doc = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")[0]
    assert doc["status"] == "OK" and "overlay" not in doc and os.listdir(same) == []
