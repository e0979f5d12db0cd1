"""Resident expected images, the host layer's side (tidal-wave_amd/host/twhost.cpp: Parameter::residentMB / TW_RESIDENT_MB)
on the stub backend, no GPU: the cache keyed by the expected file's identity, hits that go to tw_submit_image_*, misses that
keep their image, rewritten and deleted files, eviction under a budget, a palette file that cannot be opened.

The stub flags a pair whose first gray pixels differ and counts tw_image_keep, tw_submit_image_* and tw_image_release calls
(tw_stub_resident_calls).  The probe is one long-lived Manager with one consumer that executes a little script: R expect
target (request), W (wait for every response so far), C src dst (rewrite dst with src's bytes and a later mtime), D path
(delete), P (print the stub's counters).  The files are written here.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_host_png_kinds import write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")

PROBE = r'''
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <condition_variable>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>
#include "../twhost.h"
using namespace twhost;
extern "C" void tw_stub_resident_calls(long* kept, long* image_pairs, long* released);
static void counters(const char* when) {
    long k = 0, p = 0, r = 0;
    tw_stub_resident_calls(&k, &p, &r);
    printf("{\"when\": \"%s\", \"kept\": %ld, \"image_pairs\": %ld, \"released\": %ld}\n", when, k, p, r);
}
// argv[1]: Parameter::residentMB (-1: leave the default); then the script
int main(int argc, char** argv) {
    std::mutex m; std::condition_variable cv; int n = 0, asked = 0; bool fin = false;
    Observer o;
    o.onNext = [&](const Response& r) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"%s\", \"reason\": \"%s\", \"expect\": \"%s\", \"target\": \"%s\", \"width\": %d, \"height\": %d, "
               "\"vectors\": %d}\n", r.status.c_str(), r.reason.c_str(), r.expect_image.c_str(), r.target_image.c_str(), r.width,
               r.height, (int)r.vectors.size());
        n++; cv.notify_all(); };
    o.onError = [&](const std::string& e) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"ERROR\", \"reason\": \"%s\"}\n", e.c_str());
        n++; cv.notify_all(); };
    o.onCompleted = [&](const Report&) { std::lock_guard<std::mutex> lk(m); fin = true; cv.notify_all(); };
    Parameter p; tw_default_params(&p.optParam); p.numThreads = 1; p.batch = 16;
    if (atoi(argv[1]) >= 0) p.residentMB = atoi(argv[1]);
    Manager* mg = new Manager(o); mg->start(p); mg->waitReady();
    auto wait_all = [&] { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return n >= asked; }); };
    for (int i = 2; i < argc; i++) {
        const std::string op = argv[i];
        if (op == "R") { mg->request(argv[i + 1], argv[i + 2]); asked++; i += 2; }
        else if (op == "W") wait_all();
        else if (op == "P") { wait_all(); std::lock_guard<std::mutex> lk(m); counters("script"); }
        else if (op == "D") { unlink(argv[i + 1]); i += 1; }
        else if (op == "C") {
            struct stat st; stat(argv[i + 2], &st);
            { std::ifstream in(argv[i + 1], std::ios::binary); std::ofstream out(argv[i + 2], std::ios::binary | std::ios::trunc); out << in.rdbuf(); }
            struct timespec ts[2] = {st.st_atim, st.st_mtim};
            ts[1].tv_sec += 2; ts[1].tv_nsec = (ts[1].tv_nsec + 1) % 1000000000;
            utimensat(AT_FDCWD, argv[i + 2], ts, 0);
            i += 2;
        }
    }
    wait_all();
    mg->stop(); { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return fin; }); } delete mg;
    counters("stopped");
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    src = os.path.join(HOST, "build", "resident_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    exe = os.path.join(HOST, "build", "resident_probe")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, src] +
                       [os.path.join(HOST, n) for n in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")] +
                       ["-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(probe, budget, script, env_mb=None):
    """(responses in arrival order, the counter lines the script asked for, the counters after Manager::stop)"""
    env = dict(os.environ, TW_STUB_DEVICES="1", TW_NUMA="0")
    for k in ("TW_DEVICE_PNG", "TW_DEVICE_PNG_KINDS", "TW_DEVICE_RECONCILE", "TW_DEVICE_JPEG", "TW_RESIDENT_MB"):
        env.pop(k, None)
    if env_mb is not None:
        env["TW_RESIDENT_MB"] = str(env_mb)
    r = subprocess.run([probe, str(budget)] + [str(t) for t in script], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.strip().splitlines()]
    res = [x for x in lines if "status" in x]
    cnt = [x for x in lines if x.get("when") == "script"]
    end = [x for x in lines if x.get("when") == "stopped"]
    assert len(end) == 1 and len(res) == sum(1 for t in script if t == "R")
    assert end[0]["kept"] == end[0]["released"]  # Manager::stop releases everything
    return res, cnt, end[0]


def gray_png(path, first, w=37, h=21, seed=1):
    g = np.random.default_rng(seed).integers(0, 256, (h, w, 1), dtype=np.uint8)
    g[0, 0, 0] = first
    write_png(str(path), g, 0, 8)
    return str(path)


@pytest.fixture
def files(tmp_path):
    d = tmp_path
    f = {"e1": gray_png(d / "e1.png", 10, seed=1), "e2": gray_png(d / "e2.png", 20, seed=2)}
    for name, first in (("ta", 10), ("tb", 20), ("tc", 30), ("td", 10)):
        f[name] = gray_png(d / (name + ".png"), first, seed=ord(name[1]))
    return f


def answers(res):
    """what a response says, without the order of arrival"""
    return sorted(json.dumps(x, sort_keys=True) for x in res)


def four(f, expect=("e1", "e1", "e1", "e1")):
    return [t for e, tg in zip(expect, ("ta", "tb", "tc", "td")) for t in ("R", f[e], f[tg])]


def test_budget_zero_or_unset_is_todays_path(probe, files):
    script = four(files) + ["R", files["e2"], files["tb"], "R", files["e2"], files["ta"]]
    want = [("OK", 0), ("SUSPICIOUS", 1), ("SUSPICIOUS", 1), ("OK", 0), ("OK", 0), ("SUSPICIOUS", 1)]
    runs = [run(probe, -1, script), run(probe, 0, script), run(probe, -1, script, env_mb=0)]
    for res, _, end in runs:
        assert end["kept"] == end["image_pairs"] == end["released"] == 0
        by_pair = {(x["expect"], x["target"]): (x["status"], x["vectors"]) for x in res}
        assert [by_pair[(script[i + 1], script[i + 2])] for i in range(0, len(script), 3)] == want
        assert all(x["width"] == 37 and x["height"] == 21 for x in res)
    assert answers(runs[0][0]) == answers(runs[1][0]) == answers(runs[2][0])


@pytest.mark.parametrize("how", ["parameter", "environment"])
def test_one_expected_file_four_targets_is_kept_once(probe, files, how):
    script = four(files)
    off, _, _ = run(probe, 0, script)
    on, _, end = run(probe, 64, script) if how == "parameter" else run(probe, -1, script, env_mb=64)
    assert end["kept"] == 1 and end["image_pairs"] == 3
    assert answers(on) == answers(off)
    # ... and one request at a time: the first misses, the others hit the cache
    step = [t for i in range(0, len(script), 3) for t in script[i:i + 3] + ["W"]]
    on, _, end = run(probe, 64, step)
    assert end["kept"] == 1 and end["image_pairs"] == 3
    assert answers(on) == answers(off) and [x["target"] for x in on] == [files[t] for t in ("ta", "tb", "tc", "td")]


def test_a_hard_link_is_the_same_file(probe, files, tmp_path):
    link = str(tmp_path / "e1_link.png")
    os.link(files["e1"], link)
    f = dict(files, l1=link)
    for expect in (("l1", "l1", "l1", "l1"), ("e1", "l1", "e1", "l1")):
        script = four(f, expect)
        off, _, _ = run(probe, 0, script)
        for sc in (script, [t for i in range(0, len(script), 3) for t in script[i:i + 3] + ["W"]]):
            on, _, end = run(probe, 64, sc)
            assert end["kept"] == 1 and end["image_pairs"] == 3
            assert answers(on) == answers(off)


def test_a_rewritten_expected_file_is_a_miss_and_the_old_image_goes(probe, files):
    e1, e2, ta = files["e1"], files["e2"], files["ta"]
    script = ["R", e1, ta, "W", "R", e1, ta, "P", "C", e2, e1, "R", e1, ta, "P", "R", e1, ta, "W"]
    res, cnt, end = run(probe, 64, script)
    assert [(x["status"], x["vectors"]) for x in res] == [("OK", 0), ("OK", 0), ("SUSPICIOUS", 1), ("SUSPICIOUS", 1)]
    assert (cnt[0]["kept"], cnt[0]["image_pairs"], cnt[0]["released"]) == (1, 1, 0)
    assert (cnt[1]["kept"], cnt[1]["image_pairs"], cnt[1]["released"]) == (2, 1, 1)  # the new content; the old entry released
    assert (end["kept"], end["image_pairs"]) == (2, 2)
    off, _, _ = run(probe, 0, ["R", e1, ta, "W", "R", e1, ta, "W"])  # (e1 now holds e2's bytes)
    assert answers(off) == answers(res[2:])


def test_a_budget_for_one_image_evicts_each_time(probe, tmp_path, files):
    # 800 x 700 = 560 000 bytes: one fits 1 MB, two do not
    big = [gray_png(tmp_path / ("big%d.png" % i), 10 * i, w=800, h=700, seed=i) for i in (1, 2)]
    tgt = gray_png(tmp_path / "big_t.png", 10, w=800, h=700, seed=9)
    script = []
    for _ in range(3):
        for e in big:
            script += ["R", e, tgt, "W"]
    script += ["P"]
    res, cnt, end = run(probe, 1, script)
    assert [(x["status"], x["vectors"]) for x in res] == [("OK", 0), ("SUSPICIOUS", 1)] * 3
    assert (cnt[0]["kept"], cnt[0]["image_pairs"], cnt[0]["released"]) == (6, 0, 5)
    assert end["released"] == end["kept"] == 6
    # a budget for both: two misses, then hits
    res2, _, end = run(probe, 2, script)
    assert (end["kept"], end["image_pairs"]) == (2, 4) and answers(res2) == answers(res)


def test_a_deleted_expected_file_cannot_be_opened(probe, files):
    e1, ta = files["e1"], files["ta"]
    res, cnt, end = run(probe, 64, ["R", e1, ta, "W", "R", e1, ta, "W", "D", e1, "R", e1, ta, "P"])
    assert [x["status"] for x in res] == ["OK", "OK", "ERROR"]
    assert res[2]["reason"] == "Can't open " + e1
    assert (cnt[0]["kept"], cnt[0]["image_pairs"], cnt[0]["released"]) == (1, 1, 1)  # (the cached image went with the file)


def test_a_palette_file_without_the_entry_never_stays_cached(probe, files, tmp_path):
    bad = str(tmp_path / "bad_palette.png")
    idx = np.full((21, 37, 1), 2, np.uint8)
    idx[5, 7, 0] = 200  # an index beyond the four entries
    write_png(bad, idx, 3, 8, plte=[[10, 10, 10], [20, 20, 20], [30, 30, 30], [40, 40, 40]])
    res, cnt, end = run(probe, 64, ["R", bad, files["ta"], "W", "R", bad, files["tb"], "P"])
    assert [(x["status"], x["reason"]) for x in res] == [("ERROR", "Can't open " + bad)] * 2
    assert (cnt[0]["kept"], cnt[0]["image_pairs"], cnt[0]["released"]) == (2, 0, 2)
    # both in one go: the pair behind the one that keeps the image answers as that one does
    res, _, end = run(probe, 64, ["R", bad, files["ta"], "R", bad, files["tb"], "R", files["e1"], files["ta"]])
    assert sorted((x["status"], x["reason"]) for x in res) == [("ERROR", "Can't open " + bad)] * 2 + [("OK", "")]
    off, _, _ = run(probe, 0, ["R", bad, files["ta"], "R", bad, files["tb"], "R", files["e1"], files["ta"]])
    assert answers(off) == answers(res)


def test_a_jpeg_expected_image_beside_png_targets(probe, tmp_path):
    """A JPEG expected image beside half-decoded PNG rows: finished on the host on a miss, plain gray on a hit."""
    jpg = os.path.join(ROOT, "tests", "golden", "jpeg", "golden_expected.jpg")
    import jpeg_cases as J
    g = J.fixture("golden_expected")[1]
    h, w = g.shape
    same = gray_png(tmp_path / "same.png", int(g[0, 0]), w=w, h=h, seed=3)
    other = gray_png(tmp_path / "other.png", int(g[0, 0]) ^ 0x40, w=w, h=h, seed=4)
    script = ["R", jpg, same, "W", "R", jpg, other, "W", "R", jpg, same, "W", "R", jpg, jpg, "W"]
    off, _, _ = run(probe, 0, script)
    on, _, end = run(probe, 64, script)
    assert [(x["status"], x["vectors"]) for x in on] == [("OK", 0), ("SUSPICIOUS", 1), ("OK", 0), ("OK", 0)]
    assert answers(on) == answers(off)
    assert (end["kept"], end["image_pairs"]) == (1, 3)


def test_a_failing_target_does_not_take_the_pairs_behind_it_along(probe, files, tmp_path):
    """The pair that was to keep the expected image fails on its target; the pairs of the same batch decode the file themselves."""
    missing = str(tmp_path / "missing.png")
    far = gray_png(tmp_path / "far.png", 10, w=50, h=21, seed=5)
    e1 = files["e1"]
    script = ["R", e1, missing, "R", e1, far, "R", e1, files["ta"], "R", e1, files["tb"]]
    off, _, _ = run(probe, 0, script)
    on, _, end = run(probe, 64, script)
    assert answers(on) == answers(off)
    assert sorted(x["status"] for x in on) == ["ERROR", "ERROR", "OK", "SUSPICIOUS"]
    assert end["kept"] >= 1 and end["kept"] + end["image_pairs"] == 2
