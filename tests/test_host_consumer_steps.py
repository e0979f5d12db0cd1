"""The steps of twhost::Consumer::run (tidal-wave_amd/host/twhost.cpp), asserted from the engine's side: the stub backend
records every call of the C ABI (TW_STUB_TRACE, host/stub_twflow.cpp), and one consumer with every request queued before
its thread starts (tools/consumer_probe.cpp) makes the same calls on every run.  The cases are those of
tools/consumer_trace.py, which compares two versions of twhost.cpp over all of them (profiles/consumer_split.md); here a
subset is run and what the record shows is asserted.  CPU only.  The last test compiles a small program against
host/resident_cache.h and the stub alone.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import consumer_trace as CT  # noqa: E402

W, H = CT.W, CT.H


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    d = str(tmp_path_factory.mktemp("consumer_steps"))
    exe = CT.build(os.path.join(HOST, "build", "consumer_probe"))
    f = CT.write_files(d)
    return {"exe": exe, "dir": d, "files": f, "cases": CT.cases(f)}


def run(world, case, threads=4):
    """(response lines without the closing counter line, that line's fields, the trace's lines)"""
    if isinstance(case, str):
        case = world["cases"][case]
    out, trace = CT.run_case(world["exe"], case, threads, world["dir"])
    lines = out.strip().splitlines()
    end = dict(p.rsplit(" ", 1) for p in lines[-1].split("|")[1:])
    return lines[:-1], {k: int(v) for k, v in end.items()}, trace.strip().splitlines()


def calls(trace, prefix):
    return [t.split(" ", 2)[1:] for t in trace if t.split(" ", 2)[1].startswith(prefix)]


def submits(trace):
    """(name, rest of the line) of every tw_submit_* call"""
    return [(n, rest) for n, rest in calls(trace, "tw_submit_")]


def test_one_and_four_decode_threads_make_the_same_calls(world):
    for name in ("fast_ten_rgb", "pgm_target_among_pngs", "resident_twelve_share_expected", "damaged_both"):
        one, four = run(world, name, 1), run(world, name, 4)
        assert one == four, name
        assert one[2][0].endswith("tw_device_count -> 1") and one[2][-1].endswith("tw_engine_destroy")


def test_the_entry_point_of_each_kind_of_pair(world):
    f = world["files"]

    def names(script, env=None, budget=0):
        return [n for n, _ in submits(run(world, (env or {}, budget, script))[2])]

    assert names(CT.pairs(f, ("e0", "t0"))) == ["tw_submit_png"]                      # filtered rows + filtered rows
    assert names(CT.pairs(f, ("e0", "t_pgm"))) == ["tw_submit_png"]                   # rows + gray
    assert names(CT.pairs(f, ("jpg", "t_33"))) == ["tw_submit_png"]                   # a JPEG beside rows: finished on the host
    assert names(CT.pairs(f, ("jpg", "jpg_b"))) == ["tw_submit_jpeg"]                 # coefficients + coefficients
    assert names(CT.pairs(f, ("jpg", "pgm_33"))) == ["tw_submit_jpeg"]                # coefficients + gray
    assert names(CT.pairs(f, ("jpg", "jpg_b")), {"TW_DEVICE_JPEG": "0"}) == ["tw_submit_u8"]
    assert names(CT.pairs(f, ("e_pgm", "t_pgm"))) == ["tw_submit_u8"]                 # gray + gray
    assert names(["M", W, H, 1, 2]) == ["tw_submit_u8"]                               # an in-memory pair
    assert names(CT.pairs(f, ("e_pgm", "t_pgm_narrow"))) == ["tw_submit_u8_sized"]    # gray, the device reconciles
    assert names(CT.pairs(f, ("e_pgm", "t_pgm_narrow")), {"TW_DEVICE_RECONCILE": "0"}) == ["tw_submit_u8"]
    assert names(CT.pairs(f, ("e0", "t0")), {"TW_DEVICE_PNG": "0"}) == ["tw_submit_u8"]
    # a resident expected image: the pair that keeps it goes the ordinary way, the pairs behind it against the image
    assert names(CT.pairs(f, ("e0", "t0"), ("e0", "t1"), ("e0", "t_pgm")), budget=CT.MB) == \
        ["tw_submit_png", "tw_submit_image_png", "tw_submit_image_png"]
    assert names(CT.pairs(f, ("e_33", "jpg"), ("e_33", "jpg_b"), ("e_33", "t_33")), budget=CT.MB) == \
        ["tw_submit_png", "tw_submit_image_jpeg", "tw_submit_image_png"]
    # (TW_DEVICE_JPEG=0: the targets are gray; the expected image's rows still make the first pair a tw_submit_png)
    assert names(CT.pairs(f, ("e_33", "jpg"), ("e_33", "jpg_b")), {"TW_DEVICE_JPEG": "0"}, CT.MB) == ["tw_submit_png", "tw_submit_image_png"]


@pytest.mark.parametrize("name", ["fast_ten_rgb", "pgm_target_among_pngs", "narrower3_png_reconcile1", "device_jpeg1",
                                  "palette_gray2_kinds1", "resident_twelve_share_expected", "resident_jpeg_targets"])
def test_every_file_image_goes_up_from_a_page_locked_block(world, name):
    """On both decode paths: the arena path (every file a PNG the device finishes) and decode-then-copy."""
    _, _, trace = run(world, name)
    sub = submits(trace)
    assert sub and all("-> OK" in rest for _, rest in sub)
    pins = [p for _, rest in sub for p in re.findall(r"pin=(\d)", rest)]
    assert pins and set(pins) == {"1"}, name
    # (an in-memory pair in ordinary memory is handed over where it lies)
    _, _, raw = run(world, ({}, 0, ["M", W, H, 1, 2]))
    assert re.findall(r"pin=(\d)", submits(raw)[0][1]) == ["0", "0"]


@pytest.mark.parametrize("path", ["arena", "decode_then_copy"])
def test_one_allocation_per_arena_not_one_per_batch(world, path):
    f = world["files"]
    sixteen = [("e%d" % (i % 10), ("t_pgm" if path == "decode_then_copy" and i % 4 == 1 else "t%d" % (i % 10))) for i in range(16)]
    _, end, trace = run(world, ({}, 0, CT.pairs(f, *sixteen)))
    assert end["batches"] >= 4 and len(calls(trace, "tw_flush")) == end["batches"]
    allocs = calls(trace, "tw_host_alloc")
    assert len(allocs) == 3 and len(set(a[1] for a in allocs)) == 3  # three arenas, blocks 0, 1, 2: the fourth batch allocates nothing
    # ... each sized for a full batch (4 pairs) of the largest image, whatever the take was
    assert len(set(re.search(r"bytes=(\d+)", a[1]).group(1) for a in allocs)) == 1
    flushes = [i for i, t in enumerate(trace) if " tw_flush " in t]
    assert [i for i, t in enumerate(trace) if " tw_host_alloc " in t][-1] < flushes[2]
    assert [t.split()[2] for t in trace if " tw_host_free " in t] == ["block=0", "block=1", "block=2"]


@pytest.mark.parametrize("kind,own,pair", [("pgm", "37x30", "40x30"), ("png", "37x30", "40x30"), ("jpeg", "30x35", "33x31")])
def test_the_targets_own_size_when_the_device_reconciles_the_pairs_size_when_the_host_does(world, kind, own, pair):
    def target_sizes(rec):
        lines, _, trace = run(world, "narrower3_%s_reconcile%d" % (kind, rec))
        assert all(ln.startswith(("OK|", "SUSPICIOUS|")) and "|%s|" % pair in ln for ln in lines)
        return lines, [(re.search(r"a=\[(\d+x\d+)", rest).group(1), re.search(r"b=\[(\d+x\d+)", rest).group(1)) for _, rest in submits(trace)]

    on_lines, on = target_sizes(1)
    off_lines, off = target_sizes(0)
    assert sorted(on) == sorted([(pair, own), (pair, pair), (pair, own)])
    assert off == [(pair, pair)] * 3
    assert on_lines == off_lines


def test_after_the_busy_retry_every_pair_is_answered_once_and_those_in_front_first(world):
    for name, first in (("busy_at_third_submit", "tw_submit_png"), ("resident_busy_at_third_submit", "tw_submit_image_png")):
        lines, end, trace = run(world, name)
        targets = [ln.split("|")[3] for ln in lines]
        assert len(targets) == 7 and len(set(targets)) == 7 and end["pairs"] == 7 and end["inflight"] == 0
        sub = submits(trace)
        busy = [i for i, (_, rest) in enumerate(sub) if "-> BUSY" in rest]
        assert busy == [2] and sub[2][0] == sub[3][0] == first
        assert sub[2][1].replace("-> BUSY ticket=-1", "") == sub[3][1].replace("-> OK ticket=3", "")  # the same pair again
        # between the refusal and the retry: the two pairs in front are waited for, and they are the first two responses
        at = [i for i, t in enumerate(trace) if "-> BUSY" in t][0]
        between = [t.split()[1:3] for t in trace[at + 1:] if " tw_grid_capacity " not in t][:3]
        assert between[0] == ["tw_wait", "ticket=1"] and between[1] == ["tw_wait", "ticket=2"] and between[2][0] == first
        assert [t.split("/")[-1] for t in targets[:2]] == ["t0.png", "t1.png"]
        waits = [c[1].split()[0] for c in calls(trace, "tw_wait")]
        assert sorted(waits) == ["ticket=%d" % k for k in range(1, 8)]


RESIDENT = ["resident_twelve_share_expected", "resident_jpeg_targets", "resident_leader_target_missing", "resident_bad_palette_expected",
            "resident_budget_below_one_image", "resident_two_expected_budget_for_one", "resident_busy_at_third_submit"]


@pytest.mark.parametrize("name", RESIDENT)
def test_resident_images_kept_are_released_and_none_is_released_under_a_pair(world, name):
    lines, end, trace = run(world, name)
    keeps = [c for c in calls(trace, "tw_image_keep") if "-> OK" in c[1]]
    releases = [re.search(r"image=(-?\d+)", c[1]).group(1) for c in calls(trace, "tw_image_release")]
    assert len(keeps) >= 1 and len(keeps) == len(releases) == end["kept"] == end["released"]
    assert sorted(releases) == sorted(re.search(r"image=(\d+)", c[1]).group(1) for c in keeps)  # each once
    # a pair submitted against an image: the image is alive then (no release of it earlier in the record), so nothing
    # between the pair's lookup and its submit let it go
    gone = set()
    used = 0
    for t in trace:
        m = re.search(r" (tw_image_release|tw_submit_image_png|tw_submit_image_jpeg) image=(-?\d+)", t)
        if not m:
            continue
        if m.group(1) == "tw_image_release":
            assert "-> OK" in t
            gone.add(m.group(2))
        else:
            assert m.group(2) not in gone and ("-> OK" in t or "-> BUSY" in t), t
            used += 1
    assert used == end["image_pairs"] + (1 if "busy" in name else 0)
    # the answers are those of the same pairs without the cache
    off_lines, off_end, _ = run(world, (world["cases"][name][0], 0, world["cases"][name][2]))
    assert sorted(off_lines) == sorted(lines) and off_end["kept"] == 0


def test_a_damaged_expected_image_is_named_first(world):
    lines, _, _ = run(world, "damaged_both")
    d = "<dir>/"
    assert sorted(ln.split("|")[1] for ln in lines if ln.startswith("ERROR")) == sorted(
        ["Can't open " + d + "bad_e.png", "Can't open " + d + "bad_t.png", "Can't open " + d + "bad_e.png",
         "Can't open " + d + "bad_crc.png", "Can't open " + d + "bad_crc.png"])
    lines, _, _ = run(world, "empty_and_missing")
    assert sorted(ln.split("|")[1] for ln in lines if ln.startswith("ERROR")) == sorted(
        ["ExpectImagePath is empty.", "TargetImagePath is empty.", "Can't open " + d + "missing.png", "Can't open " + d + "missing.png"])


def test_with_the_extras_on_the_calls_and_the_answers_are_those_of_the_commit_before_the_steps(world):
    """tests/golden/consumer_extras_parent.json: CT.EXTRAS_CASES under every configuration of CT.extras_configs — each extra
    alone, all together, each refusal — recorded from the twhost.cpp in which create_engine and collect were one body each
    (profiles/consumer_extras.md).  Responses, call trace and diff images, for 1 and for 4 decode threads."""
    with open(os.path.join(ROOT, "tests", "golden", "consumer_extras_parent.json")) as f:
        parent = json.load(f)
    assert sorted(parent) == sorted(c + "/" + n for c in CT.extras_configs("") for n in CT.EXTRAS_CASES)
    # (run_extras_row asserts that a refused configuration answers "engine: <field>: ..." and submits nothing, extras_rows that
    # with all on every tw_ticket_* call and tw_wait_regions are made)
    rows, differ = CT.extras_rows(world["exe"], world["files"], world["dir"])
    assert differ == []
    assert rows == parent, sorted(k for k in parent if rows[k] != parent[k])


CACHE_PROGRAM = r'''
#include <stdio.h>
#include <string>
#include <vector>
#include "../resident_cache.h"
using namespace twhost;
extern "C" void tw_stub_resident_calls(long* kept, long* image_pairs, long* released);
static tw_engine* eng;
static long released() { long k, p, r; tw_stub_resident_calls(&k, &p, &r); return r; }
static long kept() { long k, p, r; tw_stub_resident_calls(&k, &p, &r); return k; }
// an image of w x h kept from a pair, as the consumer keeps one
static tw_image* image(int w, int h) {
    std::vector<uint8_t> a((size_t)w * h, 1);
    tw_ticket t; tw_image* img = nullptr;
    tw_submit_u8(eng, a.data(), a.data(), w, h, w, 10, 5.0, &t);
    tw_image_keep(eng, t, TW_KEEP_EXPECT, &img);
    tw_wait(eng, t, nullptr, 0, nullptr, nullptr);
    return img;
}
static void put(ResidentCache& c, const std::string& key, const std::string& path, int w = 16, int h = 16, tw_status r = TW_OK) {
    auto keep = std::make_shared<ResidentCache::Keep>();
    tw_image* img = image(w, h);
    c.open_pending(key, keep, img, w, h);
    c.settle(key, path, keep, img, w, h, r);
}
static void show(const char* what, ResidentCache& c, const char* keys) {
    printf("%s:", what);
    for (const char* k = keys; *k; k++) printf(" %c=%d", *k, (int)c.has(std::string(1, *k)));
    printf(" bytes=%zu released=%ld\n", c.bytes(), released());
}
int main() {
    tw_params p; tw_default_params(&p);
    tw_engine_create(0, &p, 4, &eng);
    {
        ResidentCache c(eng, 3 * 256);  // three images of 16 x 16
        put(c, "A", "/a"); put(c, "B", "/b"); put(c, "C", "/c");
        show("three", c, "ABC");
        c.unpin(c.lookup("A", "/a"));               // A is used last now: B is the oldest
        put(c, "D", "/d"); show("fourth", c, "ABCD");
        ResidentCache::Entry* d = c.lookup("D", "/d");  // pinned
        put(c, "E", "/e"); put(c, "F", "/f"); put(c, "G", "/g");
        show("pinned_evicted", c, "ACDEFG");        // D is out of the cache, its handle is not released
        c.sweep(); show("swept_pinned", c, "D");
        c.unpin(d); show("unpinned", c, "D");
        c.sweep(); show("swept", c, "D");
        put(c, "H", "/h", 64, 64); show("over_budget", c, "HEFG");
        put(c, "I", "/i", 16, 16, TW_E_BAD_IMAGE_FORMAT); show("not_ok", c, "I");
        printf("pending_after_settle: %d\n", (int)(c.find_pending("I") != nullptr));
        c.unpin(c.lookup("G", "/g_link"));          // a second path for G
        c.note_identity("/g", "G2"); show("rewritten", c, "G");
        put(c, "G", "/g"); c.note_identity("/g_link", "other"); show("link_forgotten", c, "G");
        c.note_identity("/g", "G"); show("unchanged", c, "G");
        c.note_identity("/g", ""); show("deleted", c, "G");
    }
    printf("end: kept=%ld released=%ld\n", kept(), released());
    tw_engine_destroy(eng);
    return 0;
}
'''


def test_resident_cache_on_its_own():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    src = os.path.join(HOST, "build", "resident_cache_probe.cpp")
    with open(src, "w") as f:
        f.write(CACHE_PROGRAM)
    exe = os.path.join(HOST, "build", "resident_cache_probe")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", exe, src, os.path.join(HOST, "stub_twflow.cpp"), "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if k not in CT.SWITCHES}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(env, TW_STUB_DEVICES="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert got["three"] == "A=1 B=1 C=1 bytes=768 released=0"
    assert got["fourth"] == "A=1 B=0 C=1 D=1 bytes=768 released=1"               # the least recently used goes, not the oldest insert
    assert got["pinned_evicted"] == "A=0 C=0 D=0 E=1 F=1 G=1 bytes=768 released=3"  # A and C released; D evicted but pinned
    assert got["swept_pinned"] == "D=0 bytes=768 released=3"
    assert got["unpinned"] == "D=0 bytes=768 released=3"                         # the unpin alone releases nothing
    assert got["swept"] == "D=0 bytes=768 released=4"                            # the first sweep after it does
    assert got["over_budget"] == "H=0 E=1 F=1 G=1 bytes=768 released=5"          # released at once, nothing evicted for it
    assert got["not_ok"] == "I=0 bytes=768 released=6"
    assert got["pending_after_settle"] == "0"
    assert got["rewritten"] == "G=0 bytes=512 released=7"                        # a changed identity for a known path evicts
    assert got["link_forgotten"] == "G=1 bytes=768 released=7"                   # the second path went with the old entry
    assert got["unchanged"] == "G=1 bytes=768 released=7"
    assert got["deleted"] == "G=0 bytes=512 released=8"
    assert got["end"] == "kept=10 released=10"
