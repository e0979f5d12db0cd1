"""JPEG on the device, the host layer's side (tidal-wave_amd/host/twhost.cpp) on the stub backend, no GPU: a JPEG stops at
its coefficient plane and reaches tw_submit_jpeg (the stub counts pairs and coefficient images); the answers equal those
of TW_DEVICE_JPEG=0, where the host runs the inverse DCT as before; a JPEG beside half-decoded PNG rows is finished on the
host; sizes within 5 px are handed over, sizes further apart answer the reference's "Don't match image size".

The stub flags a pair whose first gray pixels differ (for a coefficient image: the host's inverse DCT of block 0), so the
expected answers follow from the committed libjpeg decodes.
"""
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import jpeg_cases as J

HOST = J.HOST

PROBE = r'''
#include <stdio.h>
#include <condition_variable>
#include <mutex>
#include <string>
#include "../twhost.h"
using namespace twhost;
extern "C" void tw_stub_png_calls(long* pairs, long* row_images);
extern "C" void tw_stub_jpeg_calls(long* pairs, long* coef_images);
// argv: pairs of (expect path, target path); one JSON line per response, then the stub's counts
int main(int argc, char** argv) {
    std::mutex m; std::condition_variable cv; int n = 0; bool fin = false;
    Observer o;
    o.onNext = [&](const Response& r) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"%s\", \"expect\": \"%s\", \"target\": \"%s\", \"width\": %d, \"height\": %d, \"vectors\": %d}\n",
               r.status.c_str(), r.expect_image.c_str(), r.target_image.c_str(), r.width, r.height, (int)r.vectors.size());
        n++; cv.notify_all(); };
    o.onError = [&](const std::string& e) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"ERROR\", \"reason\": \"%s\"}\n", e.c_str());
        n++; cv.notify_all(); };
    o.onCompleted = [&](const Report&) { std::lock_guard<std::mutex> lk(m); fin = true; cv.notify_all(); };
    Parameter p; tw_default_params(&p.optParam); p.numThreads = 1; p.batch = 16;
    Manager* mg = new Manager(o); mg->start(p); mg->waitReady();
    for (int i = 0; i + 2 < argc; i += 2) mg->request(argv[1 + i], argv[2 + i]);
    { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return n >= (argc - 1) / 2; }); }
    mg->stop(); { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return fin; }); } delete mg;
    long pp = 0, pr = 0, jp = 0, jc = 0;
    tw_stub_png_calls(&pp, &pr);
    tw_stub_jpeg_calls(&jp, &jc);
    printf("{\"png_pairs\": %ld, \"png_row_images\": %ld, \"jpeg_pairs\": %ld, \"jpeg_coef_images\": %ld}\n", pp, pr, jp, jc);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    src = os.path.join(HOST, "build", "jpeg_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    exe = os.path.join(HOST, "build", "jpeg_probe")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, src] +
                       [os.path.join(HOST, n) for n in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")] +
                       ["-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(probe, pairs, device_jpeg, **env_more):
    args = [p for pair in pairs for p in pair]
    env = dict(os.environ, TW_STUB_DEVICES="1", TW_NUMA="0", **env_more)
    for k in ("TW_DEVICE_PNG", "TW_DEVICE_PNG_KINDS", "TW_DEVICE_RECONCILE", "TW_DEVICE_JPEG"):
        if k not in env_more:
            env.pop(k, None)
    if device_jpeg is not None:
        env["TW_DEVICE_JPEG"] = device_jpeg
    r = subprocess.run([probe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.strip().splitlines()]
    assert len(lines) == len(pairs) + 1
    return sorted(json.dumps(x, sort_keys=True) for x in lines[:-1]), lines[-1]


def jpg(name):
    return os.path.join(J.JPEG_DIR, name + ".jpg")


def pgm(name):
    return os.path.join(J.JPEG_DIR, name + ".pgm")


def first(name):
    return int(J.fixture(name)[1][0, 0])


def write_rgba_png(path, gray):
    h, w = gray.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), np.dstack([gray] * 3 + [np.full_like(gray, 255)]).reshape(h, -1)], 1)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def answer(expect, target, w, h, differs):
    return json.dumps({"status": "SUSPICIOUS" if differs else "OK", "expect": expect, "target": target, "width": w,
                       "height": h, "vectors": 1 if differs else 0}, sort_keys=True)


A, B, Cc = "progressive_420_33x31", "baseline_gray_33x31", "progressive_444_33x31"


def test_jpeg_pairs_reach_tw_submit_jpeg_and_answer_as_with_the_host_idct(probe):
    pairs = [(jpg(A), jpg(B)), (jpg(A), jpg(Cc)), (jpg(A), jpg(A)), (jpg("baseline_444_17x15"), jpg("baseline_420_17x15"))]
    want = sorted([answer(jpg(A), jpg(B), 33, 31, first(A) != first(B)), answer(jpg(A), jpg(Cc), 33, 31, first(A) != first(Cc)),
                   answer(jpg(A), jpg(A), 33, 31, False),
                   answer(jpg("baseline_444_17x15"), jpg("baseline_420_17x15"), 17, 15,
                          first("baseline_444_17x15") != first("baseline_420_17x15"))])
    assert first(A) != first(B)  # (at least one pair the stub flags)
    on, cnt_on = run(probe, pairs, "1")
    off, cnt_off = run(probe, pairs, "0")
    default, cnt_default = run(probe, pairs, None)
    assert on == want and off == want and default == want
    assert cnt_on == {"png_pairs": 0, "png_row_images": 0, "jpeg_pairs": 4, "jpeg_coef_images": 8}
    assert cnt_off == {"png_pairs": 0, "png_row_images": 0, "jpeg_pairs": 0, "jpeg_coef_images": 0}
    assert cnt_default in (cnt_on, cnt_off)  # whichever default the measurement chose (profiles/jpeg_device.md)


def test_a_jpeg_beside_a_png_or_a_pgm(probe, tmp_path):
    """JPEG + plain gray goes to tw_submit_jpeg with one coefficient image; JPEG + half-decoded PNG rows is finished on the
    host and goes on through tw_submit_png as before.  The answers are those of the host path."""
    png = str(tmp_path / "b.png")
    write_rgba_png(png, J.fixture(B)[1])
    pairs = [(jpg(A), pgm(B)), (pgm(B), jpg(A)), (jpg(A), png), (png, jpg(A)), (jpg(A), pgm(A))]
    d = first(A) != first(B)
    want = sorted([answer(jpg(A), pgm(B), 33, 31, d), answer(pgm(B), jpg(A), 33, 31, d), answer(jpg(A), png, 33, 31, d),
                   answer(png, jpg(A), 33, 31, d), answer(jpg(A), pgm(A), 33, 31, False)])
    on, cnt_on = run(probe, pairs, "1")
    off, cnt_off = run(probe, pairs, "0")
    assert on == want and off == want
    assert cnt_on == {"png_pairs": 2, "png_row_images": 2, "jpeg_pairs": 3, "jpeg_coef_images": 3}
    assert cnt_off == {"png_pairs": 2, "png_row_images": 2, "jpeg_pairs": 0, "jpeg_coef_images": 0}


@pytest.mark.parametrize("device_reconcile", ["1", "0"])
def test_unequal_jpeg_sizes_are_handed_over_or_refused(probe, device_reconcile):
    """33 x 31 expected, 30 x 35 target (3 px narrower, 4 px taller): answered at the pair's size — with the device's
    reconcile the target goes over as coefficients at its own size, without it the host finishes and resizes it.  17 x 15
    against 33 x 31 is more than 5 px off: the reference's "Don't match image size", nothing submitted."""
    T = "restart_420_30x35"
    pairs = [(jpg(A), jpg(T)), (jpg(A), jpg("baseline_444_17x15")), (jpg("baseline_444_17x15"), jpg(A))]
    got, cnt = run(probe, pairs, "1", TW_DEVICE_RECONCILE=device_reconcile)
    off, cnt_off = run(probe, pairs, "0", TW_DEVICE_RECONCILE=device_reconcile)
    errors = [x for x in got if json.loads(x)["status"] == "ERROR"]
    assert [json.loads(x)["reason"] for x in errors] == ["Don't match image size"] * 2
    answered = [json.loads(x) for x in got if json.loads(x)["status"] != "ERROR"]
    assert len(answered) == 1 and (answered[0]["width"], answered[0]["height"]) == (33, 31)
    assert answered[0]["target"] == jpg(T)
    assert cnt["jpeg_pairs"] == 1 and cnt["jpeg_coef_images"] == (2 if device_reconcile == "1" else 1)
    assert cnt_off["jpeg_pairs"] == 0
    assert got == off


def test_a_jpeg_that_cannot_be_decoded_is_cant_open(probe, tmp_path):
    bad = str(tmp_path / "cut.jpg")
    with open(bad, "wb") as f:
        f.write(J.fixture(A)[0][:40])
    rgb = str(tmp_path / "missing.jpg")
    pairs = [(jpg(A), bad), (bad, jpg(A)), (jpg(A), rgb)]
    want = sorted(json.dumps({"status": "ERROR", "reason": "Can't open " + p}, sort_keys=True) for p in (bad, bad, rgb))
    on, cnt_on = run(probe, pairs, "1")
    off, _ = run(probe, pairs, "0")
    assert on == want and off == want
    assert cnt_on["jpeg_pairs"] == 0
