"""PNG kinds on the device, the host layer's side (tidal-wave_amd/host/twhost.cpp) on the stub backend, no GPU: palette,
1- / 2- / 4-bit gray and 16-bit gray files stay half-decoded and reach tw_submit_png (the stub counts them); the answers
equal those of TW_DEVICE_PNG_KINDS=0, where the host finishes such files; interlaced and 16-bit colour files go through
the host either way; a palette index without an entry answers "Can't open <path>" from the ticket's status.

The files are written here (chunks + zlib.compress), so that 2- and 4-bit gray, short palettes and Adam7 exist, plus
PIL's own palette and 1-bit files.  The stub flags a pair whose first gray pixels differ, so the expected answers follow
from the first pixel's conversion: v * 255 // max, PLTE[v] through libpng 1.5's gray formula, the high byte.
"""
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")

PROBE = r'''
#include <stdio.h>
#include <condition_variable>
#include <mutex>
#include <string>
#include "../twhost.h"
using namespace twhost;
extern "C" void tw_stub_png_calls(long* pairs, long* row_images);
// argv: pairs of (expect path, target path); one JSON line per response, then the stub's tw_submit_png counts
int main(int argc, char** argv) {
    std::mutex m; std::condition_variable cv; int n = 0; bool fin = false;
    Observer o;
    o.onNext = [&](const Response& r) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"%s\", \"target\": \"%s\", \"width\": %d, \"height\": %d, \"vectors\": %d}\n",
               r.status.c_str(), r.target_image.c_str(), r.width, r.height, (int)r.vectors.size());
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
    long pairs = 0, rows = 0;
    tw_stub_png_calls(&pairs, &rows);
    printf("{\"png_pairs\": %ld, \"png_row_images\": %ld}\n", pairs, rows);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    src = os.path.join(HOST, "build", "png_kinds_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    exe = os.path.join(HOST, "build", "png_kinds_probe")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, src] +
                       [os.path.join(HOST, n) for n in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")] +
                       ["-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def pack_rows(samples, depth):
    """samples [h, w, ch] -> the unfiltered rows [h, ceil(w * ch * depth / 8)], samples packed most significant bit first."""
    h, w, ch = samples.shape
    s = samples.reshape(h, w * ch).astype(np.uint16)
    if depth == 16:
        return np.stack([s >> 8, s & 255], -1).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return s.astype(np.uint8)
    bits = (s[..., None] >> np.arange(depth - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(h, -1).astype(np.uint8), axis=1)


def write_png(path, samples, ctype, depth, plte=None, interlace=0):
    """A PNG of samples [h, w, ch] (sample values, palette indices for colour type 3): filter type 0 in every row."""
    h, w, _ = samples.shape

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    def rows(img):
        p = pack_rows(img, depth)
        return np.concatenate([np.zeros((p.shape[0], 1), np.uint8), p], 1).tobytes()

    if interlace:
        passes = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
        raw = b"".join(rows(samples[y0::dy, x0::dx]) for x0, y0, dx, dy in passes if samples[y0::dy, x0::dx].size)
    else:
        raw = rows(samples)
    d = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if plte is not None:
        d += chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes())
    d += chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(d)


def gray15(rgb):
    r, g, b = (int(v) for v in rgb)
    return r if r == g == b else (9797 * r + 19234 * g + 3737 * b) >> 15


def run(probe, pairs, kinds):
    args = [p for pair in pairs for p in pair]
    env = dict(os.environ, TW_DEVICE_PNG_KINDS=kinds, TW_STUB_DEVICES="1", TW_NUMA="0")
    env.pop("TW_DEVICE_PNG", None)
    env.pop("TW_DEVICE_RECONCILE", None)
    r = subprocess.run([probe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.strip().splitlines()]
    assert len(lines) == len(pairs) + 1
    return sorted(json.dumps(x, sort_keys=True) for x in lines[:-1]), lines[-1]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, gray value of the first pixel or None when the file cannot be opened)"""
    from PIL import Image
    d = tmp_path_factory.mktemp("png_kinds")
    rng = np.random.default_rng(11)
    h, w = 21, 37
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g[0, 0] = 200
    out = {}

    def add(name, first, *a, **k):
        path = str(d / (name + ".png"))
        write_png(path, *a, **k)
        out[name] = (path, first)

    add("rgba", 200, np.dstack([g, g, g, np.full_like(g, 255)]), 6, 8)
    ident = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    add("pal8_same", 200, g[..., None], 3, 8, plte=ident)
    g2 = g.copy()
    g2[0, 0] = 77
    add("pal8_diff", 77, g2[..., None], 3, 8, plte=ident)
    plte4 = np.array([[200, 200, 200], [10, 250, 30], [0, 0, 0], [255, 255, 255]], np.uint8)
    idx2 = rng.integers(0, 4, (h, w, 1))
    idx2[0, 0] = 1
    add("pal2", gray15(plte4[1]), idx2, 3, 2, plte=plte4)
    idx2b = idx2.copy()
    idx2b[0, 0] = 0
    add("pal2_same", 200, idx2b, 3, 2, plte=plte4)
    for depth in (1, 2, 4):
        v = rng.integers(0, 1 << depth, (h, w, 1))
        v[0, 0] = (1 << depth) - 2
        add("gray%d" % depth, int(v[0, 0, 0]) * 255 // ((1 << depth) - 1), v, 0, depth)
    v16 = rng.integers(0, 65536, (h, w, 1))
    v16[0, 0] = (200 << 8) | 0x5a
    add("gray16", 200, v16, 0, 16)
    ga16 = rng.integers(0, 65536, (h, w, 2))
    ga16[0, 0, 0] = (31 << 8) | 0xf0
    add("ga16", 31, ga16, 4, 16)
    # a short palette, every index inside it; then the same file with one index without an entry
    short = rng.integers(0, 256, (10, 3)).astype(np.uint8)
    short[3] = (200, 200, 200)
    i10 = rng.integers(0, 10, (h, w, 1))
    i10[0, 0] = 3
    add("short_ok", 200, i10, 3, 8, plte=short)
    bad = i10.copy()
    bad[h // 2, w // 3] = 10
    add("short_bad", None, bad, 3, 8, plte=short)
    # kinds that stay on the host: Adam7, 16-bit colour
    add("pal8_adam7", 77, g2[..., None], 3, 8, plte=ident, interlace=1)
    rgb16 = np.dstack([v16[..., 0]] * 3)
    add("rgb16", 200, rgb16, 2, 16)
    # PIL's own palette and 1-bit files (their first pixel is whatever PIL makes of it: compared between the two runs only)
    p = str(d / "pil_p.png")
    Image.fromarray(np.dstack([g, np.roll(g, 1, 1), g])).quantize(16).save(p)
    out["pil_p"] = (p, -1)
    p = str(d / "pil_1.png")
    Image.fromarray(g).convert("1").save(p)
    out["pil_1"] = (p, -1)
    return out


DEVICE_KINDS = ("pal8_same", "pal8_diff", "pal2", "pal2_same", "gray1", "gray2", "gray4", "gray16", "ga16", "short_ok", "pil_p", "pil_1")


def expected_lines(files, names):
    want = []
    for n in names:
        path, first = files[n]
        if first is None:
            want.append({"status": "ERROR", "reason": "Can't open " + path})
        elif first >= 0:
            differs = first != files["rgba"][1]
            want.append({"status": "SUSPICIOUS" if differs else "OK", "target": path, "width": 37, "height": 21,
                         "vectors": 1 if differs else 0})
    return sorted(json.dumps(x, sort_keys=True) for x in want)


def test_mixed_batch_answers_as_with_the_host_finisher_and_reaches_tw_submit_png(probe, files):
    names = ("rgba",) + DEVICE_KINDS
    pairs = [(files["rgba"][0], files[n][0]) for n in names]
    on, cnt_on = run(probe, pairs, "1")
    off, cnt_off = run(probe, pairs, "0")
    assert on == off
    known = [n for n in names if files[n][1] >= 0]
    got_known = [x for x in on if json.loads(x).get("target") in {files[n][0] for n in known}]
    assert got_known == expected_lines(files, known)
    # every image of every pair reached tw_submit_png as rows; with the switch off only the RGBA ones do, and the pairs
    # whose target the host finished are, for the engine, an RGBA expected image and a gray target
    assert cnt_on == {"png_pairs": len(pairs), "png_row_images": 2 * len(pairs)}
    assert cnt_off == {"png_pairs": len(pairs), "png_row_images": len(pairs) + 1}


def test_a_palette_index_without_an_entry_is_cant_open_from_the_tickets_status(probe, files):
    pairs = [(files["rgba"][0], files["short_ok"][0]), (files["rgba"][0], files["short_bad"][0]),
             (files["short_bad"][0], files["rgba"][0]), (files["rgba"][0], files["pal8_diff"][0])]
    want = sorted(expected_lines(files, ("short_ok", "short_bad", "short_bad", "pal8_diff")))
    on, cnt_on = run(probe, pairs, "1")
    off, cnt_off = run(probe, pairs, "0")
    assert on == want and off == want
    assert cnt_on["png_row_images"] == 8  # the bad file went to the engine like the others: the ticket answered for it
    assert cnt_off["png_row_images"] == 2  # ... and with the switch off the host's decoder refused it before any submit


def test_interlaced_and_16_bit_colour_files_still_go_through_the_host(probe, files):
    names = ("pal8_adam7", "rgb16", "pal8_same", "gray4")
    pairs = [(files["rgba"][0], files[n][0]) for n in names]
    want = expected_lines(files, names)
    on, cnt_on = run(probe, pairs, "1")
    off, _ = run(probe, pairs, "0")
    assert on == want and off == want
    # the two host-side files take the batch off the arena path, but the others are still handed over as rows
    assert cnt_on == {"png_pairs": 4, "png_row_images": 4 + 2}
