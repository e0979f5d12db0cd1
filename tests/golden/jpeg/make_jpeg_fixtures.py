"""Writes the JPEG fixtures of this directory and their libjpeg gray decodes (needs PIL = libjpeg-turbo; run by hand, the
results are committed):

    python tests/golden/jpeg/make_jpeg_fixtures.py

Together the files cover baseline and progressive streams, 4:4:4, 4:2:0 and gray sampling and restart markers, at sizes
that are no multiple of a block or of a 4:2:0 MCU (17 x 15 -> 4 x 2 stored luma blocks, 33 x 31 -> 6 x 4, 30 x 35).  The
.pgm beside each file is what cv::imread(path, GRAYSCALE) gives: libjpeg's out_color_space = JCS_GRAYSCALE, i.e. the
luma plane through jidctint (PIL's draft("L") asks libjpeg for exactly that).

golden_expected.jpg / golden_revision2.jpg are the reference's golden PNG pair (../expected_scenario2_capture2.pgm,
../revision2_scenario2_capture2.pgm, 180 x 117) written as gray quality-95 JPEGs: a JPEG pair whose flow has vectors.
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def scene(w, h, shift=0.0, seed=5):
    """A smooth colour image with a few blobs, moved `shift` pixels to the right."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x = x - shift
    img = np.zeros((h, w, 3))
    for _ in range(6):
        cx, cy, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2.0, 7.0)
        img += rng.uniform(40, 160, 3) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))[..., None]
    img += 30 + 20 * np.sin(x / 3.1)[..., None] + 15 * np.cos(y / 2.3)[..., None]
    return np.clip(img, 0, 255).astype(np.uint8)


def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = (int(v) for v in f.readline().split())
        assert f.readline().strip() == b"255"
        return np.frombuffer(f.read(), np.uint8).reshape(h, w)


def write_pgm(path, a):
    h, w = a.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h))
        f.write(a.tobytes())


def save(name, arr, **opts):
    path = os.path.join(HERE, name + ".jpg")
    Image.fromarray(arr).save(path, "JPEG", **opts)
    im = Image.open(path)
    im.draft("L", im.size)
    write_pgm(os.path.join(HERE, name + ".pgm"), np.asarray(im.convert("L"), dtype=np.uint8))
    assert os.path.getsize(path) <= 20 * 1024, name


def main():
    save("baseline_444_17x15", scene(17, 15), quality=90, subsampling=0)
    save("baseline_420_17x15", scene(17, 15, seed=6), quality=75, subsampling=2)
    save("progressive_420_33x31", scene(33, 31), quality=90, subsampling=2, progressive=True)
    save("baseline_gray_33x31", scene(33, 31, shift=1.5)[..., 1].copy(), quality=92)
    save("progressive_444_33x31", scene(33, 31, shift=-1.0), quality=85, subsampling=0, progressive=True)
    save("restart_420_30x35", scene(30, 35, shift=1.5), quality=90, subsampling=2, restart_marker_blocks=2)
    save("restart_gray_30x35", scene(30, 35, seed=8)[..., 0].copy(), quality=80, progressive=True, restart_marker_rows=1)
    golden = os.path.dirname(HERE)
    save("golden_expected", read_pgm(os.path.join(golden, "expected_scenario2_capture2.pgm")), quality=95)
    save("golden_revision2", read_pgm(os.path.join(golden, "revision2_scenario2_capture2.pgm")), quality=95)


def record_damaged(so):
    """damaged_parent.json: what decode_jpeg_gray answers for the damaged files of tests/jpeg_cases.py::damaged_variants —
    recorded once from the decoder as it was BEFORE it was split at the inverse DCT (`so`: that revision's jpeg_gray.cpp
    behind jpeg_cases.PROBE's decode_jpeg_gray), so that the split decoder is held to it."""
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import jpeg_cases as J
    lib = J.bind(so)
    out = {}
    for name, data in J.damaged_variants().items():
        img, wh = J.decode_gray(data, lib)
        out[name] = {"ok": img is not None, "size": list(wh), "crc32": J.crc(img) if img is not None else 0}
    with open(os.path.join(HERE, "damaged_parent.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "--damaged-from":
        record_damaged(sys.argv[2])
    else:
        main()
