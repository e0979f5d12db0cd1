"""The host JPEG decoder split at the inverse DCT (host/jpeg_gray.cpp): decode_jpeg_luma stops at the quantised luma
coefficients, jpeg_luma_to_gray is the IDCT + crop, decode_jpeg_gray is the two in sequence.  No GPU, no node: the three
entry points are compiled behind a C API at test time (tests/jpeg_cases.py).

Pinned to libjpeg, not to itself: the committed .pgm files and PIL's own gray decode of files written here; and to the
algorithm: a numpy int64 restatement of jidctint on random blocks, full int16 / uint16 range included (what a damaged
file reaches).  tests/golden/jpeg/damaged_parent.json holds what decode_jpeg_gray answered for the damaged files before
the split.
"""
import json
import os

import numpy as np
import pytest

import jpeg_cases as J


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if J.host_lib() is None:
        pytest.skip("no g++")


def both_ways(data):
    luma, wh = J.decode_luma(data)
    whole, wh2 = J.decode_gray(data)
    assert (luma is None) == (whole is None)
    if luma is None:
        return None, None, luma
    assert wh == wh2 == (luma.w, luma.h)
    return J.luma_to_gray(luma), whole, luma


@pytest.mark.parametrize("rev", ["expected", "revision1", "revision2"])
def test_the_reference_fixture_in_two_steps_equals_libjpeg(rev):
    data, want = J.capture1(rev)
    split, whole, luma = both_ways(data)
    assert np.array_equal(split, whole) and np.array_equal(split, want)
    assert (luma.w, luma.h) == (280, 279)
    bh, bw = luma.coef.shape[:2]
    assert bw >= 35 and bh >= 35 and bw <= 38 and bh <= 38


@pytest.mark.parametrize("name", J.fixture_names())
def test_committed_files_in_two_steps_equal_libjpeg(name):
    data, want = J.fixture(name)
    assert len(data) <= 20 * 1024
    split, whole, luma = both_ways(data)
    assert np.array_equal(split, whole) and np.array_equal(split, want), name
    assert luma.coef.shape[1] >= (luma.w + 7) // 8 and luma.coef.shape[1] <= (luma.w + 7) // 8 + 3


def test_the_committed_files_cover_what_they_claim():
    """baseline and progressive; 4:4:4, 4:2:0 and gray; restart markers; the three sizes; the 4:2:0 padding blocks"""
    kinds = set()
    for name in J.fixture_names():
        data, want = J.fixture(name)
        sof = max(data.find(b"\xff\xc0"), data.find(b"\xff\xc2"))
        prog = data[sof + 1] == 0xC2
        ncomp = data[sof + 9]
        samp = data[sof + 11]
        dri = b"\xff\xdd" in data
        kinds.add(("progressive" if prog else "baseline", "gray" if ncomp == 1 else "%x" % samp, dri, want.shape[::-1]))
        luma, _ = J.decode_luma(data)
        if ncomp == 3 and samp == 0x22:
            assert luma.coef.shape[0] % 2 == 0 and luma.coef.shape[1] % 2 == 0  # whole 16 x 16 MCUs
    assert {k[0] for k in kinds} == {"baseline", "progressive"}
    assert {k[1] for k in kinds} == {"gray", "11", "22"}
    assert any(k[2] for k in kinds)
    assert {(17, 15), (33, 31), (30, 35)} <= {k[3] for k in kinds}
    shapes = {n: J.decode_luma(J.fixture(n)[0])[0].coef.shape[:2] for n in ("baseline_420_17x15", "progressive_420_33x31")}
    assert shapes == {"baseline_420_17x15": (2, 4), "progressive_420_33x31": (4, 6)}


def test_written_variants_in_two_steps_equal_libjpeg(tmp_path):
    """Every variant of test_node_addon.py::test_jpeg_decode_matches_libjpeg_on_written_files, regenerated here: 2 images x
    baseline / progressive x 3 samplings x 2 (quality, restart interval) + 2 gray files with optimised tables = 26 files."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (157, 211, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:157, 0:211]
    smooth = np.stack([(xx * 1.2 + yy * 0.3) % 256, np.sin(xx / 9.) * 100 + 128, (yy * 1.5) % 256], -1).astype(np.uint8)
    smooth[40:80, 50:120] = noise[40:80, 50:120]
    cases = []
    for name, img in (("noise", noise), ("smooth", smooth)):
        for prog in (False, True):
            for ss in (0, 1, 2):
                for q, rst in ((35, 0), (90, 3)):
                    kw = dict(quality=q, progressive=prog, subsampling=ss)
                    if rst:
                        kw["restart_marker_blocks"] = rst
                    p = tmp_path / ("%s_p%d_s%d_q%d_r%d.jpg" % (name, prog, ss, q, rst))
                    Image.fromarray(img).save(p, **kw)
                    cases.append(p)
    for prog in (False, True):
        p = tmp_path / ("gray%d.jpg" % prog)
        Image.fromarray(smooth[..., 0]).save(p, quality=80, progressive=prog, optimize=True)
        cases.append(p)
    assert len(cases) == 26
    for p in cases:
        im = Image.open(p)
        im.draft("L", im.size)
        want = np.asarray(im.convert("L"), dtype=np.uint8)
        split, whole, _ = both_ways(p.read_bytes())
        assert split is not None and np.array_equal(split, want) and np.array_equal(whole, want), p.name


@pytest.mark.parametrize("full_range", [True, False], ids=["full_range", "valid_range"])
def test_jpeg_luma_to_gray_equals_the_numpy_jidctint(full_range):
    n = 2000
    coef, quant = J.random_blocks(n, 31 if full_range else 32, full_range)
    if full_range:
        assert coef.min() == -32768 and coef.max() == 32767 and quant.max() == 65535
    want = J.idct_reference(coef, quant)
    bw, bh = 50, 40
    luma = J.Luma(bw * 8 - 3, bh * 8 - 5, coef.reshape(bh, bw, 64), quant)
    got = J.luma_to_gray(luma)
    assert np.array_equal(got, J.blocks_to_image(want, bw, bh, luma.w, luma.h))
    if not full_range:
        assert len(np.unique(got)) > 100  # (not a saturated image)


def test_damaged_files_fail_where_they_failed_before_the_split():
    with open(os.path.join(J.JPEG_DIR, "damaged_parent.json")) as f:
        parent = json.load(f)
    variants = J.damaged_variants()
    assert sorted(parent) == sorted(variants) and len(variants) == 18
    assert any(not v["ok"] for v in parent.values()) and any(v["ok"] for v in parent.values())
    for name, data in variants.items():
        luma, wh = J.decode_luma(data)
        whole, wh2 = J.decode_gray(data)
        assert (luma is not None) == (whole is not None) == parent[name]["ok"], name
        if luma is None:
            assert wh == (0, 0) and wh2 == (0, 0), name  # no size on failure
            continue
        assert [luma.w, luma.h] == parent[name]["size"], name
        assert J.crc(whole) == parent[name]["crc32"] and J.crc(J.luma_to_gray(luma)) == parent[name]["crc32"], name
