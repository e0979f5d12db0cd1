"""tw_resize_u8 alone (tw_stage_resize_u8) against the oracle's orc_resize_u8_linear: OpticalFlow::calculate's <= 5 px size
reconcile (src/opticalflow.cpp:52-68), cv::resize on CV_8UC1 with INTER_LINEAR as OpenCV 2.4.9's fixed-point path computes it.

Parity bar: BYTE-EXACT (np.array_equal) — the arithmetic is integer after the float weights, and the weights are single
IEEE operations on both sides.  Every source below is resized to every size within 5 px of its own (except its own),
as far as both sides stay >= 1: 120 destinations for an ordinary source.  tests/test_size_reconcile.py holds the oracle
against the product's host code and a numpy restatement on the CPU.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def destinations(sw, sh):
    return [(sw + dx, sh + dy) for dy in range(-5, 6) for dx in range(-5, 6)
            if (dx, dy) != (0, 0) and sw + dx >= 1 and sh + dy >= 1]


def noise(sw, sh):
    return np.random.default_rng(sw * 131 + sh).integers(0, 256, (sh, sw), dtype=np.uint8)


def golden_pgm(sw, sh):
    import oracle as O
    img = O.read_pgm(os.path.join(GOLDEN, "revision2_scenario2_capture2.pgm"))
    assert img.shape == (sh, sw)
    return img


SOURCES = [
    ("noise: every weight matters", 67, 41, noise),
    ("all 255: the 22-bit cast", 9, 12, lambda sw, sh: np.full((sh, sw), 255, np.uint8)),
    ("a golden PGM", 180, 117, golden_pgm),
    # sx + 1 >= sw everywhere, a source of one column / one row, the exact halving (10 x 8 -> 5 x 4, 2 x 2 -> 1 x 1)
    ("1 x 1", 1, 1, noise), ("one column", 1, 7, noise), ("one row", 6, 1, noise), ("2 x 2", 2, 2, noise),
    ("10 x 8", 10, 8, noise),
]
# a row's end at every position of a lane's 4-pixel group and of a wave's 256-pixel span; dense rows of odd widths start
# at all four byte alignments
SOURCES += [("row end around one wave", sw, 3, noise) for sw in range(251, 262)]
SOURCES += [("row end around four waves", sw, 2, noise) for sw in range(1019, 1030)]


def test_enough_cases():
    """A silently skipped loop would pass everything below: the destinations are counted from the same lists."""
    n = sum(len(destinations(sw, sh)) for _, sw, sh, _ in SOURCES) + 1  # + the 1080p case
    assert n > 1200, n
    assert len(destinations(67, 41)) == 120 and len(destinations(1, 1)) == 35 and (5, 4) in destinations(10, 8)


@pytest.mark.parametrize("what,sw,sh,make", SOURCES, ids=["%dx%d" % (s[1], s[2]) for s in SOURCES])
def test_every_size_within_five_pixels(engine, oracle, what, sw, sh, make):
    src = make(sw, sh)
    engine.launch_counts(reset=True)
    done = 0
    for dw, dh in destinations(sw, sh):
        got = engine.stage_resize_u8(src, dw, dh)
        want = oracle.resize_u8_linear(src, dw, dh)
        assert got.shape == want.shape == (dh, dw)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            pytest.fail("%s: %dx%d -> %dx%d: %d of %d bytes differ, first at (y, x) = %s: got %d, want %d"
                        % (what, sw, sh, dw, dh, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
        done += 1
    assert done == len(destinations(sw, sh)) > 0
    cnt = engine.launch_counts()
    assert cnt["tw_resize_u8"] == done and cnt.last_z["tw_resize_u8"] == 1, cnt


def test_1080p_both_directions_at_once(engine, oracle):
    """1925 x 1075 -> 1920 x 1080: narrower and taller in one call, eight waves per row."""
    src = noise(1925, 1075)
    got = engine.stage_resize_u8(src, 1920, 1080)
    assert np.array_equal(got, oracle.resize_u8_linear(src, 1920, 1080))


def test_sizes_more_than_five_pixels_apart_are_refused(engine, twflow):
    src = noise(40, 30)
    for dw, dh in ((46, 30), (40, 24), (45, 36)):
        with pytest.raises(twflow.TwError) as ei:
            engine.stage_resize_u8(src, dw, dh)
        assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
