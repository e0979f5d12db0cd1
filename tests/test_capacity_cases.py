"""tests/capacity_cases.py without a device: the staging sizes against the figures they restate, the second shape, and
that the wrap-cannot-hide assertion bites on a table it must refuse."""
import pytest

import capacity_cases as CAP
from capacity_cases import P31, P32, P33


def test_staging_sizes_at_1080p_fall_short_of_2_32():
    """512 RGBA row images and 256 flow slots at 1920 x 1080 end just below 2^32 (why the second shape exists)."""
    assert 512 * 1080 * (1 + 1920 * 4) == 4247285760  # the rows themselves; a slot is rounded up to 256 bytes
    assert 512 * CAP.filtered_rows_slot(1920, 1080, 4) == 4247388160 < P32
    assert 256 * CAP.flow_stage_slot(1920, 1080) == 4246732800 < P32
    assert CAP.staged_image_bytes(1920, 1080) == 2073600 and CAP.staged_image_bytes(3, 3) == 256
    assert CAP.jpeg_coef_slot(1920, 1080) == 240 * 135 * 128
    assert CAP.sized_target_slot(1920, 1080) == CAP.round_up(1925 * 1085, 256)


def test_second_shape_is_the_smallest_16_9_size_past_2_32():
    w, h = CAP.smallest_shape_past_2_32()
    assert (w, h) == (1936, 1089) and w * 9 == h * 16
    assert 511 * CAP.filtered_rows_slot(w, h, 4) >= P32 and 255 * CAP.flow_stage_slot(w, h) >= P32
    pw, ph = w - 16, h - 9
    assert 511 * CAP.filtered_rows_slot(pw, ph, 4) < P32 or 255 * CAP.flow_stage_slot(pw, ph) < P32


def test_third_shape_takes_the_gray_images_past_2_32():
    w, h = CAP.smallest_shape_for_images_past_2_32()
    assert (w, h) == (3872, 2178) and 255 * 2 * CAP.staged_image_bytes(w, h) >= P32 > 255 * 2 * CAP.staged_image_bytes(w - 16, h - 9)
    assert 255 * 4 * w * h >= P33  # d_regof / d_lab at span 1


def test_fourth_shape_takes_the_sized_targets_past_2_32():
    w, h = CAP.smallest_shape_for_sized_targets_past_2_32()
    assert w * 9 == h * 16 and 255 * CAP.sized_target_slot(w, h) >= P32 > 255 * CAP.sized_target_slot(w - 16, h - 9)
    assert CAP.round_up(w, 32) * h <= (2 ** 32 - 1) // 20  # inside check_dims' bound on a plane


def _table(bpp, n, per):
    launches = [(0, range(j0, min(j0 + per, n))) for j0 in range(0, n, per)]
    return [CAP._row("R@L0", bpp, launches, bpp * per + 256, "synthetic")]


def test_reductions():
    assert CAP.reductions(P31 - 1) == [] and CAP.reductions(P31) == [P31]
    assert CAP.reductions(3 * P32 + 5) == [P31, P32, P33, 3 * P32]


def test_wrap_assertion_accepts_the_production_table_and_refuses_one_that_hides():
    """R at 1080p: 82 944 000 bytes a pair = 2^13 x 10125, so no power of two is a whole number of slots and a wrapped offset
    lands inside a slot.  A pair of 2^26 bytes with K = 4: slot 64 less 2^32 is slot 0, the same pair — refused; K = 5 and
    K = 7 pass.  128 + 128 with K = 4 also reuses every index for the same pair."""
    rows = _table(82944000, 256, 128)
    assert rows[0].max_index == 127 and CAP.crossings(rows[0]) == (P31, P32, P33)
    for K in (3, 5, 7):
        CAP.assert_wrap_cannot_hide(rows, K)
    rows = _table(1 << 26, 200, 200)
    with pytest.raises(AssertionError, match="choose another K"):
        CAP.assert_wrap_cannot_hide(rows, 4)
    bad = CAP.hidden_wraps(rows, 4)
    assert ("R@L0", 0, 64, 64, P32, 0) in bad and ("R@L0", 0, 32, 32, P31, 0) in bad
    for K in (5, 7):
        CAP.assert_wrap_cannot_hide(rows, K)
    # the second launch's index i held slot i in the first: the same pair when K divides 128
    stale = CAP.hidden_wraps(_table(82944000, 256, 128), 4)
    assert stale and all(lost == 0 for _, _, _, _, lost, _ in stale)
    # a second lane's base counts: 2^32 behind lane 0's slot of the same pair
    lanes = [CAP._row("R@L0", 1 << 26, [(0, range(0, 10)), (P32, range(10, 20))], 0, "synthetic")]
    assert CAP.hidden_wraps(lanes, 5) and not CAP.hidden_wraps(lanes, 7)


def test_vectors_array_round_trip():
    v = [(0, 10, 1.5, -0.25), (10, 10, 0.0, 3.0)]
    a = CAP.vectors_array(v)
    assert a.dtype == CAP.VEC and [tuple(r) for r in a.tolist()] == v and len(CAP.vectors_array([])) == 0
    with pytest.raises(AssertionError, match="slot 1 is the first"):
        CAP.first_wrong_slot([a, a[:1]], lambda s: a, "unit")
    CAP.first_wrong_slot([a, a.copy()], lambda s: a, "unit")
