"""tests/overlay_ref.py against pictures worked out by hand from the text of include/twflow.h ("Diff image").  No GPU: this is
what makes the reference of tests/test_gpu_overlay.py trustworthy."""
import numpy as np
import pytest

import overlay_ref as R

GRAY = (128, 128, 128)  # base colour of an unchanged pixel with t = 0: g = 128 + (0 >> 1)
BLUE, GREEN = (0, 0, 255), (0, 160, 0)


def _flat(w, h):
    z = np.zeros((h, w), np.uint8)
    return z, z.copy()


def _coloured(img, rgb):
    ys, xs = np.nonzero((img == np.array(rgb, np.uint8)).all(axis=-1))
    return sorted(zip(xs.tolist(), ys.tolist()))


def test_q_rounds_ties_to_even_clamps_and_maps_nan_to_zero():
    want = {0.5: 0, -0.5: 0, 1.5: 2, -1.5: -2, 2.5: 2, -2.5: -2, 3.5: 4, 0.49: 0, 0.51: 1, 1024.0: 1024, -1024.0: -1024,
            1024.5: 1024, -1024.5: -1024, 1023.5: 1024, 1022.5: 1022, float("inf"): 1024, float("-inf"): -1024,
            float("nan"): 0, 3.0e38: 1024}
    for v, r in want.items():
        assert R.q(np.float32(v)) == r, v


def test_one_hit_on_5x4_the_tie_rounds_to_two():
    E, T = _flat(5, 4)
    img = R.overlay_ref(E, T, [], [(2, 1, 2.5, -0.5)], [], 16)
    # rx = q(2.5) = 2, ry = q(-0.5) = 0, n = 2: i = 0: (2 + floor(2 / 4), 1) = (2, 1); i = 1: (2 + floor(6 / 4), 1) = (3, 1);
    # i = 2: (2 + floor(10 / 4), 1) = (4, 1); marker: x 1 .. 3, y 0 .. 2
    blue = sorted([(x, y) for x in (1, 2, 3) for y in (0, 1, 2)] + [(4, 1)])
    assert _coloured(img, BLUE) == blue
    assert len(_coloured(img, GRAY)) == 20 - len(blue)


def test_negative_components_use_floor_division():
    E, T = _flat(7, 7)
    img = R.overlay_ref(E, T, [], [(3, 3, -2.0, -1.0)], [], 16)
    # n = 2: i = 1: x = 3 + floor(-2 / 4) = 2, y = 3 + floor(0 / 4) = 3; i = 2: x = 3 + floor(-6 / 4) = 1, y = 3 + floor(-2 / 4) = 2
    marker = [(x, y) for x in (2, 3, 4) for y in (2, 3, 4)]
    assert _coloured(img, BLUE) == sorted(set(marker + [(3, 3), (2, 3), (1, 2)]))


def test_n_zero_draws_the_marker_only():
    E, T = _flat(5, 5)
    for d in ((0.0, 0.0), (0.5, -0.5), (float("nan"), float("nan")), (0.25, float("nan"))):
        img = R.overlay_ref(E, T, [], [(2, 2) + d], [], 16)
        assert _coloured(img, BLUE) == sorted((x, y) for x in (1, 2, 3) for y in (1, 2, 3))


@pytest.mark.parametrize("d,length", [((float("inf"), 0.0), 1024), ((float("-inf"), 0.0), -1024), ((1024.5, 0.0), 1024),
                                      ((-1024.5, 0.0), -1024), ((float("nan"), 1024.5), 1024)])
def test_non_finite_and_clamped_components(d, length):
    w = 2 * 1024 + 41
    E, T = _flat(w, 3)
    x0 = 1024 + 20
    img = R.overlay_ref(E, T, [], [(x0, 1) + d], [], 16)
    blue = set((x, y) for x in (x0 - 1, x0, x0 + 1) for y in (0, 1, 2))
    if np.isnan(d[0]):  # the line runs down: 1025 pixels, of which rows 1 .. 2 are inside
        blue |= {(x0, 1), (x0, 2)}
    else:
        step = 1 if length > 0 else -1
        blue |= {(x0 + step * i, 1) for i in range(1025)}
        assert (x0 + length, 1) in blue
    assert _coloured(img, BLUE) == sorted(blue)


def test_lines_leave_each_edge_and_markers_sit_in_each_corner():
    E, T = _flat(5, 5)
    for d, kept in (((4.0, 0.0), [(3, 2), (4, 2)]), ((-4.0, 0.0), [(1, 2), (0, 2)]), ((0.0, 4.0), [(2, 3), (2, 4)]),
                    ((0.0, -4.0), [(2, 1), (2, 0)])):
        img = R.overlay_ref(E, T, [], [(2, 2) + d], [], 16)
        marker = [(x, y) for x in (1, 2, 3) for y in (1, 2, 3)]
        assert _coloured(img, BLUE) == sorted(set(marker + kept)), d
    for (cx, cy), kept in (((0, 0), [(0, 0), (1, 0), (0, 1), (1, 1)]), ((4, 0), [(3, 0), (4, 0), (3, 1), (4, 1)]),
                           ((0, 4), [(0, 3), (1, 3), (0, 4), (1, 4)]), ((4, 4), [(3, 3), (4, 3), (3, 4), (4, 4)])):
        img = R.overlay_ref(E, T, [], [(cx, cy, 0.0, 0.0)], [], 16)
        assert _coloured(img, BLUE) == sorted(kept)
    # a hit outside the image still draws what reaches in
    img = R.overlay_ref(E, T, [], [(-1, 2, 3.0, 0.0)], [], 16)
    assert _coloured(img, BLUE) == sorted([(0, 1), (0, 2), (0, 3), (1, 2), (2, 2)])


def test_boxes_thin_on_the_border_and_without_area():
    E, T = _flat(6, 5)
    assert _coloured(R.overlay_ref(E, T, [], [], [(1, 1, 1, 3)], 16), GREEN) == [(1, 1), (1, 2), (1, 3)]
    assert _coloured(R.overlay_ref(E, T, [], [], [(1, 2, 4, 1)], 16), GREEN) == [(1, 2), (2, 2), (3, 2), (4, 2)]
    assert _coloured(R.overlay_ref(E, T, [], [], [(2, 2, 1, 1)], 16), GREEN) == [(2, 2)]
    assert _coloured(R.overlay_ref(E, T, [], [], [(2, 2, 0, 3), (2, 2, 3, 0)], 16), GREEN) == []
    full = R.overlay_ref(E, T, [], [], [(0, 0, 6, 5)], 16)
    assert _coloured(full, GRAY) == sorted((x, y) for x in range(1, 5) for y in range(1, 4))
    assert len(_coloured(full, GREEN)) == 30 - 12
    # a 3 x 3 box keeps its one inner pixel; a box that sticks out loses what is outside
    assert _coloured(R.overlay_ref(E, T, [], [], [(1, 1, 3, 3)], 16), GRAY).count((2, 2)) == 1
    assert _coloured(R.overlay_ref(E, T, [], [], [(4, 3, 4, 4)], 16), GREEN) == [(4, 3), (4, 4), (5, 3)]


def test_priority_vectors_over_boxes_over_base():
    E = np.zeros((8, 8), np.uint8)
    T = np.zeros((8, 8), np.uint8)
    T[2, :] = 200  # a changed row: d = 200 > 16 -> (255, 192 - 100, 0)
    boxes = [(0, 0, 8, 8), (1, 1, 4, 4), (2, 2, 2, 2)]  # nested; the inner two overlap the changed row
    hits = [(2, 2, 3.0, 0.0), (4, 2, 0.0, 0.0)]          # overlapping vectors on the changed row and on box outlines
    img = R.overlay_ref(E, T, [], hits, boxes, 16)
    assert tuple(img[2, 7]) == GREEN          # box over a changed pixel
    assert tuple(img[2, 6]) == (255, 92, 0)   # the changed base where nothing is drawn
    assert tuple(img[2, 1]) == BLUE           # vector over box over changed base: all three compete at (1, 2)
    assert tuple(img[2, 5]) == BLUE           # the line's end and the second marker
    assert tuple(img[4, 1]) == GREEN and tuple(img[3, 3]) == BLUE and tuple(img[5, 5]) == (128, 128, 128)
    # the order inside a layer does not matter
    assert np.array_equal(img, R.overlay_ref(E, T, [], hits[::-1], boxes[::-1], 16))


def test_a_rectangle_covers_a_changed_pixel_and_a_hit():
    E = np.zeros((6, 6), np.uint8)
    T = np.zeros((6, 6), np.uint8)
    T[1, 1] = 255
    T[4, 4] = 255
    rects = R.clip_rects([(-3, -3, 5, 5), (9, 9, 2, 2), (0, 0, 0, 4)], 6, 6)
    assert rects == [(0, 0, 2, 2)]
    hits = R.outside([(1, 1, 2.0, 0.0), (4, 4, 0.0, 0.0)], rects)
    assert hits == [(4, 4, 0.0, 0.0)]
    img = R.overlay_ref(E, T, rects, hits, [], 16)
    assert tuple(img[1, 1]) == (255 - 48, 255 - 48, 255)  # g = 128 + 127, inside the rectangle: not the "changed" colour
    assert tuple(img[0, 0]) == (80, 80, 128)
    assert tuple(img[4, 4]) == BLUE and tuple(img[1, 2]) == GRAY and tuple(img[1, 3]) == GRAY  # the ignored hit drew nothing


def test_tol_0_and_tol_255():
    E = np.array([[0, 10, 255, 7]], np.uint8)
    T = np.array([[0, 11, 0, 7]], np.uint8)
    a = R.overlay_ref(E, T, [], [], [], 0)
    assert [tuple(p) for p in a[0]] == [(128, 128, 128), (255, 192, 0), (255, 192 - 127, 0), (131, 131, 131)]
    b = R.overlay_ref(E, T, [], [], [], 255)
    assert [tuple(p) for p in b[0]] == [(128, 128, 128), (133, 133, 133), (128, 128, 128), (131, 131, 131)]
