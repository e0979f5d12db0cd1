"""tests/residual_ref.py, the reference of the residual tests: hand-worked tiny cases, the properties the semantics promise,
and — with the oracle's flow at 397 x 99, the smallest shape that reaches tw_flow_iter — what the feature is for: a flat
repaint that no vector reports is reported as unexplained, a moved block is mostly explained, a global shift almost wholly.
CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tidal-wave_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import residual_ref as R

SPAN, THRESHOLD, TOL = 10, 5.0, 16


def test_quantise_ties_limits_and_specials():
    f = np.float32
    # multiples of 1/64 are the ties of a 1/32 grid: half-even goes down to an even and up to an even neighbour of an odd
    d = np.array([1, 3, 5, 7, -1, -3, -5, 2, -2], f) / f(64)
    assert R.quantise(d).tolist() == [0, 2, 2, 4, 0, -2, -2, 1, -1]
    big = f(16384)
    d = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, big, -big, np.nextafter(big, f(np.inf)), np.nextafter(-big, f(-np.inf)),
                  np.nextafter(big, f(0))], f)
    assert R.quantise(d).tolist() == [0, 524288, -524288, 524288, -524288, 524288, -524288, 524288, -524288, 524288]
    # (the float below 16384 is 16384 - 2^-10: times 32 it is 524287.96875, which rounds up)
    assert R.quantise(f(2.5)) == 80 and R.quantise(f(-0.0)) == 0


def test_three_by_two_by_hand():
    T = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    fx = np.array([[-5, 0.5, 9], [-0.25, 0.75, 9]], np.float32)
    fy = np.array([[-5, 0.5, -9], [9, 0.25, 9]], np.float32)
    # (0,0): both clamps at 0 -> T[0][0].  (1,0): sx = 48, sy = 16: ix 1 ax 16, iy 0 ay 16: (20+30+50+60)*256 + 512 >> 10 = 40
    # (40.5 rounds down: + 512 then a shift).  (2,0): sx clamps at 64 -> ix 2, x1 = min(3, 2); sy clamps at 0 -> 30.
    # (0,1): sx = clamp(-8) = 0, sy = clamp(32 + 288, 32) -> iy 1, y1 = min(2, 1) -> 40.
    # (1,1): sx = 32 + 24 = 56: ix 1 ax 24; sy = 32 + 8 = 40 -> clamp 32: iy 1 ay 0: (50*8*32 + 60*24*32 + 512) >> 10 = 58
    # (2,1): both clamp at the far corner -> 60
    want = np.array([[10, 40, 30], [40, 58, 60]])
    assert np.array_equal(R.warp(T, fx, fy), want)
    E = np.array([[10, 41, 0], [44, 50, 70]], np.uint8)
    diff, u = R.pixels(E, T, fx, fy)
    assert diff.tolist() == [[0, 21, 30], [4, 0, 10]] and u.tolist() == [[0, 1, 30], [4, 0, 10]]
    c = R.cells(E, T, fx, fy, 2, 3)
    # cells of span 2: columns {0, 1} and {2}, one cell row
    assert c.tolist() == [[[2, 1, 21, 4], [2, 2, 30, 30]]]
    assert R.changes(c, 2) == [(0, 0, 2, 1, 21, 4), (2, 0, 2, 2, 30, 30)]
    assert R.changes(c, 2, ignore=[(2, 0, 1, 1)]) == [(0, 0, 2, 1, 21, 4)]
    assert R.changes(c, 2, ignore=[(1, 0, 1, 2)]) == R.changes(c, 2)  # (the grid point decides, not the cell)
    # span 1: every pixel a cell, and only the differing ones are reported; a span beyond the image: one cell
    assert [r[:2] for r in R.changes(R.cells(E, T, fx, fy, 1, 3), 1)] == [(1, 0), (2, 0), (0, 1), (2, 1)]
    assert R.cells(E, T, fx, fy, 100, 3).tolist() == [[[4, 3, 30, 30]]]
    assert R.changes(R.cells(E, T, fx, fy, 100, 254), 100) == []  # n_diff counts diff > tol


@pytest.mark.parametrize("w,h,span", [(1, 1, 1), (7, 5, 4), (33, 17, 10), (64, 64, 16), (130, 67, 1), (50, 41, 100)])
def test_properties(w, h, span):
    rng = np.random.default_rng(w * 1000 + h)
    E = rng.integers(0, 256, (h, w), dtype=np.uint8)
    T = rng.integers(0, 256, (h, w), dtype=np.uint8)
    wild = rng.uniform(-8, 8, (2, h, w)).astype(np.float32)
    wild.ravel()[::7] = np.float32(1e30)
    wild.ravel()[3::11] = np.float32(np.nan)
    wild.ravel()[5::13] = np.float32(-np.inf)
    for tol in (1, 16, 254):
        # an identical pair has no record, under any field
        c = R.cells(E, E, wild[0], wild[1], span, tol)
        assert not c.any() and R.changes(c, span) == []
        c = R.cells(E, T, wild[0], wild[1], span, tol)
        assert np.array_equal(c, R.cells_fast(E, T, wild[0], wild[1], span, tol))
        assert (c[..., 1] <= c[..., 0]).all() and (c[..., 3] <= c[..., 2]).all()
    # an exact integer shift with its true field is explained wherever the flow's end is inside the image
    for sx, sy in ((3, 0), (-2, 1), (0, -4)):
        if abs(sx) >= w or abs(sy) >= h:
            continue
        ys, xs = np.mgrid[0:h, 0:w]
        inside = (xs + sx >= 0) & (xs + sx < w) & (ys + sy >= 0) & (ys + sy < h)
        S = rng.integers(0, 256, (h, w), dtype=np.uint8)
        S[(ys + sy)[inside], (xs + sx)[inside]] = E[inside]  # S[y + sy][x + sx] = E[y][x]
        _, u = R.pixels(E, S, np.full((h, w), sx, np.float32), np.full((h, w), sy, np.float32))
        assert not u[inside].any()


# ---- with the oracle's flow ---------------------------------------------------------------------------------------------------
W, H = 397, 99


def scenes():
    """The four pairs of the feature's case, on synth's screenshot texture: name -> (expect, target)."""
    import synth
    E = synth.make_expect(np.random.default_rng(synth.BASE_SEED), H, W)
    flat_e = E.copy()
    flat_e[30:70, 150:250] = 120
    flat_t = flat_e.copy()
    flat_t[30:70, 150:250] = 150  # a 100 x 40 repaint by 30 gray levels
    moved = E.copy()
    moved[23:73, 107:267] = E[20:70, 100:260]  # a 160 x 50 block moved by (7, 3)
    shift = E.copy()
    shift[:, 3:] = E[:, :-3]
    return {"flat": (flat_e, flat_t), "moved": (E, moved), "shift": (E, shift), "identical": (E, E.copy())}


@pytest.fixture(scope="module")
def facts():
    import oracle as O
    out = {}
    for name, (e, t) in scenes().items():
        fx, fy = O.farneback(e, t)
        c, rec = R.residual_ref(e, t, (fx, fy), SPAN, TOL)
        out[name] = (O.span_scan(fx, fy, SPAN, THRESHOLD), c, rec)
    return out


def test_a_flat_change_has_no_vector_and_every_cell_unexplained(facts):
    vec, c, rec = facts["flat"]
    print("flat change: %d vectors, %d cells, %d with unexplained pixels; %d differing, %d unexplained pixels"
          % (len(vec), len(rec), sum(r[3] >= 1 for r in rec), c[..., 0].sum(), c[..., 1].sum()))
    assert len(vec) == 0
    assert len(rec) == 40 and all(r[3] >= 1 for r in rec)
    assert c[..., 0].sum() == 4000 and 2 * c[..., 1].sum() > c[..., 0].sum()


def test_a_moved_block_is_mostly_explained(facts):
    vec, c, rec = facts["moved"]
    print("moved block: %d vectors, %d cells, %d explained; %d differing, %d unexplained pixels"
          % (len(vec), len(rec), sum(r[3] == 0 for r in rec), c[..., 0].sum(), c[..., 1].sum()))
    assert len(vec) > 0
    assert sum(r[3] == 0 for r in rec) >= 40


def test_a_global_shift_is_explained(facts):
    vec, c, rec = facts["shift"]
    print("3-pixel shift: %d differing, %d unexplained pixels" % (c[..., 0].sum(), c[..., 1].sum()))
    assert c[..., 0].sum() > 1000 and 10 * c[..., 1].sum() < c[..., 0].sum()


def test_an_identical_pair_has_nothing(facts):
    vec, c, rec = facts["identical"]
    assert len(vec) == 0 and rec == [] and not c.any()
