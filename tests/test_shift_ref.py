"""tests/shift_ref.py, the reference of the shift tests: what the estimation promises on text-like pages (pure shifts come back
exactly and are applied, a fixed header does not stop that, unrelated pages and local changes are rejected), the unit cases of
the search (tie order, radius clamping, a best shift at the radius, products past 2^32), and — with the oracle's flow — what
the feature is for: a page moved by more than Farneback's reach has a garbage flow from a zero start and the right one from the
estimated shift.  CPU only."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tidal-wave_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import shift_ref as S

H, W, R = 240, 320, 100
SHIFTS = [(0, 3), (0, 40), (25, 60), (-30, 7), (60, 60)]
SEEDS = (20, 21, 22)


@functools.lru_cache(maxsize=None)
def pages(seed):
    """Per shift of SHIFTS: (E, T, Q) — a shifted pair and an unrelated page, all from one generator per seed."""
    rng = np.random.default_rng(seed)
    out = []
    for sx, sy in SHIFTS:
        E, T = S.shifted_pair(rng, H, W, sx, sy)
        Q = S.page(rng, H + 200, W + 200)[100:100 + H, 100:100 + W].copy()
        out.append((E, T, Q))
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_pure_shifts_come_back_exactly_and_are_applied(seed):
    for (sx, sy), (E, T, _) in zip(SHIFTS, pages(seed)):
        s = S.estimate(E, T, R)
        assert (s.dx, s.dy, s.applied) == (sx, sy, 1), ((sx, sy), s)
        assert s.n_zero == W * H and s.n_shift == (W - abs(sx)) * (H - abs(sy)) and s.sad_shift == 0 and s.sad_zero > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_a_fixed_header_of_50_rows_does_not_stop_the_shift(seed):
    for (sx, sy), (E, T, _) in zip(SHIFTS, pages(seed)):
        T2 = T.copy()
        T2[:50] = E[:50]
        s = S.estimate(E, T2, R)
        assert s.applied == 1, ((sx, sy), s)


@pytest.mark.parametrize("seed", SEEDS)
def test_unrelated_pages_are_rejected(seed):
    for (E, _, Q) in pages(seed):
        s = S.estimate(E, Q, R)
        assert s.applied == 0, s


def test_identical_and_locally_repainted_pairs_are_not_applied():
    E = pages(SEEDS[0])[0][0]
    s = S.estimate(E, E, R)
    assert s == S.Shift(0, 0, 0, W * H, W * H, 0, 0)
    L = E.copy()
    L[100:140, 60:200] = 30  # one repainted 140 x 40 block
    s = S.estimate(E, L, R)
    assert s.applied == 0 and s.sad_zero > 0, s


def test_ties_go_to_zero_on_constant_images():
    E = np.full((9, 12), 77, np.uint8)
    s = S.estimate(E, E, 8)
    assert (s.dx, s.dy, s.applied) == (0, 0, 0)
    # every cost is 0 on profiles that differ by a constant factor of nothing: d = 0 stays, being visited first
    p = np.full(12, 700, np.uint32)
    assert S.search(p, p, 6) == 0
    # equal cost per element at -2 and +2 and nowhere better: the negative one, visited first
    pE = np.array([5, 0, 0, 0] * 4, np.uint32)  # a comb of period 4 ...
    pT = np.array([0, 0, 5, 0] * 4, np.uint32)  # ... and the same comb two further
    assert S.cost(pE, pT, 2) == 0 and S.cost(pE, pT, -2) == 0 and min(S.cost(pE, pT, d) for d in (0, -1, 1)) > 0
    assert S.search(pE, pT, 3) == -2


@pytest.mark.parametrize("L,r", [(1, 0), (2, 1), (3, 1), (7, 3)])
def test_radius_is_clamped_to_half_the_axis(L, r):
    assert S.visit_order(min(8, L // 2)) == S.visit_order(r) and len(S.visit_order(r)) == 2 * r + 1
    # a profile whose only match lies beyond r: the answer stays within [-r, r]
    rng = np.random.default_rng(L)
    pE = rng.integers(0, 1000, L).astype(np.uint32)
    pT = rng.integers(0, 1000, L).astype(np.uint32)
    assert abs(S.search(pE, pT, 8)) <= r
    assert S.visit_order(3) == [0, -1, 1, -2, 2, -3, 3]


@pytest.mark.parametrize("d", [-5, 5, -8, 8])
def test_a_best_shift_at_exactly_the_radius_and_one_beyond_it(d):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 50000, 64 + 32).astype(np.uint32)
    pE = base[16:16 + 64]
    pT = base[16 - d:16 - d + 64]  # pE[i] = pT[i + d]
    assert S.cost(pE, pT, d) == 0
    assert S.search(pE, pT, abs(d)) == d
    # one beyond the radius: the best within reach, whatever it is, by brute force over the definition
    r = abs(d) - 1
    best = min(S.visit_order(r), key=lambda c: (S.cost(pE, pT, c) / (64 - abs(c)), S.visit_order(r).index(c)))
    assert S.search(pE, pT, r) == best and abs(best) <= r


def test_the_comparison_needs_64_bits_at_4096_by_128():
    """Black against white halves: cost * n passes 2^32 (profiles of 255 * 128 per column, 4096 columns), and a comparison in 32
    bits would choose differently."""
    w, h = 4096, 128
    E = np.zeros((h, w), np.uint8)
    E[:, w // 2:] = 255
    T = np.zeros((h, w), np.uint8)
    T[:, w // 2 + 300:] = 255  # the edge moved right by 300
    colE, colT, _, _ = S.profiles(E, T)
    c0, c300 = S.cost(colE, colT, 0), S.cost(colE, colT, 300)
    assert c0 == 300 * 255 * 128 and c300 == 0 and c0 * (w - 1) > 1 << 32
    # the products the search compares on the way wrap in 32 bits, and wrapped they order differently somewhere
    prods = [(S.cost(colE, colT, d) * w, c0 * (w - abs(d))) for d in S.visit_order(400)[1:]]
    assert max(max(p) for p in prods) > 1 << 32
    assert any((a < b) != ((a & 0xffffffff) < (b & 0xffffffff)) for a, b in prods)
    s = S.estimate(E, T, 1024)
    assert (s.dx, s.dy, s.applied) == (300, 0, 1) and s.sad_shift == 0 and s.sad_zero == 300 * 255 * 128


@pytest.mark.parametrize("shift", [(0, 40), (25, 60)])
def test_the_estimated_start_repairs_the_flow_of_a_far_moved_page(oracle, shift):
    """The test that says the feature is worth having: from a zero start the oracle's flow of a page moved by (0, 40) or
    (25, 60) is off by tens of pixels in the median (measured 47 - 66 px), from the estimated shift by hundredths (0.006 - 0.009)."""
    from test_flow_init_abi import farneback_with_init
    sx, sy = shift
    E, T, _ = pages(SEEDS[0])[SHIFTS.index(shift)]
    s = S.estimate(E, T, R)
    assert (s.dx, s.dy, s.applied) == (sx, sy, 1)
    zx, zy = oracle.farneback(E, T)
    f0 = np.empty((H, W, 2), np.float32)
    f0[..., 0] = s.dx
    f0[..., 1] = s.dy
    gx, gy = farneback_with_init(oracle, E, T, f0)

    def median_error(ax, ay):
        return float(np.median(np.hypot(ax - sx, ay - sy)[40:-40, 40:-40]))
    e0, e1 = median_error(zx, zy), median_error(gx, gy)
    print("shift %s: zero start %.3f px, seeded %.4f px" % (shift, e0, e1))
    assert e0 >= 10.0 and e1 <= 0.5, (e0, e1)
