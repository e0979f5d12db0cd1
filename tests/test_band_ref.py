"""tests/band_ref.py, the reference of the shift-band tests: what the bands promise on text-like pages with an inserted block
(every band wholly above the insertion, and every band below it whose content is still inside the image, comes back exactly),
pure shifts, local changes and identical pairs, the unit cases of the band search (the overlap rule at its edge, a last band of
one row, an image shorter than a band, odd widths, tie order, products past 2^32), and — with the oracle's flow — what the
feature is for: a page with an inserted block has a garbage flow below the insertion from a zero start and the right one from
the bands.  CPU only."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tidal-wave_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import band_ref as BR
import shift_ref as S

H, W, R = 240, 320, 100
SEEDS = (20, 21, 22, 23, 24, 25)
INSERTS = [(100, 40), (64, 32), (50, 70), (130, 24), (96, 48)]
MOVES = (0, 25, -30)
HEIGHTS = (32, 48, 64)


@functools.lru_cache(maxsize=None)
def inserted(seed, at, ins, sx):
    """The inserted-block pair of one case, from a generator of its own."""
    return BR.inserted_pair(np.random.default_rng(seed), H, W, at, ins, sx)


def expected_bands(h, B, at, ins, sx):
    """{band index: (dy, applied)} for the bands the definition promises: wholly above the insertion, or below it with their
    content still inside the image.  The others straddle the insertion or their content has left: compared with nothing."""
    out = {}
    for b, (y, rows) in enumerate(BR.band_rows(h, B)):
        if y + rows <= at:
            out[b] = (0, 1 if sx else 0)
        elif y >= at and y + rows + ins <= h:
            out[b] = (ins, 1)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_inserted_blocks_come_back_per_band(seed):
    checked = 0
    for at, ins in INSERTS:
        for sx in MOVES:
            E, T = inserted(seed, at, ins, sx)
            for B in HEIGHTS:
                g, bands = BR.estimate(E, T, R, B)
                assert g.dx == sx, ((at, ins, sx, B), g)
                assert [(b.y, b.rows) for b in bands] == BR.band_rows(H, B)
                for i, want in expected_bands(H, B, at, ins, sx).items():
                    assert (bands[i].dy, bands[i].applied) == want, ((at, ins, sx, B), i, bands[i])
                    checked += 1
    print("seed %d: %d bands checked" % (seed, checked))
    assert checked == 153  # (918 over the six seeds)


@pytest.mark.parametrize("seed", SEEDS[:3])
@pytest.mark.parametrize("B", HEIGHTS)
def test_pure_shifts_come_back_in_every_band_whose_content_stays(seed, B):
    E, T = S.shifted_pair(np.random.default_rng(seed), H, W, 25, 60)
    g, bands = BR.estimate(E, T, R, B)
    assert (g.dx, g.dy, g.applied) == (25, 60, 1)
    n = 0
    for b in bands:
        if b.y + b.rows + 60 <= H:
            assert (b.dy, b.applied, b.sad_shift) == (60, 1, 0) and b.n_shift == b.rows * (W - 25), b
            n += 1
    assert n >= 2


@pytest.mark.parametrize("B", HEIGHTS)
def test_identical_and_locally_repainted_pairs_are_not_applied(B):
    E = inserted(SEEDS[0], 100, 40, 0)[0]
    g, bands = BR.estimate(E, E, R, B)
    assert g == S.Shift(0, 0, 0, W * H, W * H, 0, 0)
    assert bands == [BR.Band(y, rows, 0, 0, rows * W, rows * W, 0, 0) for y, rows in BR.band_rows(H, B)]
    L = E.copy()
    L[100:140, 60:200] = 30
    g, bands = BR.estimate(E, L, R, B)
    assert not any(b.applied for b in bands), bands
    assert sum(b.sad_zero for b in bands) == g.sad_zero > 0


def _noise_rows(seed, h, nblk=3):
    return np.random.default_rng(seed).integers(0, 16321, (h, nblk)).astype(np.uint16)


def test_the_overlap_rule_at_its_edge():
    """h = 128, B = 64, R = 64: band 1 (rows 64 .. 127) needs 32 rows.  d = +32 leaves exactly 32 and is eligible; d = +33 leaves
    31 and is not, even at cost 0."""
    h, B = 128, 64
    sE = _noise_rows(1, h)
    sT = _noise_rows(2, h)
    sT[96:128] = sE[64:96]  # a perfect match at d = +32 over rows 64 .. 95
    assert BR.overlap(64, 64, h, 32) == (64, 96) and BR.band_cost(sE, sT, 64, 64, 32) == 0
    assert BR.search_band(sE, sT, 64, 64, 64) == 32
    sT = _noise_rows(2, h)
    sT[97:128] = sE[64:95]  # ... and one at d = +33 over rows 64 .. 94: 31 rows, one too few
    assert BR.overlap(64, 64, h, 33) == (64, 95) and BR.band_cost(sE, sT, 64, 64, 33) == 0
    d = BR.search_band(sE, sT, 64, 64, 64)
    assert d != 33 and BR.band_cost(sE, sT, 64, 64, d) > 0


def test_a_last_band_of_one_row_and_an_image_shorter_than_a_band():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (65 + 40, 70)).astype(np.uint8)
    E, T = base[20:85], base[30:95]  # E[y] = T[y - 10]
    g, bands = BR.estimate(E, T, 16, 64)
    assert [(b.y, b.rows) for b in bands] == [(0, 64), (64, 1)]
    assert (bands[1].dy, bands[1].applied, bands[1].n_zero, bands[1].n_shift, bands[1].sad_shift) == (-10, 1, 70, 70, 0)
    assert (bands[0].dy, bands[0].applied, bands[0].n_shift) == (-10, 1, 54 * 70)
    E, T = base[20:40], base[17:37]  # h = 20 < B: one band of 20 rows; E[y] = T[y + 3]
    g, bands = BR.estimate(E, T, 16, 32)
    assert len(bands) == 1 and (bands[0].y, bands[0].rows, bands[0].dy, bands[0].applied) == (0, 20, 3, 1)
    assert bands[0].n_zero == 20 * 70 and bands[0].n_shift == 17 * 70


@pytest.mark.parametrize("w,dx", [(1, 0), (63, 0), (63, -1), (64, 0), (64, 1), (65, 0), (65, 1), (65, -1), (129, 0), (129, 1),
                                  (129, -1)])
def test_signatures_at_odd_widths(w, dx):
    rng = np.random.default_rng(w)
    E = rng.integers(0, 256, (5, w)).astype(np.uint8)
    T = rng.integers(0, 256, (5, w)).astype(np.uint8)
    xa, xb, nblk = BR.columns(w, dx)
    assert nblk == -(-(w - abs(dx)) // 64)
    sE, sT = BR.signatures(E, T, dx)
    assert sE.shape == sT.shape == (5, nblk)
    for y in range(5):
        for k in range(nblk):
            xs = range(xa + 64 * k, min(xa + 64 * (k + 1), xb))
            assert sE[y, k] == sum(int(E[y, x]) for x in xs) and sT[y, k] == sum(int(T[y, x + dx]) for x in xs)
    assert int(sE.max()) <= 16320


def test_a_tie_between_minus_d_and_plus_d_goes_to_the_negative_one():
    sE = np.array([[5], [0], [0], [0]] * 4, np.uint16)  # a comb of period 4 down the rows ...
    sT = np.array([[0], [0], [5], [0]] * 4, np.uint16)  # ... and the same comb two further
    assert BR.band_cost(sE, sT, 0, 16, 2) == 0 and BR.band_cost(sE, sT, 0, 16, -2) == 0
    assert min(BR.band_cost(sE, sT, 0, 16, d) for d in (0, -1, 1)) > 0
    assert BR.search_band(sE, sT, 0, 16, 3) == -2


def products_pair():
    """The shift tests' 4096 x 128 black and white halves with the edge horizontal: one band of 128 rows and 64 blocks."""
    w, h = 4096, 128
    E = np.zeros((h, w), np.uint8)
    E[h // 2:] = 255
    T = np.zeros((h, w), np.uint8)
    T[h // 2 + 40:] = 255  # the edge moved down by 40
    return E, T


def test_the_comparison_needs_64_bits_at_4096_by_128():
    E, T = products_pair()
    h, w = E.shape
    sE, sT = BR.signatures(E, T, 0)
    c0, c40 = BR.band_cost(sE, sT, 0, h, 0), BR.band_cost(sE, sT, 0, h, 40)
    assert c0 == 40 * 255 * w and c40 == 0 and c0 * (h - 1) > 1 << 32
    prods = []
    for d in S.visit_order(64)[1:]:
        lo, hi = BR.overlap(0, h, h, d)
        prods.append((BR.band_cost(sE, sT, 0, h, d) * h, c0 * (hi - lo)))
    assert max(max(p) for p in prods) > 1 << 32
    assert any((a < b) != ((a & 0xffffffff) < (b & 0xffffffff)) for a, b in prods)
    g, bands = BR.estimate(E, T, 1024, 128)
    assert (g.dx, g.dy) == (0, 40) and len(bands) == 1
    assert (bands[0].dy, bands[0].applied, bands[0].sad_shift, bands[0].sad_zero) == (40, 1, 0, 40 * 255 * w)


@pytest.mark.parametrize("seed", [1, 2])
def test_the_band_field_repairs_the_flow_below_an_inserted_block(oracle, seed):
    """The test that says the feature is worth having: with 40 foreign rows inserted at row 100, the oracle's flow from a zero
    start is off by more than 10 px in the median over the rows the bands promise (measured 23.8 / 13.2 px when the definition
    was prototyped), from the band field by thousandths (0.0019 / 0.0012 px)."""
    from test_flow_init_abi import farneback_with_init
    at, ins, B = 100, 40, 32
    E, T = BR.inserted_pair(np.random.default_rng(seed), H, W, at, ins)
    g, bands = BR.estimate(E, T, R, B)
    for i, want in expected_bands(H, B, at, ins, 0).items():
        assert (bands[i].dy, bands[i].applied) == want, bands[i]
    F = BR.field((H, W), g.dx, bands)
    zx, zy = oracle.farneback(E, T)
    gx, gy = farneback_with_init(oracle, E, T, F)
    truth = np.where(np.arange(H) >= at, float(ins), 0.0)[:, None]
    rows = np.ones(H, bool)
    rows[:20] = False
    rows[H - (ins + 20):] = False
    rows[at - 20:at + 20] = False

    def median_error(ax, ay):
        return float(np.median(np.hypot(ax, ay - truth)[rows][:, 40:-40]))
    e0, e1 = median_error(zx, zy), median_error(gx, gy)
    print("seed %d: zero start %.3f px, band field %.4f px" % (seed, e0, e1))
    assert e0 >= 10.0 and e1 <= 0.5, (e0, e1)
