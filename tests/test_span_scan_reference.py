"""The span scan's numpy reference (tests/span_scan_cases.py) against the oracle's loop (orc_span_scan), and every
precondition the cases of tests/test_gpu_span_scan.py rest on — no GPU.  A case that stopped meaning what it is there for
(a threshold that no longer separates a double compare from a float compare, a field without ties where a count is
wanted) fails here, not silently there."""
import numpy as np
import pytest

import span_scan_cases as S

F32, F64 = np.float32, np.float64


def test_reference_equals_the_oracle_on_every_value_case(oracle):
    fields = S.value_fields()
    assert len({t for t, _, _ in fields}) == len(fields) >= 14
    seen = 0
    for thr, where, f in fields:
        ref = S.ref_scan(f[0], f[1], 1, thr)
        assert S.same_scan(ref, S.oracle_scan(oracle, f[0], f[1], 1, thr)), thr
        # the case's own expectation, point by point: the reference hits exactly the cases marked as hits
        hit_at = {int(y) * S.VALUE_W + int(x) for x, y in ref[1]}
        assert len({i for _, i in where}) == len(where)
        for c, i in where:
            assert (i in hit_at) == c.hit, c
            seen += 1
        assert hit_at <= {i for _, i in where}  # (0, 0) is no hit under any threshold
        assert any(i < 1024 for _, i in where) or len(where) < 2
    assert seen == len(S.value_cases())


def test_value_cases_mean_what_they_are_there_for():
    cases = {c.name: c for c in S.value_cases()}
    assert len(cases) == len(S.value_cases())
    L = lambda n: S.ref_len(cases[n].dx, cases[n].dy)  # noqa: E731
    # (3, 4): len is exactly 25 = 5 * 5, no hit under the strict compare; one ulp more in dx is one ulp more in len
    assert L("3_4_at_5") == 25 and L("3up_4_at_5") == np.nextafter(F32(25), F32(np.inf))
    # compare in double: t * t < len in double, and t * t rounds to len in float
    dc = [c for c in S.value_cases() if c.name.startswith("double_compare")]
    assert len(dc) == 6
    for c in dc:
        ln, t2 = S.ref_len(c.dx, c.dy), S.thr2(c.threshold)
        assert t2 < F64(ln) and F32(t2) == ln and not (ln > F32(t2)), c
    # no contraction: the contracted len differs, the threshold's square is strictly between the two in double
    fm = [c for c in S.value_cases() if c.name.startswith("fma_")]
    assert sorted(c.name for c in fm) == ["fma_x_ref_larger", "fma_x_ref_smaller", "fma_y_ref_larger", "fma_y_ref_smaller"]
    for c in fm:
        r = S.ref_len(c.dx, c.dy)
        k = (S.len_fma_x if "_x_" in c.name else S.len_fma_y)(c.dx, c.dy)
        t2 = S.thr2(c.threshold)
        assert r != k and min(F64(r), F64(k)) < t2 < max(F64(r), F64(k)), c
        assert (F64(r) > t2) == c.hit == (not F64(k) > t2) and c.hit == c.name.endswith("larger"), c
    # fmaf(dx, dx, dy * dy) as restated in double is the correctly rounded fused value: exact sum, rounded once
    import fractions
    for c in fm:
        dx, dy = F32(c.dx), F32(c.dy)
        exact = fractions.Fraction(float(dx)) ** 2 + fractions.Fraction(float(F32(dy * dy)))
        got = fractions.Fraction(float(S.len_fma_x(dx, dy)))
        lo, hi = (fractions.Fraction(float(np.nextafter(S.len_fma_x(dx, dy), F32(s) * F32(np.inf)))) for s in (-1, 1))
        assert abs(exact - got) <= min(got - lo, hi - got) / 2, c
    # denormals: 1e-20f squared is a denormal float above 0, 1e-23f squared underflows to 0
    tiny = np.finfo(F32).tiny
    assert 0 < L("denormal_len") < tiny and 0 < L("denormal_len_y") < tiny and L("underflow_len") == 0
    assert F32(cases["underflow_len"].dx) != 0
    # signed zeros: len 0; the recorded -0.0 has its sign bit
    assert L("minus_zero") == 0 and L("zero_minus_zero") == 0 and L("zero_minus_zero_neg_thr") == 0
    assert np.signbit(F32(cases["minus_zero_recorded"].dy)) and np.signbit(F32(cases["minus_zero_recorded_x"].dx))
    assert cases["minus_zero_recorded"].threshold < 0 and S.thr2(cases["minus_zero_recorded"].threshold) == 1
    # overflow: 2e19f is finite, its square is not; 1e20 * 1e20 is a finite double beyond every float; 1e200 * 1e200 is inf
    assert np.isfinite(F32(2e19)) and L("overflow_len") == np.inf and L("overflow_len_at_5") == np.inf
    with np.errstate(over="ignore"):
        assert np.isfinite(S.thr2(1e20)) and S.thr2(1e20) > F64(np.finfo(F32).max) and F32(S.thr2(1e20)) == np.inf
    assert np.isfinite(L("big_at_1e20")) and S.thr2(1e200) == np.inf
    for n, c in cases.items():
        if n.startswith("nan_"):
            assert np.isnan(S.ref_len(c.dx, c.dy)) and not c.hit, n
        if n.startswith(("inf_", "minus_inf_")) and "1e200" not in n:
            assert S.ref_len(c.dx, c.dy) == np.inf and c.hit, n
    assert {c.threshold for c in cases.values() if c.name.startswith("nan_d")} == {0.0, 5.0}
    assert S.thr2(-5.0) == S.thr2(5.0) == 25


def test_grids_are_the_sizes_asked_for():
    G = [gw * gh for gw, gh in (S.grid_dims(*g) for g in S.GRIDS)]
    assert G[:12] == [5, 1024, 1025, 2048, 2049, 16384, 16385, 32768, 32769, 32768 + 3 * 1024 + 5, 524288, 524290]
    # 524 289 has no image: its only factorisations put more than 32 768 points on a side
    assert 524289 == 3 * 174763 and all(174763 % p for p in range(2, 419)) and 174763 > 32768
    assert max(w * h for w, h, _ in S.GRIDS) <= 1090 * 481 and all(w <= 32768 and h <= 32768 for w, h, _ in S.GRIDS)
    odd = [(w, h, s) for w, h, s in S.GRIDS if S.grid_dims(w, h, s)[0] == 157]
    assert len(odd) >= 3 and {s for _, _, s in odd} >= {1, 7, 10} and 157 % 32
    assert any((w - 1) % s == 0 for w, _, s in odd if s > 1) and any((w - 1) % s != 0 for w, _, s in odd if s > 1)
    assert any(w % 32 for w, _, s in S.GRIDS if s == 1)


def small_plan(G):
    """choose_scan's segments, restated for this CPU test only (the GPU test takes them from Engine.scan_plan)."""
    seg = -(-(-(-G // 16)) // 1024) * 1024
    return (seg, -(-G // seg)) if G > 2048 and seg <= 32768 else (0, 0)


@pytest.mark.parametrize("grid", [g for g in S.GRIDS if S.grid_dims(*g)[0] * S.grid_dims(*g)[1] <= 20000], ids=str)
def test_reference_equals_the_oracle_on_every_pattern(oracle, grid):
    w, h, span = grid
    gw, gh = S.grid_dims(*grid)
    G = gw * gh
    names = set()
    for name, hits in S.patterns(G, *small_plan(G)):
        f = S.pattern_field(w, h, span, hits)
        ref = S.ref_scan(f[0], f[1], span, S.PATTERN_THRESHOLD)
        assert ref[0] == int(hits.sum()), name
        assert S.same_scan(ref, S.oracle_scan(oracle, f[0], f[1], span, S.PATTERN_THRESHOLD)), name
        # every hit value is distinct and names its own grid point
        assert np.array_equal(ref[2][:, 0], np.flatnonzero(hits).astype(F32) + F32(0.5)), name
        names.add(name)
    assert {"none", "all", "every_second", "first_segment", "last_segment", "single_0", "single_%d" % (G - 1)} <= names
    if span > 1:
        # the pixels off the grid would be hits: a sampling mistake cannot hide
        f = S.pattern_field(w, h, span, np.zeros(G, bool))
        assert S.ref_scan(f[0], f[1], 1, S.PATTERN_THRESHOLD)[0] == w * h - G


def test_patterns_hold_distinct_exact_values_on_the_largest_grid():
    w, h, span = max(S.GRIDS, key=lambda g: S.grid_dims(*g)[0] * S.grid_dims(*g)[1])
    G = w * h
    assert span == 1 and G == 524290 < 2 ** 22
    f = S.pattern_field(w, h, span, np.ones(G, bool))
    assert np.array_equal(f[0].ravel().astype(F64), np.arange(G) + 0.5) and np.array_equal(f[1].ravel().astype(F64), -(np.arange(G) + 0.25))
    n, xy, dxy = S.ref_scan(f[0], f[1], 1, S.PATTERN_THRESHOLD)
    assert n == G and np.array_equal(xy[:, 1].astype(np.int64) * w + xy[:, 0], np.arange(G))
    idx = S.seam_indices(G, 0, 0)
    assert idx == [0, 63, 64, 1023, 1024, 8191, 8192, 32767, 32768, G - 1]
    assert S.seam_indices(2049, 1024, 3) == [0, 63, 64, 1023, 1024, 2047, 2048]
    assert {S.seam_indices(16385, 2048, 9)[i] for i in (5, 6)} == {2047, 2048} and 8 * 2048 in S.seam_indices(16385, 2048, 9)


def test_readback_thresholds_give_the_counts_asked_for(oracle):
    """The oracle's own count at each threshold of the read-back tests: 0, 1, 1 023, 1 024, 1 025, every point, and the
    tw_wait count of 1 500 or so — from the oracle's field, never from the engine."""
    (a, b), (a2, b2) = S.readback_pairs()
    assert a.shape == (120, 160) and not np.array_equal(a, a2)
    for p, q in ((a, b), (a2, b2)):
        wx, wy = oracle.farneback(p, q)
        lens = S.ref_len(wx, wy)
        for k in S.READBACK_COUNTS:
            t = S.threshold_for_count(lens, k)
            assert t is not None, k
            s = np.sort(lens.ravel())[::-1].astype(F64)
            assert (k == 0 or S.thr2(t) < s[k - 1]) and S.thr2(t) > s[min(k, s.size - 1)] * (k < s.size), k
            assert len(oracle.span_scan(wx, wy, 1, t)) == k == S.ref_scan(wx, wy, 1, t)[0]
        top = len(oracle.span_scan(wx, wy, 1, 0.0))
        assert top == int((lens > 0).sum()) > 1025 and top == S.ref_scan(wx, wy, 1, 0.0)[0]
        k, t = S.wait_threshold(lens)
        assert 1500 <= k < 1564 and len(oracle.span_scan(wx, wy, 1, t)) == k
        assert S.same_scan(S.ref_scan(wx, wy, 1, t), S.oracle_scan(oracle, wx, wy, 1, t))
