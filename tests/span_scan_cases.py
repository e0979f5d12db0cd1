"""The span scan on chosen fields: the plain numpy reference, the value cases, the grids and the hit patterns that
tests/test_span_scan_reference.py (CPU: the reference against the oracle, the cases' preconditions) and
tests/test_gpu_span_scan.py (the kernels against the reference, bit for bit) share.  No test lives here.

The operation (oracle/farneback_oracle.c, orc_span_scan; src/consumer.cpp:60-76 of the reference): at every pixel with
x % span == 0 and y % span == 0, row-major, len = (dx * dx) + (dy * dy) in float — two products and one sum, each rounded —
and the point is a hit where (double)len > threshold * threshold (strict; NaN compares false)."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
INF, NAN = F32(np.inf), F32(np.nan)
FILL = np.uint32(0xFFFFFFFF)  # what tw_stage_span_scan leaves in a record the kernels did not write


def f32(v):
    return np.asarray(v, F32)


def ref_len(dx, dy):
    """float32(float32(dx * dx) + float32(dy * dy)): numpy rounds every float32 operation."""
    dx, dy = f32(dx), f32(dy)
    with np.errstate(all="ignore"):
        return (dx * dx) + (dy * dy)


def thr2(threshold):
    with np.errstate(all="ignore"):
        return F64(threshold) * F64(threshold)


def ref_scan(fx, fy, span, threshold):
    """(count, xy [count, 2] int32, dxy [count, 2] float32) of one field, vectorised."""
    gx, gy = f32(fx)[::span, ::span], f32(fy)[::span, ::span]
    hit = ref_len(gx, gy).astype(F64) > thr2(threshold)
    idx = np.flatnonzero(hit.ravel())  # row-major
    gw = gx.shape[1]
    xy = np.stack([idx % gw * span, idx // gw * span], 1).astype(np.int32)
    dxy = np.stack([gx.ravel()[idx], gy.ravel()[idx]], 1).astype(F32)
    return int(idx.size), xy, dxy


def oracle_scan(oracle, fx, fy, span, threshold):
    """oracle.span_scan in ref_scan's form (its doubles are widened floats: narrowing them back is exact)."""
    v = oracle.span_scan(fx, fy, span, threshold)
    xy = np.array([(r[0], r[1]) for r in v], np.int32).reshape(-1, 2)
    dxy = np.array([(r[2], r[3]) for r in v], F64).reshape(-1, 2)
    assert np.array_equal(dxy.astype(F32).astype(F64), dxy, equal_nan=True)
    return len(v), xy, dxy.astype(F32)


def same_scan(a, b):
    """Counts, positions and the float BITS of two scans."""
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


# ---- value cases --------------------------------------------------------------------------------------------------
# name, dx, dy, threshold, whether the point is a hit
Case = collections.namedtuple("Case", "name dx dy threshold hit")


def double_compare_threshold(dx, dy):
    """A threshold whose square is below len as a double and rounds to len as a float: a hit compared in double, no hit
    compared in float."""
    return float(np.sqrt(F64(ref_len(dx, dy)) * (1.0 - 2.0 ** -26)))


def len_fma_x(dx, dy):
    """fmaf(dx, dx, dy * dy) as the issue writes it: the product dx * dx exact (48 bits fit a double), dy * dy rounded."""
    dx, dy = F32(dx), F32(dy)
    return F32(F64(dx) * F64(dx) + F64(F32(dy * dy)))


def len_fma_y(dx, dy):
    """fmaf(dy, dy, dx * dx): the other contraction a compiler may choose."""
    dx, dy = F32(dx), F32(dy)
    return F32(F64(F32(dx * dx)) + F64(dy) * F64(dy))


def between(a, b):
    """A threshold whose square lies strictly between the floats a and b (test_span_scan_reference asserts it does)."""
    return float(np.sqrt((F64(a) + F64(b)) / 2))


def contraction_cases():
    """Four (dx, dy) from a seeded generator where a contracted len differs from the reference, the threshold's square between
    the two: for each of the two contractions one case with the reference value the larger (a hit only uncontracted) and one
    with it the smaller (a hit only contracted)."""
    rng = np.random.default_rng(20240607)
    out, want = [], [("x", True), ("x", False), ("y", True), ("y", False)]
    while want:
        dx, dy = (F32(v) for v in rng.uniform(-8, 8, 2))
        r = ref_len(dx, dy)
        for which, larger in list(want):
            c = (len_fma_x if which == "x" else len_fma_y)(dx, dy)
            if c != r and (r > c) == larger:
                want.remove((which, larger))
                out.append(Case("fma_%s_ref_%s" % (which, "larger" if larger else "smaller"), dx, dy, between(r, c), bool(larger)))
                break
    return out


def double_compare_cases():
    rng = np.random.default_rng(77)
    out = []
    for i in range(6):
        dx, dy = (F32(v) for v in rng.uniform(-40, 40, 2))
        out.append(Case("double_compare_%d" % i, dx, dy, double_compare_threshold(dx, dy), True))
    return out


def value_cases():
    up3 = np.nextafter(F32(3), INF)
    c = [
        Case("3_4_at_5", 3, 4, 5.0, False), Case("3up_4_at_5", up3, 4, 5.0, True),
        Case("3_4_at_minus5", 3, 4, -5.0, False), Case("3up_4_at_minus5", up3, 4, -5.0, True),
        Case("zero", 0, 0, 0.0, False), Case("minus_zero", -0.0, 0, 0.0, False), Case("zero_minus_zero", 0, -0.0, 0.0, False),
        Case("denormal_len", 1e-20, 0, 0.0, True), Case("denormal_len_y", 0, -1e-20, 0.0, True),
        Case("underflow_len", 1e-23, 0, 0.0, False),
        # (0, -0.0) has len 0 and is a hit under no threshold at all — threshold * threshold is never negative; the sign bit
        # of a RECORDED -0.0 is what a negative threshold can show, next to the point itself, which stays no hit
        Case("zero_minus_zero_neg_thr", 0, -0.0, -1.0, False), Case("minus_zero_recorded", 3.5, -0.0, -1.0, True),
        Case("minus_zero_recorded_x", -0.0, -3.5, -1.0, True),
        Case("overflow_len", 2e19, 0, 0.0, True), Case("overflow_len_at_5", 0, -2e19, 5.0, True),
        # threshold * threshold = 1e40 is a double beyond every float: len = +inf is above it in double, equal to it in float
        Case("overflow_len_at_1e20", 2e19, 0, 1e20, True), Case("inf_at_1e20", INF, 0, 1e20, True),
        Case("big_at_1e20", 1e19, 1e19, 1e20, False),
        Case("inf_at_1e200", INF, 0, 1e200, False), Case("minus_inf_at_1e200", 0, -INF, 1e200, False),
        Case("overflow_at_1e200", 2e19, 2e19, 1e200, False), Case("nan_at_1e200", NAN, 0, 1e200, False),
    ]
    for t in (0.0, 5.0):
        s = "_at_%g" % t
        c += [Case("nan_dx" + s, NAN, 1e3, t, False), Case("nan_dy" + s, 1e3, NAN, t, False), Case("nan_both" + s, NAN, NAN, t, False),
              Case("nan_inf" + s, NAN, INF, t, False),
              Case("inf_dx" + s, INF, 1, t, True), Case("minus_inf_dx" + s, -INF, 2, t, True), Case("minus_inf_dy" + s, 3, -INF, t, True),
              Case("inf_both" + s, INF, -INF, t, True)]
    return c + double_compare_cases() + contraction_cases()


VALUE_W, VALUE_H = 64, 40  # 2 560 points at span 1: the smallest kind of grid a single pair scans in segments


def value_fields():
    """[(threshold, [(case, grid index)], field [2, VALUE_H, VALUE_W])]: the cases of one threshold each at a grid point of
    its own, spread over the whole grid, every other point (0, 0) — no hit under any threshold."""
    groups = collections.OrderedDict()
    for c in value_cases():
        groups.setdefault(c.threshold, []).append(c)
    G = VALUE_W * VALUE_H
    out = []
    for thr, cs in groups.items():
        f = np.zeros((2, G), F32)
        where = []
        for k, c in enumerate(cs):
            i = (37 + k * 467) % G  # 467 is prime to G: distinct points, both sides of every 1 024
            f[0, i], f[1, i] = c.dx, c.dy
            where.append((c, i))
        out.append((thr, where, f.reshape(2, VALUE_H, VALUE_W)))
    return out


# ---- position patterns --------------------------------------------------------------------------------------------
# (w, h, span): G = ceil(w / span) * ceil(h / span)
GRIDS = [
    (5, 1, 1),          # 5
    (32, 32, 1),        # 1 024
    (41, 25, 1),        # 1 025
    (64, 32, 1),        # 2 048, the largest grid that keeps the one-workgroup kernel for a single pair
    (683, 3, 1),        # 2 049: S = 1 024, three segments, the last of one point
    (128, 128, 1),      # 16 384: sixteen full segments
    (145, 113, 1),      # 16 385: S = 2 048, nine segments
    (256, 128, 1),      # 32 768
    (331, 99, 1),       # 32 769: tw_span_scan runs a second round of one point
    (335, 107, 1),      # 32 768 + 3 * 1 024 + 5: the second round has four iterations
    (1024, 512, 1),     # 524 288, the largest segmented grid
    # the first grid beyond it that an image has: 524 289 = 3 * 174 763, a prime above the 32 768 pixels a side may have, so no
    # w x h and no span give it; 524 290 = 1 090 * 481 is back on the one-workgroup kernel with 17 rounds, the last of two points
    (1090, 481, 1),
    (1093, 98, 7),      # gw 157, gh 14: (w - 1) % span == 0, (h - 1) % span != 0
    (1570, 215, 10),    # gw 157, gh 22: (w - 1) % span != 0
    (157, 211, 1),      # gw 157 at span 1, no multiple of 32: 33 127 points, eleven segments of 3 072, two rounds as a batch
]
OFF_GRID = F32(1e6)  # at every pixel off the span grid: a hit under every pattern's threshold if a kernel sampled it
PATTERN_THRESHOLD = 0.25


def grid_dims(w, h, span):
    return -(-w // span), -(-h // span)


def pattern_field(w, h, span, hits):
    """[2, h, w]: grid point i (row-major) holds (i + 0.5, -(i + 0.25)) where hits[i], else (0, 0); distinct values, exact in
    float for every grid here (i < 2^22), so that a record in the wrong place cannot pass."""
    gw, gh = grid_dims(w, h, span)
    i = np.arange(gw * gh, dtype=np.int64).reshape(gh, gw)
    hits = np.asarray(hits, bool).reshape(gh, gw)
    f = np.full((2, h, w), OFF_GRID, F32)
    f[0, ::span, ::span] = np.where(hits, i + 0.5, 0).astype(F32)
    f[1, ::span, ::span] = np.where(hits, -(i + 0.25), 0).astype(F32)
    return f


def seam_indices(G, S, segments):
    """The single-hit positions: lanes 63 / 64, iterations 1 023 / 1 024, the unroll group 8 191 / 8 192, the round 32 767 /
    32 768, both sides of the first, a middle and the last segment boundary (S, segments: the single pair's plan; 0 without
    segments), the first and the last point."""
    idx = [0, 63, 64, 1023, 1024, 8191, 8192, 32767, 32768, G - 1]
    if segments > 1:
        for k in sorted({1, segments // 2, segments - 1}):
            idx += [k * S - 1, k * S]
    return sorted({i for i in idx if 0 <= i < G})


def patterns(G, S, segments):
    """[(name, hits [G] bool)].  Without segments (S = 0) the first / last "segment" is the first / last half of the grid."""
    i = np.arange(G)
    lo_end, hi_start = (S, (segments - 1) * S) if segments > 1 else ((G + 1) // 2, G // 2)
    out = [("none", np.zeros(G, bool)), ("all", np.ones(G, bool)), ("every_second", i % 2 == 1),
           ("first_segment", (i < lo_end) & (i % 3 == 0)), ("last_segment", (i >= hi_start) & ((G - 1 - i) % 3 == 0))]
    for k in seam_indices(G, S, segments):
        out.append(("single_%d" % k, i == k))
    return out


# ---- the read-back: one 160 x 120 pair at span 1 ---------------------------------------------------------------------
READBACK_COUNTS = (0, 1, 1023, 1024, 1025)  # and the largest attainable (threshold 0)
WAIT_COUNT = 1500  # "or so": the nearest attainable count at or above it


def readback_pairs():
    """The pair of test_scan_many_hits_and_dense_span and a second one for the batch's other slots."""
    def img(rng, h, w):
        a = rng.integers(0, 256, (h, w)).astype(np.float64)
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, 2, 1)) / 4  # some structure: the flow is not pure noise
        a[h // 3: h // 2, w // 4: w // 2] = 200
        return np.clip(a, 0, 255).astype(np.uint8)

    a, a2 = img(np.random.default_rng(4), 120, 160), img(np.random.default_rng(5), 120, 160)
    return (a, np.roll(a, 3, axis=1)), (a2, np.roll(a2, 2, axis=0))


def threshold_for_count(lens, k):
    """A threshold under which exactly k of the float lens are hits: its square strictly between the k-th and the (k + 1)-th
    largest, which must differ; None when they are equal.  k = 0: above the largest."""
    s = np.sort(np.asarray(lens, F32).ravel())[::-1].astype(F64)
    if k == 0:
        return float(np.sqrt(s[0] * 2 + 1))
    if k >= s.size or not s[k - 1] > s[k]:
        return None
    return float(np.sqrt((s[k - 1] + s[k]) / 2))


def wait_threshold(lens):
    for k in range(WAIT_COUNT, WAIT_COUNT + 64):
        t = threshold_for_count(lens, k)
        if t is not None:
            return k, t
    raise AssertionError("no attainable count near %d" % WAIT_COUNT)
