"""The CPU oracle against an INDEPENDENT float64 reference, stage by stage, every pixel (tests/farneback_f64.py).

"Exact" in this project means GPU == oracle; these tests ask whether the oracle is Farneback's algorithm as SURVEY.md
Appendix A states it, in the branches no golden vector reaches: FarnebackUpdateMatrices, the Gaussian / box window and
the solve, the flow upsample, INTER_AREA seeding, pyramid levels at any pyrScale, the level plan, the span scan.

  (a) oracle stage == reference stage within the reference's own propagated float32 error bound; no pixel is left out;
  (b) two global quadratic images f1(x) = f0(x - d) with ANALYTIC expansion coefficients: one update from zero flow
      returns d (Farneback's estimate is exact for quadratics) — independent of SURVEY.md too;
  (c) single-change mutants of the reference (wrong border mode, sigma, tap count, scale, table, factor, rounding ...)
      must each violate the bound on the inputs of (a): the comparison is sharp enough to see them;
  (d) one iteration at one level, end to end.

The only tolerance anywhere is the bound the reference returns.  Each comparison prints `f64ref <who> <stage> <case>
ratio=<max |got - ref| / bound>` (run with -s); profiles/f64_reference.md records what was observed.  CPU only.
"""
import numpy as np
import pytest
from scipy import ndimage

import farneback_f64 as F
from test_flow_init_abi import init_level_flow

F32 = np.float32


# ---- comparison -----------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """(max |got - ref| / bound over EVERY element, index of the worst element, number of elements beyond the bound).
    An element whose bound is 0 must be equal; one whose bound is infinite (a denominator that may vanish) must be finite."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)
        r = np.where(d == 0, 0.0, np.where(np.isinf(bound) & np.isfinite(got), 0.0, d / bound))
    r = np.where(np.isnan(r), np.inf, r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i), int((r > 1.0).sum())


def check(who, stage, case, got, ref, bound):
    r, at, bad = ratio(got, ref, bound)
    print("f64ref %s %s %s ratio=%.4g worst_at=%s pixels=%d" % (who, stage, case, r, at, ref.size))
    assert bad == 0, "%s %s %s: %d of %d values beyond the bound, worst %.4g x bound at %s (got %r, reference %r)" % (
        who, stage, case, bad, ref.size, r, at, float(np.asarray(got)[at]), float(ref[at]))
    return r


# ---- inputs (shared with tests/test_gpu_stages_f64.py) -------------------------------------------------------------------------
UPD_SIZES = [(33, 47), (117, 180), (270, 480), (64, 700)]  # (h, w)


def fields(rng, h, w):
    R0 = (rng.standard_normal((h, w, 5)) * 10).astype(F32)
    R1 = (R0 + rng.standard_normal((h, w, 5)).astype(F32)).astype(F32)
    return R0, R1


def flow_cases(rng, h, w):
    """sigma 2 px; sigma 40 px (the out-of-image branch is dense); a flow landing EXACTLY on integer positions, on 0,
    w-1 / h-1 among them, and one pixel either side."""
    xs = np.arange(w, dtype=F32)[None, :]
    ys = np.arange(h, dtype=F32)[:, None]
    tx = rng.integers(-2, w + 2, (h, w)).astype(F32)
    ty = rng.integers(-2, h + 2, (h, w)).astype(F32)
    tx[::3, ::2] = w - 1
    ty[1::3, ::2] = h - 1
    tx[::5, 1::4] = 0
    ty[::4, 1::5] = 0
    tx[2::7, :] = w - 2
    ty[:, 3::7] = h - 2
    exact = np.stack([tx - xs, ty - ys], -1).astype(F32)
    return [("sigma2", (rng.standard_normal((h, w, 2)) * 2).astype(F32)),
            ("sigma40", (rng.standard_normal((h, w, 2)) * 40).astype(F32)),
            ("integer", exact)]


def matrices(oracle, rng, h, w):
    """A realistic M: FarnebackUpdateMatrices of random expansions, with a zeroed quadrant (det = the 1e-3 regulariser)."""
    R0, R1 = fields(rng, h, w)
    M = oracle.update_matrices(R0, R1, (rng.standard_normal((h, w, 2))).astype(F32))
    M[h // 2:, w // 2:] = 0
    return M


WIN_CASES = [(True, 30), (True, 31), (True, 50), (True, 51), (True, 2), (True, 3), (True, 65),
             (False, 30), (False, 31), (False, 50), (False, 5)]
WIN_SIZES = [(117, 180), (12, 40), (40, 12), (64, 300)]


def textured(h, w, seed):
    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    t = (t - t.min()) / (t.max() - t.min()) * 255
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def ups_cases():
    """(ph, pw, h, w, pyrScale): the two fixtures' shapes at 0.5 and consecutive levels of 0.6 / 0.75 / 0.8 plans."""
    out = [(58, 90, 117, 180, 0.5), (35, 35, 70, 70, 0.5)]
    for s in (0.6, 0.75, 0.8):
        for (w0, h0) in ((333, 257), (480, 270)):
            plan = F.level_plan(w0, h0, s, 3)
            for k in range(len(plan) - 1):
                out.append((plan[k + 1][1], plan[k + 1][0], plan[k][1], plan[k][0], s))
    return out


# ---- (a) stage by stage ----------------------------------------------------------------------------------------------------------
def run_update_matrices(who, fn, mut=F.NONE, sizes=UPD_SIZES):
    """fn(R0, R1, flow) -> M, all interleaved.  Returns the worst ratio (asserting only without a mutant)."""
    worst = (-1.0, "")
    for h, w in sizes:
        rng = np.random.default_rng(1000 * h + w)
        R0, R1 = fields(rng, h, w)
        for name, flow in flow_cases(rng, h, w):
            got = fn(R0, R1, flow)
            ref, bound = F.update_matrices(R0, R1, flow, mut=mut)
            case = "%dx%d/%s" % (w, h, name)
            if mut:
                r, at, bad = ratio(got, ref, bound)
                worst = max(worst, (r, "%s at %s, %d values" % (case, at, bad)))
            else:
                worst = max(worst, (check(who, "update_matrices", case, got, ref, bound), case))
    return worst


def run_window_solve(who, fn, mut=F.NONE, cases=WIN_CASES, sizes=WIN_SIZES, oracle=None):
    """fn(M, win, gaussian) -> flow (h, w, 2)."""
    worst = (-1.0, "")
    for h, w in sizes:
        M = matrices(oracle, np.random.default_rng(7 * h + w), h, w)
        for gaussian, win in cases:
            got = fn(M, win, gaussian)
            ref, bound = F.window_solve(M, 0.0, win, gaussian, mut=mut)
            case = "%dx%d/%s%d" % (w, h, "gauss" if gaussian else "box", win)
            if mut:
                r, at, bad = ratio(got, ref, bound)
                worst = max(worst, (r, "%s at %s, %d values" % (case, at, bad)))
            else:
                worst = max(worst, (check(who, "window_solve", case, got, ref, bound), case))
    return worst


def run_flow_upsample(who, fn, mut=F.NONE, cases=None):
    """fn(prev (ph, pw, 2), w, h, pyrScale) -> flow (h, w, 2)."""
    worst = (-1.0, "")
    for ph, pw, h, w, s in (cases or ups_cases()):
        rng = np.random.default_rng(ph * 31 + w)
        prev = (rng.standard_normal((ph, pw, 2)) * 2).astype(F32)
        prev[0, 0, 0] = -0.0
        got = fn(prev, w, h, s)
        ref, bound = F.flow_upsample(prev, 0.0, w, h, s, mut=mut)
        case = "%dx%d->%dx%d@%g" % (pw, ph, w, h, s)
        if mut:
            r, at, bad = ratio(got, ref, bound)
            worst = max(worst, (r, "%s at %s, %d values" % (case, at, bad)))
        else:
            worst = max(worst, (check(who, "flow_upsample", case, got, ref, bound), case))
    return worst


PYR_SCALES = (0.3, 0.6, 0.75, 0.8, 0.9)


def run_pyr_level(who, fn_plan_level, mut=F.NONE, big=True):
    """fn_plan_level(img, pyrScale, levels, k) -> I of level k.  333x257 at every scale, 1080p once (pyrScale 0.6)."""
    worst = (-1.0, "")
    jobs = [(257, 333, s) for s in PYR_SCALES] + ([(1080, 1920, 0.6)] if big else [])
    for h0, w0, s in jobs:
        img = np.random.default_rng(h0 + w0).integers(0, 256, (h0, w0)).astype(np.uint8)
        img[: h0 // 5, : w0 // 7] = 255
        plan = F.level_plan(w0, h0, s, 6)
        for k, lv in enumerate(plan):
            got = fn_plan_level(img, s, 6, k)
            ref, bound = F.pyr_level(img, lv, mut=mut)
            case = "%dx%d@%g/level%d(%dx%d,k%d)" % (w0, h0, s, k, lv[0], lv[1], lv[2])
            if got.shape != ref.shape:
                assert mut, case
                worst = max(worst, (np.inf, case + " shape"))
                continue
            if mut:
                r, at, bad = ratio(got, ref, bound)
                worst = max(worst, (r, "%s at %s, %d values" % (case, at, bad)))
            else:
                worst = max(worst, (check(who, "pyr_level", case, got, ref, bound), case))
    return worst


def oracle_fns(oracle):
    def upd(R0, R1, flow):
        return oracle.update_matrices(R0, R1, flow)

    def win(M, w, gaussian):
        z = np.zeros(M.shape[:2] + (5,), F32)
        return oracle.update_flow(z, z, np.zeros(M.shape[:2] + (2,), F32), M, w, 0, gaussian=gaussian)[0]

    def ups(prev, w, h, s):
        return oracle.flow_upsample(prev, w, h, s)

    def pyr(img, s, levels, k):
        return oracle.pyr_level(img, oracle.level_plan(img.shape[1], img.shape[0], s, levels)[k])
    return upd, win, ups, pyr


def test_update_matrices(oracle):
    run_update_matrices("oracle", oracle_fns(oracle)[0])


def test_window_solve(oracle):
    run_window_solve("oracle", oracle_fns(oracle)[1], oracle=oracle)


def test_flow_upsample(oracle):
    run_flow_upsample("oracle", oracle_fns(oracle)[2])


def test_pyr_level(oracle):
    run_pyr_level("oracle", oracle_fns(oracle)[3])


def plan_grid():
    for s in PYR_SCALES + (0.5,):
        for n in range(1, 701):
            for (w, h) in ((n, n), (n, 257), (333, n)):
                yield w, h, s
    yield 180, 117, 0.5  # 58.5: half to even


def plan_mismatches(oracle, mut=F.NONE):
    bad = []
    for w, h, s in plan_grid():
        got = [(lv.width, lv.height, lv.smooth_sz) for lv in oracle.level_plan(w, h, s, 6)]
        want = [lv[:3] for lv in F.level_plan(w, h, s, 6, mut=mut)]
        if got != want:
            bad.append((w, h, s, got, want))
    return bad


def test_level_plan(oracle):
    """Widths, heights, smooth_sz and the level count for sizes 1 .. 700 at six scales, 6 levels asked."""
    bad = plan_mismatches(oracle)
    print("f64ref oracle level_plan grid mismatches=%d of %d" % (len(bad), sum(1 for _ in plan_grid())))
    assert not bad, bad[:3]
    assert [lv[:2] for lv in F.level_plan(180, 117, 0.5, 3)] == [(180, 117), (90, 58)]


AREA_CASES = [(64, 96, 32, 48), (64, 96, 16, 24), (64, 96, 8, 12), (117, 180, 58, 90), (257, 333, 93, 120),
              (270, 480, 34, 60), (101, 97, 33, 40), (70, 70, 70, 70)]  # (h0, w0, h, w): ratios 2, 4, 8, mixed, non-integer, 1


def run_area_init(who, fn):
    worst = 0.0
    for h0, w0, h, w in AREA_CASES:
        rng = np.random.default_rng(h0 + w)
        f0 = (rng.standard_normal((h0, w0, 2)) * 5).astype(F32)
        scale = w / w0 if (h0, w0) != (h, w) else 1.0
        got = fn(f0, w, h, scale)
        ref, bound = F.area_init(f0, w, h, scale)
        worst = max(worst, check(who, "area_init", "%dx%d->%dx%d" % (w0, h0, w, h), got, ref, bound))
    return worst


def test_area_init():
    """The INTER_AREA seeding of an initial flow: the float32 restatement the GPU is pinned against
    (tests/test_flow_init_abi.py) against the bin-overlap matrix."""
    run_area_init("restatement", init_level_flow)


def scan_field(rng, h, w):
    fx = (rng.standard_normal((h, w)) * 3).astype(F32)
    fy = (rng.standard_normal((h, w)) * 3).astype(F32)
    fx[::2, ::3], fy[::2, ::3] = 3.0, 4.0      # |v|^2 == 25 exactly
    fx[1::2, ::5], fy[1::2, ::5] = 0.5, 0.0    # == 0.25
    fx[::7, 1::2], fy[::7, 1::2] = 0.0, -0.0   # == 0
    fx[::3, ::7], fy[::3, ::7] = -4.0, 3.0
    return fx, fy


def scan_mismatches(oracle, mut=F.NONE):
    fx, fy = scan_field(np.random.default_rng(11), 117, 180)
    bad = []
    for span in range(1, 15):
        for thr in (0.0, 0.5, 5.0):
            if oracle.span_scan(fx, fy, span, thr) != F.span_scan(fx, fy, span, thr, mut=mut):
                bad.append((span, thr))
    return bad


def test_span_scan(oracle):
    bad = scan_mismatches(oracle)
    print("f64ref oracle span_scan mismatching (span, threshold) cases=%d of 42" % len(bad))
    assert not bad, bad


# ---- (b) exact for quadratics -------------------------------------------------------------------------------------------------------
QUADS = [((1.5, -0.8, 0.6), (2.25, -1.5)), ((0.9, 1.3, -0.7), (-3.0, 0.75)), ((-1.1, 0.7, 0.4), (0.3, 4.6)),
         ((2.0, 1.0, 0.0), (-0.625, -2.125)), ((0.6, -1.4, 1.2), (7.0, -5.0))]  # ((ayy, axx, axy), (dx, dy))


@pytest.mark.parametrize("gaussian,win", [(True, 30), (True, 31), (False, 30), (False, 13)])
def test_one_update_recovers_the_shift_of_a_quadratic(oracle, gaussian, win):
    """f0(x, y) = axx x^2 + axy x y + ayy y^2 + bx x + by y + c and f1(p) = f0(p - d).  Around a pixel p the expansion of
    f0 is (dy: 2 ayy y + axy x + by, dx: 2 axx x + axy y + bx, yy: ayy, xx: axx, xy: axy) and that of f1 the same at
    p - d: written down here, not produced by polyexp.  With A' = [[ayy, axy/2], [axy/2, axx]], FarnebackUpdateMatrices
    from zero flow gives r = A' d, G = A'^2, h = A'^2 d at every pixel, so the window average changes nothing and the
    solve returns d * det / (det + 1e-3), det = (c det A')^2 — OpenCV's regulariser, stated analytically; c = 1 for the
    Gaussian window (its taps sum to 1) and (2m+1)^2 / winSize^2 for the box, which sums 2m+1 taps and divides by winSize.  Away from the
    attenuated border (5 px + the window) the oracle must return exactly that, to within the bound the reference
    propagates from the float32 rounding of the coefficients it is given (relative 2^-24 each).  A wrong sign, a swapped
    coefficient, a wrong 0.5 / 0.25 factor or a wrong (r4 + r5) r6 term misses by O(|d|)."""
    h, w = 96, 128
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    worst = 0.0
    for (ayy, axx, axy), (dx, dy) in QUADS:
        bx, by = 0.37, -1.21

        def coef(x, y):
            return np.stack([2 * ayy * y + axy * x + by, 2 * axx * x + axy * y + bx,
                             np.full_like(x, ayy), np.full_like(x, axx), np.full_like(x, axy)], -1)
        R0e, R1e = coef(xs, ys), coef(xs - dx, ys - dy)
        R0, R1 = R0e.astype(F32), R1e.astype(F32)
        zero = np.zeros((h, w, 2), F32)
        M = oracle.update_matrices(R0, R1, zero)
        got = oracle.update_flow(R0, R1, zero, M, win, 0, gaussian=gaussian)[0]
        Mr, eM = F.update_matrices(R0, R1, zero, F.U32 * np.abs(R0e), F.U32 * np.abs(R1e))
        ref, bound = F.window_solve(Mr, eM, win, gaussian)
        c = 1.0 if gaussian else (2 * (win // 2) + 1) ** 2 / win ** 2  # the box sums 2m+1 taps and divides by winSize
        det = (c * (ayy * axx - axy * axy / 4)) ** 2
        want = np.broadcast_to(np.array([dx, dy]) * det / (det + 1e-3), (h, w, 2))
        b = 5 + win // 2
        inner = (slice(b, h - b), slice(b, w - b))
        case = "A=%r d=%r %s%d" % ((ayy, axx, axy), (dx, dy), "gauss" if gaussian else "box", win)
        assert np.isfinite(bound[inner]).all() and bound[inner].max() < 1e-2 * np.hypot(dx, dy), case
        worst = max(worst, check("oracle", "quadratic", case, got[inner], want[inner].copy(), bound[inner]))
        check("reference", "quadratic", case, ref[inner], want[inner].copy(), bound[inner])
        assert np.abs(got[inner] + want[inner]).min() > 0.1  # and it is d, not -d


# ---- (c) mutants ------------------------------------------------------------------------------------------------------------------------
def _kill_update(oracle, mut):
    return run_update_matrices("oracle", oracle_fns(oracle)[0], mut=frozenset([mut]))


def _kill_window(oracle, mut):
    return run_window_solve("oracle", oracle_fns(oracle)[1], mut=frozenset([mut]), oracle=oracle)


def _kill_ups(oracle, mut):
    return run_flow_upsample("oracle", oracle_fns(oracle)[2], mut=frozenset([mut]))


def _kill_ups06(oracle, mut):
    return run_flow_upsample("oracle", oracle_fns(oracle)[2], mut=frozenset([mut]), cases=[c for c in ups_cases() if c[4] == 0.6])


def _kill_pyr(oracle, mut):
    return run_pyr_level("oracle", oracle_fns(oracle)[3], mut=frozenset([mut]), big=False)


def _kill_plan(oracle, mut):
    bad = plan_mismatches(oracle, frozenset([mut]))
    return (np.inf if bad else 0.0, "%d plans differ, first %r" % (len(bad), bad[:1]))


def _kill_scan(oracle, mut):
    bad = scan_mismatches(oracle, frozenset([mut]))
    return (np.inf if bad else 0.0, "%d (span, threshold) cases differ, first %r" % (len(bad), bad[:1]))


MUTANTS = [
    ("win_reflect", "window borders replicate -> reflect-101", _kill_window),
    ("win_sigma", "window sigma 0.3 m -> 0.3 m + 0.05", _kill_window),
    ("win_even_taps", "2m+1 -> winSize taps for even winSize", _kill_window),
    ("box_scale", "box scale 1/winSize^2 -> 1/(2m+1)^2", _kill_window),
    ("border_swap", "border table entries swapped (0.14 <-> 0.4472)", _kill_update),
    ("border4", "5 -> 4 border pixels", _kill_update),
    ("r6_half", "0.25 -> 0.5 on r6", _kill_update),
    ("oob_r6", "out-of-image r6 * 0.5 -> r6", _kill_update),
    ("inb_w", "in-bounds limit w-1 -> w", _kill_update),
    ("ups_two", "upsample factor 1/pyrScale -> 2 at pyrScale 0.6", _kill_ups06),
    ("no_centre", "the +0.5 / -0.5 centre rule dropped in the resize", _kill_pyr),
    ("no_centre", "the centre rule dropped in the flow upsample", _kill_ups),
    ("size_floor", "cvRound -> floor in level sizes", _kill_plan),
    ("size_half_away", "half away from zero instead of half to even at 58.5", _kill_plan),
    ("scan_ge", "> -> >= in the scan", _kill_scan),
]


@pytest.mark.parametrize("mut,what,kill", MUTANTS, ids=[m[0] + "-" + m[2].__name__[6:] for m in MUTANTS])
def test_mutant_is_caught(oracle, mut, what, kill):
    """Each single-change mutant of the reference must disagree with the oracle beyond the bound on the inputs of (a)."""
    r, where = kill(oracle, mut)
    print("f64ref mutant %s (%s): ratio=%.4g caught in %s" % (mut, what, r, where))
    assert r > 1.0, "mutant %s (%s) survives: worst ratio %.4g (%s) — strengthen the inputs" % (mut, what, r, where)


# ---- (d) end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(117, 180), (270, 480)])
@pytest.mark.parametrize("gaussian", [True, False])
def test_one_iteration_one_level_end_to_end(oracle, h, w, gaussian):
    """pyrLevels 0, one iteration: pyramid level 0 -> expansion -> matrices from zero flow -> window -> solve, the bound
    propagated through all of them.  (Chains of iterations pass the flow through the floor of the sample position, a
    discontinuity no bound crosses: those are left to the warp-recovery test of test_oracle_algorithm.py.)"""
    import synth
    a = textured(h, w, 3)
    b, _, _ = synth.warp_with_flow(a, np.random.default_rng(4))
    p = oracle.default_params(pyrLevels=0, pyrIterations=1, flags=256 if gaussian else 0)
    fx, fy = oracle.farneback(a, b, p)
    ref, bound = F.farneback(a, b, levels=0, iters=1, gaussian=gaussian)
    print("f64ref end_to_end bound: median %.3g max %.3g infinite %d of %d" % (
        float(np.median(bound)), float(bound.max()), int(np.isinf(bound).sum()), bound.size))
    assert np.isfinite(bound).all() and np.median(bound) < 1e-3
    check("oracle", "end_to_end", "%dx%d/%s" % (w, h, "gauss" if gaussian else "box"), np.stack([fx, fy], -1), ref, bound)


def test_polyexp_every_pixel(oracle):
    """The expansion on every pixel (test_oracle_algorithm.py solves the least-squares fit at 68 of them).  Three points of
    the parameter axis; tests/test_oracle_params.py runs polyN 1..7 x five sigmas with this same judge, and
    tests/test_gpu_params.py the kernels — a case added here belongs there too."""
    for (h, w, n, sg) in ((40, 52, 7, 1.5), (117, 180, 5, 1.1), (33, 47, 7, 0.0)):
        I = (ndimage.gaussian_filter(np.random.default_rng(h).random((h, w)), 1.0) * 255).astype(F32)
        ref, bound = F.polyexp(I, 0.0, n, sg)
        check("oracle", "polyexp", "%dx%d/n%d/s%g" % (w, h, n, sg), oracle.polyexp(I, n, sg), ref, bound)
