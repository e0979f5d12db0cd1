"""Algorithm-level checks of the CPU oracle in the branches NO reference vector reaches.

The reference pins one 180x117 pair (two pyramid levels, 3/5-tap smoothing, generic bilinear resize).  Everything a
1080p / 4K run adds — RowFilter order for ksize > 5, the exact-halving resize, >= 3 levels, winSize 50 — is a
restatement of OpenCV 2.4.9 from memory (OpenCV itself is not in this image).  These tests cannot
make those branches "pinned"; they catch a from-memory border mode, sigma, coordinate rule or sign that is simply
wrong, by checking the oracle against what the ALGORITHM must produce, computed independently with numpy / scipy:

  (a) a known smooth warp of a well-textured image is recovered (1080p defaults; 4K with config-5 parameters),
  (b) FarnebackPolyExp equals a direct Gaussian-weighted least-squares quadratic fit (polyN 5 and 7),
  (c) a pyramid level equals scipy's mirror-border Gaussian correlation of the full-resolution image followed by the
      explicit 2x2 mean the bilinear resize degenerates to at power-of-two ratios (ksize 3 / 9 / 19 / 39 / 79).

Since then tests/test_oracle_stages_f64.py checks EVERY stage, on every pixel, against an independent float64 reference
(tests/farneback_f64.py) within that reference's propagated float32 bound: FarnebackUpdateMatrices, the Gaussian and box
windows with the solve, the flow upsample, INTER_AREA seeding, pyramid levels at any pyrScale, the level plan, the span
scan and the expansion at every pixel.  What stays here: the multi-level, multi-iteration warp recovery (a chain no
bound crosses, because each iteration floors its sample position), the sparse least-squares fit and the 0.5-scale
pyramid.  Bit-for-bit parity with a real OpenCV 2.4.9 build remains unpinned.

Reference call site: /root/reference/src/opticalflow.cpp:83-85.  CPU only.
"""
import numpy as np
import pytest
from scipy import ndimage


def _textured(h, w, seed):
    """Band-limited noise: gradients everywhere, no flat panels (the aperture problem is not what is being tested)."""
    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random((h, w)), 3.0)
    t = (t - t.min()) / (t.max() - t.min()) * 255
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w,kw,bounds", [
    (1080, 1920, {}, (0.05, 0.15, 0.30)),
    (2160, 3840, dict(pyrLevels=5, winSize=50, pyrIterations=5), (0.05, 0.15, 0.30)),
])
def test_known_warp_is_recovered(oracle, h, w, kw, bounds):
    """target(x) = expect(x - v(x)) with a smooth |v| <= 6 px field (tidal-wave_amd/synth.py): away from the borders
    the flow must come back as v — median / 95th / 99th percentile endpoint error bounded (measured at the time of
    writing: 0.022 / 0.061 / 0.086 px at 1080p).  A wrong sign, a transposed coefficient, a wrong upsample factor or
    a wrong window sigma at any of the 4 (6) levels breaks this by orders of magnitude."""
    import synth
    e = _textured(h, w, 5)
    t, vx, vy = synth.warp_with_flow(e, np.random.default_rng(9))
    assert 2.0 < np.hypot(vx, vy).max() <= 6.0 * np.sqrt(2)
    fx, fy = oracle.farneback(e, t, oracle.default_params(**kw))
    m = np.zeros((h, w), bool)
    m[64:-64, 64:-64] = True
    epe = np.hypot(fx - vx, fy - vy)[m]
    med, p95, p99 = np.median(epe), np.quantile(epe, 0.95), np.quantile(epe, 0.99)
    assert med <= bounds[0] and p95 <= bounds[1] and p99 <= bounds[2], (med, p95, p99)
    # and it is v, not -v or 0
    assert med < 0.1 * np.median(np.hypot(vx, vy)[m])


def test_screenshot_like_pair_recovers_the_warp_where_there_is_texture(oracle):
    """The bench's own synthetic 1080p pair (piecewise-flat panels + weak texture): where the local gradient energy is
    high the flow follows the warp; the estimate is far closer to v than to -v."""
    import synth
    a, b, vx, vy = synth.make_pair(0, 1080, 1920, with_flow=True)
    fx, fy = oracle.farneback(a, b)
    gy, gx = np.gradient(ndimage.gaussian_filter(a.astype(np.float64), 2.0))
    tex = ndimage.uniform_filter(np.hypot(gx, gy), 31)
    m = tex > 2.0
    m[:48] = m[-48:] = False
    m[:, :48] = m[:, -48:] = False
    assert m.mean() > 0.05
    err = np.median(np.hypot(fx - vx, fy - vy)[m])
    anti = np.median(np.hypot(fx + vx, fy + vy)[m])
    assert err < 0.5 and anti > 3 * err, (err, anti)


@pytest.mark.parametrize("n,sigma", [(7, 1.5), (5, 1.1), (5, 1.5), (7, 0.0)])
def test_polyexp_is_the_weighted_least_squares_quadratic_fit(oracle, n, sigma):
    """FarnebackPolyExp: per pixel the coefficients (y, x, yy, xx, xy) of the quadratic that best fits
    the (2n+1)^2 neighbourhood under the separable Gaussian applicability g(y)g(x), borders replicated.  Solved here
    with numpy.linalg.lstsq on the edge-padded image; agreement <= 1e-4 (measured 4e-7) on an image of range 16."""
    rng = np.random.default_rng(3)
    h, w = 40, 52
    I = (ndimage.gaussian_filter(rng.random((h, w)), 1.0) * 16).astype(np.float32)
    R = oracle.polyexp(I, n, sigma)
    sg = sigma if sigma >= np.finfo(np.float32).eps else n * 0.3
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sg * sg))
    g /= g.sum()
    Y, X = np.meshgrid(x, x, indexing="ij")
    B = np.stack([np.ones_like(X), Y, X, Y * Y, X * X, X * Y], -1).reshape(-1, 6)
    sw = np.sqrt(np.outer(g, g)).reshape(-1, 1)
    P = np.pad(I.astype(np.float64), n, mode="edge")
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (3, 5), (20, 26), (h - 2, 10), (17, w - 3)]
    pts += [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(60)]
    worst = 0.0
    for yy, xx in pts:
        patch = P[yy:yy + 2 * n + 1, xx:xx + 2 * n + 1].reshape(-1, 1)
        coef = np.linalg.lstsq(B * sw, patch * sw, rcond=None)[0].ravel()
        worst = max(worst, float(np.abs(R[yy, xx] - coef[1:]).max()))
    assert worst <= 1e-4, worst


def test_polyexp_recovers_an_exact_quadratic(oracle):
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float64)
    I = (3 + 0.5 * xx - 0.25 * yy + 0.01 * xx * xx - 0.02 * yy * yy + 0.015 * xx * yy).astype(np.float32)
    R = oracle.polyexp(I, 7, 1.5)[10:-10, 10:-10]  # away from the replicated borders
    y, x = yy[10:-10, 10:-10], xx[10:-10, 10:-10]
    want = np.stack([-0.25 - 0.04 * y + 0.015 * x, 0.5 + 0.02 * x + 0.015 * y,
                     np.full_like(x, -0.02), np.full_like(x, 0.01), np.full_like(x, 0.015)], -1)
    assert np.abs(R - want).max() < 2e-3  # the image itself is float32 at magnitude ~100


def test_pyramid_levels_equal_mirror_gaussian_then_2x2_mean(oracle):
    """level k = GaussianBlur(full-res, ksize, sigma, REFLECT_101) then resize(INTER_LINEAR), which at
    a ratio of 2^k reads the 2x2 block at (2^k x + 2^(k-1) - 1, +1) with weights 1/4 (k = 1: the exact-halving
    area-fast branch; k >= 2: bilinear at fraction 1/2).  scipy.ndimage.correlate1d(mode='mirror') is REFLECT_101.
    ksize 3, 3, 9, 19, 39, 79 (a 6-level plan as config 5 has); agreement <= 1e-4 on the 0..255 scale (measured
    3.6e-5: float32 accumulation against float64)."""
    rng = np.random.default_rng(3)
    h0, w0 = 1088, 1280
    img = rng.integers(0, 256, (h0, w0)).astype(np.uint8)
    plan = oracle.level_plan(w0, h0, 0.5, 5)
    assert [lv.smooth_sz for lv in plan] == [3, 3, 9, 19, 39, 79]
    assert [(lv.width, lv.height) for lv in plan] == [(1280 >> k, 1088 >> k) for k in range(6)]
    f = img.astype(np.float64)
    for k, lv in enumerate(plan):
        n, sg = lv.smooth_sz, lv.sigma
        assert abs(sg - (2 ** k - 1) * 0.5) < 1e-12
        if sg <= 0:
            kern = np.array([0.25, 0.5, 0.25])  # getGaussianKernel's fixed table for sigma <= 0, n = 3
        else:
            x = np.arange(n) - (n - 1) / 2
            kern = np.exp(-x * x / (2 * sg * sg))
            kern /= kern.sum()
        bl = ndimage.correlate1d(ndimage.correlate1d(f, kern, axis=1, mode="mirror"), kern, axis=0, mode="mirror")
        if k == 0:
            ref = bl
        else:
            s = 2 ** k
            c0 = s * np.arange(lv.width) + s // 2 - 1
            r0 = s * np.arange(lv.height) + s // 2 - 1
            ref = (bl[np.ix_(r0, c0)] + bl[np.ix_(r0, c0 + 1)] + bl[np.ix_(r0 + 1, c0)] + bl[np.ix_(r0 + 1, c0 + 1)]) / 4
        got = oracle.pyr_level(img, lv)
        assert np.abs(got - ref).max() <= 1e-4, (k, float(np.abs(got - ref).max()))
