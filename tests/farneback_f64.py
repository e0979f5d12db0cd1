"""Independent float64 reference of every Farneback stage, with a running error bound — TEST INFRASTRUCTURE.

Written from SURVEY.md Appendix A (A.1 - A.7) and Farneback's paper, in vectorised numpy / scipy; it shares no loop with
oracle/farneback_oracle.c.  Formulations: scipy.ndimage.correlate1d for the separable windows, cumulative sums for the
box window, explicit coordinate maps and fancy indexing for the resizes and the warp, an explicit bin-overlap matrix for
INTER_AREA, moments + the inverse Gram matrix (the normal equations of the weighted least-squares fit) for the expansion.

DECISIONS follow OpenCV's float32 rules, ARITHMETIC is float64.  Computed on float32 values, because a reference on the
other side of a discontinuity is no reference: fx = float32(x) + dx, its floor and its fraction; the in-bounds test; the
resize coordinate float32((d + 0.5) * scale - 0.5); cvRound sizes (half to even); every stored kernel / table
coefficient (Gaussian kernels, window kernels, g / xg / xxg, resize weights 1 - f and f, INTER_AREA alphas, the Gram
sums).  Every sum and product of DATA is float64.

Every stage returns (value, bound).  `bound` is a running bound on |float32 evaluation - value| for ANY evaluation order
of the same expression, computed by the same dataflow on absolute values:
  - a sum of n products: gamma(n + 1) * sum |a_i| |b_i|, gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1: n - 1 additions and one product per term, one to spare);
  - an input that itself carries a bound e: the bound passes through the stage to first order (e through the same
    weights, |x| + e wherever |x| multiplies a rounding term);
  - short fixed expressions (the warp's combine step): one relative rounding u per operation on (|value| + error), plus
    2^-149 for a gradual underflow;
  - the solve's division: (err_num + |q| err_den) / (|den| - err_den), infinite where the denominator may vanish;
  - one ulp of the float32 result for the final store (store32).
Steps OpenCV evaluates in double (the expansion's horizontal pass, the box sums, the solve) use u = 2^-53 — except the
two float32 operations inside the box window's column sums, which window_solve names and bounds with u = 2^-24.
No other tolerance exists in the tests that use this module.

`mut` (a set of names, default empty) switches single deliberate errors on: the mutants of tests/test_oracle_stages_f64.py,
each of which the oracle must contradict beyond the bound.
"""
import numpy as np
from scipy import ndimage

F32 = np.float32
F64 = np.float64
U32 = 2.0 ** -24
U64 = 2.0 ** -53
ETA32 = 2.0 ** -149
NONE = frozenset()


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def store32(v, e):
    """Bound after the final float32 store of a value known to within e: one ulp of the float32 result."""
    with np.errstate(over="ignore", invalid="ignore"):
        return e + np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


# ---- (value, error) arithmetic for short fixed expressions -----------------------------------------------------------
def _r(v, e, u):
    return e + u * (np.abs(v) + e) + (ETA32 if u == U32 else 0.0)


def _mul(a, b, u=U32):
    v = a[0] * b[0]
    return v, _r(v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1], u)


def _add(a, b, u=U32):
    v = a[0] + b[0]
    return v, _r(v, a[1] + b[1], u)


def _sub(a, b, u=U32):
    v = a[0] - b[0]
    return v, _r(v, a[1] + b[1], u)


def _x(v):
    return np.asarray(v, F64), 0.0


def _f32floor(f):
    """cvFloor of a float32 array as int64; non-finite and out-of-int-range values give INT_MIN like cvtsd2si."""
    f = np.asarray(f, F32)
    ok = np.isfinite(f) & (f > F32(-2147483648.0)) & (f < F32(2147483648.0))
    out = np.full(f.shape, -2 ** 31, np.int64)
    out[ok] = np.floor(f[ok].astype(F64)).astype(np.int64)
    return out


# ---- A.1 level plan ------------------------------------------------------------------------------------------------------
def level_plan(w0, h0, pyr_scale=0.5, levels=3, mut=NONE):
    """[(width, height, smooth_sz, sigma, scale)] for k = 0 .. levels actually used (A.1).  scale = pyr_scale^k by
    repeated multiplication in double; sizes cvRound (half to even); a level enters while both sides are >= 32."""
    scales = np.concatenate([[1.0], np.multiply.accumulate(np.full(max(levels, 0), float(pyr_scale)))])
    ok = (w0 * scales[1:] >= 32) & (h0 * scales[1:] >= 32)
    n = int(np.argmin(ok)) if not ok.all() else len(ok)
    if "size_floor" in mut:
        rnd = lambda v: int(np.floor(v))  # noqa: E731
    elif "size_half_away" in mut:
        rnd = lambda v: int(np.floor(v + 0.5))  # noqa: E731
    else:
        rnd = lambda v: int(round(float(v)))  # Python's round: half to even  # noqa: E731
    out = []
    for s in scales[: n + 1]:
        sigma = (1.0 / s - 1) * 0.5
        out.append((rnd(w0 * s), rnd(h0 * s), max(int(round(sigma * 5)) | 1, 3), sigma, float(s)))
    return out


# ---- A.2 pyramid level ------------------------------------------------------------------------------------------------------
def gaussian_kernel(n, sigma):
    """getGaussianKernel(n, sigma, CV_32F): float32 coefficients (a stored table: float32 rules)."""
    if sigma <= 0 and n % 2 == 1 and n <= 7:
        t = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}[n]
        k = np.array(t, F32)
    else:
        sg = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
        x = np.arange(n) - (n - 1) * 0.5
        k = np.exp(-0.5 / (sg * sg) * x * x).astype(F32)
    return (k.astype(F64) * (1.0 / k.astype(F64).sum())).astype(F32)


def _corr2(v, e, k, mode):
    """Separable correlation (rows first, then columns) of a field known to within e; a float32 evaluation of each
    pass is a sum of len(k) products."""
    k = np.asarray(k, F64)
    g = gamma(len(k) + 1)
    e = np.broadcast_to(np.asarray(e, F64), v.shape)
    for ax in (1, 0):
        a = ndimage.correlate1d(np.abs(v) + e, np.abs(k), axis=ax, mode=mode)
        e = ndimage.correlate1d(e, np.abs(k), axis=ax, mode=mode) + g * a + ETA32
        v = ndimage.correlate1d(v, k, axis=ax, mode=mode)
    return v, e


def _axis_map(ssize, dsize, mut=NONE):
    """The INTER_LINEAR coordinate rule of A.2 for one axis: (floor, fraction) of float32((d + 0.5) * scale - 0.5), the
    fraction float32 as OpenCV's tables store it.  Clamping is the caller's (x and y differ)."""
    scale = 1.0 / (dsize / ssize)
    d = np.arange(dsize, dtype=F64)
    f = (d * scale if "no_centre" in mut else (d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f.astype(F64)).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    return s, f


def resize_linear(v, e, dw, dh, mut=NONE):
    """cv::resize(INTER_LINEAR) of a float field (h, w[, c]) known to within e.  In x a coordinate left of 0 / at or past
    the last column is clamped WITH its fraction zeroed; in y the rows are clipped and the weights are kept (A.2).  An
    exact halving is OpenCV's area-fast branch: the same four samples and weights 1/4, so one formula serves both."""
    sh, sw = v.shape[:2]
    if (sw, sh) == (dw, dh):
        return v.copy(), np.broadcast_to(np.asarray(e, F64), v.shape).copy()
    sx, fx = _axis_map(sw, dw, mut)
    sy, fy = _axis_map(sh, dh, mut)
    lo, hi = sx < 0, sx >= sw - 1
    fx = np.where(lo | hi, F32(0), fx)
    sx = np.where(lo, 0, np.where(hi, sw - 1, sx))
    x0, x1 = sx, np.minimum(sx + 1, sw - 1)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    ax = [(F32(1) - fx).astype(F64), fx.astype(F64)]
    ay = [(F32(1) - fy).astype(F64), fy.astype(F64)]
    e = np.broadcast_to(np.asarray(e, F64), v.shape)
    shp = (dh, dw) + (1,) * (v.ndim - 2)
    out = np.zeros((dh, dw) + v.shape[2:], F64)
    ab = np.zeros_like(out)
    er = np.zeros_like(out)
    for yi, wy in ((y0, ay[0]), (y1, ay[1])):
        for xi, wx in ((x0, ax[0]), (x1, ax[1])):
            wgt = np.abs(wy[:, None] * wx[None, :]).reshape(shp)
            sgn = (wy[:, None] * wx[None, :]).reshape(shp)
            s = v[np.ix_(yi, xi)]
            out += sgn * s
            ab += wgt * (np.abs(s) + e[np.ix_(yi, xi)])
            er += wgt * e[np.ix_(yi, xi)]
    # four terms, each two products (or one sum and the 1/4), three additions: at most five roundings on any term
    return out, er + gamma(5) * ab + ETA32


def pyr_level(img, lv, mut=NONE):
    """Level lv = (width, height, smooth_sz, sigma, ...) of a uint8 image: GaussianBlur at full resolution, REFLECT_101
    borders, then the bilinear resize (A.2)."""
    w, h, n, sigma = lv[:4]
    k = gaussian_kernel(n, sigma)
    v, e = _corr2(np.asarray(img, F64), 0.0, k, "mirror")
    v, e = resize_linear(v, e, w, h, mut)
    return v, e


# ---- A.3 polynomial expansion ---------------------------------------------------------------------------------------------
def polyexp_setup(n, sigma):
    """g, xg, xxg (float32 tables) and the inverse Gram matrix of the basis (1, y, x, yy, xx, xy) under g(y) g(x)."""
    sg = sigma if sigma >= np.finfo(F32).eps else n * 0.3
    x = np.arange(-n, n + 1)
    g = np.exp(-x * x / (2 * sg * sg)).astype(F32)
    g = (g.astype(F64) * (1.0 / g.astype(F64).sum())).astype(F32)
    xf = x.astype(F32)
    xg = (xf * g).astype(F32)
    xxg = ((xf * xf) * g).astype(F32)  # the integer x * x is exact
    P = (g[:, None] * g[None, :]).astype(F32)  # the Gram sums: float32 products, double accumulation (A.3)
    X = np.broadcast_to(xf[None, :], P.shape)
    Y = np.broadcast_to(xf[:, None], P.shape)
    G = np.zeros((6, 6))
    G[0, 0] = P.astype(F64).sum()
    G[1, 1] = ((P * X) * X).astype(F64).sum()
    G[3, 3] = ((((P * X) * X) * X) * X).astype(F64).sum()
    G[5, 5] = ((((P * X) * X) * Y) * Y).astype(F64).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    return g, xg, xxg, np.linalg.inv(G), float(np.linalg.cond(G))


def polyexp(I, eI=0.0, n=7, sigma=1.5):
    """(h, w, 5) coefficients (y, x, yy, xx, xy) of the Gaussian-weighted least-squares quadratic at every pixel, borders
    replicated: the moments b = B^T W f by separable correlation, then G^-1 b.  Vertical pass float32, horizontal double."""
    I = np.asarray(I, F64)
    g, xg, xxg, iG, cond = polyexp_setup(n, sigma)
    eI = np.broadcast_to(np.asarray(eI, F64), I.shape)
    gv = gamma(2 * n + 2)
    gh = gamma(2 * n + 2, U64)
    col = {}
    for name, kern in (("1", g), ("y", xg), ("yy", xxg)):
        kk = kern.astype(F64)
        v = ndimage.correlate1d(I, kk, axis=0, mode="nearest")
        a = ndimage.correlate1d(np.abs(I) + eI, np.abs(kk), axis=0, mode="nearest")
        e = ndimage.correlate1d(eI, np.abs(kk), axis=0, mode="nearest") + gv * a + ETA32
        col[name] = (v, e)

    def hz(name, kern):
        kk = kern.astype(F64)
        v, e = col[name]
        a = ndimage.correlate1d(np.abs(v) + e, np.abs(kk), axis=1, mode="nearest")
        return (ndimage.correlate1d(v, kk, axis=1, mode="nearest"),
                ndimage.correlate1d(e, np.abs(kk), axis=1, mode="nearest") + gh * a)
    b1, b2, b3 = hz("1", g), hz("1", xg), hz("y", g)
    b4, b5, b6 = hz("1", xxg), hz("yy", g), hz("y", xg)
    # G^-1 b: the Gram matrix couples only (1, yy, xx); the inverse itself is known to ~ cond(G) * 36 u64
    ig = 36 * cond * U64

    def lin(terms):
        v = sum(c * t[0] for c, t in terms)
        a = sum(abs(c) * (np.abs(t[0]) + t[1]) for c, t in terms)
        e = sum(abs(c) * t[1] for c, t in terms)
        return v, e + (ig + gamma(3, U64)) * a
    out = [lin([(iG[1, 1], b3)]), lin([(iG[1, 1], b2)]), lin([(iG[0, 3], b1), (iG[3, 3], b5)]),
           lin([(iG[0, 3], b1), (iG[3, 3], b4)]), lin([(iG[5, 5], b6)])]
    v = np.stack([o[0] for o in out], -1)
    e = np.stack([o[1] for o in out], -1)
    return v, store32(v, e)


# ---- A.4 FarnebackUpdateMatrices -----------------------------------------------------------------------------------------
def update_matrices(R0, R1, flow, eR0=0.0, eR1=0.0, mut=NONE):
    """M (h, w, 5) from the two expansions (h, w, 5) and a float32 flow (h, w, 2), interleaved layouts.  The flow is a
    float32 field taken exactly (the sample position is a decision); R0 / R1 may carry bounds."""
    R0 = np.asarray(R0, F64)
    R1 = np.asarray(R1, F64)
    flow = np.asarray(flow, F32)
    h, w = R0.shape[:2]
    eR0 = np.broadcast_to(np.asarray(eR0, F64), R0.shape)
    eR1 = np.broadcast_to(np.asarray(eR1, F64), R1.shape)
    dx, dy = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        fx = (np.arange(w, dtype=F32)[None, :] + dx).astype(F32)
        fy = (np.arange(h, dtype=F32)[:, None] + dy).astype(F32)
        x1, y1 = _f32floor(fx), _f32floor(fy)
        lim = 0 if "inb_w" in mut else 1
        inb = (x1 >= 0) & (x1 < w - lim) & (y1 >= 0) & (y1 < h - lim)
        ax = np.where(inb, (fx - x1.astype(F32)).astype(F32), F32(0)).astype(F64)
        ay = np.where(inb, (fy - y1.astype(F32)).astype(F32), F32(0)).astype(F64)
    xa = np.clip(x1, 0, w - 1)
    ya = np.clip(y1, 0, h - 1)
    xb = np.minimum(xa + 1, w - 1)
    yb = np.minimum(ya + 1, h - 1)
    one = _x(1.0)
    wx1, wy1 = _x(ax), _x(ay)
    wx0, wy0 = _sub(one, wx1), _sub(one, wy1)
    a = [_mul(wx0, wy0), _mul(wx1, wy0), _mul(wx0, wy1), _mul(wx1, wy1)]
    idx = [(ya, xa), (ya, xb), (yb, xa), (yb, xb)]
    r = []
    for c in range(5):
        acc = None
        for wgt, (yy, xx) in zip(a, idx):
            t = _mul(wgt, (R1[yy, xx, c], eR1[yy, xx, c]))
            acc = t if acc is None else _add(acc, t)
        r.append(acc)
    p0 = [(R0[..., c], eR0[..., c]) for c in range(5)]
    k6 = 0.5 if "r6_half" in mut else 0.25
    in4, in5, in6 = _mul(_add(p0[2], r[2]), _x(0.5)), _mul(_add(p0[3], r[3]), _x(0.5)), _mul(_add(p0[4], r[4]), _x(k6))
    out6 = p0[4] if "oob_r6" in mut else _mul(p0[4], _x(0.5))

    def sel(i, o):
        return np.where(inb, i[0], o[0]), np.where(inb, i[1], o[1])
    r4, r5, r6 = sel(in4, p0[2]), sel(in5, p0[3]), sel(in6, out6)
    r2 = _mul(_sub(p0[0], sel(r[0], _x(0.0))), _x(0.5))
    r3 = _mul(_sub(p0[1], sel(r[1], _x(0.0))), _x(0.5))
    fdx, fdy = _x(dx), _x(dy)
    with np.errstate(all="ignore"):
        r2 = _add(r2, _add(_mul(r4, fdy), _mul(r6, fdx)))
        r3 = _add(r3, _add(_mul(r6, fdy), _mul(r5, fdx)))
    # border attenuation: the product of up to four float32 table entries
    tab = [0.14, 0.14, 0.4472, 0.4472, 0.4472]
    if "border_swap" in mut:
        tab = [0.4472, 0.4472, 0.14, 0.14, 0.14]
    if "border4" in mut:
        tab = tab[:4]
    nb = len(tab)
    tab = np.array(tab, F32).astype(F64)

    def side(n):
        i = np.arange(n)
        lo = np.where(i < nb, tab[np.minimum(i, nb - 1)], 1.0)
        hi = np.where(i >= n - nb, tab[np.clip(n - i - 1, 0, nb - 1)], 1.0)
        return lo, hi
    xl, xh = side(w)
    yl, yh = side(h)
    sc = _mul(_mul(_mul(_x(xl[None, :]), _x(xh[None, :])), _x(yl[:, None])), _x(yh[:, None]))
    edge = sc[0] != 1.0

    def att(t):
        m = _mul(t, sc)
        return np.where(edge, m[0], t[0]), np.where(edge, m[1], t[1])
    with np.errstate(all="ignore"):
        r2, r3, r4, r5, r6 = att(r2), att(r3), att(r4), att(r5), att(r6)
        M = [_add(_mul(r4, r4), _mul(r6, r6)), _mul(_add(r4, r5), r6), _add(_mul(r5, r5), _mul(r6, r6)),
             _add(_mul(r4, r2), _mul(r6, r3)), _add(_mul(r6, r2), _mul(r5, r3))]
        v = np.stack([m[0] for m in M], -1)
        e = np.stack([m[1] for m in M], -1)
        return v, store32(v, e)


# ---- A.5 window average and the 2x2 solve -----------------------------------------------------------------------------------
def window_kernel(win, mut=NONE):
    """The 2m+1 float32 taps of FarnebackUpdateFlow_GaussianBlur's window, m = win / 2, sigma = 0.3 m."""
    m = win // 2
    sigma = m * 0.3 + (0.05 if "win_sigma" in mut else 0.0)
    i = np.arange(1, m + 1)
    t = np.exp(-i * i / (2 * sigma * sigma)).astype(F32) if m else np.zeros(0, F32)
    s = 1.0 / (1.0 + 2.0 * t.astype(F64).sum())
    half = (np.concatenate([[1.0], t.astype(F64)]) * s).astype(F32)
    return np.concatenate([half[:0:-1], half])


def _solve(H, eH):
    """flow = G^-1 h with the 1e-3 regulariser, in double; H (h, w, 5) = (g11, g12, g22, h1, h2) known to within eH."""
    g11, g12, g22, h1, h2 = [(H[..., c], eH[..., c]) for c in range(5)]
    u = U64
    det = _add(_sub(_mul(g11, g22, u), _mul(g12, g12, u), u), _x(1e-3), u)
    nx = _sub(_mul(g11, h2, u), _mul(g12, h1, u), u)
    ny = _sub(_mul(g22, h1, u), _mul(g12, h2, u), u)
    out = []
    with np.errstate(all="ignore"):
        room = np.abs(det[0]) - det[1]
        for num in (nx, ny):
            q = num[0] / det[0]
            e = np.where(room > 0, (num[1] + np.abs(q) * det[1]) / np.where(room > 0, room, 1.0), np.inf)
            out.append((q, e + 3 * u * np.abs(q)))
    v = np.stack([o[0] for o in out], -1)
    e = np.stack([o[1] for o in out], -1)
    return v, store32(v, e)


def window_solve(M, eM=0.0, win=30, gaussian=True, mut=NONE):
    """New flow (h, w, 2) from M (h, w, 5): the window average with REPLICATED borders, then the solve (A.5).
    Gaussian: float32 separable passes of 2m+1 taps.  Box: double sums over the (2m+1)^2 window, scaled by 1 / win^2."""
    M = np.asarray(M, F64)
    h, w = M.shape[:2]
    eM = np.broadcast_to(np.asarray(eM, F64), M.shape)
    m = win // 2
    if gaussian:
        k = window_kernel(win, mut).astype(F64)
        origin = 0
        if "win_even_taps" in mut and win % 2 == 0:
            k = k[:-1] / k[:-1].sum()  # winSize taps instead of 2m+1
            k = np.concatenate([k, [0.0]])
        mode = "mirror" if "win_reflect" in mut else "nearest"
        g = gamma(2 * m + 2)
        H, eH = M, eM
        for ax in (0, 1):
            a = ndimage.correlate1d(np.abs(H) + eH, np.abs(k), axis=ax, mode=mode, origin=origin)
            eH = ndimage.correlate1d(eH, np.abs(k), axis=ax, mode=mode, origin=origin) + g * a + ETA32
            H = ndimage.correlate1d(H, k, axis=ax, mode=mode, origin=origin)
        return _solve(H, eH)
    # box: cumulative sums of the edge-padded field
    def boxsum(a):
        p = np.pad(a, ((m + 1, m), (m + 1, m), (0, 0)), mode="edge")
        c = p.cumsum(0).cumsum(1)
        n = 2 * m + 1
        return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    scale = 1.0 / ((2 * m + 1) ** 2 if "box_scale" in mut else win * win)
    S = boxsum(M)
    # Double steps: OpenCV slides sums down the columns and along the rows, one rounding per addition or subtraction, each
    # of at most u64 times the absolute sum inside some window; a pixel's sums have seen at most 2 (h + w + 4 m + 4).
    A = boxsum(np.abs(M) + eM)
    nops = 2 * (h + w + 4 * m + 4) + 2
    eS = boxsum(eM) + nops * U64 * A.max(axis=(0, 1), keepdims=True)
    # The float32 steps (found by this test): the column update is vsum += M(y+m) - M(y-m-1) with
    # the difference of the two float32 rows taken in float32 before it is widened.  Its rounding never leaves the running
    # sum again, so row y carries every row's above it: u32 * cumsum |M(y'+m) - M(y'-m-1)|, then the horizontal window.
    pe = np.pad(eM, ((m + 1, m), (0, 0), (0, 0)), mode="edge")
    ps = np.pad(M, ((m + 1, m), (0, 0), (0, 0)), mode="edge")
    eV = U32 * np.cumsum(np.abs(ps[2 * m + 1:] - ps[:h]) + pe[2 * m + 1:] + pe[:h], axis=0)
    eV = eV + U32 * (m + 2) * (np.abs(M[:1]) + eM[:1])  # and the start value row0 * (m + 2): a float32 product as well
    ce = np.pad(eV, ((0, 0), (m + 1, m), (0, 0)), mode="edge").cumsum(1)
    eS = eS + ce[:, 2 * m + 1:] - ce[:, :w]
    return _solve(S * scale, eS * scale)


# ---- A.6 flow upsample -----------------------------------------------------------------------------------------------------
def flow_upsample(prev, ePrev, w, h, pyr_scale=0.5, mut=NONE):
    """resize(prevFlow, (w, h), INTER_LINEAR) * float32(1 / pyr_scale) on an interleaved (ph, pw, 2) field."""
    v, e = resize_linear(np.asarray(prev, F64), ePrev, w, h, mut)
    s = 2.0 if "ups_two" in mut else float(F32(1.0 / pyr_scale))
    v, e = _mul((v, e), _x(s))
    return v, store32(v, e)


# ---- A.1 OPTFLOW_USE_INITIAL_FLOW: INTER_AREA seeding ------------------------------------------------------------------------
def _area_matrix(ssize, dsize):
    """(dsize, ssize) INTER_AREA overlaps for one axis, and the bins' widths: the overlap of source cell [s, s+1) with
    the destination bin [d scale, (d+1) scale), clipped to the image; partial overlaps of at most 1e-3 are dropped, as
    OpenCV's table does."""
    scale = 1.0 / (dsize / ssize)
    lo = np.arange(dsize)[:, None] * scale
    hi = lo + scale
    s = np.arange(ssize)[None, :]
    ov = np.clip(np.minimum(s + 1.0, hi) - np.maximum(s, lo), 0.0, 1.0)
    ov[ov <= 1e-3] = 0.0
    return ov, np.minimum(scale, ssize - lo), scale


def area_init(flow0, w, h, scale):
    """resize(flow0, (w, h), INTER_AREA); flow *= scale — the coarsest level's start from a caller's field (h0, w0, 2)."""
    f = np.asarray(flow0, F64)
    h0, w0 = f.shape[:2]
    if (w0, h0) == (w, h):
        v, e = f.copy(), np.zeros_like(f)
        n = 1
    else:
        (Wy, cy, sy), (Wx, cx, sx) = _area_matrix(h0, h), _area_matrix(w0, w)
        eps = np.finfo(F64).eps
        if abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps:
            # integer ratios: OpenCV sums the block and multiplies by float32(1 / area)
            Wy = Wy * float(F32(1.0) / F32(round(sx) * round(sy)))
        else:
            Wy, Wx = (Wy / cy).astype(F32).astype(F64), (Wx / cx).astype(F32).astype(F64)  # float32 alphas
        with np.errstate(all="ignore"):
            v = np.einsum("ys,stc,xt->yxc", Wy, f, Wx)
            a = np.einsum("ys,stc,xt->yxc", Wy, np.abs(f), Wx)
        n = int((Wy != 0).sum(1).max() * (Wx != 0).sum(1).max())
        e = gamma(n + 3) * a + ETA32
    if abs(scale - 1.0) >= np.finfo(F64).eps:
        v, e = _mul((v, e), _x(float(F32(scale))))
    return v, store32(v, e)


# ---- span scan ---------------------------------------------------------------------------------------------------------------
def span_scan(fx, fy, span=10, threshold=5.0, mut=NONE):
    """[(x, y, dx, dy)] of the span-grid points whose float32 squared length exceeds threshold^2 (double), row-major."""
    fx = np.asarray(fx, F32)
    fy = np.asarray(fy, F32)
    gx, gy = fx[::span, ::span], fy[::span, ::span]
    with np.errstate(all="ignore"):
        ln = ((gx * gx).astype(F32) + (gy * gy).astype(F32)).astype(F32).astype(F64)
    t2 = float(threshold) * float(threshold)
    hit = ln >= t2 if "scan_ge" in mut else ln > t2
    ys, xs = np.nonzero(hit)
    return [(int(x) * span, int(y) * span, float(gx[y, x]), float(gy[y, x])) for y, x in zip(ys, xs)]


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def farneback(prev, nxt, pyr_scale=0.5, levels=3, win=30, iters=3, n=7, sigma=1.5, gaussian=True):
    """A.1: (flow (h, w, 2), bound).  The bound is propagated through every stage EXCEPT through the sample position of
    FarnebackUpdateMatrices, which is a decision taken on the float32 rounding of this reference's own flow; it is
    therefore meaningful for one iteration at one level only (from the zero flow), which is all the tests ask of it."""
    h0, w0 = prev.shape
    plan = level_plan(w0, h0, pyr_scale, levels)
    flow = eflow = None
    for lv in plan[::-1]:
        w, h = lv[:2]
        if flow is None:
            flow, eflow = np.zeros((h, w, 2)), np.zeros((h, w, 2))
        else:
            flow, eflow = flow_upsample(flow, eflow, w, h, pyr_scale)
        R = [polyexp(*pyr_level(im, lv), n=n, sigma=sigma) for im in (prev, nxt)]
        for i in range(iters):
            M, eM = update_matrices(R[0][0], R[1][0], flow.astype(F32), R[0][1], R[1][1])
            flow, eflow = window_solve(M, eM, win, gaussian)
    return flow, eflow
