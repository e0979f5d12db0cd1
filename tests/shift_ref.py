"""The shift estimation (TW_OPT_SHIFT) restated in plain numpy from the definition in include/twflow.h: the four profiles,
the per-axis search, the acceptance check on the pixels.  Everything is integer (Python ints where 64 bits matter), so the
kernels, the stub and this file agree value for value.  Also the page generator of the shift tests."""
import collections

import numpy as np

Shift = collections.namedtuple("Shift", "dx dy applied n_shift n_zero sad_shift sad_zero")
U64 = (1 << 64) - 1


def profiles(E, T):
    """(colE [w], colT [w], rowE [h], rowT [h]) as uint32."""
    E = np.asarray(E, np.uint8)
    T = np.asarray(T, np.uint8)
    assert E.ndim == 2 and E.shape == T.shape
    return (E.sum(axis=0, dtype=np.uint32), T.sum(axis=0, dtype=np.uint32),
            E.sum(axis=1, dtype=np.uint32), T.sum(axis=1, dtype=np.uint32))


def visit_order(r):
    """0, -1, +1, -2, +2, ..., -r, +r"""
    out = [0]
    for a in range(1, r + 1):
        out += [-a, a]
    return out


def cost(pE, pT, d):
    L = len(pE)
    lo, hi = max(0, -d), min(L, L - d)
    a = np.asarray(pE[lo:hi], np.int64)
    b = np.asarray(pT[lo + d:hi + d], np.int64)
    return int(np.abs(a - b).sum())


def search(pE, pT, R):
    """One axis: the best d in [-r, r], r = min(R, L // 2); a candidate replaces the best one only when
    cost(d) * n(best) < cost(best) * n(d) in unsigned 64 bits."""
    L = len(pE)
    assert len(pT) == L and L >= 1
    r = min(int(R), L // 2)
    best = None
    for d in visit_order(r):
        c, n = cost(pE, pT, d), L - abs(d)
        if best is None:
            best = (d, c, n)
            continue
        lhs, rhs = c * best[2], best[1] * n
        assert lhs <= U64 and rhs <= U64  # (the definition's bound: nothing wraps)
        if lhs < rhs:
            best = (d, c, n)
    return best[0]


def sad(E, T, dx, dy):
    """(sum |E[y][x] - T[y + dy][x + dx]| over the overlap rectangle, its area)"""
    h, w = E.shape
    x0, x1 = max(0, -dx), min(w, w - dx)
    y0, y1 = max(0, -dy), min(h, h - dy)
    a = E[y0:y1, x0:x1].astype(np.int64)
    b = T[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int64)
    return int(np.abs(a - b).sum()), (y1 - y0) * (x1 - x0)


def estimate(E, T, R):
    """Steps 1 - 3 for one pair: the Shift record tw_ticket_shift returns."""
    E = np.asarray(E, np.uint8)
    T = np.asarray(T, np.uint8)
    colE, colT, rowE, rowT = profiles(E, T)
    dx = search(colE, colT, R)
    dy = search(rowE, rowT, R)
    sad0, n0 = sad(E, T, 0, 0)
    if (dx, dy) == (0, 0):
        return Shift(0, 0, 0, n0, n0, sad0, sad0)
    sads, ns = sad(E, T, dx, dy)
    lhs, rhs = sads * n0, (sad0 >> 1) * ns
    assert lhs <= U64 and rhs <= U64
    return Shift(dx, dy, 1 if lhs <= rhs else 0, ns, n0, sads, sad0)


def page(rng, H, W):
    """A text-like page: rows of random dark boxes on 245."""
    img = np.full((H, W), 245, np.uint8)
    y = 6
    while y < H - 14:
        lh = int(rng.integers(8, 22))
        x = int(rng.integers(4, 40))
        while x < W - 30:
            ww = int(rng.integers(6, 60))
            img[y:y + lh, x:x + ww] = rng.integers(20, 200)
            x += ww + int(rng.integers(4, 20))
        y += lh + int(rng.integers(4, 18))
    return img


def shifted_pair(rng, h, w, sx, sy, pad=100):
    """(E, T) cut from one page such that E[y][x] = T[y + sy][x + sx] wherever both exist."""
    P = page(rng, h + 2 * pad, w + 2 * pad)
    E = P[pad:pad + h, pad:pad + w].copy()
    T = P[pad - sy:pad - sy + h, pad - sx:pad - sx + w].copy()
    return E, T
