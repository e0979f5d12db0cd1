"""The residual (TW_OPT_RESIDUAL) in numpy, written from the semantics in include/twflow.h and from nothing else: which
differing pixels of a pair does its flow field not explain?  All integer after one float32 -> int conversion per flow
component.  The reference of tests/test_gpu_residual.py; tests/test_residual_ref.py checks it by hand-worked cases."""
import numpy as np


def quantise(d):
    """q(d): 0 for NaN, else round-half-even of min(max(d, -16384), 16384) * 32 — in float32, where the product is exact."""
    d = np.asarray(d, np.float32)
    nan = np.isnan(d)
    c = np.minimum(np.maximum(np.where(nan, np.float32(0), d), np.float32(-16384)), np.float32(16384)) * np.float32(32)
    assert c.dtype == np.float32
    return np.where(nan, 0, np.rint(c)).astype(np.int64)  # (np.rint rounds half to even)


def warp(T, fx, fy):
    """v: the target sampled at each pixel's flow end, 1/32-pixel positions, clamped to the image, rounded as the header says."""
    T = np.asarray(T, np.uint8).astype(np.int64)
    h, w = T.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    sx = np.clip(32 * xs + quantise(fx), 0, 32 * (w - 1))
    sy = np.clip(32 * ys + quantise(fy), 0, 32 * (h - 1))
    ix, ax = sx >> 5, sx & 31
    iy, ay = sy >> 5, sy & 31
    x1 = np.minimum(ix + 1, w - 1)
    y1 = np.minimum(iy + 1, h - 1)
    return (T[iy, ix] * (32 - ax) * (32 - ay) + T[iy, x1] * ax * (32 - ay) + T[y1, ix] * (32 - ax) * ay + T[y1, x1] * ax * ay
            + 512) >> 10


def pixels(E, T, fx, fy):
    """(diff, u) per pixel."""
    Ei = np.asarray(E, np.uint8).astype(np.int64)
    Ti = np.asarray(T, np.uint8).astype(np.int64)
    diff = np.abs(Ei - Ti)
    return diff, np.minimum(diff, np.abs(Ei - warp(T, fx, fy)))


def cells(E, T, fx, fy, span, tol):
    """[gh, gw, 4] int64: n_diff, n_unexplained, max_diff, max_unexplained of every cell of the span grid."""
    diff, u = pixels(E, T, fx, fy)
    h, w = diff.shape
    gh, gw = -(-h // span), -(-w // span)
    out = np.zeros((gh, gw, 4), np.int64)
    for gy in range(gh):
        for gx in range(gw):
            d = diff[gy * span:min((gy + 1) * span, h), gx * span:min((gx + 1) * span, w)]
            q = u[gy * span:min((gy + 1) * span, h), gx * span:min((gx + 1) * span, w)]
            out[gy, gx] = (int((d > tol).sum()), int((q > tol).sum()), int(d.max()), int(q.max()))
    return out


def cells_of(diff, u, span, tol):
    """The cells of per-pixel (diff, u) without a Python loop over cells (large grids)."""
    h, w = diff.shape
    gh, gw = -(-h // span), -(-w // span)
    idx = ((np.arange(h) // span)[:, None] * gw + (np.arange(w) // span)[None, :]).ravel()
    out = np.zeros((gh * gw, 4), np.int64)
    out[:, 0] = np.bincount(idx, (diff > tol).ravel(), gh * gw)
    out[:, 1] = np.bincount(idx, (u > tol).ravel(), gh * gw)
    np.maximum.at(out[:, 2], idx, diff.ravel())
    np.maximum.at(out[:, 3], idx, u.ravel())
    return out.reshape(gh, gw, 4)


def cells_fast(E, T, fx, fy, span, tol):
    """cells() by cells_of; the tests hold the two against each other."""
    diff, u = pixels(E, T, fx, fy)
    return cells_of(diff, u, span, tol)


def records(cell, span):
    """[n, 6] int64: x, y and the four values of every cell with n_diff >= 1, in row-major order."""
    gy, gx = np.nonzero(cell[..., 0] >= 1)  # (np.nonzero walks in row-major order)
    return np.concatenate([gx[:, None] * span, gy[:, None] * span, cell[gy, gx]], axis=1).astype(np.int64)


def changes(cell, span, ignore=()):
    """The reported records (x, y, n_diff, n_unexplained, max_diff, max_unexplained) as tuples: records() minus the cells
    whose grid point lies in one of the (clipped) rectangles (x, y, width, height)."""
    return [tuple(int(v) for v in r) for r in records(cell, span)
            if not any(rx <= r[0] < rx + rw and ry <= r[1] < ry + rh for rx, ry, rw, rh in ignore)]


def residual_ref(E, T, flow, span, tol, ignore=()):
    """flow = (fx, fy) as oracle.farneback returns it.  (cells [gh, gw, 4], records)."""
    c = cells_fast(E, T, flow[0], flow[1], span, tol)
    return c, changes(c, span, ignore)
