"""The shift bands (TW_OPT_SHIFT_BANDS) restated in plain numpy from the definition in include/twflow.h, on top of
tests/shift_ref.py: the row signatures at the pair's global dx, the per-band search with its overlap rule, the acceptance check
on the pixels, the start field.  Everything is integer (Python ints where 64 bits matter), so the kernels, the stub and this
file agree value for value.  Also the generator of pages with an inserted block."""
import collections

import numpy as np

import shift_ref

Band = collections.namedtuple("Band", "y rows dy applied n_shift n_zero sad_shift sad_zero")
U64 = shift_ref.U64


def columns(w, dx):
    """(xa, xb, nblk): the overlap's columns of E at the global dx, and the signature blocks per row."""
    xa, xb = max(0, -dx), min(w, w - dx)
    return xa, xb, (xb - xa + 63) // 64


def signatures(E, T, dx):
    """(sigE, sigT), each (h, nblk) uint16: sums over blocks of 64 columns of E[y][x] and T[y][x + dx], x in [xa, xb)."""
    E = np.asarray(E, np.uint8)
    T = np.asarray(T, np.uint8)
    h, w = E.shape
    xa, xb, nblk = columns(w, dx)
    sE = np.zeros((h, nblk), np.uint16)
    sT = np.zeros((h, nblk), np.uint16)
    for k in range(nblk):
        x0, x1 = xa + 64 * k, min(xa + 64 * (k + 1), xb)
        sE[:, k] = E[:, x0:x1].sum(axis=1, dtype=np.uint32)
        sT[:, k] = T[:, x0 + dx:x1 + dx].sum(axis=1, dtype=np.uint32)
    return sE, sT


def band_rows(h, B):
    """[(y, rows)] of the nb = ceil(h / B) bands."""
    return [(y, min(B, h - y)) for y in range(0, h, B)]


def overlap(y, rows, h, d):
    """(lo, hi) of candidate d for the band [y, y + rows)."""
    return max(y, -d), min(y + rows, h - d)


def band_cost(sE, sT, y, rows, d):
    h = sE.shape[0]
    lo, hi = overlap(y, rows, h, d)
    if hi <= lo:
        return 0
    return int(np.abs(sE[lo:hi].astype(np.int64) - sT[lo + d:hi + d].astype(np.int64)).sum())


def search_band(sE, sT, y, rows, R):
    """The band's dy: the least cost per row among the eligible candidates, the earliest in visit order among equals."""
    h = sE.shape[0]
    r = min(int(R), h // 2)
    need = (rows + 1) // 2
    best = None
    for d in shift_ref.visit_order(r):
        lo, hi = overlap(y, rows, h, d)
        n = hi - lo
        if d != 0 and n < need:
            continue
        c = band_cost(sE, sT, y, rows, d)
        if best is None:
            best = (d, c, n)
            continue
        lhs, rhs = c * best[2], best[1] * n
        assert lhs <= U64 and rhs <= U64
        if lhs < rhs:
            best = (d, c, n)
    return best[0]


def accept(E, T, dx, y, rows, dy):
    """The band's record from its search answer."""
    h, w = E.shape
    sad0 = int(np.abs(E[y:y + rows].astype(np.int64) - T[y:y + rows].astype(np.int64)).sum())
    n0 = rows * w
    if (dx, dy) == (0, 0):
        return Band(y, rows, 0, 0, n0, n0, sad0, sad0)
    xa, xb, _ = columns(w, dx)
    lo, hi = overlap(y, rows, h, dy)
    a = E[lo:hi, xa:xb].astype(np.int64)
    b = T[lo + dy:hi + dy, xa + dx:xb + dx].astype(np.int64)
    sads, ns = int(np.abs(a - b).sum()), (hi - lo) * (xb - xa)
    lhs, rhs = sads * n0, (sad0 >> 2) * ns
    assert lhs <= U64 and rhs <= U64
    return Band(y, rows, dy, 1 if lhs <= rhs else 0, ns, n0, sads, sad0)


def estimate(E, T, R, B, own_field=False):
    """(the pair's global Shift record, [Band] per band).  own_field: the pair has a tw_flow_in of its own — measured, never
    applied."""
    E = np.asarray(E, np.uint8)
    T = np.asarray(T, np.uint8)
    assert B >= 32 and B <= 1024 and B % 16 == 0
    g = shift_ref.estimate(E, T, R)
    if own_field:
        g = g._replace(applied=0)
    sE, sT = signatures(E, T, g.dx)
    out = []
    for y, rows in band_rows(E.shape[0], B):
        rec = accept(E, T, g.dx, y, rows, search_band(sE, sT, y, rows, R))
        out.append(rec._replace(applied=0) if own_field else rec)
    return g, out


def field(shape, dx, bands):
    """The full-resolution start field F (h, w, 2) float32 of the band records."""
    h, w = shape
    F = np.zeros((h, w, 2), np.float32)
    for b in bands:
        b = Band(*b)
        if b.applied:
            F[b.y:b.y + b.rows, :, 0] = np.float32(dx)
            F[b.y:b.y + b.rows, :, 1] = np.float32(b.dy)
    return F


def inserted_pair(rng, h, w, at, ins, sx=0, pad=100):
    """(E, T): T is E's page moved by sx columns with `ins` foreign rows inserted at row `at`; what was at row y >= at of the
    moved page is at row y + ins of T, the rows pushed past h are lost."""
    P = shift_ref.page(rng, h + 2 * pad, w + 2 * pad)
    E = P[pad:pad + h, pad:pad + w].copy()
    Tb = P[pad:pad + h, pad - sx:pad - sx + w]
    ban = shift_ref.page(rng, ins + 40, w + 2 * pad)[20:20 + ins, pad:pad + w]
    T = np.concatenate([Tb[:at], ban, Tb[at:]])[:h].copy()
    return E, T
