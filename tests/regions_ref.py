"""Independent reference for hit regions (include/twflow.h, TW_OPT_REGIONS): a breadth-first flood fill in plain Python /
numpy, written from the semantics alone — no union-find, no labels, nothing the device kernel does.

A pair's hits are grid points (x, y multiples of span) with their samples (dx, dy).  Two hits are adjacent when their grid
coordinates differ by at most `gap` in x and in y; a region is a connected component.  Regions are ordered by their first
hit in row-major order (y, then x).  A region's record is the tuple
    (x, y, width, height, count, peak_x, peak_y, peak_dx, peak_dy)
with x, y the smallest hit coordinates, width = min(max hit x + span, image width) - x (height likewise), and the peak the
hit with the largest float32 len = dx * dx + dy * dy (each product and the sum rounded to float32, as the scan computes it),
the first in row-major order among equal len.
"""
import collections

import numpy as np

MAX_REGIONS = 256


def flen(dx, dy):
    """The scan's len: float32 products, float32 sum (no fused multiply-add)."""
    dx, dy = np.float32(dx), np.float32(dy)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float32(dx * dx) + np.float32(dy * dy))


def regions(hits, gap, span, width, height):
    """hits: [(x, y, dx, dy)] in row-major order.  Returns (records, region_of): every region's record in order (ALL of
    them: the caller cuts at MAX_REGIONS) and, parallel to hits, the index of each hit's region."""
    assert 1 <= gap <= 8 and span >= 1
    cell = {}
    for i, (x, y, _, _) in enumerate(hits):
        assert x % span == 0 and y % span == 0 and (x // span, y // span) not in cell
        cell[(x // span, y // span)] = i
    assert [(h[1], h[0]) for h in hits] == sorted((h[1], h[0]) for h in hits), "hits must be row-major"
    region_of = [-1] * len(hits)
    records = []
    for start in range(len(hits)):
        if region_of[start] >= 0:
            continue
        r = len(records)
        region_of[start] = r
        members = []
        queue = collections.deque([start])
        while queue:
            i = queue.popleft()
            members.append(i)
            gx, gy = hits[i][0] // span, hits[i][1] // span
            for ny in range(gy - gap, gy + gap + 1):
                for nx in range(gx - gap, gx + gap + 1):
                    k = cell.get((nx, ny))
                    if k is not None and region_of[k] < 0:
                        region_of[k] = r
                        queue.append(k)
        members.sort()  # row-major order = the order of hits
        xs = [hits[i][0] for i in members]
        ys = [hits[i][1] for i in members]
        peak = members[0]
        for i in members[1:]:
            if flen(hits[i][2], hits[i][3]) > flen(hits[peak][2], hits[peak][3]):
                peak = i
        x0, y0 = min(xs), min(ys)
        records.append((x0, y0, min(max(xs) + span, width) - x0, min(max(ys) + span, height) - y0, len(members),
                        hits[peak][0], hits[peak][1], np.float32(hits[peak][2]), np.float32(hits[peak][3])))
    return records, region_of


def hits_of_field(field, span, threshold, rects=()):
    """The hits of one dense field (2, h, w) as the scan plus the ignore filter report them: grid points with
    (double)len > threshold * threshold, minus the points inside a rectangle (x, y, w, h) clipped to the image; row-major."""
    _, h, w = field.shape
    clipped = []
    for (x, y, rw, rh) in rects:
        x0, x1 = max(x, 0), min(x + rw, w)
        y0, y1 = max(y, 0), min(y + rh, h)
        if x0 < x1 and y0 < y1:
            clipped.append((x0, y0, x1, y1))
    thr2 = float(threshold) * float(threshold)
    sub = np.asarray(field, np.float32)[:, ::span, ::span]
    with np.errstate(over="ignore", invalid="ignore"):
        ln = (sub[0] * sub[0]) + (sub[1] * sub[1])  # float32 products, float32 sum
    assert ln.dtype == np.float32
    out = []
    for gy, gx in zip(*np.nonzero(ln.astype(np.float64) > thr2)):  # (np.nonzero is row-major)
        x, y = int(gx) * span, int(gy) * span
        if any(x0 <= x < x1 and y0 <= y < y1 for (x0, y0, x1, y1) in clipped):
            continue
        out.append((x, y, sub[0, gy, gx], sub[1, gy, gx]))
    return out


def same_record(a, b):
    """Bit for bit: the integers equal, the floats' bit patterns equal."""
    return (tuple(int(v) for v in a[:7]) == tuple(int(v) for v in b[:7]) and
            np.float32(a[7]).tobytes() == np.float32(b[7]).tobytes() and
            np.float32(a[8]).tobytes() == np.float32(b[8]).tobytes())
