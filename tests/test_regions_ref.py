"""tests/regions_ref.py, the reference of the hit-region tests, against an implementation it shares nothing with:
scipy.ndimage.label with a 3 x 3 structure is 8-connectivity, which is gap 1.  CPU only."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage  # (a plain import: without scipy the reference's independent check fails, it does not skip)

import regions_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hits_of_mask(mask, span, rng):
    gh, gw = mask.shape
    return [(int(x) * span, int(y) * span, np.float32(rng.normal() * 10 + 20), np.float32(rng.normal()))
            for y, x in zip(*np.nonzero(mask))]


@pytest.mark.parametrize("gh,gw,density", [(1, 1, 1.0), (1, 30, 0.5), (30, 1, 0.5), (23, 37, 0.2), (23, 37, 0.45), (40, 40, 0.6),
                                            (17, 19, 0.0), (17, 19, 1.0)])
def test_gap_one_is_scipy_label_with_a_full_structure(gh, gw, density):
    rng = np.random.default_rng(gh * 100 + gw)
    span = 3
    w, h = gw * span - 1, gh * span - 2 if gh * span > 2 else gh * span  # the last column (and row) of cells is clipped
    for _ in range(5):
        mask = rng.random((gh, gw)) < density
        hits = hits_of_mask(mask, span, rng)
        records, region_of = R.regions(hits, 1, span, w, h)
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
        assert n == len(records)
        # scipy numbers components by their first pixel in row-major order too: the same partition, the same order
        assert [int(lab[y // span, x // span]) - 1 for x, y, _, _ in hits] == region_of
        for k, obj in enumerate(ndimage.find_objects(lab)):
            ys, xs = obj
            x, y, bw, bh, count = records[k][:5]
            assert (x, y) == (xs.start * span, ys.start * span)
            assert (x + bw, y + bh) == (min(xs.stop * span, w), min(ys.stop * span, h))
            assert count == int((lab == k + 1).sum())
            members = [i for i, r in enumerate(region_of) if r == k]
            lens = [R.flen(hits[i][2], hits[i][3]) for i in members]
            peak = members[int(np.argmax(lens))]  # (argmax: the first among equal values)
            assert records[k][5:7] == (hits[peak][0], hits[peak][1])
            assert records[k][7] == hits[peak][2] and records[k][8] == hits[peak][3]


def test_a_wider_gap_against_a_brute_force_union_of_all_pairs():
    rng = np.random.default_rng(7)
    for gap in (2, 3, 8):
        mask = rng.random((31, 45)) < 0.04
        hits = hits_of_mask(mask, 1, rng)
        records, region_of = R.regions(hits, gap, 1, 45, 31)
        parent = list(range(len(hits)))

        def find(i):
            while parent[i] != i:
                i = parent[i]
            return i
        for i in range(len(hits)):
            for j in range(i):
                if abs(hits[i][0] - hits[j][0]) <= gap and abs(hits[i][1] - hits[j][1]) <= gap:
                    parent[find(i)] = find(j)
        roots = [find(i) for i in range(len(hits))]
        order = []
        for r in roots:
            if r not in order:
                order.append(r)
        assert region_of == [order.index(r) for r in roots] and len(records) == len(order)


def test_tie_clipping_and_the_golden_fixture():
    recs, of = R.regions([(0, 0, 3.0, 4.0), (4, 0, 5.0, 0.0), (8, 0, -5.0, 0.0), (20, 4, np.inf, 0.0)], 1, 4, 22, 6)
    assert of == [0, 0, 0, 1]
    assert recs[0][:7] == (0, 0, 12, 4, 3, 0, 0) and recs[1][:7] == (20, 4, 2, 2, 1, 20, 4)  # the first of equal len; clipped boxes
    with open(os.path.join(GOLDEN, "expected_responses.json")) as f:
        case = next(c for c in json.load(f).values() if len(c["vector"]) == 24)
    with open(os.path.join(GOLDEN, "regions_golden.json")) as f:
        fix = json.load(f)
    hits = [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    recs, of = R.regions(hits, fix["gap"], case["span"], case["width"], case["height"])
    assert 0 < len(recs) < 10 and of == fix["region_of"]
    assert [dict(x=r[0], y=r[1], width=r[2], height=r[3], count=r[4], peak=dict(x=r[5], y=r[6], dx=float(r[7]), dy=float(r[8])))
            for r in recs] == fix["regions"]
