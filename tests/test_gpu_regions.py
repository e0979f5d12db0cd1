"""Hit regions on the device: tw_hit_regions, TW_OPT_REGIONS and tw_wait_regions (DESIGN.md §7 "Hit regions").

Every result is compared bit for bit with tests/regions_ref.py, a breadth-first flood fill written from the semantics.

The kernel alone goes through tw_stage_hit_regions on fields built so that chosen grid points are hits.  A hit's sample is
(+-m, 0) with m = (2048 + k % 2048) * 2^(k / 2048 - 10) for a k of its own: m * m is exact in float32 and different for every
k below 34 816, so the magnitudes are distinct wherever a tie is not the point of the case; every other grid point holds
(0.5, 0), below the threshold of 1.  Grids: 1 x 1, 40 x 1, 1 x 40; 37 x 23 at span 3 on a 110 x 68 image (the last column and
row are clipped cells); 200 x 170 at span 1 — G = 34 000 is beyond the scan's round of 32 768 points and beyond the grids
whose label plane lives in LDS, so it runs the kernel's device-memory path.

The pipeline uses the shapes and image builders of tests/test_gpu_ignore.py (97 x 61 and 333 x 41, span 4, threshold 0).
"""
import json
import os

import numpy as np
import pytest

import regions_ref as R
from test_gpu_resident import SPAN, THR, frames, shape, small, vectors  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- fields with chosen hits -------------------------------------------------------------------------------------------
def mag(k):
    return np.float32((2048 + k % 2048) * 2.0 ** (k // 2048 - 10))


def field_of(mask, span, w, h, seed=0):
    """(2, h, w): the grid points where mask [gh, gw] is set are hits with distinct magnitudes in a shuffled order"""
    gh, gw = mask.shape
    assert gw == -(-w // span) and gh == -(-h // span) and gw * gh <= 34816
    ks = np.random.default_rng(seed).permutation(gw * gh).reshape(gh, gw)
    m = np.array([mag(int(k)) for k in ks.ravel()], np.float32).reshape(gh, gw)
    m[(ks & 1) == 1] *= -1
    f = np.zeros((2, h, w), np.float32)
    f[0, ::span, ::span] = np.where(mask, m, np.float32(0.5))
    return f


def check(eng, fields, span, thr, gap, ignore=None):
    """one tw_stage_hit_regions call against the reference, pair by pair; returns the reference's records per pair"""
    fields = np.ascontiguousarray(fields, np.float32)
    npairs, _, h, w = fields.shape
    eng.launch_counts(reset=True)
    nreg, regs, rof = eng.stage_hit_regions(fields, span, thr, gap, ignore)
    cnt = eng.launch_counts()
    assert cnt["tw_hit_regions"] == 1 and cnt["tw_span_gather"] == 1 and cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1
    out = []
    for j in range(npairs):
        hits = R.hits_of_field(fields[j], span, thr, ignore[j] if ignore is not None else ())
        records, region_of = R.regions(hits, gap, span, w, h)
        assert int(nreg[j]) == len(records), (j, int(nreg[j]), len(records))
        kept = min(len(records), R.MAX_REGIONS)
        want = np.zeros(kept, regs.dtype)
        for i, rec in enumerate(records[:kept]):
            want[i] = tuple(rec)
        assert regs[j, :kept].tobytes() == want.tobytes(), (j, regs[j, :kept], want)
        assert (np.frombuffer(regs[j, kept:].tobytes(), np.uint8) == 0xFF).all(), "a record beyond the kept prefix was written"
        assert rof[j, :len(hits)].tolist() == region_of
        assert (rof[j, len(hits):] == -1).all(), "region_of was written beyond the pair's hits"
        out.append(records)
    return out


# ---- hit patterns [gh, gw] ---------------------------------------------------------------------------------------------
def boustrophedon(gh, gw):
    """every other row, joined at alternating ends: one path of about G / 2 points whose ends are G / 2 steps apart"""
    m = np.zeros((gh, gw), bool)
    m[::2] = True
    for i, y in enumerate(range(1, gh - 1, 2)):
        m[y, gw - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(gh, gw):
    """a walker that turns right whenever the cell two ahead is taken: one arm, a blank cell between its turns"""
    m = np.zeros((gh, gw), bool)
    inside = lambda y, x: 0 <= y < gh and 0 <= x < gw  # noqa: E731
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    turned = False
    while True:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = True
            turned = False
        elif turned:
            return m
        else:
            dy, dx = dx, -dy
            turned = True


def u_shape(gh, gw):
    """two arms that meet only on the last row: the smaller label has to travel back up the second arm"""
    m = np.zeros((gh, gw), bool)
    m[:, 1] = m[:, gw - 2] = True
    m[gh - 1, 1:gw - 1] = True
    return m


def ring_and_dot(gh, gw, gap):
    """a square ring whose centre holds one dot at distance gap + 1 from it: nested boxes, two regions"""
    m = np.zeros((gh, gw), bool)
    cy, cx, r = gh // 2, gw // 2, gap + 1
    m[cy - r, cx - r:cx + r + 1] = m[cy + r, cx - r:cx + r + 1] = True
    m[cy - r:cy + r + 1, cx - r] = m[cy - r:cy + r + 1, cx + r] = True
    m[cy, cx] = True
    return m


def even_points(gh, gw):
    m = np.zeros((gh, gw), bool)
    m[::2, ::2] = True
    return m


GRIDS = {  # name: (w, h, span)
    "1x1": (1, 1, 1), "40x1": (40, 1, 1), "1x40": (1, 40, 1), "37x23_span3": (110, 68, 3), "200x170": (200, 170, 1)}


def grid_of(name):
    w, h, span = GRIDS[name]
    return w, h, span, -(-h // span), -(-w // span)


@pytest.mark.parametrize("name", list(GRIDS))
def test_kernel_none_every_point_and_the_long_paths(engine, name):
    w, h, span, gh, gw = grid_of(name)
    assert (gw * gh > 32768) == (name == "200x170")
    for mask in (np.zeros((gh, gw), bool), np.ones((gh, gw), bool)):
        recs, = check(engine, field_of(mask, span, w, h)[None], span, 1.0, 1)
        assert len(recs) == int(mask.any())
        if mask.any():
            assert recs[0][:5] == (0, 0, w, h, gw * gh)  # boxes end at the image's edge, not at the cell's
    for mask in (boustrophedon(gh, gw), spiral(gh, gw)):
        recs, = check(engine, field_of(mask, span, w, h, seed=1)[None], span, 1.0, 1)
        assert len(recs) == 1 and recs[0][4] == int(mask.sum())
        if min(gh, gw) > 4:
            assert recs[0][4] > gw * gh // 3


@pytest.mark.parametrize("name", ["37x23_span3", "200x170"])
def test_kernel_u_ring_and_the_even_points(engine, name):
    w, h, span, gh, gw = grid_of(name)
    recs, = check(engine, field_of(u_shape(gh, gw), span, w, h)[None], span, 1.0, 1)
    assert len(recs) == 1
    for gap in (1, 2, 3):
        recs, = check(engine, field_of(ring_and_dot(gh, gw, gap), span, w, h)[None], span, 1.0, gap)
        assert len(recs) == 2 and recs[1][4] == 1
        (x0, y0, bw, bh), (x1, y1, cw, ch) = recs[0][:4], recs[1][:4]
        assert x0 < x1 and y0 < y1 and x1 + cw < x0 + bw and y1 + ch < y0 + bh  # the dot's box lies inside the ring's
    ev = field_of(even_points(gh, gw), span, w, h)[None]
    recs, = check(engine, ev, span, 1.0, 1)
    assert len(recs) == -(-gw // 2) * -(-gh // 2)
    # 228 regions on the small grid, just below the kept 256; 8 500 on the large one: the true count, the kept prefix
    assert len(recs) == (8500 if name == "200x170" else 228)
    recs, = check(engine, ev, span, 1.0, 2)
    assert len(recs) == 1


@pytest.mark.parametrize("gap,want", [(1, 2), (2, 2), (3, 1), (8, 1)])
def test_kernel_two_blobs_three_steps_apart(engine, gap, want):
    w, h, span, gh, gw = grid_of("37x23_span3")
    m = np.zeros((gh, gw), bool)
    m[5:9, 4:8] = True
    m[6:12, 10:13] = True  # columns 7 and 10: three steps
    recs, = check(engine, field_of(m, span, w, h)[None], span, 1.0, gap)
    assert len(recs) == want


def test_kernel_peak_tie_infinity_and_the_threshold_itself(engine):
    w, h, span, gh, gw = grid_of("37x23_span3")
    f = np.zeros((2, h, w), np.float32)

    def put(gx, gy, dx, dy):
        f[0, gy * span, gx * span], f[1, gy * span, gx * span] = dx, dy

    # a region of three with len 25, 25, 16: the first of the two ties is the peak
    put(3, 2, 0.0, 4.0), put(4, 2, 3.0, 4.0), put(5, 2, -5.0, 0.0)
    # a region with an infinite sample, and one whose len overflows to infinity in front of it
    put(20, 10, 1e30, 1.0), put(21, 10, np.inf, 0.0), put(22, 10, 7.0, 7.0)
    # len == threshold * threshold exactly is no hit: (3, 4) at threshold 5 — it would join the two hits next to it
    recs, = check(engine, f[None], span, 2.0, 1)
    assert len(recs) == 2
    assert recs[0][4:7] == (3, 4 * span, 2 * span) and recs[1][4:7] == (3, 20 * span, 10 * span)
    g = np.zeros((2, h, w), np.float32)
    g[0, 0, 0], g[0, 0, span], g[1, 0, span], g[0, 0, 2 * span] = 6.0, 3.0, 4.0, 6.0
    recs, = check(engine, g[None], span, 5.0, 1)
    assert len(recs) == 2 and recs[0][4] == 1 and recs[1][4] == 1
    recs, = check(engine, g[None], span, 4.999, 1)
    assert len(recs) == 1 and recs[0][4] == 3


def test_kernel_ignore_band_cuts_or_is_bridged(engine):
    w, h, span, gh, gw = grid_of("37x23_span3")
    m = np.zeros((gh, gw), bool)
    m[7, 2:30] = True  # a stripe
    f = field_of(m, span, w, h)[None]
    wide, narrow = (15 * span, 0, 2 * span, h), (15 * span, 0, span, h)  # grid columns 15-16, and column 15 alone
    assert len(check(engine, f, span, 1.0, 2)[0]) == 1
    recs, = check(engine, f, span, 1.0, 2, [[wide]])  # columns 14 and 17: three steps apart
    assert len(recs) == 2 and recs[0][4] + recs[1][4] == 28 - 2
    recs, = check(engine, f, span, 1.0, 2, [[narrow]])  # columns 14 and 16: bridged at gap 2
    assert len(recs) == 1 and recs[0][4] == 28 - 1
    recs, = check(engine, f, span, 1.0, 1, [[narrow]])
    assert len(recs) == 2
    # clipped and empty rectangles, and all 32 of them
    many = [(-5, 7 * span, 4 * span, 1), (w - 2, 0, 50, h), (w, 0, 3, 3), (5, 5, 0, 9)] + [(i * span, 7 * span, 1, 1) for i in range(3, 31)]
    assert len(many) == 32
    check(engine, f, span, 1.0, 1, [many])


@pytest.mark.parametrize("name", ["37x23_span3", "200x170"])
def test_kernel_three_pairs_do_not_leak_into_each_other(engine, name):
    """a component at the end of pair z's grid and one at the start of pair z + 1's; different rectangles per pair"""
    w, h, span, gh, gw = grid_of(name)
    masks = []
    for z in range(3):
        m = np.zeros((gh, gw), bool)
        m[gh - 2:, gw - 3:] = True
        m[:2, :3] = True
        m[gh // 2, 2 + z:gw - 2] = True
        masks.append(m)
    fields = np.stack([field_of(m, span, w, h, seed=z) for z, m in enumerate(masks)])
    ign = [[((gw // 2) * span, 0, 2 * span, h)], [], [(0, 0, 3 * span, 2 * span), ((gw // 3) * span, (gh // 2) * span, span, span)]]
    recs = check(engine, fields, span, 1.0, 1, ign)
    assert [len(r) for r in recs] == [4, 3, 3]
    check(engine, fields, span, 1.0, 1)


def test_stage_call_refuses_bad_arguments(twflow, engine):
    f = np.zeros((1, 2, 8, 8), np.float32)
    for gap in (0, 9, -1):
        with pytest.raises(twflow.TwError) as ei:
            engine.stage_hit_regions(f, 1, 1.0, gap)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER
    with pytest.raises(twflow.TwError):
        engine.stage_hit_regions(f, 1, 1.0, 1, [[(0, 0, -1, 2)]])


# ---- the pipeline ------------------------------------------------------------------------------------------------------
def clip_out(vecs, rects, w, h):
    cl = [(max(x, 0), max(y, 0), min(x + rw, w), min(y + rh, h)) for x, y, rw, rh in rects]
    return [v for v in vecs if not any(x0 <= v[0] < x1 and y0 <= v[1] < y1 for x0, y0, x1, y1 in cl)]


def check_wait(e, ticket, want_vecs, gap, span, w, h, cap=None):
    """tw_wait_regions of a ticket against the reference over the expected vectors"""
    status, vecs, rof, regs, nreg = e.wait_regions(ticket, cap=cap)
    records, region_of = R.regions(want_vecs, gap, span, w, h)
    m = len(want_vecs) if cap is None else min(cap, len(want_vecs))
    assert vecs == want_vecs[:m] and status == ("SUSPICIOUS" if want_vecs else "OK")
    assert nreg == len(records) and rof == region_of[:m]
    assert len(regs) == min(len(records), R.MAX_REGIONS)
    for got, want in zip(regs, records):
        assert R.same_record(got, want), (got, want)
    return records


def test_batch_with_and_without_rectangles(twflow, shape):
    w, h, _ = shape
    f0, f1, f2, f3 = frames(w, h)
    pairs = [(f0, f1), (f1, f2), (f2, f3), (f0, f0)]
    ign = [[], [(w // 3 + 1, h // 4 + 1, w // 3, h // 2), (w - 9, -3, 20, 11)], [], []]
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        e.launch_counts(reset=True)
        plain = [vectors(e, e.submit(a, b, SPAN, THR, ignore=r))[1] for (a, b), r in zip(pairs, ign)]
        off = e.launch_counts(reset=True)
        assert off["tw_hit_regions"] == 0
        assert plain[1] == clip_out(plain[1], ign[1], w, h) and len(plain[1]) > 0
        e.set_regions(1)
        tks = [e.submit(a, b, SPAN, THR, ignore=r) for (a, b), r in zip(pairs, ign)]
        recs = [check_wait(e, t, v, 1, SPAN, w, h) for t, v in zip(tks, plain)]
        on = e.launch_counts(reset=True)
        assert on["tw_hit_regions"] == 1  # one batch, one launch behind its one scan
        assert on["tw_span_scan"] + on["tw_span_scan_seg"] == 1
        assert any(len(r) > 0 for r in recs)
        # plain tw_wait on a regions batch works as before
        tks = [e.submit(a, b, SPAN, THR, ignore=r) for (a, b), r in zip(pairs, ign)]
        assert [vectors(e, t)[1] for t in tks] == plain
        # a wider gap on the same pairs
        e.set_regions(3)
        tks = [e.submit(a, b, SPAN, THR, ignore=r) for (a, b), r in zip(pairs, ign)]
        for t, v in zip(tks, plain):
            check_wait(e, t, v, 3, SPAN, w, h)
        # off again: the launches of the first round, and nothing of tw_hit_regions
        e.set_regions(0)
        e.launch_counts(reset=True)
        assert [vectors(e, e.submit(a, b, SPAN, THR, ignore=r))[1] for (a, b), r in zip(pairs, ign)] == plain
        again = e.launch_counts()
        assert dict(again) == dict(off)


def test_two_lanes(twflow, small, monkeypatch):
    monkeypatch.setenv("TW_LANES", "2")
    w, h = small
    f0, f1, f2, f3 = frames(w, h)
    pairs = [(f0, f1), (f1, f2), (f2, f3), (f3, f0)]
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        plain = [vectors(e, e.submit(a, b, SPAN, THR))[1] for a, b in pairs]
        e.set_regions(2)
        e.launch_counts(reset=True)
        tks = [e.submit(a, b, SPAN, THR) for a, b in pairs]
        for t, v in zip(tks, plain):
            check_wait(e, t, v, 2, SPAN, w, h)
        cnt = e.launch_counts()
        assert cnt["tw_hit_regions"] == cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] >= 1


def test_single_pair_schedule(twflow, monkeypatch):
    import synth
    monkeypatch.setenv("TW_LATENCY_MIN_PX", "0")
    h, w = 240, 320
    a, b = (np.ascontiguousarray(x) for x in synth.make_pair(5, h, w))
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        plain = vectors(e, e.submit(a, b, SPAN, 1.0))[1]
        assert len(plain) > 0
        e.set_regions(1)
        e.launch_counts(reset=True)
        check_wait(e, e.submit(a, b, SPAN, 1.0), plain, 1, SPAN, w, h)
        cnt = e.launch_counts()
        assert cnt["tw_pair_same"] == 0, cnt  # a single-pair schedule ran
        assert cnt["tw_span_scan_seg"] == 1 and cnt["tw_hit_regions"] == 1


def test_more_hits_than_the_eager_copy_holds_and_a_small_cap(twflow):
    import synth
    w, h = 180, 117
    a, b = (np.ascontiguousarray(x) for x in synth.make_pair(0, h, w))
    rects = [(40, 30, 60, 40)]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        plain = vectors(e, e.submit(a, b, 2, THR, ignore=rects))[1]
        assert len(plain) > 1024
        e.set_regions(1)
        check_wait(e, e.submit(a, b, 2, THR, ignore=rects), plain, 1, 2, w, h)
        check_wait(e, e.submit(a, b, 2, THR, ignore=rects), plain, 1, 2, w, h, cap=7)
        check_wait(e, e.submit(a, b, 2, THR, ignore=rects), plain, 1, 2, w, h, cap=1500)
        status, vecs, rof, regs, nreg = e.wait_regions(e.submit(a, b, 2, THR), region_cap=1)
        assert len(regs) == min(nreg, 1)


def test_device_pair(twflow, small):
    w, h = small
    f0, f1, _, _ = frames(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        plain = vectors(e, e.submit(f0, f1, SPAN, THR))[1]
        e.set_regions(1)
        da, db = e.upload(f0), e.upload(f1)
        e.launch_counts(reset=True)
        check_wait(e, e.submit_dev(da, db, w, h, w, SPAN, THR), plain, 1, SPAN, w, h)
        assert e.launch_counts()["tw_hit_regions"] == 1
        # span 0: no scan, no hits, no regions
        status, vecs, rof, regs, nreg = e.wait_regions(e.submit(f0, f1, 0, THR))
        assert (status, vecs, rof, regs, nreg) == ("OK", [], [], [], 0)


def test_option_off_refuses_and_leaves_the_ticket_waitable(twflow, small):
    w, h = small
    f0, f1, _, _ = frames(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        for bad in (-1, 9, 100):
            with pytest.raises(twflow.TwError) as ei:
                e.set_regions(bad)
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        e.launch_counts(reset=True)
        tk = e.submit(f0, f1, SPAN, THR)
        with pytest.raises(twflow.TwError) as ei:
            e.wait_regions(tk)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        plain = vectors(e, tk)[1]  # still waitable
        assert len(plain) > 0 and e.launch_counts()["tw_hit_regions"] == 0


def test_changing_the_option_does_not_change_an_open_batch(twflow, small):
    w, h = small
    f0, f1, f2, _ = frames(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        p01, p12 = vectors(e, e.submit(f0, f1, SPAN, THR))[1], vectors(e, e.submit(f1, f2, SPAN, THR))[1]
        e.set_regions(1)
        t0 = e.submit(f0, f1, SPAN, THR)  # opens a batch at gap 1
        e.set_regions(4)
        t1 = e.submit(f1, f2, SPAN, THR)  # joins it
        e.set_regions(0)
        t2 = e.submit(f0, f1, SPAN, THR)
        check_wait(e, t0, p01, 1, SPAN, w, h)
        check_wait(e, t1, p12, 1, SPAN, w, h)
        check_wait(e, t2, p01, 1, SPAN, w, h)
        t3 = e.submit(f0, f1, SPAN, THR)  # a new batch: off
        with pytest.raises(twflow.TwError):
            e.wait_regions(t3)
        assert vectors(e, t3)[1] == p01


def test_golden_pair(twflow, golden):
    case = next(c for c in golden.values() if c["expect_img"].shape == (117, 180) and len(c["vector"]) == 24)
    with open(os.path.join(GOLDEN, "regions_golden.json")) as f:
        fix = json.load(f)
    a, b = np.ascontiguousarray(case["expect_img"]), np.ascontiguousarray(case["target_img"])
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_regions(fix["gap"])
        status, vecs, rof, regs, nreg = e.wait_regions(e.submit(a, b, case["span"], float(case["threshold"])))
    assert vecs == [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    assert nreg == len(fix["regions"]) < 10 and rof == fix["region_of"]
    got = [dict(x=r[0], y=r[1], width=r[2], height=r[3], count=r[4], peak=dict(x=r[5], y=r[6], dx=float(r[7]), dy=float(r[8])))
           for r in regs]
    assert got == fix["regions"]
