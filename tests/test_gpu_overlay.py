"""The diff image on the device (tw_ticket_hits, tw_ticket_overlay; kernels tw_overlay_base, tw_overlay_marks).
Part 1: the kernels alone (tw_stage_overlay) against tests/overlay_ref.py, byte for byte, the bytes behind every row untouched.
Part 2: batches of every kind against overlay_ref on the oracle's vectors, to device, page-locked and pageable destinations.
Part 3: a batch without an overlay call launches, holds and records what it did before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as R  # noqa: E402
import regions_ref  # noqa: E402
from test_gpu_ignore import edit, outside  # noqa: E402
from test_gpu_resident import as_jpeg, as_rgba  # noqa: E402

pytestmark = pytest.mark.gpu
HOST_RECS = 1024
FILL = 0xA5
NAN, INF = float("nan"), float("inf")
SPECIAL = [NAN, INF, -INF, 1024.0, -1024.0, 1024.5, -1024.5, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5]
SIZES = [(1, 1, None), (7, 5, None), (33, 17, None), (64, 64, None), (130, 67, 136), (397, 99, None)]


# ---- part 1: the kernels alone ------------------------------------------------------------------------------------------------
def pitches(w):
    return [3 * w, 3 * w + 1, 3 * w + 5, (3 * w // 4 + 1) * 4]


def rects32(w, h, rng):
    """32 rectangles as a caller hands them over: inside, across every border, empty, outside"""
    rs = [(-3, -2, 6, 5), (w - 2, h - 2, 9, 9), (w // 2, -5, 3, 7), (-4, h // 2, 6, 2), (w + 3, 0, 4, 4), (2, 2, 0, 5)]
    while len(rs) < 32:
        rs.append((int(rng.integers(-2, w)), int(rng.integers(-2, h)), int(rng.integers(1, max(2, w // 6))),
                   int(rng.integers(1, max(2, h // 6)))))
    return rs


def grid_hits(w, h, span):
    """one hit per grid point, its components cycling through SPECIAL (dx and dy at different phases)"""
    hits, k = [], 0
    for y in range(0, h, span):
        for x in range(0, w, span):
            hits.append((x, y, np.float32(SPECIAL[k % 13]), np.float32(SPECIAL[(k // 13 + 3 * k + 5) % 13])))
            k += 1
    return hits


def border_hits(w, h):
    """hits on all four borders and in the corners, pointing out of and into the image"""
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]
    ds = [(-3.0, -2.0), (4.0, -1.5), (-2.5, 3.0), (5.0, 6.0), (0.5, -7.0), (1.0, 9.0), (-8.0, 0.0), (2.5, 2.5)]
    return [(x, y, np.float32(dx), np.float32(dy)) for (x, y), (dx, dy) in zip(pts, ds)]


def boxes(w, h, n, rng):
    """n region boxes inside the image: thin ones, ones on the border, nested and overlapping ones"""
    bs = [(0, 0, w, h), (0, 0, 1, h), (0, h - 1, w, 1), (w // 2, h // 2, 1, 1), (w // 4, h // 4, max(1, w // 2), max(1, h // 2))]
    while len(bs) < n:
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        bs.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    return bs[:n]


_VARIANTS = {}


def variant(w, h, v):
    """(E, T, rects as handed over, hits as recorded, boxes, tol, expected picture): computed once per size and variant"""
    key = (w, h, v)
    if key not in _VARIANTS:
        rng = np.random.default_rng(1000 * w + 10 * h + v)
        span = 10 if w * h > 2000 else 2 if w * h > 1 else 1
        yy, xx = np.mgrid[0:h, 0:w]
        if v == 0:    # random bytes; a hit per grid point; 32 rectangles; the most boxes; tol 16
            E, T = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
            rs, hits, bs, tol = rects32(w, h, rng), grid_hits(w, h, span), boxes(w, h, 256, rng), 16
        elif v == 1:  # a checkerboard against its inverse; hits on the borders; no rectangle; one box; tol 255
            E = (((xx + yy) & 1) * 255).astype(np.uint8)
            T = 255 - E
            rs, hits, bs, tol = [], border_hits(w, h), boxes(w, h, 1, rng), 255
        else:         # an identical pair; no hit; no rectangle; no box; tol 0
            E = rng.integers(0, 256, (h, w), dtype=np.uint8)
            T = E.copy()
            rs, hits, bs, tol = [], [], [], 0
        cl = R.clip_rects(rs, w, h)
        want = R.overlay_ref(E, T, cl, R.outside(hits, cl), bs, tol)
        _VARIANTS[key] = (E, T, rs, hits, bs, tol, want)
    return _VARIANTS[key]


@pytest.mark.parametrize("w,h,stride", SIZES, ids=["%dx%d" % s[:2] for s in SIZES])
def test_stage_equals_the_reference_at_every_pitch_and_alignment(engine, w, h, stride):
    paths = set()
    k = 0
    for mis in (0, 1, 2, 3):
        for pitch in pitches(w):
            if mis >= 2 and pitch != 3 * w + 5 and pitch != (3 * w // 4 + 1) * 4:
                continue
            E, T, rs, hits, bs, tol, want = variant(w, h, k % 3)
            k += 1
            engine.launch_counts(reset=True)
            buf, path = engine.stage_overlay(E, T, rs, hits, bs, tol, pitch=pitch, stride=stride, misalign=mis, fill=FILL)
            cnt = engine.launch_counts(reset=True)
            what = "%dx%d pitch %d misalign %d variant %d" % (w, h, pitch, mis, (k - 1) % 3)
            assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want), what
            assert (buf[:, 3 * w:] == FILL).all(), what + ": a byte behind a row was written"
            # the path is the pure function's answer for such addresses (the device images sit `mis` bytes off a 256-byte boundary)
            st = stride if stride else w
            assert path == engine.overlay_plan(256 + mis, 512 + mis, st, 1024, pitch, w, h)[0], what
            assert path == int(mis == 0 and st % 4 == 0 and pitch % 4 == 0), what
            paths.add(path)
            assert cnt["tw_overlay_base"] == 1 and cnt["tw_overlay_marks"] == int(len(bs) > 0) + int(len(hits) > 0), (what, cnt)
    assert 0 in paths and (1 in paths or (stride or w) % 4 != 0), paths


def test_both_paths_ran_on_the_aligned_sizes(engine):
    for w, h, stride in ((64, 64, None), (130, 67, 136)):
        E, T, rs, hits, bs, tol, want = variant(w, h, 0)
        got = {}
        for mis, pitch in ((0, (3 * w // 4 + 1) * 4), (1, (3 * w // 4 + 1) * 4), (0, 3 * w + 1)):
            buf, path = engine.stage_overlay(E, T, rs, hits, bs, tol, pitch=pitch, stride=stride, misalign=mis, fill=FILL)
            got[(mis, pitch % 4)] = path
            assert np.array_equal(buf[:, :3 * w].reshape(h, w, 3), want) and (buf[:, 3 * w:] == FILL).all()
        assert list(got.values()) == [1, 0, 0], got


def test_the_stage_cases_reach_what_they_are_there_for():
    w, h = 397, 99
    E, T, rs, hits, bs, tol, want = variant(w, h, 0)
    comps = np.array([c for hit in hits for c in hit[2:]], np.float32)
    fin = comps[np.isfinite(comps)]
    assert (fin > 1024).any() and (fin < -1024).any() and np.isnan(comps).any() and np.isinf(comps).any()  # both clamps
    ties = fin[(np.abs(fin) < 1024) & (np.abs(fin - np.trunc(fin)) == 0.5)]
    assert (np.rint(ties) > ties).any() and (np.rint(ties) < ties).any()  # a tie rounded each way
    cl = R.clip_rects(rs, w, h)
    kept = R.outside(hits, cl)
    assert 0 < len(kept) < len(hits) and len(cl) < len(rs) == 32 and len(bs) == 256
    vec = set(p for hit in kept for p in R.line_pixels(int(hit[0]), int(hit[1]), hit[2], hit[3]))
    assert any(x < 0 for x, y in vec) and any(x >= w for x, y in vec) and any(y < 0 for x, y in vec) and any(y >= h for x, y in vec)
    box = set(p for b in bs for p in R.box_pixels(*b))
    d = np.abs(E.astype(int) - T.astype(int))
    both = [(x, y) for x, y in vec & box if 0 <= x < w and 0 <= y < h]
    assert any(d[y, x] > tol or R.inside(cl, x, y) for x, y in both)  # a pixel where all three layers compete
    assert tuple(want[both[0][1], both[0][0]]) == R.VEC_RGB
    # the border variant drops pixels on every edge as well, and the small sizes have more than one workgroup row
    bw_, bh_ = 33, 17
    bvec = set(p for hit in border_hits(bw_, bh_) for p in R.line_pixels(int(hit[0]), int(hit[1]), hit[2], hit[3]))
    assert any(x < 0 for x, y in bvec) and any(x >= bw_ for x, y in bvec) and any(y < 0 for x, y in bvec) and any(y >= bh_ for x, y in bvec)


def test_stage_call_refuses_bad_arguments_and_launches_nothing(twflow, engine):
    E, T, rs, hits, bs, tol, _ = variant(7, 5, 0)
    engine.launch_counts(reset=True)
    bad = [dict(tol=-1), dict(tol=256), dict(pitch=20), dict(misalign=4), dict(misalign=-1)]
    for kw in bad:
        args = dict(tol=tol, pitch=21, stride=None, misalign=0)
        args.update(kw)
        with pytest.raises(twflow.TwError) as ei:
            engine.stage_overlay(E, T, rs, hits, bs, args.pop("tol"), **args)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER, kw
    for many in (dict(rects=[(0, 0, 1, 1)] * 33), dict(regions=[(0, 0, 1, 1)] * 257), dict(rects=[(0, 0, -1, 1)])):
        with pytest.raises(twflow.TwError) as ei:
            engine.stage_overlay(E, T, many.get("rects", []), [], many.get("regions", []), 16)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER, many
    cnt = engine.launch_counts()
    assert cnt["tw_overlay_base"] == 0 and cnt["tw_overlay_marks"] == 0


# ---- part 2: batches ----------------------------------------------------------------------------------------------------------
CW, CH = 200, 120
TOL = 16
_FRAMES, _WANT = {}, {}


def frames():
    import synth
    if not _FRAMES:
        _FRAMES["v"] = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, CH, CW, kind=k)) for i, k in ((0, 0), (1, 1), (2, 2))]
    return _FRAMES["v"]


def expected(oracle, key, E, T, span, thr, rects=()):
    """(the vectors tw_wait reports, the clipped rectangles): T is the target as the batch sees it.  Cached by `key`."""
    if key not in _WANT:
        h, w = E.shape
        if span > 0:
            fx, fy = oracle.farneback(E, T)
            vec = outside(oracle.span_scan(fx, fy, span, thr), rects, w, h)
        else:
            vec = []
        _WANT[key] = (vec, R.clip_rects(rects, w, h))
    return _WANT[key]


def bad_parameter(twflow, call):
    with pytest.raises(twflow.TwError) as ei:
        call()
    assert ei.value.code == twflow.TW_E_BAD_PARAMETER


def check_pictures(twflow, e, tk, want, tol):
    """the pair's picture to pageable memory (twice), to a page-locked block and to device memory, each with a pitch of its
    own, the bytes behind the rows untouched"""
    h, w = want.shape[:2]
    first = e.overlay(tk, tol)
    assert np.array_equal(first, want), "pageable destination"
    assert np.array_equal(e.overlay(tk, tol), first), "the second call"
    pitch = 3 * w + 5
    odd = np.full(h * pitch, FILL, np.uint8)
    assert np.array_equal(e.overlay(tk, tol, out=odd, pitch=pitch), want), "pageable destination, odd pitch"
    assert (odd.reshape(h, pitch)[:, 3 * w:] == FILL).all()
    pinned = e.host_array((h * pitch,))
    pinned[:] = FILL
    assert np.array_equal(e.overlay(tk, tol, out=pinned, pitch=pitch), want), "page-locked destination"
    assert (pinned.reshape(h, pitch)[:, 3 * w:] == FILL).all()
    for dp in (pitch, (3 * w // 4 + 1) * 4):
        n = dp * (h - 1) + 3 * w  # an allocation that holds the picture exactly
        d = e.upload(np.full(n, FILL, np.uint8))
        assert e.overlay(tk, tol, out=d, pitch=dp) is None
        got = np.concatenate([e.dev_download(d, n), np.full(dp - 3 * w, FILL, np.uint8)]).reshape(h, dp)
        assert (got[:, 3 * w:] == FILL).all(), "device destination: a byte behind a row was written"
        assert np.array_equal(got[:, :3 * w].reshape(h, w, 3), want), "device destination, pitch %d" % dp
        # a destination one byte too short for the picture is refused before anything is launched
        before = e.launch_counts()["tw_overlay_base"]
        bad_parameter(twflow, lambda: e.overlay(tk, tol, out=C.c_void_p(d.value + 1), pitch=dp))
        assert e.launch_counts()["tw_overlay_base"] == before


PICTURE_CALLS = 6  # check_pictures' calls that render: pageable twice and once more at an odd pitch, page-locked, device twice


def check_ticket(twflow, e, tk, E, T, vec, rects, tol=TOL, boxes_=()):
    """both new calls in front of the collecting wait: the count, and the picture to every kind of destination, twice"""
    want = R.overlay_ref(E, T, rects, vec, boxes_, tol)
    assert e.hits(tk) == len(vec)
    check_pictures(twflow, e, tk, want, tol)
    assert e.hits(tk) == len(vec)
    return want


def after_wait(twflow, e, tk):
    bad_parameter(twflow, lambda: e.hits(tk))
    bad_parameter(twflow, lambda: e.overlay(tk, TOL))


def test_golden_pair_single_pair_schedule(twflow, oracle, golden):
    case = next(c for c in golden.values() if c["expect_img"].shape == (117, 180) and len(c["vector"]) == 24)
    a, b = np.ascontiguousarray(case["expect_img"]), np.ascontiguousarray(case["target_img"])
    span, thr = case["span"], float(case["threshold"])
    vec, _ = expected(oracle, "golden", a, b, span, thr)
    assert vec == [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        e.launch_counts(reset=True)
        tk = e.submit(a, b, span, thr)
        want = check_ticket(twflow, e, tk, a, b, vec, [])
        cnt = e.launch_counts()
        assert cnt["tw_overlay_base"] == PICTURE_CALLS and cnt["tw_overlay_marks"] == PICTURE_CALLS, cnt  # no boxes: one marks launch each
        assert e.wait(tk)["vector"] == vec
        after_wait(twflow, e, tk)
        assert len(set(map(tuple, want.reshape(-1, 3)))) > 3 and (want == np.array(R.VEC_RGB, np.uint8)).all(-1).sum() >= 24 * 9 // 2
        # refused before anything is launched: tol, pitch, format, null
        tk = e.submit(a, b, span, thr)
        e.launch_counts(reset=True)
        out = np.full(117 * 540, FILL, np.uint8)
        bad_parameter(twflow, lambda: e.overlay(tk, -1, out=out))
        bad_parameter(twflow, lambda: e.overlay(tk, 256, out=out))
        bad_parameter(twflow, lambda: e.overlay(tk, TOL, out=out, pitch=539))
        L, bad = twflow.lib(), twflow.TW_E_BAD_PARAMETER
        assert L.tw_ticket_overlay(e._h, tk[0], TOL, None) == bad
        assert L.tw_ticket_overlay(e._h, tk[0], TOL, C.byref(twflow.OverlayOut(None, 540, 0))) == bad
        assert L.tw_ticket_overlay(e._h, tk[0], TOL, C.byref(twflow.OverlayOut(out.ctypes.data, 540, 1))) == bad
        assert L.tw_ticket_hits(e._h, tk[0], None) == bad and L.tw_ticket_hits(e._h, tk[0] + 5, C.byref(C.c_int())) == bad
        cnt = e.launch_counts()
        assert sum(cnt.values()) == 0 and (out == FILL).all(), cnt
        assert e.wait(tk)["vector"] == vec


def test_24_small_host_pairs(twflow, oracle):
    import synth
    h, w, n = 48, 64, 24
    pairs = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, h, w, kind=i % 3)) for i in range(6)]
    want = [expected(oracle, ("small", i), a, b, 4, 0.5)[0] for i, (a, b) in enumerate(pairs)]
    assert any(len(v) > 0 for v in want)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        tks = [e.submit(*pairs[i % 6], 4, 0.5) for i in range(n)]
        for i in (0, 7, 23, 4):  # (in any order, while later tickets of the batch are still open)
            check_ticket(twflow, e, tks[i], *pairs[i % 6], want[i % 6], [])
        for i in range(n):
            assert e.hits(tks[i]) == len(want[i % 6])
            assert e.wait(tks[i])["vector"] == want[i % 6], i
        after_wait(twflow, e, tks[7])


def test_rgba_rows_jpeg_and_a_resident_expected_image(twflow, oracle):
    a, b = frames()[2]
    pa, ga, keep_a = as_rgba(twflow, a)
    pb, gb, keep_b = as_rgba(twflow, b)
    vec_p, _ = expected(oracle, "rgba", ga, gb, 10, 1.0)
    la, ja, _k = as_jpeg(twflow, a)
    lb, jb, _k2 = as_jpeg(twflow, b)
    vec_j, _ = expected(oracle, "jpeg", ja, jb, 10, 1.0)
    a0, b0 = frames()[0]
    vec_r, _ = expected(oracle, "f0", a0, b0, 10, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        tk = e.submit_png(pa, pb, 10, 1.0)
        check_ticket(twflow, e, tk, ga, gb, vec_p, [])
        assert e.wait(tk)["vector"] == vec_p and len(vec_p) > 0
        tk = e.submit_jpeg(la, lb, 10, 1.0)
        check_ticket(twflow, e, tk, ja, jb, vec_j, [])
        assert e.wait(tk)["vector"] == vec_j
        img = e.image(a0)
        tk = e.submit_image(img, b0, 10, 1.0)
        img.release()  # (the batch holds the block until the ticket is collected)
        check_ticket(twflow, e, tk, a0, b0, vec_r, [])
        assert e.wait(tk)["vector"] == vec_r
        after_wait(twflow, e, tk)


def test_a_target_three_pixels_larger_and_ignore_rectangles(twflow, oracle):
    a, b = frames()[1]
    wide = oracle.resize_u8_linear(b, CW + 3, CH + 3)
    seen = oracle.reconcile_target(wide, CW, CH)
    vec, _ = expected(oracle, "wide", a, seen, 10, 1.0)
    a0, b0 = frames()[0]
    rects = [(CW // 3 + 1, CH // 4 + 1, CW // 3, CH // 2), (CW - 9, -3, 20, 11), (70, 70, 1, 1), (CW + 4, 3, 5, 5)]
    seen0 = edit(a0, b0, rects)
    vec0, cl = expected(oracle, "ignore", a0, seen0, 10, 1.0, rects)
    plain = expected(oracle, "f0", a0, b0, 10, 1.0)[0]
    assert len(cl) == 3 and 0 < len(vec0) < len(plain)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        tk = e.submit(a, wide, 10, 1.0, reconcile=True)
        check_ticket(twflow, e, tk, a, seen, vec, [])
        assert e.wait(tk)["vector"] == vec and len(vec) > 0
        tk = e.submit(a0, b0, 10, 1.0, ignore=rects)
        want = check_ticket(twflow, e, tk, a0, seen0, vec0, cl)
        assert e.wait(tk)["vector"] == vec0
        x, y = rects[0][0] + 2, rects[0][1] + 2
        g = 128 + (int(seen0[y, x]) >> 1)
        assert tuple(want[y, x]) == (g - 48, g - 48, g)


def test_device_pairs_at_an_odd_stride_and_a_reconciled_device_target(twflow, oracle):
    a, b = frames()[1]
    stride = CW + 3

    def strided(g, fill, st):
        buf = np.full(1 + st * g.shape[0], fill, np.uint8)
        buf[1:].reshape(g.shape[0], st)[:, :g.shape[1]] = g
        return buf

    vec, _ = expected(oracle, "f1", a, b, 10, 1.0)
    wide = oracle.resize_u8_linear(b, CW + 3, CH + 3)
    vec_w, _ = expected(oracle, "wide", a, oracle.reconcile_target(wide, CW, CH), 10, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        da, db = e.upload(strided(a, 0x11, stride)), e.upload(strided(b, 0xEE, stride))
        tk = e.submit_dev(C.c_void_p(da.value + 1), C.c_void_p(db.value + 1), CW, CH, stride, 10, 1.0)
        check_ticket(twflow, e, tk, a, b, vec, [])
        assert e.wait(tk)["vector"] == vec and len(vec) > 0
        dw = e.upload(strided(wide, 0x77, CW + 8))
        tk = e.submit_dev(C.c_void_p(da.value + 1), C.c_void_p(dw.value + 1), CW, CH, stride, 10, 1.0, target_size=(CW + 3, CH + 3),
                          target_stride=CW + 8)
        check_ticket(twflow, e, tk, a, oracle.reconcile_target(wide, CW, CH), vec_w, [])
        assert e.wait(tk)["vector"] == vec_w
        after_wait(twflow, e, tk)


def test_a_regions_batch_draws_its_boxes(twflow, oracle):
    a, b = frames()[0]
    vec, _ = expected(oracle, "f0", a, b, 10, 1.0)
    records, region_of = regions_ref.regions(vec, 1, 10, CW, CH)
    assert len(records) > 0
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_regions(1)
        tk = e.submit(a, b, 10, 1.0)
        e.launch_counts(reset=True)
        want = check_ticket(twflow, e, tk, a, b, vec, [], boxes_=[r[:4] for r in records])
        cnt = e.launch_counts()
        assert cnt["tw_overlay_base"] == PICTURE_CALLS and cnt["tw_overlay_marks"] == 2 * PICTURE_CALLS, cnt  # the boxes, then the vectors
        assert (want == np.array(R.BOX_RGB, np.uint8)).all(-1).any()
        status, got, rof, regs, nreg = e.wait_regions(tk)
        assert got == vec and rof == region_of and nreg == len(records)
        assert all(regions_ref.same_record(g, w_) for g, w_ in zip(regs, records))
        after_wait(twflow, e, tk)


def test_a_residual_and_shift_batch_keeps_its_other_answers(twflow, oracle):
    a, b = frames()[0]
    vec, _ = expected(oracle, "f0", a, b, 10, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        e.set_shift(8)
        tk = e.submit(a, b, 10, 1.0)
        chg0, sh0 = e.changes(tk), e.shift(tk)
        vec0 = e.wait(tk)["vector"]
        tk = e.submit(a, b, 10, 1.0)
        check_ticket(twflow, e, tk, a, b, vec0, [])
        assert e.changes(tk) == chg0 and e.shift(tk) == sh0
        check_ticket(twflow, e, tk, a, b, vec0, [], tol=0)
        assert e.wait(tk)["vector"] == vec0
        assert sh0[2] == 1 or vec0 == vec  # (a pair whose shift was not applied computes the plain flow)
        after_wait(twflow, e, tk)


def test_span_0_is_the_base(twflow, oracle):
    a, b = frames()[0]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        tk = e.submit(a, b, 0, 1.0)
        assert e.hits(tk) == 0
        e.launch_counts(reset=True)
        want = check_ticket(twflow, e, tk, a, b, [], [])
        cnt = e.launch_counts()
        assert np.array_equal(want, R.base_ref(a, b, [], TOL)) and cnt["tw_overlay_base"] == PICTURE_CALLS and cnt["tw_overlay_marks"] == 0, cnt
        assert e.wait(tk)["vector"] == []
        after_wait(twflow, e, tk)


def test_more_hits_than_the_eager_copy_holds(twflow, oracle):
    """two independent noise images: the picture is drawn from the device's records, of which the host holds 1024"""
    rng = np.random.default_rng(77)
    w, h = 130, 67
    a, b = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    rects = [(20, 10, 40, 30)]
    vec, _ = expected(oracle, "noise", a, b, 1, 0.01)
    seen = edit(a, b, rects)
    vec_i, cl = expected(oracle, "noise_i", a, seen, 1, 0.01, rects)
    assert len(vec) > HOST_RECS and len(vec_i) > HOST_RECS
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        tks = [e.submit(a, b, 1, 0.01), e.submit(a, b, 1, 0.01, ignore=rects)]
        want = check_ticket(twflow, e, tks[0], a, b, vec, [])
        # the hits behind the first 1024 are in the picture
        assert not np.array_equal(want, R.overlay_ref(a, b, [], vec[:HOST_RECS], [], TOL))
        check_ticket(twflow, e, tks[1], a, seen, vec_i, cl)
        assert e.wait(tks[0])["vector"] == vec and e.wait(tks[1])["vector"] == vec_i


def test_a_palette_index_error_answers_both_calls_and_stays_waitable(twflow, oracle):
    from test_gpu_png_kinds import filter_bytes
    a, b = frames()[0]
    h, w = a.shape
    plte = np.repeat((np.arange(10) * 25).astype(np.uint8)[:, None], 3, 1)
    ia, ib = (a.astype(np.int64) * 10 // 256).astype(np.uint8), (b.astype(np.int64) * 10 // 256).astype(np.uint8)
    bad = ia.copy()
    bad[h // 2, w // 2] = 10
    types = np.arange(h) % 5
    P = lambda idx: twflow.PngRows(filter_bytes(idx, 1, types), w, h, 3, 8, plte)  # noqa: E731
    E, T = plte[ia][..., 0], plte[ib][..., 0]
    vec, _ = expected(oracle, "plte", E, T, 10, 2.0)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        t0, t1 = e.submit_png(P(ia), P(ib), 10, 2.0), e.submit_png(P(bad), P(ib), 10, 2.0)
        for call in (lambda: e.hits(t1), lambda: e.overlay(t1, TOL), lambda: e.hits(t1), lambda: e.wait(t1)):
            with pytest.raises(twflow.TwError) as ei:
                call()
            assert ei.value.code == twflow.TW_E_BAD_IMAGE_FORMAT and "expected" in str(ei.value)
        check_ticket(twflow, e, t0, E, T, vec, [])
        assert e.wait(t0)["vector"] == vec


# ---- part 3: nothing else moves -----------------------------------------------------------------------------------------------
def test_a_batch_without_the_call_is_the_batch_it_was_and_the_books_stay_flat(twflow, oracle):
    a, b = frames()[0]
    a1, b1 = frames()[1]
    vec, _ = expected(oracle, "f0", a, b, 10, 1.0)
    want = R.overlay_ref(a, b, [], vec, [], TOL)
    new = ("tw_overlay_base", "tw_overlay_marks")

    def run(with_call):
        with twflow.Engine(0, twflow.default_params(), slots=2) as e:
            born = e.memory()
            e.wait(e.submit(a1, b1, 10, 1.0))  # (the engine's buffers exist)
            warm = e.memory()
            e.launch_counts(reset=True)
            m0 = e.memory()
            tks = [e.submit(a, b, 10, 1.0), e.submit(a1, b1, 10, 1.0)]
            if with_call:
                d = e.upload(np.zeros(CH * CW * 3, np.uint8))  # (through the bounce buffer, which grows for it)
                m0 = e.memory()
                for _ in range(3):
                    e.overlay(tks[0], TOL, out=d)
                assert e.memory() == m0  # a device destination: nothing of the engine's grows
                assert np.array_equal(e.dev_download(d, CH * CW * 3).reshape(CH, CW, 3), want)
                pinned = e.host_array((CH * CW * 3,))
                m0 = e.memory()
                assert np.array_equal(e.overlay(tks[0], TOL, out=pinned), want)
                m1 = e.memory()
                stage = (3 * CW + 3) // 4 * 4 * CH + 256
                assert m1["device_bytes"] - m0["device_bytes"] == stage, (m0, m1)
                assert {k: v for k, v in m1.items() if k != "device_bytes"} == {k: v for k, v in m0.items() if k != "device_bytes"}
                for _ in range(200):
                    e.overlay(tks[0], TOL, out=pinned)
                assert e.memory() == m1  # the staging is made once, and nothing else is kept
            res = [e.wait(t)["vector"] for t in tks]
            return res, dict(e.launch_counts()), born, warm

    res0, cnt0, born0, warm0 = run(False)
    res1, cnt1, born1, warm1 = run(True)
    # tw_debug_memory needs a live engine, so "back to the start after tw_engine_destroy" is asserted on the engine that
    # follows: the engine made after the one that had a staging buffer was destroyed is born as that one was, and grows to
    # what it had grown to before its first picture — the staging is absent again, and nothing process-wide (the page-lock
    # table) is left over.  (That the device memory itself went back is tw_engine_destroy's hipFree: the books cannot see it.)
    res2, cnt2, born2, warm2 = run(False)
    assert born0 == born1 == born2 and warm0 == warm1 == warm2, (born0, born1, born2, warm0, warm1, warm2)
    assert res2 == res0 and cnt2 == cnt0
    assert res0 == res1 and res0[0] == vec
    assert cnt0["tw_overlay_base"] == 0 and cnt0["tw_overlay_marks"] == 0
    assert cnt1["tw_overlay_base"] == 204 and cnt1["tw_overlay_marks"] == 204
    assert {k: v for k, v in cnt0.items() if k not in new} == {k: v for k, v in cnt1.items() if k not in new}
