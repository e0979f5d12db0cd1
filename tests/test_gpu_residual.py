"""The residual (TW_OPT_RESIDUAL): tw_warp_residual and tw_change_scan against tests/residual_ref.py, value for value.

Part 1: tw_stage_warp_residual on chosen images and fields: the cell plane, the count, the ordered records, and 0xff bytes
        behind the count.
Part 2: batches.  Expected values are residual_ref(E, T, oracle.farneback(E, T)) with T as the batch sees it; the vectors are
        oracle.span_scan's as before; the launch counters say which schedule ran.
Part 3: the option: off by default and launch for launch, refused values, the books of tw_debug_memory.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref  # noqa: E402
import residual_ref as R  # noqa: E402
from test_flow_init_abi import farneback_with_init  # noqa: E402
from test_gpu_grid_final import batch_pairs, oracle_field  # noqa: E402  (their caches are shared with that module's tests)
from test_gpu_ignore import clip, edit, outside  # noqa: E402
from test_gpu_resident import as_rgba  # noqa: E402
from test_gpu_stages_f64 import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 16
HOST_RECS = 1024  # records per pair the batch copies back eagerly


# ---- part 1: the two kernels alone ------------------------------------------------------------------------------------------
SIZES = [(1, 1, None), (7, 5, None), (33, 17, None), (64, 64, None), (130, 67, 136), (397, 99, None)]
SPANS = [1, 4, 10, 16, 100]
TOLS = [1, 16, 254]


def stage_fields(w, h, rng):
    big = F32(16384)
    specials = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, big, -big, np.nextafter(big, F32(np.inf)),
                         np.nextafter(-big, F32(-np.inf))], F32)
    wild = rng.uniform(-8, 8, (2, h, w)).astype(F32)
    pos = rng.permutation(2 * h * w)
    for k in range(min(len(pos), 4 * len(specials))):
        wild.ravel()[pos[k]] = specials[k % len(specials)]
    if w * h == 1:
        wild[:, 0, 0] = (np.nan, -np.inf)
    small = rng.uniform(-2, 2, (h, w)).astype(F32)
    out = [("zero", np.zeros((2, h, w), F32)),
           ("constant (3, -2)", np.stack([np.full((h, w), 3, F32), np.full((h, w), -2, F32)])),
           ("multiples of 1/64", (rng.integers(-512, 513, (2, h, w)) / 64.0).astype(F32)),
           ("uniform [-8, 8]", rng.uniform(-8, 8, (2, h, w)).astype(F32)),
           ("leaves on the left", np.stack([np.full((h, w), -w - 3.3, F32), small])),
           ("leaves on the right", np.stack([np.full((h, w), w + 3.3, F32), small])),
           ("leaves at the top", np.stack([small, np.full((h, w), -h - 2.7, F32)])),
           ("leaves at the bottom", np.stack([small, np.full((h, w), h + 2.7, F32)])),
           ("NaN, inf, 1e30, +-16384 and beyond", wild)]
    return out


def stage_images(w, h, rng):
    ys, xs = np.mgrid[0:h, 0:w]
    board = (((xs + ys) & 1) * 255).astype(np.uint8)
    rnd = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return [("random bytes", rnd, rng.integers(0, 256, (h, w), dtype=np.uint8)),
            ("checkerboard against its inverse", board, 255 - board),
            ("identical", rnd, rnd.copy())]


@pytest.mark.parametrize("w,h,stride", SIZES, ids=["%dx%d" % s[:2] for s in SIZES])
def test_stage_equals_the_reference(engine, w, h, stride):
    rng = np.random.default_rng(w * 7 + h)
    images = stage_images(w, h, rng)
    n_calls = 0
    for fname, f in stage_fields(w, h, rng):
        for iname, E, T in images:
            diff, u = R.pixels(E, T, f[0], f[1])
            for span in SPANS:
                for tol in TOLS:
                    want = R.cells_of(diff, u, span, tol)
                    rec = R.records(want, span)
                    engine.launch_counts(reset=True)
                    cells, n, chg = engine.stage_warp_residual(E, T, f, span, tol, stride=stride)
                    cnt = engine.launch_counts(reset=True)
                    what = "%dx%d span %d tol %d, %s, %s" % (w, h, span, tol, fname, iname)
                    assert cnt["tw_warp_residual"] == 1 and cnt["tw_change_scan"] == 1, (what, cnt)
                    assert np.array_equal(cells, want.reshape(-1, 4)), what
                    assert n == len(rec), what
                    assert np.array_equal(chg[:n], rec), what
                    assert (chg[n:] == -1).all(), what  # still 0xff bytes
                    if iname == "identical":
                        assert n == 0, what
                    n_calls += 1
    assert n_calls == 9 * 3 * len(SPANS) * len(TOLS)


def test_the_stage_cases_reach_what_they_are_there_for():
    """Computed from the reference: ties that round both ways, both clamps of the sample point, the largest sums."""
    w, h = 33, 17
    rng = np.random.default_rng(w * 7 + h)
    fields = dict(stage_fields(w, h, rng))
    q = R.quantise(fields["multiples of 1/64"])
    odd_halves = (np.round(fields["multiples of 1/64"].astype(np.float64) * 64).astype(np.int64) & 1) == 1
    assert odd_halves.any() and (q[odd_halves] % 2 == 0).all()  # every tie went to an even 1/32 step
    wild = fields["NaN, inf, 1e30, +-16384 and beyond"]
    assert np.isnan(wild).any() and np.isinf(wild).any() and (np.abs(R.quantise(wild)) == 524288).any()
    _, E, T = stage_images(w, h, rng)[1]
    c = R.cells_fast(E, T, fields["zero"][0], fields["zero"][1], 100, 1)
    assert c.tolist() == [[[w * h, w * h, 255, 255]]]


def test_stage_call_refuses_bad_arguments(twflow, engine):
    E = np.zeros((8, 8), np.uint8)
    f = np.zeros((2, 8, 8), F32)
    for span, tol in ((0, 16), (-1, 16), (4, 0), (4, 255), (4, -1)):
        with pytest.raises(twflow.TwError) as ei:
            engine.stage_warp_residual(E, E, f, span, tol)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER


# ---- part 2: batches --------------------------------------------------------------------------------------------------------
def expected(oracle, E, T, span, tol, thr, rects=(), field=None):
    """(vectors, records, field) a pair must report: T is the target as the batch sees it, rects the pair's rectangles"""
    h, w = E.shape
    f = np.stack(oracle.farneback(E, T)) if field is None else field
    cl = [(x0, y0, x1 - x0, y1 - y0) for x0, y0, x1, y1 in clip(rects, w, h)]
    _, rec = R.residual_ref(E, T, f, span, tol, cl)
    return outside(oracle.span_scan(f[0], f[1], span, thr), rects, w, h), rec, f


def collect(e, tk):
    """tw_ticket_changes, then the collecting wait"""
    chg, n = e.changes(tk)
    assert n == len(chg)
    return chg, e.wait(tk)["vector"]


def test_golden_pair_single_pair_schedule(twflow, oracle, golden):
    case = next(c for c in golden.values() if c["expect_img"].shape == (117, 180) and len(c["vector"]) == 24)
    a, b = np.ascontiguousarray(case["expect_img"]), np.ascontiguousarray(case["target_img"])
    span, thr = case["span"], float(case["threshold"])
    vec, rec, _ = expected(oracle, a, b, span, TOL, thr)
    assert vec == [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]] and len(rec) > 0
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        chg, got = collect(e, e.submit(a, b, span, thr))
        cnt = e.launch_counts(reset=True)
        assert got == vec and chg == rec
        assert cnt["tw_warp_residual"] == 1 and cnt["tw_change_scan"] == 1 and cnt["tw_flow_iter_grid"] == 0, cnt
        assert cnt["tw_blur_grid"] == 0, cnt


@pytest.mark.parametrize("h,w,graph", [(240, 320, 0), (240, 320, 1), (1080, 1920, 0)], ids=["two_stream", "graph", "twin_1080p"])
def test_single_pair_schedules(twflow, oracle, monkeypatch, h, w, graph):
    """One pair on the single-pair schedules (no tw_pair_same launch says one ran; 1080p takes the twin launches); with
    TW_LAT_GRAPH=1 a residual pair is enqueued directly — its launches are counted, which a replayed graph's are not — and
    the plain pair still replays"""
    import synth
    for name in ("TW_LATENCY_STREAMS", "TW_LAT_FUSED"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TW_LATENCY_MIN_PX", "0")
    monkeypatch.setenv("TW_LAT_GRAPH", str(graph))
    a, b = (np.ascontiguousarray(x) for x in synth.make_pair(5, h, w))
    vec, rec, _ = expected(oracle, a, b, 10, TOL, 1.0)
    assert len(vec) > 0 and len(rec) > 0
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        assert e.wait(e.submit(a, b, 10, 1.0))["vector"] == vec
        e.set_residual(TOL)
        for _ in range(2):
            e.launch_counts(reset=True)
            chg, got = collect(e, e.submit(a, b, 10, 1.0))
            cnt = e.launch_counts(reset=True)
            assert got == vec and chg == rec
            assert cnt["tw_pair_same"] == 0 and cnt["tw_warp_residual"] == 1 and cnt["tw_change_scan"] == 1, cnt
            assert cnt["tw_polyexp"] + cnt["tw_twin"] > 0, cnt  # (enqueued, not replayed)
            assert cnt["tw_twin"] > 0 or h != 1080, cnt
        e.set_residual(0)
        assert e.wait(e.submit(a, b, 10, 1.0))["vector"] == vec


BH, BW = 99, 397


@pytest.fixture
def gate_lifted(monkeypatch):
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.setenv("TW_RAMP", "0")
    monkeypatch.delenv("TW_LANES", raising=False)
    monkeypatch.delenv("TW_GRID_FINAL", raising=False)
    return monkeypatch


_EIGHT = {}


def eight_pairs(oracle):
    """[(E, T, vectors at threshold 5, records)]: the moved block, the flat change, synth kinds 0 - 3, and the first two again"""
    if not _EIGHT:
        from test_residual_ref import scenes
        sc = scenes()
        pairs = [sc["moved"], sc["flat"]] + batch_pairs(BH, BW, 4)
        assert np.array_equal(*pairs[5])
        _EIGHT["v"] = [(np.ascontiguousarray(a), np.ascontiguousarray(b)) + expected(oracle, a, b, 10, TOL, 5.0)[:2] for a, b in pairs]
    return _EIGHT["v"] + _EIGHT["v"][:2]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("slots", [4, 8])
def test_batches_on_the_flow_iter_path(twflow, oracle, gate_lifted, slots, lanes):
    if lanes == 2:
        gate_lifted.setenv("TW_LANES", "2")
    cases = eight_pairs(oracle)
    assert len(cases[1][2]) == 0 and len(cases[1][3]) == 40  # the flat change: no vector, forty cells
    with twflow.Engine(0, twflow.default_params(), slots=slots) as e:
        assert e.level_runs_flow_iter(BW, BH, 0, slots // lanes)
        plan = e.level_plan(BW, BH, 10, slots, residual=True)
        assert not plan.grid_final and e.level_plan(BW, BH, 10, slots).grid_final
        chunks = sum(part[0].launches for part in plan.parts)
        e.set_residual(TOL)
        for lo in range(0, 8, slots):
            e.launch_counts(reset=True)
            tks = [e.submit(a, b, 10, 5.0) for a, b, _, _ in cases[lo:lo + slots]]
            got = [collect(e, t) for t in tks]
            cnt = e.launch_counts(reset=True)
            for i, ((chg, vec), (_, _, want_vec, want_rec)) in enumerate(zip(got, cases[lo:lo + slots])):
                assert vec == want_vec, "pair %d: vectors" % (lo + i)
                assert chg == want_rec, "pair %d: change records" % (lo + i)
            assert cnt["tw_flow_iter_grid"] == 0 and cnt.flow_iter() > 0, cnt
            assert cnt["tw_span_gather"] == chunks and cnt["tw_warp_residual"] == chunks, (cnt, chunks)
            assert cnt.last_z["tw_warp_residual"] == cnt.last_z["tw_span_gather"] == plan.parts[-1][0].tail, cnt.last_z
            assert cnt["tw_change_scan"] == 1, cnt


def test_default_gate(twflow, oracle, monkeypatch):
    """24 pairs of 640 x 480 under the default gate (test_gpu_grid_final.test_default_gate's shape), four distinct pairs"""
    for name in ("TW_MFREE", "TW_LATENCY_STREAMS", "TW_RAMP", "TW_LANES", "TW_GRID_FINAL"):
        monkeypatch.delenv(name, raising=False)
    h, w, n = 480, 640, 24
    pairs = batch_pairs(h, w, n)
    want = []
    for i in range(4):
        a, b = pairs[i]
        f = oracle_field(oracle, h, w, i, 3)
        want.append(expected(oracle, a, b, 10, TOL, 1.0, field=f)[:2])
    assert not want[3][1] and all(len(want[i][1]) > 0 for i in range(3))
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_runs_flow_iter(w, h, 0, n)
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        tks = [e.submit(a, b, 10, 1.0) for a, b in pairs]
        got = [collect(e, t) for t in tks]
        cnt = e.launch_counts(reset=True)
        assert cnt["tw_flow_iter_grid"] == 0 and cnt["tw_warp_residual"] == cnt["tw_span_gather"] >= 1, cnt
        assert cnt["tw_change_scan"] == 1, cnt
        for i in range(n):
            assert got[i][1] == want[i % 4][0], i
            assert got[i][0] == want[i % 4][1], i


# -- combinations: one small test each
CW, CH = 200, 120
_FRAMES = {}


def frames():
    import synth
    if not _FRAMES:
        _FRAMES["v"] = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, CH, CW, kind=k)) for i, k in ((0, 0), (1, 1), (2, 2))]
    return _FRAMES["v"]


def test_ignore_rectangles(twflow, oracle):
    a, b = frames()[0]
    rects = [(CW // 3 + 1, CH // 4 + 1, CW // 3, CH // 2), (CW - 9, -3, 20, 11), (70, 70, 1, 1)]
    vec, rec, _ = expected(oracle, a, edit(a, b, rects), 10, TOL, 1.0, rects)
    plain = expected(oracle, a, b, 10, TOL, 1.0)[1]
    assert 0 < len(rec) < len(plain)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        chg, got = collect(e, e.submit(a, b, 10, 1.0, ignore=rects))
        assert e.launch_counts()["tw_mask_rects"] == 1
        assert got == vec and chg == rec
        # nothing of a cell whose grid point is inside a rectangle; a small cap still reports the true count
        assert not any(CW // 3 + 1 <= r[0] < CW // 3 + 1 + CW // 3 and CH // 4 + 1 <= r[1] < CH // 4 + 1 + CH // 2 for r in chg)
        tk = e.submit(a, b, 10, 1.0, ignore=rects)
        few, n = e.changes(tk, cap=3)
        assert few == rec[:3] and n == len(rec)
        assert e.wait(tk)["vector"] == vec


def test_a_target_three_pixels_wider(twflow, oracle):
    a, b = frames()[1]
    wide = oracle.resize_u8_linear(b, CW + 3, CH)
    vec, rec, _ = expected(oracle, a, oracle.reconcile_target(wide, CW, CH), 10, TOL, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        chg, got = collect(e, e.submit(a, wide, 10, 1.0, reconcile=True))
        assert e.launch_counts()["tw_resize_u8"] == 1
        assert got == vec and chg == rec and len(rec) > 0


def test_filtered_png_rows(twflow, oracle):
    a, b = frames()[2]
    pa, ga, keep_a = as_rgba(twflow, a)
    pb, gb, keep_b = as_rgba(twflow, b)
    vec, rec, _ = expected(oracle, ga, gb, 10, TOL, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        chg, got = collect(e, e.submit_png(pa, pb, 10, 1.0))
        assert e.launch_counts()["tw_png_unfilter"] >= 1
        assert got == vec and chg == rec and len(rec) > 0


def test_a_resident_expected_image(twflow, oracle):
    a, b = frames()[0]
    vec, rec, _ = expected(oracle, a, b, 10, TOL, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        img = e.image(a)
        chg, got = collect(e, e.submit_image(img, b, 10, 1.0))
        assert got == vec and chg == rec and len(rec) > 0
        img.release()


def test_device_pair_at_an_odd_offset_and_stride(twflow, oracle):
    a, b = frames()[1]
    stride = CW + 3
    assert stride % 2 == 1

    def strided(g, fill):
        buf = np.full(1 + stride * CH, fill, np.uint8)
        buf[1:].reshape(CH, stride)[:, :CW] = g
        return buf

    vec, rec, _ = expected(oracle, a, b, 10, TOL, 1.0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        da, db = e.upload(strided(a, 0x11)), e.upload(strided(b, 0xEE))
        tk = e.submit_dev(C.c_void_p(da.value + 1), C.c_void_p(db.value + 1), CW, CH, stride, 10, 1.0)
        chg, got = collect(e, tk)
        assert got == vec and chg == rec and len(rec) > 0


def test_a_flow_destination_and_an_initial_field_in_one_batch(twflow, oracle):
    (a0, b0), (a1, b1) = frames()[0], frames()[1]
    init = (np.random.default_rng(5).random((2, CH, CW), F32) * 4 - 2).astype(F32)
    f1 = np.stack(farneback_with_init(oracle, a1, b1, init))
    vec0, rec0, f0 = expected(oracle, a0, b0, 10, TOL, 1.0)
    vec1, rec1, _ = expected(oracle, a1, b1, 10, TOL, 1.0, field=f1)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(TOL)
        out0, out1 = e.host_array((2, CH, CW), F32), e.host_array((2, CH, CW), F32)
        e.launch_counts(reset=True)
        t0 = e.submit(a0, b0, 10, 1.0, flow=out0)
        t1 = e.submit(a1, b1, 10, 1.0, flow=out1, init=init)
        (chg0, got0), (chg1, got1) = collect(e, t0), collect(e, t1)
        cnt = e.launch_counts()
        assert cnt["tw_flow_export"] >= 1 and cnt["tw_flow_area_init"] >= 1 and cnt["tw_warp_residual"] >= 1, cnt
        same_bits(np.array(out0), f0, "exported field of the pair without an initial field")
        same_bits(np.array(out1), f1, "exported field of the pair with one")
        assert got0 == vec0 and chg0 == rec0 and got1 == vec1 and chg1 == rec1


def test_regions_and_residual_together(twflow, oracle):
    a, b = frames()[0]
    vec, rec, _ = expected(oracle, a, b, 10, TOL, 1.0)
    records, region_of = regions_ref.regions(vec, 1, 10, CW, CH)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_regions(1)
        e.set_residual(TOL)
        e.launch_counts(reset=True)
        tk = e.submit(a, b, 10, 1.0)
        chg, n = e.changes(tk)
        again, _ = e.changes(tk)  # (the ticket is not consumed)
        status, got, rof, regs, nreg = e.wait_regions(tk)
        cnt = e.launch_counts()
        assert chg == rec and again == rec and n == len(rec)
        assert got == vec and rof == region_of and nreg == len(records) > 0
        assert all(regions_ref.same_record(g, w_) for g, w_ in zip(regs, records))
        assert cnt["tw_hit_regions"] == 1 and cnt["tw_change_scan"] == 1, cnt
        with pytest.raises(twflow.TwError) as ei:
            e.changes(tk)  # already waited
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER


def test_more_records_than_the_eager_copy_holds(twflow, oracle):
    a, b = frames()[0]
    rects = [(40, 30, 60, 40)]
    vec, rec, f = expected(oracle, a, b, 2, 1, 1.0)
    assert len(rec) > HOST_RECS
    vec_i, rec_i, _ = expected(oracle, a, edit(a, b, rects), 2, 1, 1.0, rects)
    assert len(rec_i) > HOST_RECS
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(1)
        tks = [e.submit(a, b, 2, 1.0), e.submit(a, b, 2, 1.0, ignore=rects)]
        chg, n = e.changes(tks[0])
        assert chg == rec and n == len(rec)
        few, n = e.changes(tks[0], cap=HOST_RECS + 7)
        assert few == rec[:HOST_RECS + 7] and n == len(rec)
        none, n = e.changes(tks[0], cap=0)
        assert none == [] and n == len(rec)
        chg_i, n_i = e.changes(tks[1])
        assert chg_i == rec_i and n_i == len(rec_i)
        assert e.wait(tks[0])["vector"] == vec and e.wait(tks[1])["vector"] == vec_i
        # span 0: no scan, no cells
        tk = e.submit(a, b, 0, 1.0)
        assert e.changes(tk) == ([], 0)
        e.wait(tk)


# ---- part 3: the option -----------------------------------------------------------------------------------------------------
def test_option_off_refuses_and_leaves_the_ticket_waitable(twflow, oracle):
    a, b = frames()[0]
    vec = expected(oracle, a, b, 10, TOL, 1.0)[0]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        for bad in (-1, 255, 256):
            with pytest.raises(twflow.TwError) as ei:
                e.set_residual(bad)
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        e.launch_counts(reset=True)
        tk = e.submit(a, b, 10, 1.0)  # (a refused value left the option off)
        with pytest.raises(twflow.TwError) as ei:
            e.changes(tk)
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        assert e.wait(tk)["vector"] == vec
        cnt = e.launch_counts()
        assert cnt["tw_warp_residual"] == 0 and cnt["tw_change_scan"] == 0, cnt
        e.set_residual(254)
        e.set_residual(1)
        with pytest.raises(twflow.TwError):
            e.set_residual(255)
        tk = e.submit(a, b, 10, 1.0)  # (a refused value left the option at 1)
        assert e.changes(tk)[0] == expected(oracle, a, b, 10, 1, 1.0)[1]
        e.wait(tk)


def run_batch(e, pairs, span=10, thr=1.0):
    tks = [e.submit(a, b, span, thr) for a, b in pairs]
    return [e.wait(t)["vector"] for t in tks]


def test_off_is_the_engine_without_the_feature_and_on_adds_its_buffers(twflow, gate_lifted):
    """Launch for launch and byte for byte: an engine that set the option and cleared it again, one that never touched it"""
    pairs = batch_pairs(BH, BW, 4)
    slots = 4
    G = -(-BW // 10) * -(-BH // 10)
    with twflow.Engine(0, twflow.default_params(), slots=slots) as never, \
            twflow.Engine(0, twflow.default_params(), slots=slots) as e:
        never.launch_counts(reset=True)
        v_never = run_batch(never, pairs)
        cnt_never, mem_never = never.launch_counts(reset=True), never.memory()
        assert cnt_never["tw_warp_residual"] == 0 and cnt_never["tw_change_scan"] == 0
        assert cnt_never["tw_flow_iter_grid"] == 1 and cnt_never["tw_span_gather"] == 0, cnt_never
        e.launch_counts(reset=True)
        v_off = run_batch(e, pairs)
        cnt_off, mem_off = e.launch_counts(reset=True), e.memory()
        # the figure of an engine without the feature, recorded before the option is first set
        assert v_off == v_never and dict(cnt_off) == dict(cnt_never) and mem_off == mem_never
        e.set_residual(TOL)
        v_on = run_batch(e, pairs)  # (plain tw_wait on a residual batch works as before)
        cnt_on, mem_on = e.launch_counts(reset=True), e.memory()
        assert v_on == v_off
        assert cnt_on["tw_warp_residual"] == 1 and cnt_on["tw_change_scan"] == 1 and cnt_on["tw_flow_iter_grid"] == 0, cnt_on
        # one context's counts [cap], records [cap][G] of 24 bytes and their pinned copies (counts, HOST_RECS records per
        # pair), and the engine's cell plane [cap][G] of 16 bytes; every device allocation carries 256 bytes of slack
        dev = (4 * slots + 256) + (24 * G * slots + 256) + (16 * G * slots + 256)
        pinned = 4 * slots + 24 * HOST_RECS * slots
        assert mem_on["device_bytes"] - mem_off["device_bytes"] == dev, (mem_on, mem_off)
        assert mem_on["pinned_host_bytes"] - mem_off["pinned_host_bytes"] == pinned, (mem_on, mem_off)
        assert {k: v for k, v in mem_on.items() if k not in ("device_bytes", "pinned_host_bytes")} == \
               {k: v for k, v in mem_off.items() if k not in ("device_bytes", "pinned_host_bytes")}
        e.set_residual(0)
        v_again = run_batch(e, pairs)
        cnt_again = e.launch_counts(reset=True)
        assert v_again == v_off and dict(cnt_again) == dict(cnt_off) and e.memory() == mem_on


def test_changing_the_option_affects_only_the_later_batch(twflow, oracle):
    (a0, b0), (a1, b1) = frames()[0], frames()[1]
    r16 = [expected(oracle, a, b, 10, 16, 1.0)[1] for a, b in ((a0, b0), (a1, b1))]
    r3 = expected(oracle, a0, b0, 10, 3, 1.0)[1]
    assert r3 != r16[0]
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        e.set_residual(16)
        t0 = e.submit(a0, b0, 10, 1.0)  # opens a batch at tolerance 16
        e.set_residual(3)
        t1 = e.submit(a1, b1, 10, 1.0)  # joins it
        e.set_residual(0)
        t2 = e.submit(a0, b0, 10, 1.0)
        assert [e.changes(t)[0] for t in (t0, t1, t2)] == [r16[0], r16[1], r16[0]]
        for t in (t0, t1, t2):
            e.wait(t)
        t3 = e.submit(a0, b0, 10, 1.0)  # a new batch: off
        with pytest.raises(twflow.TwError):
            e.changes(t3)
        e.wait(t3)
        e.set_residual(3)
        t4 = e.submit(a0, b0, 10, 1.0)
        assert e.changes(t4)[0] == r3
        e.wait(t4)
