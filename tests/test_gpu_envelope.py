"""The admitted size envelope against the CPU oracle, bit for bit.

check_dims admits w, h <= 32768 with round_up(w, 32) * h <= (2^32 - 1) / 20 = 214 748 364 (tw_debug_check_size): the
stencil kernels reach the five float planes of R0, R1 or M through one raw buffer resource with 32-bit offsets.
tests/test_gpu_parity.py compares the kernels with the oracle up to about 8 Mpixel; this file does it at the edges:

  * the largest planes, in row bands.  The oracle runs on full-width crops that reach past each band by the stage's
    dependency radius, so the band's rows are exact: the first and the last 64 rows (the largest offsets) and three
    seeded interior bands.  One step past the bound is refused by every submit and every stage entry point;
  * 32768-pixel widths and heights, whole fields;
  * the deepest pyramids with the largest smoothing kernels (125 taps admitted, 179 refused);
  * the kernel families no other test asserts by name: tw_blur_solve_generic, tw_box, tw_blur_solve_pp, tw_pyr_level.
"""
import gc
import os
import resource
import sys
import time

import numpy as np
import pytest

from conftest import interleaved, planar

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_init_abi import farneback_with_init  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_PS = (2 ** 32 - 1) // 20  # the largest admitted round_up(w, 32) * h
# (h, w) of the largest planes: ld * h = 214 748 352, the largest admitted (238 * 32 columns), and 214 745 088 (16384 wide)
BIG = [(28197, 7616), (13107, 16384)]
BAND = 64


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d values differ, the first at %s" % (what, len(bad), got.size, tuple(bad[0])))


def _texture(seed, h, w, period=521):
    """A u8 image of any size without an h x w float64 temporary: `period` rows of smoothed noise with a flat block,
    repeated down the image, each repeat shifted by its own grey level (mod 256), so no two bands are alike."""
    rng = np.random.default_rng(seed)
    p = min(period, h)
    a = rng.integers(0, 256, (p, w)).astype(F32)
    a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, 2, 1)) / 4
    a[p // 3: p // 2, w // 4: w // 2] = 200
    tile = a.astype(np.uint8)
    out = np.empty((h, w), np.uint8)
    for k, y in enumerate(range(0, h, p)):
        n = min(p, h - y)
        np.add(tile[:n], np.uint8(k * 37 % 256), out=out[y:y + n])
    return out


def _field(seed, c, h, w, amp, period=263):
    """c float32 planes (c, h, w) with |v| <= amp, repeated like _texture with a per-repeat scale."""
    rng = np.random.default_rng(seed)
    p = min(period, h)
    tile = (np.clip(rng.standard_normal((c, p, w)), -1, 1) * amp).astype(F32)
    out = np.empty((c, h, w), F32)
    for k, y in enumerate(range(0, h, p)):
        n = min(p, h - y)
        np.multiply(tile[:, :n], F32(1 - (k % 97) / 200), out=out[:, y:y + n])
    return out


def _bands(h, seed):
    rng = np.random.default_rng(seed)
    mid = sorted(int(y) for y in rng.integers(BAND, h - 2 * BAND, 3))
    return [(0, BAND), (h - BAND, h)] + [(y, y + BAND) for y in mid]


def _crop(a, y0, y1, r):
    """Rows [y0 - r, y1 + r) of a (..., h, w) array, clipped to the image, and the row of y0 in the crop."""
    c0, c1 = max(0, y0 - r), min(a.shape[-2], y1 + r)
    return np.ascontiguousarray(a[..., c0:c1, :]), y0 - c0


def _crops(y0, y1, r, *fields):
    """The same rows of several planar fields, interleaved as the oracle takes them, and the row of y0 in them."""
    cs = [_crop(f, y0, y1, r) for f in fields]
    return [interleaved(c) for c, _ in cs], cs[0][1]


def _um_rows(oracle, r0, r1, f, c0, h, a, b):
    """Rows [a, b) of the oracle's update_matrices at the IMAGE's row numbers, from interleaved crops whose first row is
    row c0 of an h-row image: the oracle's float y + dy rounds as in the whole image (a crop-relative y would round
    differently).  The crops must hold rows a - 1 - max |flow y| .. b + 1 + max |flow y|: nothing else is read."""
    import ctypes as C
    w = r0.shape[1]
    M = np.zeros_like(r0)
    at = lambda arr, ch: C.cast(C.c_void_p(arr.ctypes.data - c0 * w * ch * 4), C.POINTER(C.c_float))  # noqa: E731
    oracle.lib().orc_update_matrices(at(r0, 5), at(r1, 5), at(f, 2), at(M, 5), w, h, a, b)
    return M[a - c0:b - c0]


def _window_of_matrices(oracle, r0, r1, f, c0, h, y0, y1):
    """Rows [y0, y1) (planar) of one iteration from the flow f: the matrices at the image's row numbers over the
    window's reach (m = 15 rows), then the oracle's window + solve on those rows.  Crops as _um_rows, 20 rows past."""
    a, b = max(0, y0 - 15), min(h, y1 + 15)
    s = slice(a - c0, b - c0)
    wf, _ = oracle.update_flow(r0[s], r1[s], f[s], _um_rows(oracle, r0, r1, f, c0, h, a, b), 30, 0)
    return planar(wf)[:, y0 - a:y1 - a]


def _peak_rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6


def _stages_in_bands(e, oracle, h, w, seed):
    """Every stage entry point at h x w, chained as the pipeline does (pyramid level 0 -> polyexp -> matrices -> window
    + solve), each output compared with the oracle in five row bands (the pyramid level whole)."""
    t0 = time.time()
    bands = _bands(h, seed)
    a = _texture(seed, h, w)
    b = np.roll(a, (1, 2), (0, 1))
    lv0 = oracle.level_plan(w, h)[0]
    I0, I1 = e.stage_pyr_level(a, 0), e.stage_pyr_level(b, 0)
    assert_same(I0, oracle.pyr_level(a, lv0), "pyramid level 0 of %dx%d" % (w, h))
    assert_same(I1, oracle.pyr_level(b, lv0), "pyramid level 0 of the target %dx%d" % (w, h))
    del a, b
    R0, R1 = e.stage_polyexp(I0), e.stage_polyexp(I1)
    for y0, y1 in bands:  # dependency radius: polyN
        for I, R, what in ((I0, R0, "R0"), (I1, R1, "R1")):
            c, o = _crop(I, y0, y1, 7)
            assert_same(R[:, y0:y1], planar(oracle.polyexp(c, 7, 1.5))[:, o:o + y1 - y0],
                        "polyexp %s %dx%d rows %d-%d" % (what, w, h, y0, y1))
    del I0, I1

    # the matrices from a bounded non-zero flow: radius ceil(max |flow|) + 1, at least the 5-pixel border ramp
    flow = _field(seed + 1, 2, h, w, 3.0)
    M = e.stage_update_matrices(R0, R1, flow)
    for y0, y1 in bands:
        (r0, r1, f), o = _crops(y0, y1, 5, R0, R1, flow)
        assert_same(M[:, y0:y1], planar(_um_rows(oracle, r0, r1, f, y0 - o, h, y0, y1)),
                    "update_matrices %dx%d rows %d-%d" % (w, h, y0, y1))

    # the coarser level's flow upsampled (x 2: |flow| <= 2.8), then the matrices
    prev = _field(seed + 2, 2, (h + 1) // 2, (w + 1) // 2, 1.4)
    gflow, gM = e.stage_flow_upsample_update(R0, R1, prev)
    up = oracle.flow_upsample(interleaved(prev), w, h, 0.5)
    assert_same(gflow[0], up[..., 0], "upsampled flow x %dx%d" % (w, h))
    assert_same(gflow[1], up[..., 1], "upsampled flow y %dx%d" % (w, h))
    del gflow
    upP = planar(up)
    del up
    for y0, y1 in bands:
        (r0, r1, f), o = _crops(y0, y1, 5, R0, R1, upP)
        assert_same(gM[:, y0:y1], planar(_um_rows(oracle, r0, r1, f, y0 - o, h, y0, y1)),
                    "upsample + update_matrices %dx%d rows %d-%d" % (w, h, y0, y1))
    del gM

    # the window (m = 15) and the solve; with update 1 also the matrices refreshed at the new flow, which gather R1
    # |flow y| rows away: the crop reaches that far too
    for upd in (0, 1):
        gf, gMo = e.stage_blur_solve(R0, R1, M, upd)
        for y0, y1 in bands:
            r = 15
            if upd:
                r = max(r, int(np.ceil(np.abs(gf[1, y0:y1]).max())) + 2)
                assert r <= 4096, "a solved flow of %d rows" % r
            (r0, r1, f, m), o = _crops(y0, y1, r, R0, R1, flow, M)
            wf, _ = oracle.update_flow(r0, r1, f, m, 30, 0)  # the window + solve: no absolute row number
            n = y1 - y0
            assert_same(gf[:, y0:y1], planar(wf)[:, o:o + n], "blur+solve %d flow %dx%d rows %d-%d" % (upd, w, h, y0, y1))
            if upd:  # the refresh is update_matrices at the new flow (FarnebackUpdateFlow's update_matrices branch)
                assert_same(gMo[:, y0:y1], planar(_um_rows(oracle, r0, r1, wf, y0 - o, h, y0, y1)),
                            "blur+solve refresh %dx%d rows %d-%d" % (w, h, y0, y1))
        del gf, gMo
    del M

    # one whole iteration without M in memory (tw_flow_iter): radius m + the matrices' 5
    for kw, fin in ((dict(flow=flow), flow), (dict(prev=prev), upP)):
        got = e.stage_flow_iter(R0, R1, **kw)
        for y0, y1 in bands:
            (r0, r1, f), o = _crops(y0, y1, 20, R0, R1, fin)
            wf = _window_of_matrices(oracle, r0, r1, f, y0 - o, h, y0, y1)
            assert_same(got[:, y0:y1], wf, "flow_iter(%s) %dx%d rows %d-%d" % (list(kw)[0], w, h, y0, y1))
        del got
    print("stages at %dx%d (ld*h %d): %.0f s, peak RSS %.1f GB, engine device bytes %.2f GB" %
          (w, h, -(-w // 32) * 32 * h, time.time() - t0, _peak_rss_gb(), e.memory()["device_bytes"] / 1e9))


def test_largest_planes_in_bands(twflow, oracle):
    """All the 214-Mpixel work in one function, so that one set of large host arrays exists at a time: every stage at
    the two largest admitted plane sizes, then the whole product path — a 2-pair batch at the largest admitted ld * h,
    pyrLevels 0 and one iteration (local, so the bands stay exact), dense fields through flow=, pair 0 started from an
    initial field with |f| <= 3.  That sends the non-zero-flow R1 gather and tw_flow_iter's plane offsets through the
    largest planes, and pair 1 the per-pair offsets."""
    L = twflow.lib()
    for h, w in BIG:
        assert L.tw_debug_check_size(w, h) == twflow.TW_OK and -(-w // 32) * 32 * h <= MAX_PS
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        e.launch_counts(reset=True)
        for i, (h, w) in enumerate(BIG):
            _stages_in_bands(e, oracle, h, w, 11 + i)
            gc.collect()
        cnt = e.launch_counts()
        print("stage launches:", {k: v for k, v in cnt.items() if v})
        n = len(BIG)
        assert cnt["tw_polyexp"] == 2 * n and cnt["tw_update_matrices"] >= 2 * n, cnt
        assert cnt["tw_flow_iter"] == n and cnt["tw_flow_iter_ups"] == n and cnt["tw_blur_solve4"] == 2 * n, cnt

    h, w = BIG[0]
    op = oracle.default_params(pyrLevels=0, pyrIterations=1)
    t0 = time.time()
    a = _texture(21, h, w)
    b = np.roll(a, (2, -1), (0, 1))
    init = _field(22, 2, h, w, 3.0)
    with twflow.Engine(0, twflow.default_params(pyrLevels=0, pyrIterations=1), slots=2) as e:
        out = e.host_array((2, 2, h, w), F32)
        e.launch_counts(reset=True)
        t = [e.submit(a, b, 10, 1e9, flow=out[0], init=init), e.submit(b, a, 10, 1e9, flow=out[1])]
        res = [e.wait(x) for x in t]
        cnt = e.launch_counts()
        mem = e.memory()
        print("batch launches:", {k: v for k, v in cnt.items() if v}, "last_z:", {k: v for k, v in cnt.last_z.items() if v})
        assert all(r["vector"] == [] for r in res)
        assert cnt["tw_flow_area_init"] >= 1 and cnt["tw_flow_export"] >= 1, cnt
        if e.level_runs_flow_iter(w, h, 0, 2):
            assert cnt.flow_iter() >= 1, cnt
        else:
            assert cnt["tw_update_matrices"] >= 1, cnt
        # dependency radius: window 15 + matrices 5 (|init| <= 3) + polyN 7 + the 3-tap level-0 blur 1
        # (farneback_with_init's level-0 loop with the matrices at the image's own row numbers)
        for i, (x, y, f0) in enumerate(((a, b, init), (b, a, None))):
            for y0, y1 in _bands(h, 23 + i):
                xc, o = _crop(x, y0, y1, 28)
                yc, _ = _crop(y, y0, y1, 28)
                lv = oracle.level_plan(w, xc.shape[0], op.pyrScale, 0)[0]
                r0 = oracle.polyexp(oracle.pyr_level(xc, lv), op.polyN, op.polySigma)
                r1 = oracle.polyexp(oracle.pyr_level(yc, lv), op.polyN, op.polySigma)
                f = np.zeros(r0.shape[:2] + (2,), F32) if f0 is None else interleaved(_crop(f0, y0, y1, 28)[0])
                assert_same(out[i, :, y0:y1], _window_of_matrices(oracle, r0, r1, f, y0 - o, h, y0, y1),
                            "pair %d flow rows %d-%d" % (i, y0, y1))
        # the same composition on a whole small pair equals farneback_with_init (the oracle's own loop)
        sa, sb = a[:96, :400], b[:96, :400]
        lv = oracle.level_plan(400, 96, op.pyrScale, 0)[0]
        r0 = oracle.polyexp(oracle.pyr_level(sa, lv), op.polyN, op.polySigma)
        r1 = oracle.polyexp(oracle.pyr_level(sb, lv), op.polyN, op.polySigma)
        f = interleaved(np.ascontiguousarray(init[:, :96, :400]))
        assert_same(_window_of_matrices(oracle, r0, r1, f, 0, 96, 0, 96),
                    np.stack(farneback_with_init(oracle, sa, sb, f, op)), "the composition itself")
        print("2-pair batch at %dx%d: %.0f s, peak RSS %.1f GB, engine device bytes %.2f GB, page-locked %.2f GB" %
              (w, h, time.time() - t0, _peak_rss_gb(), mem["device_bytes"] / 1e9, mem["pinned_host_bytes"] / 1e9))


def test_one_step_past_the_bound_is_refused_everywhere(twflow):
    """Sizes the old w * h <= 2^28 bound admitted (or nearly) and the plane offsets cannot address: every host submit
    flavour and every stage entry point answers TW_E_UNSUPPORTED before it reads an input (the arrays are zero pages
    nobody touches), and 32769 in either dimension is TW_E_BAD_PARAMETER.  tw_submit_dev[_flow[_init]] runs the same
    Submit::check_arguments first, before it could dereference a device pointer."""
    L = twflow.lib()
    past = [(13108, 16384), (28198, 7616), (16385, 16383), (16384, 16384), (13082, 16385)]
    for h, w in past:
        assert L.tw_debug_check_size(w, h) == twflow.TW_E_UNSUPPORTED, (w, h)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        def refused(fn, *args, code=twflow.TW_E_UNSUPPORTED, **kw):
            with pytest.raises(twflow.TwError) as ei:
                fn(*args, **kw)
            assert ei.value.code == code, (fn.__name__, str(ei.value))
        for h, w in past:
            img = np.zeros((h, w), np.uint8)
            rows = np.zeros(h * (1 + w), np.uint8)
            refused(e.submit, img, img)
            refused(e.submit, img, img, flow=(0, 8 * w, twflow.FLOW_INTERLEAVED))
            refused(e.submit, img, img, init=np.zeros((2, h, w), F32))
            refused(e.submit_png8, rows, 1, img, 0, w, h)
            refused(e.stage_png_unfilter, rows, 1, w, h)
            refused(e.stage_pyr_level, img, 0)
            refused(e.stage_pyr_fused01, img)
            refused(e.stage_pyr_fused23, img)
            I, R, f2 = np.zeros((h, w), F32), np.zeros((5, h, w), F32), np.zeros((2, h, w), F32)
            refused(e.stage_polyexp, I)
            refused(e.stage_update_matrices, R, R, f2)
            refused(e.stage_flow_upsample_update, R, R, np.zeros((2, 8, 8), F32))
            refused(e.stage_blur_solve, R, R, R, 1)
            refused(e.stage_flow_iter, R, R, flow=f2)
            refused(e.stage_flow_iter, R, R, prev=np.zeros((2, 8, 8), F32))
            del img, rows, I, R, f2
        for h, w in ((1, 32769), (32769, 1)):
            img = np.zeros((h, w), np.uint8)
            refused(e.submit, img, img, code=twflow.TW_E_BAD_PARAMETER)
            refused(e.stage_polyexp, np.zeros((h, w), F32), code=twflow.TW_E_BAD_PARAMETER)
        a = _texture(3, 64, 96)  # and the engine still computes
        fx, _, _ = e.calculate_internal(a, np.roll(a, 1, 1))
        assert np.isfinite(fx).all()


@pytest.mark.parametrize("h,w", [(128, 32768), (32768, 128)])
def test_widest_and_tallest_images(engine, oracle, h, w):
    """32768 columns or rows, default parameters, whole fields."""
    a = _texture(h + 7, h, w)
    b = np.roll(a, (1, -2), (0, 1))
    gx, gy, _ = engine.calculate_internal(a, b)
    wx, wy = oracle.farneback(a, b)
    assert_same(gx, wx, "flow x %dx%d" % (w, h))
    assert_same(gy, wy, "flow y %dx%d" % (w, h))


def test_tall_strip_through_flow_iter_and_the_box_window(twflow, oracle, monkeypatch):
    """A 2-pair batch of 320 x 32768 runs tw_flow_iter down one tall strip at level 0 (TW_MFREE=2 lifts the launch-size
    gate), and the box window (flags 0) covers 32768 rows with its double running sums (tw_box)."""
    h, w = 32768, 320
    a = _texture(5, h, w)
    pairs = [(a, np.roll(a, (2, 1), (0, 1))), (np.roll(a, 3, 1), a)]
    monkeypatch.setenv("TW_MFREE", "2")
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        assert e.level_runs_flow_iter(w, h, 0, 2)
        e.launch_counts(reset=True)
        out, _ = e.flow_batch([x for x, _ in pairs], [y for _, y in pairs], layout="planar")
        cnt = e.launch_counts()
        assert cnt["tw_flow_iter"] >= 1 and cnt.last_z["tw_flow_iter"] == 2, (cnt, cnt.last_z)
        for i, (x, y) in enumerate(pairs):
            wx, wy = oracle.farneback(x, y)
            assert_same(out[i, 0], wx, "tall pair %d flow x" % i)
            assert_same(out[i, 1], wy, "tall pair %d flow y" % i)
    monkeypatch.delenv("TW_MFREE")
    with twflow.Engine(0, twflow.default_params(flags=0), slots=2) as e:
        e.launch_counts(reset=True)
        out, _ = e.flow_batch([x for x, _ in pairs], [y for _, y in pairs], layout="planar")
        cnt = e.launch_counts()
        assert cnt["tw_box"] >= 2 and cnt.last_z["tw_box"] == 2, (cnt, cnt.last_z)
        for i, (x, y) in enumerate(pairs):
            wx, wy = oracle.farneback(x, y, oracle.default_params(flags=0))
            assert_same(out[i, 0], wx, "box window, tall pair %d flow x" % i)
            assert_same(out[i, 1], wy, "box window, tall pair %d flow y" % i)


@pytest.mark.parametrize("n,scale,levels,taps", [(1200, 0.6, 7, 87), (1640, 0.7, 11, 125), (2400, 0.7, 11, 125)])
def test_deepest_pyramids_and_largest_smoothing_kernels(twflow, oracle, n, scale, levels, taps):
    """Kernels above 63 taps take the unstaged tw_pyr_level (4-row tiles where an 8-row tile's row buffer would pass
    32 KB): every level of the plan, then one whole field."""
    import synth
    plan = oracle.level_plan(n, n, scale, levels)
    assert len(plan) - 1 == levels and plan[-1].smooth_sz == taps
    a, b = synth.make_pair(0, n, n)
    with twflow.Engine(0, twflow.default_params(pyrScale=scale, pyrLevels=levels), slots=1) as e:
        assert e.num_levels(n, n) == levels
        e.launch_counts(reset=True)
        for k, lv in enumerate(plan):
            assert_same(e.stage_pyr_level(a, k), oracle.pyr_level(a, lv), "level %d (%d taps) of %d^2" % (k, lv.smooth_sz, n))
        wide = sum(lv.smooth_sz > 63 for lv in plan)
        cnt = e.launch_counts()
        assert wide >= 1 and cnt["tw_pyr_level"] >= wide and cnt.last_z["tw_pyr_level"] == 1, cnt
        gx, gy, _ = e.calculate_internal(a, b)
        wx, wy = oracle.farneback(a, b, oracle.default_params(pyrScale=scale, pyrLevels=levels))
        assert_same(gx, wx, "flow x %d^2" % n)
        assert_same(gy, wy, "flow y %d^2" % n)


def test_smoothing_kernel_above_127_taps_is_refused(twflow, oracle):
    """2400^2 at pyrScale 0.7 has a 12th level with a 179-tap kernel: TW_E_UNSUPPORTED.  The same engine then computes a
    1640^2 pair, whose plan stops at 11 levels (125 taps), bit for bit."""
    import synth
    assert oracle.level_plan(2400, 2400, 0.7, 12)[-1].smooth_sz == 179
    assert len(oracle.level_plan(1640, 1640, 0.7, 12)) - 1 == 11
    with twflow.Engine(0, twflow.default_params(pyrScale=0.7, pyrLevels=12), slots=1) as e:
        a, b = synth.make_pair(1, 2400, 2400)
        with pytest.raises(twflow.TwError) as ei:
            e.calculate_internal(a, b)
        assert ei.value.code == twflow.TW_E_UNSUPPORTED
        with pytest.raises(twflow.TwError) as ei:
            e.stage_pyr_level(a, 0)
        assert ei.value.code == twflow.TW_E_UNSUPPORTED
        a, b = synth.make_pair(1, 1640, 1640)
        gx, gy, _ = e.calculate_internal(a, b)
        wx, wy = oracle.farneback(a, b, oracle.default_params(pyrScale=0.7, pyrLevels=12))
        assert_same(gx, wx, "flow x after the refusal")
        assert_same(gy, wy, "flow y after the refusal")


@pytest.mark.parametrize("win", [2, 3, 64, 65])
def test_generic_window_in_a_batch(twflow, oracle, win):
    """winSize 2 / 3 (m = 1) and 64 / 65 (m = 32) take tw_blur_solve_generic: a 16-pair batch on a level 520 px wide."""
    import synth
    h, w, n = 40, 520, 16
    pairs = [synth.make_pair(i, h, w) for i in range(4)]
    with twflow.Engine(0, twflow.default_params(winSize=win), slots=n) as e:
        e.launch_counts(reset=True)
        out, _ = e.flow_batch([pairs[i % 4][0] for i in range(n)], [pairs[i % 4][1] for i in range(n)], layout="planar")
        cnt = e.launch_counts()
        assert cnt["tw_blur_solve_generic"] >= 1 and cnt.last_z["tw_blur_solve_generic"] >= 2, (cnt, cnt.last_z)
        op = oracle.default_params(winSize=win)
        for i in range(4):
            wx, wy = oracle.farneback(*pairs[i], op)
            for j in range(i, n, 4):
                assert_same(out[j, 0], wx, "winSize %d pair %d flow x" % (win, j))
                assert_same(out[j, 1], wy, "winSize %d pair %d flow y" % (win, j))


def test_plane_parallel_window_kernel(engine, oracle):
    """A level too small for two 2-wave workgroups per SIMD takes tw_blur_solve_pp (the 31-tap window on plane-parallel
    32 x 8 tiles): the per-stage entry on 90 x 58, with and without the matrix refresh."""
    h, w = 58, 90
    rng = np.random.default_rng(58)
    R0 = (rng.standard_normal((5, h, w)) * 10).astype(F32)
    R1 = (R0 + rng.standard_normal((5, h, w))).astype(F32)
    flow0 = rng.standard_normal((2, h, w)).astype(F32)
    M = planar(oracle.update_matrices(interleaved(R0), interleaved(R1), interleaved(flow0)))
    for upd in (0, 1):
        engine.launch_counts(reset=True)
        gf, gM = engine.stage_blur_solve(R0, R1, M, upd)
        cnt = engine.launch_counts()
        assert cnt["tw_blur_solve_pp"] == 1 and cnt.last_z["tw_blur_solve_pp"] == 1, cnt
        wf, wM = oracle.update_flow(interleaved(R0), interleaved(R1), interleaved(flow0), interleaved(M), 30, upd)
        assert_same(gf, planar(wf), "plane-parallel window, update %d" % upd)
        if upd:
            assert_same(gM, planar(wM), "plane-parallel window refresh")
