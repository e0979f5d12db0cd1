"""The HIP kernels against the independent float64 reference (tests/farneback_f64.py), and hostile flows GPU == oracle.

Part 1 runs the reference, the inputs and the bounds of tests/test_oracle_stages_f64.py against the KERNELS, through the
per-stage entry points — a check that does not load the oracle's shared library to judge a kernel (the oracle only helps
to build a realistic M as an input).  Shapes: the oracle-test shapes, tile-edge shapes (190- and 240-column edges +- 1,
the 160-output strips of tw_flow_iter, 320 x 20 — its minimum) and 1080p once per stage.  The kernel family that ran is
asserted from the launch counters.  Each comparison prints `f64ref gpu <stage> <case> ratio=...` (run with -s).

Part 2 feeds non-finite, huge and boundary-exact flows to the stages and the submissions and compares GPU and oracle:
NaN masks are identical, and every value that is not NaN is bit-identical as a uint32 view (so -0.0 is not 0.0, and
+inf is not -inf).  NaN payload and sign are NOT compared: x86 and gfx950 generate different default NaNs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import farneback_f64 as F  # noqa: E402
import test_oracle_stages_f64 as S  # noqa: E402
from conftest import interleaved, planar  # noqa: E402
from test_flow_init_abi import farneback_with_init  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

EDGES = [(37, 189), (37, 190), (37, 191), (37, 239), (37, 240), (37, 241), (20, 320)]  # (h, w)
ITER_SIZES = [(20, 320), (37, 321), (41, 349), (37, 350), (37, 351), (64, 479), (117, 480), (37, 481), (64, 700)]
PYR_FAMILIES = ("tw_pyr_k3", "tw_pyr_k3f", "tw_pyr_23", "tw_pyr_taps", "tw_pyr_level")
BLUR_FAMILIES = ("tw_blur_solve4", "tw_blur_solve4y", "tw_blur_solve8", "tw_blur_solve_pp", "tw_blur_solve_generic",
                 "tw_blur_variant", "tw_blur_grid", "tw_blur_solve4q")


def ran(e, fams, n=None):
    """Launches of the families `fams` since the last call, asserted non-zero (or == n)."""
    cnt = e.launch_counts(reset=True)
    got = sum(cnt[f] for f in ((fams,) if isinstance(fams, str) else fams))
    assert (got >= 1) if n is None else (got == n), (fams, dict((k, v) for k, v in cnt.items() if v))
    return cnt


# ---- part 1: kernels against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.6, 0.75, 0.8])
def test_stage_pyr_level(twflow, scale):
    with twflow.Engine(0, twflow.default_params(pyrScale=scale, pyrLevels=6), slots=1) as e:
        e.launch_counts(reset=True)

        def pyr(img, s, levels, k):
            assert (s, levels) == (scale, 6)
            got = e.stage_pyr_level(img, k)
            cnt = ran(e, PYR_FAMILIES)
            # ... and it is the one launch of the family choose_pyr names for this level (tests/test_gpu_pyr_dispatch.py)
            fam = e.pyr_plan(img.shape[1], img.shape[0], k).family
            assert cnt[fam] == 1 and sum(cnt[f] for f in PYR_FAMILIES) == 1, (k, fam, cnt)
            return got
        for h0, w0 in ((257, 333),) + (((1080, 1920),) if scale == 0.6 else ()):
            img = np.random.default_rng(h0 + w0).integers(0, 256, (h0, w0)).astype(np.uint8)
            img[: h0 // 5, : w0 // 7] = 255
            plan = F.level_plan(w0, h0, scale, 6)
            assert e.num_levels(w0, h0) == len(plan) - 1
            for k, lv in enumerate(plan):
                ref, bound = F.pyr_level(img, lv)
                case = "%dx%d@%g/level%d(%dx%d,k%d)" % (w0, h0, scale, k, lv[0], lv[1], lv[2])
                S.check("gpu", "pyr_level", case, pyr(img, scale, 6, k), ref, bound)


@pytest.mark.parametrize("h,w", S.UPD_SIZES + EDGES + [(1080, 1920)])
def test_stage_polyexp(engine, h, w):
    from scipy import ndimage
    rng = np.random.default_rng(h * 7 + w)
    I = (ndimage.gaussian_filter(rng.random((h, w)), 1.0) * 255).astype(F32)
    I[h // 4: h // 2, w // 3: w // 2] = 17.25
    engine.launch_counts(reset=True)
    got = interleaved(engine.stage_polyexp(I))
    ran(engine, "tw_polyexp")
    ref, bound = F.polyexp(I, 0.0, 7, 1.5)
    S.check("gpu", "polyexp", "%dx%d" % (w, h), got, ref, bound)


@pytest.mark.parametrize("h,w", S.UPD_SIZES + EDGES + [(1080, 1920)])
def test_stage_update_matrices(engine, h, w):
    engine.launch_counts(reset=True)

    def upd(R0, R1, flow):
        got = interleaved(engine.stage_update_matrices(planar(R0), planar(R1), planar(flow)))
        ran(engine, "tw_update_matrices", 1)
        return got
    S.run_update_matrices("gpu", upd, sizes=[(h, w)])


@pytest.mark.parametrize("scale", [0.5, 0.6, 0.75, 0.8])
def test_stage_flow_upsample_update(twflow, scale):
    """The upsampled flow against the reference; M against the reference's FarnebackUpdateMatrices of THE KERNEL'S OWN
    float32 flow (the sample position is a decision on that float32 value)."""
    with twflow.Engine(0, twflow.default_params(pyrScale=scale), slots=1) as e:
        e.launch_counts(reset=True)
        for ph, pw, h, w, s in [c for c in S.ups_cases() if c[4] == scale]:
            rng = np.random.default_rng(ph * 31 + w)
            prev = (rng.standard_normal((ph, pw, 2)) * 2).astype(F32)
            prev[0, 0, 0] = -0.0
            R0, R1 = S.fields(rng, h, w)
            gflow, gM = e.stage_flow_upsample_update(planar(R0), planar(R1), planar(prev))
            ran(e, "tw_update_matrices", 1)
            case = "%dx%d->%dx%d@%g" % (pw, ph, w, h, s)
            ref, bound = F.flow_upsample(prev, 0.0, w, h, s)
            S.check("gpu", "flow_upsample", case, interleaved(gflow), ref, bound)
            ref, bound = F.update_matrices(R0, R1, interleaved(gflow))
            S.check("gpu", "upsample+update_matrices", case, interleaved(gM), ref, bound)


@pytest.mark.parametrize("gaussian,win", [(True, 30), (True, 31), (True, 50), (True, 51), (False, 30), (False, 31), (False, 5)])
def test_stage_blur_solve(twflow, oracle, gaussian, win):
    """The window average + solve of every window size, and the fused matrix refresh (update = 1) against the
    reference's FarnebackUpdateMatrices of the kernel's own float32 flow."""
    sizes = S.WIN_SIZES + EDGES + ([(1080, 1920)] if win in (30, 50) else [])
    with twflow.Engine(0, twflow.default_params(winSize=win, flags=256 if gaussian else 0), slots=1) as e:
        e.launch_counts(reset=True)
        for h, w in sizes:
            rng = np.random.default_rng(7 * h + w)
            M = S.matrices(oracle, rng, h, w)
            R0, R1 = S.fields(rng, h, w)
            gflow, gM = e.stage_blur_solve(planar(R0), planar(R1), planar(M), 1)
            cnt = ran(e, BLUR_FAMILIES if gaussian else "tw_box", None if gaussian else 2)
            assert (cnt["tw_box"] == 0) == gaussian
            case = "%dx%d/%s%d" % (w, h, "gauss" if gaussian else "box", win)
            ref, bound = F.window_solve(M, 0.0, win, gaussian)
            S.check("gpu", "window_solve", case, interleaved(gflow), ref, bound)
            ref, bound = F.update_matrices(R0, R1, interleaved(gflow))
            S.check("gpu", "solve+update_matrices", case, interleaved(gM), ref, bound)


def _iter_ref(R0, R1, flow):
    M, eM = F.update_matrices(R0, R1, flow)
    return F.window_solve(M, eM, 30, True)


@pytest.mark.parametrize("h,w", ITER_SIZES + [(1080, 1920)])
def test_stage_flow_iter_three_sources(engine, h, w):
    """tw_flow_iter — FarnebackUpdateMatrices, the window and the solve without M in memory — with its three flow
    sources: memory, the coarser level's flow upsampled, zero.  The upsampled float32 flow the reference samples at is
    the one tw_stage_flow_upsample_update returns for the same input (checked against the reference above)."""
    rng = np.random.default_rng(h * 11 + w)
    R0, R1 = S.fields(rng, h, w)
    R0[h // 2:, w // 2:] = 0
    R1[h // 2:, w // 2:] = 0
    case = "%dx%d" % (w, h)
    engine.launch_counts(reset=True)
    for name, flow in S.flow_cases(rng, h, w)[:2 if w > 1000 else 3]:
        got = engine.stage_flow_iter(planar(R0), planar(R1), flow=planar(flow))
        ran(engine, "tw_flow_iter", 1)
        S.check("gpu", "flow_iter", case + "/memory/" + name, interleaved(got), *_iter_ref(R0, R1, flow))
    got = engine.stage_flow_iter(planar(R0), planar(R1))
    ran(engine, "tw_flow_iter_zero", 1)
    S.check("gpu", "flow_iter", case + "/zero", interleaved(got), *_iter_ref(R0, R1, np.zeros((h, w, 2), F32)))
    ph, pw = int(round(h * 0.5)), int(round(w * 0.5))
    prev = (rng.standard_normal((ph, pw, 2)) * 2).astype(F32)
    up, _ = engine.stage_flow_upsample_update(planar(R0), planar(R1), planar(prev))
    engine.launch_counts(reset=True)
    got = engine.stage_flow_iter(planar(R0), planar(R1), prev=planar(prev))
    ran(engine, "tw_flow_iter_ups", 1)
    S.check("gpu", "flow_iter", case + "/upsampled", interleaved(got), *_iter_ref(R0, R1, interleaved(up)))


@pytest.mark.parametrize("h,w,levels", [(117, 180, 3), (480, 640, 3), (257, 333, 2), (70, 70, 0)])
def test_area_init_kernel_through_a_submission_without_iterations(twflow, h, w, levels):
    """tw_flow_area_init, which no stage entry point exposes: with pyrIterations = 0 a submission returns the seeded field
    passed through the upsamples alone, and neither holds a data-dependent decision, so the reference's bound carries
    from INTER_AREA through every upsample to the field the submission stores (generic, fast and ratio-1 paths)."""
    import synth
    f0 = (np.random.default_rng(h + w).standard_normal((h, w, 2)) * 5).astype(F32)
    a, b = synth.make_pair(0, h, w)
    with twflow.Engine(0, twflow.default_params(pyrLevels=levels, pyrIterations=0), slots=1) as e:
        out = e.host_array((h, w, 2), np.float32)
        e.launch_counts(reset=True)
        e.wait(e.submit(a, b, 0, 5.0, flow=out, init=f0))
        ran(e, "tw_flow_area_init", 1)
        got = np.array(out)  # (page-locked memory of the engine: copied before it closes)
    plan = F.level_plan(w, h, 0.5, levels)
    ref, bound = F.area_init(f0, plan[-1][0], plan[-1][1], plan[-1][4])
    for lv in plan[-2::-1]:
        ref, bound = F.flow_upsample(ref, bound, lv[0], lv[1], 0.5)
    S.check("gpu", "area_init", "%dx%d levels %d" % (w, h, len(plan) - 1), got, ref, bound)


# ---- part 2: hostile flows, GPU == oracle ------------------------------------------------------------------------------------------
def same_bits(got, want, what):
    """NaN masks identical; everything else identical as uint32 (NaN payload and sign are not compared)."""
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN masks differ at %d values, first %r" % (
        what, int((gn != wn).sum()), tuple(int(v[0]) for v in np.nonzero(gn != wn)))
    g, w_ = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = g != w_
    assert not bad.any(), "%s: %d of %d non-NaN values differ in bits, first got %r want %r" % (
        what, int(bad.sum()), g.size, got[~gn][bad][:1], want[~wn][bad][:1])


def hostile_flow(rng, h, w, per=40):
    """sigma-2 noise seeded with +-inf, NaN, +-1e30, +-2^31, +-2^24, -0.0 and with displacements that put x + dx (y + dy)
    exactly on 0, w-2, w-1 (h-2, h-1) and on the float32 neighbours either side of them.  `per`: seeds of each special
    value (one non-finite seed turns a whole window of the next flow into NaN: the iteration tests take few)."""
    f = (rng.standard_normal((h, w, 2)) * 2).astype(F32)
    specials = [np.inf, -np.inf, np.nan, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 24, -2.0 ** 24, -0.0]
    n = h * w
    idx = rng.choice(n, size=min(n // 3, per * len(specials)), replace=False)
    for j, i in enumerate(idx):
        f[i // w, i % w, rng.integers(0, 2)] = specials[j % len(specials)]
    xs = np.arange(w, dtype=F32)
    ys = np.arange(h, dtype=F32)
    rows = rng.permutation(h)
    r = 0
    for axis, size, pos in ((0, w, xs), (1, h, ys)):
        for t in (0, size - 2, size - 1):
            for tt in (F32(t), np.nextafter(F32(t), F32(-np.inf)), np.nextafter(F32(t), F32(np.inf))):
                if axis == 0:
                    f[rows[r % h], :, 0] = tt - pos
                else:
                    f[:, rows[r % h] % w, 1] = tt - pos
                r += 1
    return f


def _oracle_iter(oracle, R0, R1, flow):
    with np.errstate(all="ignore"):
        M = oracle.update_matrices(R0, R1, flow)
        return oracle.update_flow(R0, R1, flow, M, 30, 0)[0]


@pytest.mark.parametrize("h,w", [(33, 47), (117, 180), (64, 700), (37, 191)])
def test_hostile_flows_update_matrices(engine, oracle, h, w):
    rng = np.random.default_rng(h + w)
    R0, R1 = S.fields(rng, h, w)
    for rep in range(2):
        flow = hostile_flow(rng, h, w)
        got = engine.stage_update_matrices(planar(R0), planar(R1), planar(flow))
        same_bits(got, planar(oracle.update_matrices(R0, R1, flow)), "update_matrices %dx%d #%d" % (w, h, rep))


@pytest.mark.parametrize("ph,pw,h,w", [(58, 90, 117, 180), (17, 24, 33, 47), (32, 350, 64, 700)])
def test_hostile_flows_upsample_update(engine, oracle, ph, pw, h, w):
    rng = np.random.default_rng(ph + w)
    R0, R1 = S.fields(rng, h, w)
    prev = hostile_flow(rng, ph, pw)
    gflow, gM = engine.stage_flow_upsample_update(planar(R0), planar(R1), planar(prev))
    with np.errstate(all="ignore"):
        wflow = oracle.flow_upsample(prev, w, h, 0.5)
        wM = oracle.update_matrices(R0, R1, wflow)
    same_bits(gflow, planar(wflow), "upsampled hostile flow %dx%d" % (w, h))
    same_bits(gM, planar(wM), "M of the upsampled hostile flow %dx%d" % (w, h))


@pytest.mark.parametrize("h,w", [(20, 320), (64, 700), (117, 481)])
def test_hostile_flows_flow_iter(engine, oracle, h, w):
    rng = np.random.default_rng(3 * h + w)
    R0, R1 = S.fields(rng, h, w)
    flow = hostile_flow(rng, h, w, per=1)
    got = engine.stage_flow_iter(planar(R0), planar(R1), flow=planar(flow))
    same_bits(got, planar(_oracle_iter(oracle, R0, R1, flow)), "flow_iter from memory %dx%d" % (w, h))
    ph, pw = int(round(h * 0.5)), int(round(w * 0.5))
    prev = hostile_flow(rng, ph, pw, per=1)
    got = engine.stage_flow_iter(planar(R0), planar(R1), prev=planar(prev))
    with np.errstate(all="ignore"):
        up = oracle.flow_upsample(prev, w, h, 0.5)
    same_bits(got, planar(_oracle_iter(oracle, R0, R1, up)), "flow_iter upsampled %dx%d" % (w, h))


def hostile_fields(h, w):
    rng = np.random.default_rng(h * w)
    mixed = np.where(rng.random((h, w, 2)) < 0.5, np.inf, -np.inf).astype(F32)
    holes = (rng.standard_normal((h, w, 2)) * 3).astype(F32)
    holes[rng.random((h, w)) < 0.002] = np.nan
    holes[0, 0, 0] = holes[h - 1, w - 1, 1] = np.nan
    return [("all-inf", np.full((h, w, 2), np.inf, F32)), ("all-NaN", np.full((h, w, 2), np.nan, F32)),
            ("mixed +-inf", mixed), ("1e30", np.full((h, w, 2), 1e30, F32)), ("isolated NaNs", holes)]


def same_vectors(got, want, what):
    assert len(got) == len(want), "%s: %d vectors, want %d" % (what, len(got), len(want))
    if got:
        g, w_ = np.array(got, np.float64), np.array(want, np.float64)
        assert np.array_equal(g[:, :2], w_[:, :2]), what
        same_bits(g[:, 2:].astype(F32), w_[:, 2:].astype(F32), what)


@pytest.mark.parametrize("hw", [(117, 180), (480, 640)])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_hostile_initial_flows_through_submissions(twflow, oracle, hw, layout, path):
    """tw_submit_u8_flow_init (host images and fields) and tw_submit_dev_flow_init (device images and fields), one batch
    of five pairs, one hostile field each: the dense fields and the vector lists against farneback_with_init."""
    import synth
    h, w = hw
    kinds = hostile_fields(h, w)
    n = len(kinds)
    pairs = [synth.make_pair(i, h, w) for i in range(n)]
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        out = e.host_array((n, 2, h, w), np.float32)
        out[...] = 7.0
        tk = []
        for i, (name, f) in enumerate(kinds):
            field = f if layout == "interleaved" else planar(f)
            if path == "host":
                tk.append(e.submit(pairs[i][0], pairs[i][1], 10, 5.0, flow=out[i], init=field))
            else:
                da, db, df = e.upload(pairs[i][0]), e.upload(pairs[i][1]), e.upload(field)
                init = (df.value, (w * 8) if layout == "interleaved" else (w * 4),
                        twflow.FLOW_INTERLEAVED if layout == "interleaved" else twflow.FLOW_PLANAR)
                tk.append(e.submit_dev(da, db, w, h, w, 10, 5.0, flow=out[i], init=init))
        res = [e.wait(t) for t in tk]
        assert e.launch_counts()["tw_flow_area_init"] >= 1
        for i, (name, f) in enumerate(kinds):
            with np.errstate(all="ignore"):
                want = np.stack(farneback_with_init(oracle, pairs[i][0], pairs[i][1], f))
                wvec = oracle.span_scan(want[0], want[1], 10, 5.0)
            what = "%s, %s %s %dx%d" % (name, path, layout, w, h)
            same_bits(out[i], want, what)
            same_vectors(res[i]["vector"], wvec, what + " vectors")
