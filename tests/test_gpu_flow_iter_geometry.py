"""tw_flow_iter's strip, step and row-segment geometry, proven from the plan the launch itself uses.

A tw_flow_iter launch is right only if three pieces of geometry line up: strips of 190 columns with 160 outputs (the last
one ragged), steps of 5 rows through an 8-block LDS ring primed with 7 chunks (the last step partial, the loop unrolled by
two with a tail, two tap-register sets in modes 0 and 2), and 1 .. 4 row segments per strip that the host picks by a cost
rule (CU count, pairs, TW_FI_MAXSEG, TW_FI_MINSTEPS), each re-priming its ring from rows ys - 15.  The kernel admits any
number of steps per segment >= 1; only the tuning constants keep the product away from segments shorter than the ring.
These tests set the two knobs (read once, in tw_engine_create) to reach those geometries with the PRODUCT library, ask
`Engine.flow_iter_plan` — tw_debug_flow_iter_plan, the function launch_flow_iter takes its grid from — which geometry each
launch ran, and assert that every class of geometry listed in CLASSES was reached.

Part A: the stage entry point (one pair), every case with the three flow sources, bit for bit against the oracle and, one
width per height, against the float64 reference within its own propagated bound (tests/farneback_f64.py: no new tolerance).
Part B: whole submissions under TW_MFREE=2 / TW_LATENCY_STREAMS=0 (the kernel for every launch of an eligible level, also
for a batch of one) — pair offsets, workgroup-count remainders mod 8 (xcd_remap), the segment count changing with the
batch size, and the handoff to the tile kernels at the 320 x 20 eligibility edge — dense fields against oracle.farneback.

Each stage case prints `figeom ...` (its resolved geometry) and `f64ref gpu flow_iter ...` lines under -s;
profiles/flow_iter_geometry.md records a run.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_oracle_stages_f64 as S  # noqa: E402
from conftest import interleaved, planar  # noqa: E402
from test_gpu_stages_f64 import _iter_ref, _oracle_iter, ran, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
NCH = 7  # chunks that prime a segment's ring (tw_flow_iter: RING / TH)
TH = 5   # rows per step (FI_TH)

# (TW_FI_MAXSEG, TW_FI_MINSTEPS) -> heights; None: the variable is not set.  What the rule makes of a height today is in
# profiles/flow_iter_geometry.md; the tests never restate the rule — if a retune moves a class out of reach, change the
# heights, not the assertion of test_every_geometry_class_is_reached.
DEFAULT, TINY, THREE, EIGHT = (None, None), (64, 2), (3, 5), (8, 7)
HEIGHTS = {
    DEFAULT: [21, 34, 36, 161, 162, 164, 241, 321, 326, 403],
    TINY: [20, 21, 31, 103, 116],
    THREE: [61, 66, 76, 91],
    EIGHT: [61, 91],
}
MODES = ("memory", "zero", "upsampled")
FAMILY = {"memory": "tw_flow_iter", "zero": "tw_flow_iter_zero", "upsampled": "tw_flow_iter_ups"}
RAN = {}  # (knobs, scale, h, w, mode) -> classes of the launch that was compared (filled by the stage tests)


def widths(h):
    """323: the third strip holds 3 columns (a partial quad), judged by the float64 reference as well; and 320 (exactly
    two strips) or 481 (a fourth strip of one column), alternating with the height."""
    return [(323, True), (481 if h % 2 else 320, False)]


def set_knobs(monkeypatch, knobs):
    for name, v in zip(("TW_FI_MAXSEG", "TW_FI_MINSTEPS"), knobs):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def classes_of(plan, h):
    """The classes (CLASSES) of one launch, from the plan of the launch and the height alone."""
    nsteps = (plan.segments - 1) * plan.nt + plan.nt_last
    last_rows = h - TH * (nsteps - 1)
    assert 1 <= plan.nt_last <= plan.nt and 1 <= last_rows <= TH and plan.segments >= 1 and plan.strips >= 1, (plan, h)
    c = set()
    if plan.segments == 1:
        if plan.nt < NCH:
            c.add("a: one segment of fewer than 7 steps")
        if plan.nt == NCH:
            c.add("b: one segment of exactly 7 steps")
        return c
    if plan.nt_last < plan.nt:
        c.add("c: several segments, the last one shorter")
    if plan.nt_last < NCH:
        c.add("d: a last segment of fewer than 7 steps")
    if plan.nt_last == 1:
        c.add("e: a last segment of one step")
    if plan.nt < NCH:
        c.add("f: several segments of fewer than 7 steps each")
    c.add("g: nt %s, last segment %s" % ("odd" if plan.nt % 2 else "even", "odd" if plan.nt_last % 2 else "even"))
    c.add("h: a last step of %d rows ends a multi-segment launch" % last_rows)
    return c


CLASSES = (["a: one segment of fewer than 7 steps", "b: one segment of exactly 7 steps",
            "c: several segments, the last one shorter", "d: a last segment of fewer than 7 steps",
            "e: a last segment of one step", "f: several segments of fewer than 7 steps each"] +
           ["g: nt %s, last segment %s" % (a, b) for a in ("odd", "even") for b in ("odd", "even")] +
           ["h: a last step of %d rows ends a multi-segment launch" % r for r in range(1, TH + 1)])
IN_EVERY_MODE = CLASSES[2:5]  # (i): classes (c) to (e) in each of the three modes


# ---- part A: one pair through the stage entry point ------------------------------------------------------------------------
def run_stage_case(twflow, oracle, monkeypatch, knobs, h, scale=0.5):
    set_knobs(monkeypatch, knobs)
    with twflow.Engine(0, twflow.default_params(pyrScale=scale), slots=1) as e:
        for w, with_f64 in widths(h):
            plan = e.flow_iter_plan(w, h, 1)
            cls = classes_of(plan, h)
            nsteps = (plan.segments - 1) * plan.nt + plan.nt_last
            assert nsteps == (h + TH - 1) // TH, (plan, h)
            print("figeom h=%d w=%d knobs=%s scale=%g pairs=1 strips=%d segments=%d nt=%d last=%d last_rows=%d classes=%s" % (
                h, w, knobs, scale, plan.strips, plan.segments, plan.nt, plan.nt_last, h - TH * (nsteps - 1),
                ",".join(sorted(k[0] for k in cls))))
            rng = np.random.default_rng(h * 11 + w)
            R0, R1 = S.fields(rng, h, w)
            R0[h // 2:, w // 2:] = 0  # flat quadrant: the regulariser decides there
            R1[h // 2:, w // 2:] = 0
            flow = S.flow_cases(rng, h, w)[0][1]  # sigma 2
            ph, pw = int(round(h * scale)), int(round(w * scale))
            prev = (rng.standard_normal((ph, pw, 2)) * 2).astype(F32)
            prev[0, 0, 0] = -0.0
            up = oracle.flow_upsample(prev, w, h, scale)
            sources = {"memory": (dict(flow=planar(flow)), flow), "zero": (dict(), np.zeros((h, w, 2), F32)),
                       "upsampled": (dict(prev=planar(prev)), up)}
            e.launch_counts(reset=True)
            for mode in MODES:
                kw, fin = sources[mode]
                got = e.stage_flow_iter(planar(R0), planar(R1), **kw)
                cnt = ran(e, FAMILY[mode], 1)
                assert cnt.flow_iter() == 1 and cnt.last_z[FAMILY[mode]] == 1, cnt
                case = "%dx%d/%s/seg%dx%d+%d%s" % (w, h, mode, plan.segments, plan.nt, plan.nt_last,
                                                  "" if knobs == DEFAULT else "/knobs%d,%d" % knobs)
                same_bits(got, planar(_oracle_iter(oracle, R0, R1, fin)), "tw_stage_flow_iter " + case)
                if with_f64:
                    S.check("gpu", "flow_iter", case + ("@%g" % scale if mode == "upsampled" else ""), interleaved(got),
                            *_iter_ref(R0, R1, fin))
                RAN[(knobs, scale, h, w, mode)] = cls


@pytest.mark.parametrize("h", HEIGHTS[DEFAULT])
def test_stage_geometry_default_knobs(twflow, oracle, monkeypatch, h):
    """The rule as tuned (at most 4 segments of at least 16 steps): fewer steps than the ring primes, exactly as many, one
    more; last segments shorter than the others by one to three steps; last steps of 1 .. 4 rows."""
    run_stage_case(twflow, oracle, monkeypatch, DEFAULT, h)


@pytest.mark.parametrize("h", HEIGHTS[TINY])
def test_stage_geometry_two_step_segments(twflow, oracle, monkeypatch, h):
    """TW_FI_MAXSEG=64, TW_FI_MINSTEPS=2: segments of two steps — every segment's warm-up spans several others — and a last
    segment of ONE step, of one row at 21 rows."""
    run_stage_case(twflow, oracle, monkeypatch, TINY, h)


@pytest.mark.parametrize("h", HEIGHTS[THREE])
def test_stage_geometry_three_short_segments(twflow, oracle, monkeypatch, h):
    """TW_FI_MAXSEG=3, TW_FI_MINSTEPS=5: segments of 5 .. 7 steps (shorter than, and as long as, the ring's priming), odd and
    even, with shorter last segments."""
    run_stage_case(twflow, oracle, monkeypatch, THREE, h)


@pytest.mark.parametrize("h", HEIGHTS[EIGHT])
def test_stage_geometry_seven_step_segments(twflow, oracle, monkeypatch, h):
    """TW_FI_MAXSEG=8, TW_FI_MINSTEPS=7: segments of exactly 7 steps with a shorter last one."""
    run_stage_case(twflow, oracle, monkeypatch, EIGHT, h)


@pytest.mark.parametrize("h", HEIGHTS[THREE])
def test_stage_geometry_three_short_segments_pyr_scale_075(twflow, oracle, monkeypatch, h):
    """The same launches with pyrScale 0.75: the upsampling mode's resize tables are inexact fractions at every segment's
    first and last rows (at 0.5 they are 0.25 / 0.75 throughout)."""
    run_stage_case(twflow, oracle, monkeypatch, THREE, h, scale=0.75)


def test_every_geometry_class_is_reached(twflow, monkeypatch):
    """The classes the heights above are there for, computed from the launch's own plan function and the height — never
    from a restatement of the rule.  A class out of reach (a retune, say) fails here by name: change the heights."""
    reached = {}
    for knobs, heights in HEIGHTS.items():
        set_knobs(monkeypatch, knobs)
        with twflow.Engine(0, twflow.default_params(), slots=1) as e:
            for h in heights:
                for w, _ in widths(h):
                    for c in classes_of(e.flow_iter_plan(w, h, 1), h):
                        reached.setdefault(c, []).append((knobs, h, w))
    for c in sorted(reached):
        print("figeom class %s: %s" % (c, " ".join("%dx%d%s" % (w, h, "" if k == DEFAULT else "@%d,%d" % k)
                                                   for k, h, w in reached[c])))
    missing = [c for c in CLASSES if c not in reached]
    assert not missing, "geometry classes no case reaches: %s" % "; ".join(missing)
    # (i): every case runs the three modes (run_stage_case loops over MODES); when the stage tests above ran in this
    # process, what they recorded must say so as well
    assert set(FAMILY) == set(MODES) and len(MODES) == 3
    ncases = sum(len(widths(h)) for hs in HEIGHTS.values() for h in hs) * len(MODES)
    if sum(1 for k in RAN if k[1] == 0.5) == ncases:
        for c in IN_EVERY_MODE:
            for mode in MODES:
                assert any(c in cls for k, cls in RAN.items() if k[4] == mode), "class '%s' never ran in mode %s" % (c, mode)


# ---- part B: whole submissions --------------------------------------------------------------------------------------------
@pytest.fixture
def mfree_everywhere(monkeypatch):
    """tw_flow_iter for every launch of an eligible level, batches of one included; one launch per level and batch
    (TW_RAMP=0: an idle engine would otherwise start a 64-pair batch in three pieces)."""
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.setenv("TW_RAMP", "0")
    return monkeypatch


_WANT = {}


def oracle_fields(oracle, h, w, n, **params):
    """(pairs, planar oracle fields) of the first n synth pairs of h x w, computed once per (size, parameters)."""
    import synth
    key = (h, w, tuple(sorted(params.items())))
    have = _WANT.setdefault(key, [])
    while len(have) < n:
        a, b = synth.make_pair(len(have), h, w)
        have.append(((a, b), np.stack(oracle.farneback(a, b, oracle.default_params(**params)))))
    return [p for p, _ in have[:n]], [f for _, f in have[:n]]


def run_batch(e, pairs, want, n, what):
    """n pairs (the distinct ones cycled) as one batch; every dense field bit for bit; returns the launch counters."""
    k = len(pairs)
    e.launch_counts(reset=True)
    out, _ = e.flow_batch([pairs[i % k][0] for i in range(n)], [pairs[i % k][1] for i in range(n)], layout="planar")
    cnt = e.launch_counts(reset=True)
    for i in range(n):
        same_bits(out[i], want[i % k], "%s, pair %d of %d" % (what, i, n))
    return cnt


def test_batches_change_the_segment_count(twflow, oracle, mfree_everywhere):
    """646 x 326 (level 0: 5 strips, 66 steps; level 1, 323 x 163: 3 strips, 33 steps), batches of 1 .. 64 pairs: the rule
    trades segments against rounds of workgroups, so the segment count of BOTH levels changes with the batch size, with
    uneven last segments among them; every pair's offset into the planes is a multiple of a different plane size per level."""
    h, w = 326, 646
    pairs, want = oracle_fields(oracle, h, w, 4)
    seen = {0: set(), 1: set()}
    for n in (1, 3, 8, 24, 64):
        with twflow.Engine(0, twflow.default_params(), slots=n) as e:
            assert [e.level_runs_flow_iter(w, h, k, n) for k in range(4)] == [True, True, False, False]
            cnt = run_batch(e, pairs, want, n, "%dx%d" % (w, h))
            assert cnt["tw_flow_iter_ups"] == 2 and cnt["tw_flow_iter"] == 4 and cnt["tw_flow_iter_zero"] == 0, cnt
            assert cnt.last_z["tw_flow_iter"] == n and cnt.last_z["tw_flow_iter_ups"] == n, cnt.last_z
            for k, (lw, lh) in enumerate(((w, h), (w // 2, h // 2))):
                plan = e.flow_iter_plan(lw, lh, n)
                seen[k].add(plan.segments)
                print("figeom h=%d w=%d knobs=%s pairs=%d level=%d strips=%d segments=%d nt=%d last=%d last_rows=%d" % (
                    lh, lw, DEFAULT, n, k, plan.strips, plan.segments, plan.nt, plan.nt_last, lh - TH * ((lh + TH - 1) // TH - 1)))
    for k in (0, 1):
        assert len(seen[k]) >= 2, "level %d ran with %r segments per strip at every batch size" % (k, sorted(seen[k]))


@pytest.mark.parametrize("knobs", [DEFAULT, TINY])
def test_batches_cover_the_workgroup_remainders(twflow, oracle, mfree_everywhere, knobs):
    """323 x 101 with pyrLevels 0 — level 0 is the coarsest level: tw_flow_iter_zero, then tw_flow_iter twice — in batches
    of 1, 2, 3, 5 and 7 pairs: strips x segments x pairs workgroups leave odd and even remainders mod 8 for xcd_remap.
    Under (64, 2) the same submissions run mode 2 in two-step segments with a one-step last segment."""
    h, w = 101, 323
    set_knobs(mfree_everywhere, knobs)
    pairs, want = oracle_fields(oracle, h, w, 4, pyrLevels=0)
    rem = set()
    for n in (1, 2, 3, 5, 7):
        with twflow.Engine(0, twflow.default_params(pyrLevels=0), slots=n) as e:
            assert e.num_levels(w, h) == 0 and e.level_runs_flow_iter(w, h, 0, n)
            cnt = run_batch(e, pairs, want, n, "%dx%d levels 0 knobs %s" % (w, h, knobs))
            assert cnt["tw_flow_iter_zero"] == 1 and cnt["tw_flow_iter"] == 2 and cnt["tw_flow_iter_ups"] == 0, cnt
            assert cnt.last_z["tw_flow_iter"] == n and cnt.last_z["tw_flow_iter_zero"] == n, cnt.last_z
            assert cnt["tw_update_matrices"] == 0, cnt
            plan = e.flow_iter_plan(w, h, n)
            wgs = plan.strips * plan.segments * cnt.last_z["tw_flow_iter"]
            rem.add(wgs % 8)
            print("figeom h=%d w=%d knobs=%s pairs=%d level=0 strips=%d segments=%d nt=%d last=%d last_rows=%d workgroups=%d" % (
                h, w, knobs, n, plan.strips, plan.segments, plan.nt, plan.nt_last, h - TH * ((h + TH - 1) // TH - 1), wgs))
            if knobs == TINY:
                assert "e: a last segment of one step" in classes_of(plan, h), plan
    assert len(rem) >= 5 and sum(r % 2 for r in rem) >= 3, "workgroup counts mod 8 covered only %r" % sorted(rem)


# (h, w) -> does level k run tw_flow_iter?  One entry per level of the plan: a level exists only while both sides stay >= 32
# pixels, so the four 38 .. 40-row sizes have ONE level (no level of 20 rows above level 0 can exist) and the 20-row edge is
# reached at level 0 alone; the 320-column edge is reached at level 1 of 64-row images, 639 columns among them (319.5 rounds
# half to even, to 320).
EDGE_SIZES = [(40, 640, [True]), (39, 640, [True]), (38, 640, [True]), (40, 638, [True]),
              (20, 640, [True]), (19, 640, [False]),
              (64, 640, [True, True]), (64, 639, [True, True]), (64, 638, [True, False]), (65, 640, [True, True])]


@pytest.mark.parametrize("it", [1, 2, 3])
@pytest.mark.parametrize("h,w,want_runs", EDGE_SIZES)
def test_handoff_between_kernel_families_at_the_eligibility_edge(twflow, oracle, mfree_everywhere, h, w, want_runs, it):
    """320 columns x 20 rows is the smallest level tw_flow_iter takes.  Two pairs per batch, one to three iterations (the
    ping-pong between the flow planes ends differently): a 20-row image runs it from zero flow and a 19-row image the tile
    kernels alone; level 1 of 640 x 64 (320 x 32) runs it, level 1 of 638 x 64 (319 columns) runs the tile kernels and hands
    their flow to tw_flow_iter<UPS> at level 0.  Which level ran what is asserted from the schedule's own predicate and the
    launch counters."""
    pairs, want = oracle_fields(oracle, h, w, 2, pyrIterations=it)
    with twflow.Engine(0, twflow.default_params(pyrIterations=it), slots=2) as e:
        levels = e.num_levels(w, h)
        runs = [e.level_runs_flow_iter(w, h, k, 2) for k in range(levels + 1)]
        assert runs == want_runs, (levels, runs)
        cnt = run_batch(e, pairs, want, 2, "%dx%d, %d iterations" % (w, h, it))
        nfi, coarsest = sum(runs), int(runs[levels])
        assert cnt["tw_flow_iter_zero"] == coarsest and cnt["tw_flow_iter_ups"] == nfi - coarsest, cnt
        assert cnt["tw_flow_iter"] == nfi * (it - 1), cnt
        assert all(cnt.last_z[f] == 2 for f in FAMILY.values() if cnt[f]), cnt.last_z
        # the other levels: one first update each, by tw_update_matrices; none at a level tw_flow_iter ran
        assert cnt["tw_update_matrices"] == levels + 1 - nfi, cnt
