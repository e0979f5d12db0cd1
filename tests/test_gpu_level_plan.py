"""The level schedule: what a batch launches for each pyramid level is one pure choice (choose_level_schedule), the enqueue
executes it, and Engine.level_plan shows it.

Every case submits a batch, predicts the launches of every kernel family of the level loop — and the pairs (grid z) of each
family's last launch — from the plan (the twin schedule's side jobs: from the plan and the window launches' own choice,
Engine.blur_plan — predict_twin), compares them with the engine's launch counters, checks that level_runs_flow_iter
and level_chunk are views of the same plan, and compares the hit vectors with the oracle's at span 10, threshold 0 (every
grid point).  Nothing is expected from constants: tw_flow_iter's gate depends on the CU count.  The last test asserts that the
cases together take every value of every field of the plan, so that reading the expectation from the plan hides no branch.

TW_RAMP=0 in every case: the pieces of a cold-start ramp depend on what the stream is doing when the batch arrives, and no
plan made in advance knows them (each piece gets the choice for its own pairs from the same function).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_grid_final import batch_pairs, oracle_field  # noqa: E402  (the pairs and the oracle's fields, computed once)

pytestmark = pytest.mark.gpu

OWN, FROM_COARSER, WITH_FINER = 0, 1, 2
PYR_OWN = ("tw_pyr_k3", "tw_pyr_taps", "tw_pyr_level")
WINDOWS = ("tw_blur_solve4", "tw_blur_solve4y", "tw_blur_solve8", "tw_blur_solve_pp", "tw_blur_solve_generic",
           "tw_blur_variant", "tw_blur_solve4q", "tw_box")
SWITCHES = ("TW_MFREE", "TW_LANES", "TW_CHUNK_TILES", "TW_CHUNK_PAIRS_LEVELS", "TW_GRID_FINAL", "TW_LAT_FUSED", "TW_LAT_GRAPH",
            "TW_LATENCY_STREAMS", "TW_LATENCY_MIN_PX", "TW_PYR_FUSED", "TW_PYR_GENERIC", "TW_SAME_IMAGE", "TW_LAT_QUADS",
            "TW_LAT_PLAN", "TW_LAT_ALONE", "TW_LAT_BANDS", "TW_SCAN_SEG")

# name: (w, h, pairs, environment, scan-fused option, a host flow destination for pair 1)
CASES = {
    "32_default": (640, 480, 32, {}, False, False),
    "24_default": (640, 480, 24, {}, False, False),
    "3_under_the_gate": (640, 480, 3, {}, False, False),
    "24_chunk_tiles_100": (640, 480, 24, {"TW_CHUNK_TILES": "100"}, False, False),
    "24_chunk_tiles_100_lanes_2": (640, 480, 24, {"TW_CHUNK_TILES": "100", "TW_LANES": "2"}, False, False),
    "24_mfree_0": (640, 480, 24, {"TW_MFREE": "0"}, False, False),
    "24_scan_fused_final": (640, 480, 24, {}, True, False),
    "24_flow_destination": (640, 480, 24, {}, False, True),
    "24_grid_final_0": (640, 480, 24, {"TW_GRID_FINAL": "0"}, False, False),
    "24_of_645x483": (645, 483, 24, {}, False, False),
    "1_default": (640, 480, 1, {}, False, False),
    "1_lat_fused_0": (640, 480, 1, {"TW_LAT_FUSED": "0"}, False, False),
    "1_of_645x483": (645, 483, 1, {}, False, False),
    "1_of_180x117": (180, 117, 1, {}, False, False),
}
_PLANS = {}  # case -> the plan its batch ran with (test_the_cases_reach_every_value_of_the_plan)
SPAN, IT = 10, 3


def set_env(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TW_RAMP", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_engine(twflow, monkeypatch, case):
    """The case's engine, in the case's environment, and the plan of the case's batch."""
    w, h, n, env, scan_fused, fout = CASES[case]
    set_env(monkeypatch, env)
    e = twflow.Engine(0, twflow.default_params(), slots=n)
    if scan_fused:
        e.set_option(twflow.OPT_SCAN_FUSED_FINAL, 1)
    _PLANS[case] = e.level_plan(w, h, SPAN, n, any_fout=fout)
    return e, _PLANS[case]


def predict_twin(e, plan, it, w, h, launch):
    """The twin schedule's launches, every one of a single pair.  The plan says where the images come from: tw_pyr_23 for levels
    3 and 2, tw_pyr_k3f for levels 1 and 0 — a side job that the coarsest level's expansion carries (one tw_twin launch).  The
    expansions of levels 2, 1 and 0 are side jobs too (plan_twin_side_jobs with the default TW_LAT_PLAN / TW_LAT_BANDS /
    TW_LAT_ALONE, which set_env restores): level 2's as one job on any launch of the chain; when level 1's window launches take the
    96 x 8 two-wave tiles by their size (blur_plan: small class 1, not forced) level 1's in `it` bands of tile rows on level 3's
    window launches and level 0's in `it` bands on level 1's, otherwise level 1's as one job and level 0's image by image on
    any launch.  A chain launch of levels 3 .. 1 that may take the next job carries it — the update launch always (tw_twin), a
    window launch when its kernel has a twin (the small-grid classes 1 and 4 of blur_plan) — and every job not carried by the time
    its level starts, or offered to a window kernel without a twin, goes out alone (tw_polyexp).  Every job is launched once."""
    assert [r.images for r in plan.parts[0]] == [FROM_COARSER, WITH_FINER, FROM_COARSER, WITH_FINER] and plan.levels == 3
    size = [(w >> k, h >> k) for k in range(4)]  # (the twin schedule needs the exact halving pyramid)
    gy = [-(-size[k][1] // 8) for k in range(4)]  # tile rows of a level's expansion
    jobs = [(2, -1, False)]  # (the level that needs it, the only level whose launches may carry it or -1, window launches only)
    c1 = e.blur_plan(size[1][0], size[1][1], level=1, npairs=1, update=True, quads=False)
    if c1.small == 1 and not c1.forced:
        for k, carry in ((1, 3), (0, 1)):
            rows = -(-gy[k] // it)
            jobs += [(k, carry, True)] * -(-gy[k] // rows)
    else:
        jobs += [(1, -1, False), (0, -1, False), (0, -1, False)]
    launch("tw_pyr_23", 2)
    launch("tw_twin", 1)  # level 3's expansion with tw_pyr_k3f (twin grids are one-dimensional: z = 1)

    def offered(k, window):
        return bool(jobs) and jobs[0][1] in (-1, k) and (window or not jobs[0][2])

    for k in range(3, -1, -1):
        while jobs and jobs[0][0] >= k:
            jobs.pop(0)
            launch("tw_polyexp", 1)  # (a band launch: grid x only)
        if k >= 1 and offered(k, False):
            jobs.pop(0)
            launch("tw_twin", 1)
        else:
            launch("tw_update_matrices", 1)
        for i in range(it):
            if k >= 1 and offered(k, True):
                jobs.pop(0)
                c = e.blur_plan(size[k][0], size[k][1], level=k, npairs=1, update=i < it - 1, quads=False)
                if c.small in (1, 4):
                    launch("tw_twin", 1)
                else:
                    launch("windows", 1)
                    launch("tw_polyexp", 1)
            else:
                launch("windows", 1)
    assert not jobs


def predict(plan, it, span, e=None, w=0, h=0):
    """({family or group: launches}, {family or group: [grid z of every launch, in launch order]}) of the level loop."""
    z = {}

    def launch(fam, gz):
        z.setdefault(fam, []).append(gz)

    if plan.kind == "twin":
        predict_twin(e, plan, it, w, h, launch)

    if plan.kind == "batch":
        for rows in plan.parts:
            launch("tw_pair_same", rows[0].pairs)  # (every part of the batch schedule: TW_SAME_IMAGE is left alone)
            for k in range(plan.levels, -1, -1):
                r = rows[k]
                for i in range(r.launches):
                    nc = r.per if i < r.launches - 1 else r.tail
                    fi = r.flow_iter if nc == r.per else r.flow_iter_last
                    if r.images == OWN:
                        launch("pyr_own", 2 * nc)
                    elif r.images == WITH_FINER:
                        launch("tw_pyr_23" if k == 3 else "tw_pyr_k3f", 2 * nc)
                    launch("tw_polyexp", 2 * nc)
                    grid_only = k == 0 and plan.fused_final
                    grid_last = k == 0 and plan.grid_final and fi
                    if fi:
                        nfi = it - 1 if grid_only else it
                        first = "tw_flow_iter_ups" if k < plan.levels else "tw_flow_iter" if r.init else "tw_flow_iter_zero"
                        for j in range(nfi):
                            launch(first if j == 0 else "tw_flow_iter", nc)
                        if grid_last:
                            launch("tw_flow_iter_grid", nc)
                        if grid_only:
                            launch("tw_update_matrices", nc)
                            launch("tw_blur_grid", nc)
                    else:
                        launch("tw_update_matrices", nc)
                        for j in range(it):
                            launch("tw_blur_grid" if grid_only and j == it - 1 else "windows", nc)
                    if k == 0 and span > 0 and not grid_only and not grid_last:
                        launch("tw_span_gather", nc)
    elif plan.kind == "two_stream":
        # the image-only work is enqueued one level ahead of the chain; every launch covers the one pair
        for k in range(plan.levels, -1, -1):
            launch("pyr_own", 2)
            launch("tw_polyexp", 2)
            launch("tw_update_matrices", 1)
            for j in range(it):
                launch("tw_blur_grid" if k == 0 and plan.fused_final and j == it - 1 else "windows", 1)
    return {f: len(v) for f, v in z.items()}, z


def grouped(cnt):
    """The counters with the pyramid kernels of a level of its own and the fixed-window kernels summed."""
    out = dict(cnt)
    out["pyr_own"] = sum(out.pop(f) for f in PYR_OWN)
    out["windows"] = sum(out.pop(f) for f in WINDOWS)
    return out


def predict_own_pyramid(e, plan, w, h):
    """{family: launches} of the pyramid launches of a level's own, each from the family Engine.pyr_plan (choose_pyr, the
    function launch_pyr itself launches from) names for that level; a staged generic launch counts in tw_pyr_level as well."""
    want = dict.fromkeys(PYR_OWN + ("tw_pyr_level_lds",), 0)
    for rows in plan.parts:
        for k, r in enumerate(rows):
            if r.images == OWN:
                fam = e.pyr_plan(w, h, k).family
                assert fam in want, (k, fam)
                want[fam] += r.launches
                if fam == "tw_pyr_level_lds":
                    want["tw_pyr_level"] += r.launches
    return want


LEVEL_LOOP = ("pyr_own", "tw_pyr_23", "tw_pyr_k3f", "tw_polyexp", "tw_update_matrices", "tw_flow_iter", "tw_flow_iter_ups",
              "tw_flow_iter_zero", "tw_flow_iter_grid", "windows", "tw_blur_grid", "tw_twin", "tw_pair_same", "tw_span_gather")


@pytest.mark.parametrize("case", list(CASES))
def test_the_enqueue_launches_what_the_plan_says(twflow, oracle, monkeypatch, case):
    w, h, n, env, scan_fused, fout = CASES[case]
    pairs = batch_pairs(h, w, n)
    span, it = SPAN, IT
    engine, plan = make_engine(twflow, monkeypatch, case)
    with engine as e:
        print("levelplan %s: %s" % (case, plan))
        out = e.host_array((2, h, w), np.float32) if fout else None
        e.launch_counts(reset=True)
        tk = [e.submit(a, b, span, 0.0, flow=(out if fout and i == 1 else None)) for i, (a, b) in enumerate(pairs)]
        got = [e.wait(t)["vector"] for t in tk]
        cnt = e.launch_counts(reset=True)
        g = grouped(cnt)
        print("levelplan %s: launches %s last z %s" % (case, {k: v for k, v in cnt.items() if v}, {k: v for k, v in cnt.last_z.items() if cnt[k]}))

        # the exports are views of the plan: a batch that returns records only, its first part
        view = e.level_plan(w, h, span, n)
        assert e.num_levels(w, h) == plan.levels
        for k in range(plan.levels + 1):
            r = view.parts[0][k]
            assert e.level_runs_flow_iter(w, h, k, n) == r.flow_iter, (case, k)
            chunk = e.level_chunk(w, h, k)
            assert 1 <= chunk <= n
            if plan.kind == "batch":
                assert r.per == -(-r.pairs // -(-r.pairs // chunk)) and r.launches == -(-r.pairs // r.per), (case, k, r, chunk)
                assert r.tail == r.pairs - r.per * (r.launches - 1) and 1 <= r.tail <= r.per
        assert len(plan.parts) == plan.nlanes and sum(rows[0].pairs for rows in plan.parts) == n

        # the launches
        assert plan.kind in ("batch", "two_stream", "twin")
        assert cnt["tw_box"] == 0
        want, wz = predict(plan, it, span, e, w, h)
        assert {f: g[f] for f in LEVEL_LOOP} == {f: want.get(f, 0) for f in LEVEL_LOOP}, (case, cnt, want)
        # every level's pyramid launch of its own comes from the family choose_pyr names for it
        # (the twin schedule has no such launch: tw_pyr_23 and tw_pyr_k3f write all four levels, predict_twin asserts it)
        if plan.kind != "twin":
            own = predict_own_pyramid(e, plan, w, h)
            assert {f: cnt[f] for f in own} == own, (case, cnt, own)
            assert sum(own[f] for f in PYR_OWN) == want.get("pyr_own", 0)
        else:
            assert g["pyr_own"] == 0 and cnt["tw_pyr_level_lds"] == 0, cnt
        # (tw_flow_iter_grid is ALSO counted in tw_flow_iter, twflow_debug.h: predict() launches it into both, as the counters do)
        for fam, zs in wz.items():
            members = PYR_OWN if fam == "pyr_own" else WINDOWS if fam == "windows" else (fam,)
            last = [cnt.last_z[f] for f in members if cnt[f]]
            assert last and set(last) <= set(zs) and zs[-1] in last, (case, fam, last, zs)
        if plan.kind == "twin":
            assert want["tw_twin"] >= 2, want  # (the head's and at least the update launch of level 3: side jobs were carried)
        if fout:
            assert cnt["tw_flow_export"] >= 1, cnt

        # the results
        for i in range(n):
            f = oracle_field(oracle, h, w, i, it)
            assert got[i] == oracle.span_scan(f[0], f[1], span, 0.0), (case, i)
        if fout:
            assert np.array_equal(np.array(out).view(np.uint32), oracle_field(oracle, h, w, 1, it).view(np.uint32))


def test_own_pyramid_launches_at_pyr_scale_06_come_from_the_planned_families(twflow, oracle, monkeypatch):
    """pyrScale 0.6, 333 x 257, four pairs: no level halves exactly, so every level launches a pyramid kernel of its own — level 0
    tw_pyr_k3<0>, level 1 (3 taps, INTER_LINEAR) the staged generic kernel, levels 2 and 3 (5 / 9 taps) the staged generic
    kernel and tw_pyr_taps — each from the family Engine.pyr_plan names, and the fields are the oracle's."""
    w, h, n = 333, 257, 4
    import synth
    pairs = [synth.make_pair(i, h, w) for i in range(n)]
    set_env(monkeypatch, {})
    with twflow.Engine(0, twflow.default_params(pyrScale=0.6), slots=n) as e:
        plan = e.level_plan(w, h, 0, n, any_fout=True)
        assert plan.kind == "batch" and plan.levels == 3 and all(r.images == OWN for rows in plan.parts for r in rows), plan
        fams = [e.pyr_plan(w, h, k).family for k in range(4)]
        assert fams[0] == "tw_pyr_k3" and set(fams) == {"tw_pyr_k3", "tw_pyr_level_lds", "tw_pyr_taps"}, fams
        out = e.host_array((n, 2, h, w), np.float32)
        e.launch_counts(reset=True)
        tk = [e.submit(a, b, 0, 5.0, flow=out[i]) for i, (a, b) in enumerate(pairs)]
        for t in tk:
            e.wait(t)
        cnt = e.launch_counts(reset=True)
        own = predict_own_pyramid(e, plan, w, h)
        assert {f: cnt[f] for f in own} == own and sum(own[f] for f in PYR_OWN) == sum(r.launches for rows in plan.parts for r in rows), (cnt, own)
        assert cnt["tw_pyr_23"] == 0 and cnt["tw_pyr_k3f"] == 0, cnt
        for i, (a, b) in enumerate(pairs):
            f = np.stack(oracle.farneback(a, b, oracle.default_params(pyrScale=0.6)))
            assert np.array_equal(np.array(out[i]).view(np.uint32), f.view(np.uint32)), i


def test_the_cases_reach_every_value_of_the_plan(twflow, monkeypatch):
    """Across the cases every field of the plan takes each of its values (the expectations above come from the plan)."""
    for case in CASES:
        if case not in _PLANS:  # (this test alone: the plans without the batches)
            make_engine(twflow, monkeypatch, case)[0].close()
    plans = list(_PLANS.values())
    rows = [r for p in plans for part in p.parts for r in part]
    assert {p.kind for p in plans} == {"batch", "two_stream", "twin"}
    assert {r.flow_iter for r in rows} == {True, False}
    assert {r.images for r in rows} == {OWN, FROM_COARSER, WITH_FINER}
    # both launches that write two levels, in the batch schedule too
    batch_rows = [(k, r) for p in plans if p.kind == "batch" for part in p.parts for k, r in enumerate(part)]
    assert {k for k, r in batch_rows if r.images == WITH_FINER} == {1, 3}
    assert {p.fused_final for p in plans} == {True, False}
    assert {p.grid_final for p in plans} == {True, False}
    assert {p.nlanes for p in plans} == {1, 2}
    assert {r.same for r in rows} == {True, False} and any(r.same01 for r in rows)
    assert any(r.launches > 1 for r in rows) and any(p.lat_quads for p in plans)
    # the named cases are what their names say
    assert _PLANS["1_default"].kind == "twin" and _PLANS["1_lat_fused_0"].kind == "two_stream"
    assert _PLANS["1_of_645x483"].kind == "two_stream" and _PLANS["1_of_180x117"].kind == "batch"
    assert not any(r.flow_iter for r in _PLANS["3_under_the_gate"].parts[0])
    assert not any(r.flow_iter for r in _PLANS["24_mfree_0"].parts[0])
    assert _PLANS["24_scan_fused_final"].fused_final and not _PLANS["24_flow_destination"].grid_final
    assert not _PLANS["24_grid_final_0"].grid_final and _PLANS["24_default"].grid_final
    assert _PLANS["24_default"].parts[0][0].flow_iter and _PLANS["32_default"].parts[0][1].images == WITH_FINER


def test_an_engine_reads_its_switches_once(twflow, monkeypatch):
    """An engine's switches are read when it is created: its plans do not move when the environment does, and an engine
    created afterwards takes the new values (no launches: the plan exports only)."""
    for name in SWITCHES + ("TW_FI_MAXSEG", "TW_RAMP"):
        monkeypatch.delenv(name, raising=False)

    def plans(e):
        return {"level": e.level_plan(1920, 1080, 10, 16), "flow_iter": e.flow_iter_plan(1920, 1080, 16),
                "blur": e.blur_plan(1920, 1080, 2, 16), "pyr": e.pyr_plan(1920, 1080, 3)}

    with twflow.Engine(0, twflow.default_params(), slots=16) as first:
        before = plans(first)
        for name, value in (("TW_MFREE", "0"), ("TW_PYR_GENERIC", "1"), ("TW_LANES", "2"), ("TW_FI_MAXSEG", "8"),
                            ("TW_CHUNK_TILES", "1000")):
            monkeypatch.setenv(name, value)
        assert plans(first) == before
        with twflow.Engine(0, twflow.default_params(), slots=16) as second:
            after = plans(second)
        assert after["level"] != before["level"] and after["pyr"] != before["pyr"], (before, after)
        assert plans(first) == before
