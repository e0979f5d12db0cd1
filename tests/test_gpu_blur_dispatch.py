"""The choice of the window average + solve kernel (choose_blur in twflow.hip), edge by edge.

Every case is a single tw_stage_blur_solve call, with and without the fused matrix refresh, bit-exact against the oracle's
stage.  The sizes sit on both sides of an edge of the choice; which side a size is on is read off `Engine.blur_plan`
(tw_debug_blur_plan: the function launch_blur itself takes its kernel and grid from) and asserted as reached, and the
launch counters prove that the planned family is the one that ran.
"""
import numpy as np
import pytest

from conftest import interleaved, planar
from test_gpu_parity import _rand_fields, assert_same

pytestmark = pytest.mark.gpu


def _ceil_div(a, b):
    return -(-a // b)


def _run_stage(e, oracle, w, h, win=30, gaussian=True):
    """Both kinds of launch at w x h on engine e against one oracle call; returns the plan of the refreshing one."""
    rng = np.random.default_rng(w * 7 + h)
    R0, R1, flow0 = _rand_fields(rng, h, w, mag=1.0)
    M = planar(oracle.update_matrices(interleaved(R0), interleaved(R1), interleaved(flow0)))
    M[:, h // 2:, w // 2:] = 0  # flat region: det ~ regulariser 1e-3
    # (the flow of an iteration does not depend on whether M is refreshed after it: one reference serves both launches)
    wflow, wM = oracle.update_flow(interleaved(R0), interleaved(R1), interleaved(flow0), interleaved(M), win, 1, gaussian)
    plans = []
    for update in (0, 1):
        plan = e.blur_plan(w, h, level=-1, npairs=1, update=update)
        if gaussian:
            assert (plan.grid_x, plan.grid_y) == (_ceil_div(w + plan.xsh, plan.tile_cols), _ceil_div(h, plan.rows)), plan
        e.launch_counts(reset=True)
        gflow, gM = e.stage_blur_solve(R0, R1, M, update)
        cnt = e.launch_counts()
        ran = {k: v for k, v in cnt.items() if v}
        if gaussian:
            assert ran == {plan.family: 1}, (w, h, update, plan, ran)
        else:
            assert ran == dict({"tw_box": 2}, **({"tw_update_matrices": 1} if update else {})), (w, h, update, plan, ran)
        assert_same(gflow, planar(wflow), "flow %dx%d win %d update %d %r" % (w, h, win, update, plan))
        if update:
            assert_same(gM, planar(wM), "refreshed M %dx%d win %d %r" % (w, h, win, plan))
        plans.append(plan)
    # the default build has no kernel whose choice depends on `update` (TW_BLUR_PIPE is the variants library's)
    assert plans[0] == plans[1], plans
    return plans[1]


# (edge, size on one side, what the plan must say there, size on the other side, what it must say there)
EDGES = [
    # 96 x 8 tiles: 4 x 64 = 256 workgroups of two waves reach TW_PP_WAVES = 512, 4 x 63 = 252 do not
    ("pp_waves", (384, 512), dict(family="tw_blur_solve4", small=0, block=128, tile_cols=96, rows=8),
     (384, 504), dict(family="tw_blur_solve_pp", small=4, block=320, tile_cols=32, rows=8)),
    # w > 480 is "wide": both run the 96-column tw_blur_solve4, the narrow level as class 0, the wide one as class 1
    ("narrow/wide", (480, 520), dict(family="tw_blur_solve4", small=0, block=128, tile_cols=96),
     (481, 520), dict(family="tw_blur_solve4", small=1, block=128, tile_cols=96)),
    # two-wave 96 x 8 class: 560 + 16 still fits six tile columns, 576 + 16 would need a seventh
    ("shift, 96 x 8", (560, 344), dict(family="tw_blur_solve4", small=1, xsh=16, grid_x=6),
     (576, 344), dict(family="tw_blur_solve4", small=1, xsh=0, grid_x=6)),
    # plane-parallel 32 x 8 class: 18 tile columns hold 560 + 16, 576 fills them
    ("shift, 32 x 8", (560, 64), dict(family="tw_blur_solve_pp", small=4, xsh=16, grid_x=18),
     (576, 64), dict(family="tw_blur_solve_pp", small=4, xsh=0, grid_x=18)),
    # 224 x 8 tiles: 8 x 128 = 1024 workgroups are the throughput regime, 8 x 127 = 1016 take the 96 x 8 tiles
    ("throughput", (1792, 1024), dict(family="tw_blur_solve4", small=0, block=256, tile_cols=224),
     (1792, 1016), dict(family="tw_blur_solve4", small=1, block=128, tile_cols=96)),
]


@pytest.mark.parametrize("edge,size_a,want_a,size_b,want_b", EDGES, ids=[c[0] for c in EDGES])
def test_both_sides_of_each_edge_of_the_31_tap_choice(engine, oracle, edge, size_a, want_a, size_b, want_b):
    for (w, h), want in ((size_a, want_a), (size_b, want_b)):
        plan = _run_stage(engine, oracle, w, h)
        assert not plan.forced, plan
        got = {k: getattr(plan, k) for k in want}
        assert got == want, (edge, w, h, plan)


def test_51_tap_window_narrow_and_wide(twflow, oracle):
    """winSize 50: tw_blur_solve8 up to 480 columns, tw_blur_solve4y (two sub-tiles per workgroup) above."""
    with twflow.Engine(0, twflow.default_params(winSize=50), slots=1) as e:
        narrow = _run_stage(e, oracle, 480, 72, win=50)
        wide = _run_stage(e, oracle, 481, 72, win=50)
    assert (narrow.family, narrow.block, narrow.tile_cols, narrow.rows, narrow.xsh) == ("tw_blur_solve8", 128, 64, 8, 0), narrow
    assert (wide.family, wide.block, wide.tile_cols, wide.rows, wide.xsh) == ("tw_blur_solve4y", 256, 192, 16, 0), wide


def test_any_other_window_size_takes_the_generic_kernel(twflow, oracle):
    with twflow.Engine(0, twflow.default_params(winSize=13), slots=1) as e:
        plan = _run_stage(e, oracle, 203, 131, win=13)
    assert (plan.family, plan.block, plan.tile_cols, plan.rows) == ("tw_blur_solve_generic", 256, 64, 8), plan


def test_box_window_takes_the_two_scan_kernels(twflow, oracle):
    with twflow.Engine(0, twflow.default_params(flags=0), slots=1) as e:
        plan = _run_stage(e, oracle, 203, 131, gaussian=False)
    assert plan.family == "tw_box" and (plan.grid_x, plan.grid_y) == (4, 5), plan


def test_forced_class_is_reported_as_forced(twflow, oracle, monkeypatch):
    """TW_BLUR_SMALL sets the class whatever the grid's size: the plan says so (what keeps level 1 of the single-pair
    schedule from planning side jobs onto launches that were switched to another kernel)."""
    monkeypatch.setenv("TW_BLUR_SMALL", "4")
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        assert e.blur_plan(1792, 1024, level=1).forced and e.blur_plan(1792, 1024, level=1).small == 4
        plan = _run_stage(e, oracle, 203, 131)
    assert (plan.family, plan.small, plan.forced) == ("tw_blur_solve_pp", 4, True), plan


def test_level_1_of_a_1080p_pair_still_carries_level_0s_expansion(twflow):
    """The single-pair schedule plans level 0's polynomial expansion onto level 1's window launches when choose_blur gives
    level 1 (960 x 540) the 96 x 8 two-wave tiles by its size: those launches are TW_DF_TWIN launches (tw_twin_s4_poly), not
    plain tw_blur_solve4 ones.  (The values are checked in test_gpu_parity.py: test_single_pair_schedule_of_twin_launches.)"""
    import synth
    a, b = synth.make_pair(7, 1080, 1920)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        l1 = e.blur_plan(960, 540, level=1, npairs=1, update=True)
        assert (l1.family, l1.small, l1.forced, l1.tile_cols, l1.rows) == ("tw_blur_solve4", 1, False, 96, 8), l1
        l0 = e.blur_plan(1920, 1080, level=0, npairs=1, update=True, quads=True)
        assert (l0.family, l0.small, l0.block) == ("tw_blur_solve4q", 0, 256), l0
        e.diff(a, b, 10, 0.5)
        cnt = e.launch_counts()
    # twins: the coarsest level's expansion, level 3's update and 3 window launches, level 1's 3 window launches
    assert cnt["tw_twin"] == 8 and cnt["tw_blur_solve4"] == 0 and cnt["tw_blur_solve4q"] == 3, cnt
    assert cnt["tw_polyexp"] == 0 and cnt["tw_blur_solve_pp"] == 3, cnt
