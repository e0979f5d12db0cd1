"""The cases of the pyramid kernel choice (choose_pyr in twflow.hip), edge by edge: one table for tests/test_pyr_cases.py
(CPU: the oracle's level against the float64 reference, and that the table holds what it claims) and
tests/test_gpu_pyr_dispatch.py (each case one tw_stage_pyr_level call, the plan read from Engine.pyr_plan).

A level's kernel depends on its scale and tap count, not on the image's area, so every image is the smallest the plan admits
for its purpose: a level exists only while both of its sides are at least 32 pixels (plan_levels), which is why no level
below level 0 is narrower than 32 columns or shorter than 32 rows.

What the table CANNOT hold, because no admitted parameters reach it (profiles/pyr_dispatch.md has the derivations):
  * tw_pyr_taps<39>: a 39-tap level has 1 / scale >= 16, its 8-row tile a row buffer of at least 151 rows and a staged span of
    at least 534 bytes — 39 KB + 80 KB against plan_geometry's 64 KB budget.  The largest staged kernel has 25 taps.
  * tw_pyr_23<256>: only TW_PYR23_THREADS=256 selects it (tested once under that switch).
  * the generic kernels' mode == 2 branch: an exact halving is level 1 of pyrScale 0.5, whose 3 taps take tw_pyr_k3<2> whenever
    the image is at least 16 columns wide — and an image narrower than 64 has no level 1.  Width 14 "halves exactly" on paper
    only: its plan has level 0 alone.  TW_PYR_GENERIC=1 / 2 reach the branch (two cases below carry that switch).
  * single-tap tail columns (xmax < w) or clipped source rows (yofs + 1 > h0 - 1) in tw_pyr_taps, and in tw_pyr_level without
    TW_PYR_GENERIC=1.  A level has them only when ONE of its sides rounds back to the image's own while the other shrinks (a
    level with both sides unchanged is a copy, mode 0): w0 (1 - scale) < 0.5 with w0 >= 32 needs scale > 0.984, so such a level
    has 3 taps and takes tw_pyr_level_lds — the tail_* and clip_* cases below, 33 x 64 / 40 x 100 and 64 x 33 / 100 x 40 at
    pyrScale 0.99, with the unstaged kernel under the switch.  test_pyr_cases.py proves both directions over non-square sizes.
  * tw_pyr_level's interior path on an image narrower than ksize + 3, or narrower than the radius: the level must be at least
    32 columns wide, so the image is at least 32 / scale columns wide, and ksize ~ 2.5 (1 / scale - 1) is less than a tenth of that.
  * fused23's `w0, h0 >= 64`: a plan with a level 3 has w0, h0 >= 256.  The 64 / 72 / 56 / 68-pixel sizes below have no level 2
    at all and are refused by tw_stage_pyr_fused23; 256 x 256 and 264 x 256 are the smallest eligible ones.
  * `ksize <= 63` as a cause of its own: every level of 27 taps or more already fails the LDS budget, so 63 and 65 taps both take
    the unstaged kernel (kept as cases: 63 = 15 dwords + 3 tail taps, 65 = 16 dwords + 1).
  * level-1 heights 3 / 4 / 5: the same residues of tw_pyr_k3<2>'s 4-row tiles at the smallest heights a level 1 has, 35 / 36 / 37.
"""
import collections
import functools

import numpy as np

import farneback_f64 as F

Case = collections.namedtuple("Case", "name w0 h0 scale levels level rows want env what")

# rows of the edge list (test_pyr_cases.py: every row has its cases, on either side of an edge told apart by `want`)
ROWS = ("register_w16", "k3_grid_l0", "k3_grid_l1", "fused23", "fused01", "lds_vs_taps", "taps_template", "budget", "k63_65",
        "tile_height", "w_mod_32", "h_mod_rows", "generic_mode2", "tail_columns", "clipped_rows")


def _c(name, w0, h0, scale, levels, level, rows, want, what, env=None):
    return Case(name, w0, h0, scale, levels, level, tuple(rows.split()), want, env or {}, what)


K3_0 = dict(kernel="tw_pyr_k3", targ=0, family="tw_pyr_k3", tile_cols=256, rows=8)
K3_2 = dict(kernel="tw_pyr_k3", targ=2, family="tw_pyr_k3", tile_cols=256, rows=4)
LDS = dict(kernel="tw_pyr_level_lds", targ=0, family="tw_pyr_level_lds", tile_cols=32, rows=8)
GEN8 = dict(kernel="tw_pyr_level", targ=0, family="tw_pyr_level", tile_cols=32, rows=8, pitch=0)
GEN4 = dict(kernel="tw_pyr_level", targ=0, family="tw_pyr_level", tile_cols=32, rows=4, pitch=0)


def TAPS(ks):
    return dict(kernel="tw_pyr_taps", targ=ks, family="tw_pyr_taps", tile_cols=32, rows=8)


CASES = [
    # ---- the register path needs w0 >= 16 (narrower images take the staged generic kernel in its mode == 0 branch)
    _c("w16", 16, 40, 0.5, 3, 0, "register_w16", dict(K3_0, mode=0, ksize=3), "the narrowest image of tw_pyr_k3<0>"),
    _c("w15", 15, 40, 0.5, 3, 0, "register_w16", dict(LDS, mode=0, ksize=3), "one column less: tw_pyr_level_lds, mode 0"),
    _c("w14", 14, 40, 0.5, 3, 0, "register_w16", dict(LDS, mode=0, ksize=3, levels=0), "even, but no level 1 to halve into"),
    # ---- tw_pyr_k3<0>: 256 columns x 8 rows per workgroup
    _c("k3l0_w255", 255, 9, 0.5, 0, 0, "k3_grid_l0", dict(K3_0, grid_x=1, grid_y=2), "one tile column, a lane short"),
    _c("k3l0_w256", 256, 9, 0.5, 0, 0, "k3_grid_l0", dict(K3_0, grid_x=1, grid_y=2), "one tile column, full"),
    _c("k3l0_w257", 257, 9, 0.5, 0, 0, "k3_grid_l0", dict(K3_0, grid_x=2, grid_y=2), "a second tile column of one pixel"),
    _c("k3l0_h7", 40, 7, 0.5, 0, 0, "k3_grid_l0 h_mod_rows", dict(K3_0, grid_y=1), "rows - 1"),
    _c("k3l0_h8", 40, 8, 0.5, 0, 0, "k3_grid_l0 h_mod_rows", dict(K3_0, grid_y=1), "a full tile row"),
    _c("k3l0_h9", 40, 9, 0.5, 0, 0, "k3_grid_l0 h_mod_rows", dict(K3_0, grid_y=2), "a second tile row of one row"),
    # ---- tw_pyr_k3<2>: 256 columns x 4 rows of level 1
    _c("k3l1_w255", 510, 64, 0.5, 1, 1, "k3_grid_l1 fused01", dict(K3_2, w=255, grid_x=1, fused01=True), "level 1 255 wide"),
    _c("k3l1_w256", 512, 64, 0.5, 1, 1, "k3_grid_l1 fused01", dict(K3_2, w=256, grid_x=1, fused01=True), "level 1 256 wide"),
    _c("k3l1_w257", 514, 64, 0.5, 1, 1, "k3_grid_l1 fused01", dict(K3_2, w=257, grid_x=2, fused01=True), "level 1 257 wide"),
    _c("k3l1_h35", 64, 70, 0.5, 1, 1, "k3_grid_l1 h_mod_rows", dict(K3_2, h=35, grid_y=9), "level 1 35 rows: rows - 1"),
    _c("k3l1_h36", 64, 72, 0.5, 1, 1, "k3_grid_l1 h_mod_rows", dict(K3_2, h=36, grid_y=9), "level 1 36 rows: full tiles"),
    _c("k3l1_h37", 64, 74, 0.5, 1, 1, "k3_grid_l1 h_mod_rows", dict(K3_2, h=37, grid_y=10), "level 1 37 rows: one row over"),
    # ---- tw_pyr_23 eligibility (Plan::fused23); each level's own launch is tw_pyr_taps<9> / <19> either way
    _c("f23_256_l2", 256, 256, 0.5, 3, 2, "fused23 taps_template w_mod_32 h_mod_rows", dict(TAPS(9), fused23=True, w=64, h=64), "eligible, smallest"),
    _c("f23_256_l3", 256, 256, 0.5, 3, 3, "fused23 taps_template w_mod_32 h_mod_rows", dict(TAPS(19), fused23=True, w=32, h=32), "eligible, smallest"),
    _c("f23_264_l2", 264, 256, 0.5, 3, 2, "fused23", dict(TAPS(9), fused23=True, w=66), "eligible, 8 columns wider"),
    _c("f23_264_l3", 264, 256, 0.5, 3, 3, "fused23 w_mod_32", dict(TAPS(19), fused23=True, w=33), "eligible, 8 columns wider"),
    _c("f23_260_l3", 260, 256, 0.5, 3, 3, "fused23", dict(TAPS(19), fused23=False, w=32), "260 / 8 = 32.5: not exact by 8"),
    _c("f23_levels2", 256, 256, 0.5, 2, 2, "fused23", dict(TAPS(9), fused23=False, levels=2), "pyrLevels = 2: no level 3"),
    _c("f23_scale06", 256, 256, 0.6, 3, 3, "fused23", dict(fused23=False, levels=3, kernel="tw_pyr_taps"), "pyrScale 0.6"),
    _c("f23_64x64", 64, 64, 0.5, 3, 1, "fused23 fused01", dict(K3_2, fused23=False, fused01=True, levels=1), "64 x 64: no level 2"),
    _c("f23_72x64", 72, 64, 0.5, 3, 1, "fused23", dict(K3_2, fused23=False, levels=1), "72 x 64: no level 2"),
    _c("f23_68x64", 68, 64, 0.5, 3, 1, "fused23", dict(K3_2, fused23=False, levels=1), "68 x 64: no level 2"),
    _c("f23_56x64", 56, 64, 0.5, 3, 0, "fused23", dict(K3_0, fused23=False, levels=0), "56 x 64: level 0 alone"),
    _c("f23_64x56", 64, 56, 0.5, 3, 0, "fused23", dict(K3_0, fused23=False, levels=0), "64 x 56: level 0 alone"),
    # ---- tw_pyr_k3f eligibility (pyr01_fusable): an exact halving
    _c("f01_odd", 65, 65, 0.5, 1, 1, "fused01", dict(LDS, fused01=False, mode=1, ksize=3), "odd: level 1 is INTER_LINEAR, 3 taps staged"),
    _c("f01_scale06", 56, 56, 0.6, 1, 1, "fused01 w_mod_32", dict(LDS, fused01=False, mode=1, ksize=3, w=34), "pyrScale 0.6"),
    # ---- tw_pyr_level_lds (up to 5 taps) against tw_pyr_taps (7 and more), and the residues inside each
    _c("lds5_32", 80, 80, 0.4, 1, 1, "lds_vs_taps w_mod_32 h_mod_rows", dict(LDS, ksize=5, w=32, h=32), "5 taps, full tiles"),
    _c("lds5_33", 82, 82, 0.4, 1, 1, "w_mod_32 h_mod_rows", dict(LDS, ksize=5, w=33, h=33), "5 taps, one over"),
    _c("lds5_63x39", 157, 97, 0.4, 1, 1, "w_mod_32 h_mod_rows", dict(LDS, ksize=5, w=63, h=39), "5 taps, one short"),
    _c("taps7_32", 107, 107, 0.3, 1, 1, "lds_vs_taps taps_template w_mod_32 h_mod_rows", dict(TAPS(0), ksize=7, w=32, h=32), "7 taps: the any-size template at its smallest"),
    _c("taps7_33", 110, 110, 0.3, 1, 1, "w_mod_32 h_mod_rows", dict(TAPS(0), ksize=7, w=33, h=33), "7 taps, one over"),
    _c("taps7_63x39", 210, 130, 0.3, 1, 1, "w_mod_32 h_mod_rows", dict(TAPS(0), ksize=7, w=63, h=39), "7 taps, one short"),
    # ---- each tw_pyr_taps template (39: unreachable, see the module docstring)
    _c("taps9", 132, 131, 0.25, 1, 1, "taps_template", dict(TAPS(9), ksize=9, w=33, h=33), "9 taps outside the 0.5 pyramid"),
    _c("taps19", 264, 264, 0.125, 1, 1, "taps_template", dict(TAPS(19), ksize=19, w=33, h=33), "19 taps outside the 0.5 pyramid"),
    _c("taps25", 358, 358, 0.091, 1, 1, "taps_template budget", dict(TAPS(0), ksize=25, w=33), "the largest staged kernel: 64 072 B of LDS"),
    # ---- staged against unstaged: the 64 KB budget, then 63 / 65 taps
    _c("gen25", 362, 362, 0.09, 1, 1, "budget w_mod_32 h_mod_rows", dict(GEN8, ksize=25, w=33, h=33), "25 taps again, one row of source too many"),
    _c("gen25_32", 356, 356, 0.09, 1, 1, "w_mod_32 h_mod_rows", dict(GEN8, ksize=25, w=32, h=32), "unstaged, full tiles"),
    _c("gen25_63x39", 700, 433, 0.09, 1, 1, "w_mod_32 h_mod_rows", dict(GEN8, ksize=25, w=63, h=39), "unstaged, one short"),
    _c("gen39_l4", 512, 512, 0.5, 4, 4, "taps_template budget", dict(GEN4, ksize=39), "level 4 of the 0.5 pyramid: 39 taps are never staged"),
    _c("gen63", 856, 856, 0.038, 1, 1, "k63_65", dict(GEN4, ksize=63), "63 taps: over the budget long before ksize <= 63 is asked"),
    _c("gen65", 867, 867, 0.0375, 1, 1, "k63_65", dict(GEN4, ksize=65), "65 taps"),
    # ---- the unstaged kernel's tile height: 8 rows while the row buffer is at most 32 KB (128 rows)
    _c("gen31_th8", 434, 434, 0.075, 1, 1, "tile_height", dict(GEN8, ksize=31, nrows_max=124), "124 rows of 256 B: 8-row tiles"),
    _c("gen33_th4", 452, 452, 0.072, 1, 1, "tile_height w_mod_32 h_mod_rows", dict(GEN4, ksize=33, w=33, h=33), "an 8-row tile would need more than 128 rows"),
    _c("gen33_32", 445, 445, 0.072, 1, 1, "w_mod_32 h_mod_rows", dict(GEN4, ksize=33, w=32, h=32), "4-row tiles, full"),
    _c("gen33_63x35", 875, 486, 0.072, 1, 1, "w_mod_32 h_mod_rows", dict(GEN4, ksize=33, w=63, h=35), "4-row tiles, one short"),
    # ---- single-tap tail columns and clipped last rows: one side of the level is the image's own, the other shrinks
    _c("tail_33x64", 33, 64, 0.99, 1, 1, "tail_columns", dict(LDS, mode=1, ksize=3, w=33, h=63, xmax=32, yclip=0), "the smallest: the tail column is the second tile column's only one"),
    _c("tail_40x100", 40, 100, 0.99, 1, 1, "tail_columns", dict(LDS, mode=1, ksize=3, w=40, h=99, xmax=39, yclip=0), "the tail column last of eight in its tile"),
    _c("clip_64x33", 64, 33, 0.99, 1, 1, "clipped_rows", dict(LDS, mode=1, ksize=3, w=63, h=33, xmax=63, yclip=1), "the smallest: the clipped row is the fifth tile row's only one"),
    _c("clip_100x40", 100, 40, 0.99, 1, 1, "clipped_rows", dict(LDS, mode=1, ksize=3, w=99, h=40, xmax=99, yclip=1), "the clipped row last of its tile"),
    _c("tail_40x100_generic1", 40, 100, 0.99, 1, 1, "tail_columns", dict(GEN8, mode=1, ksize=3, xmax=39, yclip=0), "TW_PYR_GENERIC=1: the unstaged kernel's tail branch", {"TW_PYR_GENERIC": "1"}),
    _c("clip_100x40_generic1", 100, 40, 0.99, 1, 1, "clipped_rows", dict(GEN8, mode=1, ksize=3, xmax=99, yclip=1), "TW_PYR_GENERIC=1: the unstaged kernel's clipped row", {"TW_PYR_GENERIC": "1"}),
    # ---- the generic kernels' mode == 2 branch: only under TW_PYR_GENERIC
    _c("generic1_mode2", 64, 66, 0.5, 1, 1, "generic_mode2", dict(GEN8, mode=2, ksize=3), "TW_PYR_GENERIC=1", {"TW_PYR_GENERIC": "1"}),
    _c("generic2_mode2", 64, 66, 0.5, 1, 1, "generic_mode2", dict(LDS, mode=2, ksize=3), "TW_PYR_GENERIC=2", {"TW_PYR_GENERIC": "2"}),
]
BY_NAME = {c.name: c for c in CASES}

# (kernel, template argument) -> reachable without an environment switch?  test_pyr_cases.py: the table reaches every True one
KERNELS = {("tw_pyr_k3", 0): True, ("tw_pyr_k3", 2): True, ("tw_pyr_taps", 9): True, ("tw_pyr_taps", 19): True,
           ("tw_pyr_taps", 39): False, ("tw_pyr_taps", 0): True, ("tw_pyr_level_lds", 0): True, ("tw_pyr_level", 0): True}
# tw_pyr_k3f and tw_pyr_23<1024> run through tw_stage_pyr_fused01 / _fused23 at the eligible sizes, tw_pyr_23<512> in a batch,
# tw_pyr_23<256> under TW_PYR23_THREADS=256 (tests/test_gpu_pyr_dispatch.py)


def image(case):
    """uint8 noise with a saturated block against the top left corner (as tests/test_oracle_stages_f64.py: run_pyr_level)."""
    img = np.random.default_rng(case.h0 * 4099 + case.w0).integers(0, 256, (case.h0, case.w0)).astype(np.uint8)
    img[: max(case.h0 // 5, 1), : max(case.w0 // 7, 1)] = 255
    return img


def level(case):
    """The float64 reference's (width, height, taps, sigma, scale) of the case's level, None when the plan has no such level."""
    plan = F.level_plan(case.w0, case.h0, case.scale, case.levels)
    return plan[case.level] if case.level < len(plan) else None


def resize_mode(case):
    """0: the level is the image, 2: an exact halving, 1: any other INTER_LINEAR resize (make_resize_tab's rule)."""
    w, h = level(case)[:2]
    return 0 if (w, h) == (case.w0, case.h0) else 2 if (2 * w, 2 * h) == (case.w0, case.h0) else 1


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference, bound) of the case in float64: computed once, shared by the CPU and the GPU tests, never written to."""
    case = BY_NAME[name]
    ref, bound = F.pyr_level(image(case), level(case))
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def tail_and_clip(case):
    """(xmax, clipped rows) of the case's level from the reference's coordinate rule (make_resize_tab's: output columns from
    the first whose right tap sx + 1 lies past the image take a single tap; a row whose lower tap does is clipped)."""
    w, h = level(case)[:2]
    if resize_mode(case) != 1:
        return w, 0
    sx, _ = F._axis_map(case.w0, w)
    sy, _ = F._axis_map(case.h0, h)
    tail = np.nonzero(sx + 1 >= case.w0)[0]
    return (int(tail[0]) if tail.size else w), int((sy + 1 > case.h0 - 1).sum())


def oracle_level(oracle, case):
    return oracle.pyr_level(image(case), oracle.level_plan(case.w0, case.h0, case.scale, case.levels)[case.level])
