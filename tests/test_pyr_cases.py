"""The table of tests/pyr_cases.py on the CPU: the expected values of tests/test_gpu_pyr_dispatch.py are pinned to the algorithm,
and the table holds what it claims.

  * for every case the oracle's level agrees with the float64 reference (tests/farneback_f64.py) inside the reference's own
    propagated bound, every pixel (the judge of tests/test_oracle_stages_f64.py);
  * tap counts, resize modes, level sizes and level counts are what each case says, computed here from the reference's level
    plan (what only the engine knows — kernel, tile, LDS — is asserted on the GPU from Engine.pyr_plan);
  * every row of the edge list has its cases, every kernel the residues of its tile, every reachable kernel and template a
    case without an environment switch;
  * which levels have single-tap tail columns or clipped source rows, over non-square sizes: exactly those with one side the
    image's own, all of them 3-tap levels (why the table has such cases for tw_pyr_level_lds, and for tw_pyr_level under its
    switch, and none for tw_pyr_taps).
"""
import numpy as np
import pytest

import farneback_f64 as F
import pyr_cases as PC
import test_oracle_stages_f64 as S

# cases the edge list names for each row (the issue's table): the floor of the table's size comes from here
REQUIRED = {"register_w16": 3, "k3_grid_l0": 6, "k3_grid_l1": 6, "fused23": 7, "fused01": 2, "lds_vs_taps": 2, "taps_template": 4,
            "budget": 2, "k63_65": 2, "tile_height": 2, "w_mod_32": 12, "h_mod_rows": 12, "generic_mode2": 1, "tail_columns": 2,
            "clipped_rows": 2}


@pytest.mark.parametrize("name", [c.name for c in PC.CASES])
def test_oracle_level_is_the_reference_level(oracle, name):
    case = PC.BY_NAME[name]
    lv = oracle.level_plan(case.w0, case.h0, case.scale, case.levels)[case.level]
    assert (lv.width, lv.height, lv.smooth_sz) == PC.level(case)[:3], name
    ref, bound = PC.reference(name)
    S.check("oracle", "pyr_case", name, PC.oracle_level(oracle, case), ref, bound)


def test_the_table_holds_what_it_claims():
    assert len({c.name for c in PC.CASES}) == len(PC.CASES)
    for c in PC.CASES:
        lv = PC.level(c)
        assert lv is not None, c.name
        plan = F.level_plan(c.w0, c.h0, c.scale, c.levels)
        have = dict(w=lv[0], h=lv[1], ksize=lv[2], mode=PC.resize_mode(c), levels=len(plan) - 1)
        have["xmax"], have["yclip"] = PC.tail_and_clip(c)
        for k, v in have.items():
            assert c.want.get(k, v) == v, (c.name, k, v)
        # a case says so when its level has tail columns or clipped rows, and only the rows made for them have any
        assert (have["xmax"] < lv[0]) == ("tail_columns" in c.rows) and (have["yclip"] > 0) == ("clipped_rows" in c.rows), c.name
        if "tail_columns" in c.rows or "clipped_rows" in c.rows:
            assert "xmax" in c.want and "yclip" in c.want, c.name
        assert set(c.rows) <= set(PC.ROWS) and c.rows and c.what, c.name
        # the taps decide between the staged kernels, the mode and the width the register path: the claim must agree
        if c.want.get("kernel") == "tw_pyr_k3" and not c.env:
            assert lv[2] == 3 and PC.resize_mode(c) == c.want["targ"] and c.w0 >= 16, c.name
        if c.want.get("kernel") == "tw_pyr_taps":
            assert 7 <= lv[2] <= 63 and PC.resize_mode(c) == 1, c.name
            if "targ" in c.want:
                assert c.want["targ"] == (lv[2] if lv[2] in (9, 19, 39) else 0), c.name
        if c.want.get("kernel") == "tw_pyr_level_lds" and not c.env:
            assert lv[2] <= 5 or PC.resize_mode(c) == 0, c.name


def test_every_row_of_the_edge_list_has_its_cases():
    assert set(REQUIRED) == set(PC.ROWS)
    for row, n in REQUIRED.items():
        cases = [c for c in PC.CASES if row in c.rows]
        assert len(cases) >= n, (row, len(cases), n)
    assert len(PC.CASES) >= max(REQUIRED.values()) + len(REQUIRED) and len(PC.CASES) >= 45

    def sides(row, key):
        return {c.want.get(key) for c in PC.CASES if row in c.rows}
    # both sides of each edge
    assert sides("register_w16", "kernel") == {"tw_pyr_k3", "tw_pyr_level_lds"}
    assert {c.w0 for c in PC.CASES if "register_w16" in c.rows} == {16, 15, 14}
    assert {(c.w0, c.want["grid_x"]) for c in PC.CASES if c.name.startswith("k3l0_w")} == {(255, 1), (256, 1), (257, 2)}
    assert {(c.h0, c.want["grid_y"]) for c in PC.CASES if c.name.startswith("k3l0_h")} == {(7, 1), (8, 1), (9, 2)}
    assert {(c.want["w"], c.want["grid_x"]) for c in PC.CASES if c.name.startswith("k3l1_w")} == {(255, 1), (256, 1), (257, 2)}
    assert {(c.want["h"], c.want["grid_y"]) for c in PC.CASES if c.name.startswith("k3l1_h")} == {(35, 9), (36, 9), (37, 10)}
    assert sides("fused23", "fused23") == {True, False} and sides("fused01", "fused01") == {True, False}
    assert {(c.w0, c.h0) for c in PC.CASES if "fused23" in c.rows} >= {(64, 64), (72, 64), (56, 64), (64, 56), (68, 64), (256, 256)}
    assert {(c.want["kernel"], c.want["ksize"]) for c in PC.CASES if "lds_vs_taps" in c.rows} == {("tw_pyr_level_lds", 5), ("tw_pyr_taps", 7)}
    assert {(c.want["kernel"], c.want["ksize"]) for c in PC.CASES if "budget" in c.rows} >= {("tw_pyr_taps", 25), ("tw_pyr_level", 25)}
    assert {c.want["ksize"] for c in PC.CASES if "k63_65" in c.rows} == {63, 65}
    assert {c.want["rows"] for c in PC.CASES if "tile_height" in c.rows} == {8, 4}
    generic0 = [c.want["ksize"] for c in PC.CASES if "taps_template" in c.rows and c.want.get("targ") == 0 and c.want["kernel"] == "tw_pyr_taps"]
    assert len(set(generic0)) >= 2 and max(generic0) == 25
    assert {c.env["TW_PYR_GENERIC"] for c in PC.CASES if "generic_mode2" in c.rows} == {"1", "2"}
    assert all(PC.resize_mode(c) == 2 for c in PC.CASES if "generic_mode2" in c.rows)
    # tail columns and clipped rows: in the staged generic kernel without a switch, in the unstaged one under TW_PYR_GENERIC=1
    for row in ("tail_columns", "clipped_rows"):
        assert {(c.want["kernel"], c.env.get("TW_PYR_GENERIC")) for c in PC.CASES if row in c.rows} == \
            {("tw_pyr_level_lds", None), ("tw_pyr_level", "1")}, row
    assert all(c.want["xmax"] < c.want.get("w", 1 << 30) or c.env for c in PC.CASES if "tail_columns" in c.rows)
    # every reachable kernel and template without an environment switch, and no case that claims an unreachable one
    reached = {(c.want["kernel"], c.want["targ"]) for c in PC.CASES if not c.env and "targ" in c.want}
    assert reached == {k for k, ok in PC.KERNELS.items() if ok}, reached
    # the residues of each kernel's tile: level width mod 32 and level height mod tile rows in {0, 1, rows - 1}
    for kernel, rows in (("tw_pyr_level_lds", 8), ("tw_pyr_taps", 8), ("tw_pyr_level", 8), ("tw_pyr_level", 4)):
        mine = [c for c in PC.CASES if c.want.get("kernel") == kernel and c.want.get("rows") == rows and not c.env]
        assert {PC.level(c)[0] % 32 for c in mine if "w_mod_32" in c.rows} >= {0, 1, 31}, kernel
        assert {PC.level(c)[1] % rows for c in mine if "h_mod_rows" in c.rows} >= {0, 1, rows - 1}, (kernel, rows)
    for targ, rows in ((0, 8), (2, 4)):
        mine = [c for c in PC.CASES if c.want.get("kernel") == "tw_pyr_k3" and c.want.get("targ") == targ and "h_mod_rows" in c.rows]
        assert {PC.level(c)[1] % rows for c in mine} >= {0, 1, rows - 1}, targ


def test_most_images_are_small():
    big = [c.name for c in PC.CASES if max(c.w0, c.h0) >= 600]
    assert len(big) <= len(PC.CASES) // 8, big
    assert max(max(c.w0, c.h0) for c in PC.CASES) < 900


def test_which_levels_have_single_tap_tails_or_clipped_rows():
    """A level has single-tap tail columns (make_resize_tab: sx + 1 >= w0 from some column on, xmax < w) exactly when its width
    is the image's own while its height shrank, and clipped rows (yofs + 1 > h0 - 1) exactly when its height is the image's own
    while its width shrank: at a per-axis scale of 1 the last sample sits ON the last source column / row, and at any scale
    above 1 it sits at w0 - 0.5 w0 / w - 0.5 < w0 - 1.  (Both sides unchanged is a copy, mode 0, which reads no table.)  Checked
    with the reference's own float32 coordinate rule over non-square and square sizes at scales up to 0.999, every level of a
    six-level plan.  Every such level has 3 taps — w0 (1 - scale) < 0.5 with w0 >= 32 needs scale > 0.984 — so it takes
    tw_pyr_level_lds (tw_pyr_level under TW_PYR_GENERIC=1) and never tw_pyr_taps, whose own tail branch nothing reaches."""
    sizes = list(range(32, 72)) + [99, 100, 101, 128, 200, 257, 333, 640, 1000, 1920]
    n = tails = clips = 0
    for s in (0.0375, 0.09, 0.3, 0.5, 0.6, 0.8, 0.9, 0.95, 0.97, 0.98, 0.985, 0.99, 0.995, 0.999):
        for w0 in sizes:
            for h0 in sizes:
                for lv in F.level_plan(w0, h0, s, 6)[1:]:
                    w, h, ks = lv[:3]
                    if (w, h) == (w0, h0):
                        continue  # mode 0
                    sx, _ = F._axis_map(w0, w)
                    sy, _ = F._axis_map(h0, h)
                    assert sx.min() >= -1 and sy.min() >= -1 and np.all(np.diff(sx) >= 0) and np.all(np.diff(sy) >= 0)
                    tail, clip = bool((sx + 1 >= w0).any()), bool((sy + 1 > h0 - 1).any())
                    assert tail == (w == w0) and clip == (h == h0), (w0, h0, s, lv)
                    if tail or clip:
                        assert ks == 3 and s > 0.984, (w0, h0, s, lv)
                        assert int((sx + 1 >= w0).sum()) <= 1 and int((sy + 1 > h0 - 1).sum()) <= 1
                    n += 1
                    tails += tail
                    clips += clip
    assert n > 50000 and tails > 100 and clips > 100, (n, tails, clips)
