"""The composition recipes of tests/compose_cases.py on the CPU: that they cover what they are there for, that the reference
builder returns the images it is given, that their inputs are not degenerate, and that the builder refuses what the ABI
does not have.  No device: tests/test_gpu_compose.py runs the same recipes on the GPU.
"""
import dataclasses

import numpy as np
import pytest

import compose_cases as CC
from compose_cases import PairSpec as P
from test_gpu_resident import as_jpeg, as_pal4, as_rgba


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_every_legal_pair_of_factor_values_meets_in_a_grid_only_recipe():
    """8 expected forms, 6 target forms, sized / ignore / init / keep / identical, regions 0 / 1 / 3, span 5 / 7 / 10, lanes
    1 / 2, ramp: every pair of values of two factors occurs in one pair (or one batch) of a recipe that ends in the grid-only
    iteration, or is listed in compose_cases.ILLEGAL with its reason — and nothing listed there occurs."""
    names = CC.PAIR_FACTORS + CC.BATCH_FACTORS
    cov = CC.coverage()
    pairs = CC.value_pairs(names)
    assert len(CC.VALUES["expected"]) == 8 and len(CC.VALUES["target"]) == 6
    assert set(CC.ILLEGAL) <= set(pairs), "an illegal pair that is no pair of factor values"
    print("recipes on the grid-only path: %s" % ", ".join(r.name for r in CC.RECIPES.values() if r.grid_only))
    print("%-44s %-22s %s" % ("value", "with", "first recipe / reason"))
    missing = []
    for p in pairs:
        (fa, a), (fb, b) = p
        where = "ILLEGAL: " + CC.ILLEGAL[p] if p in CC.ILLEGAL else cov[p][0] if p in cov else "UNCOVERED"
        print("%-44s %-22s %s" % ("%s=%s" % (fa, a), "%s=%s" % (fb, b), where))
        if p not in cov and p not in CC.ILLEGAL:
            missing.append(p)
        assert not (p in cov and p in CC.ILLEGAL), (p, cov[p])
    # the same, recipe by factor value: which recipes hold a value at all
    print("\n%-26s %s" % ("recipe", " ".join(CC.PAIR_FACTORS + CC.BATCH_FACTORS)))
    for r in CC.RECIPES.values():
        row = []
        for f in CC.PAIR_FACTORS:
            vals = sorted({str(getattr(s, f)) for s in r.specs})
            row.append("%d/%d" % (len(vals), len(CC.VALUES[f])))
        row += [str(v) for _, v in CC.recipe_values(r)]
        print("%-26s %s%s" % (r.name, " ".join(row), "" if r.grid_only else "  (not grid-only)"))
    assert not missing, missing
    # the recipes the issue names are what they say
    R = CC.RECIPES
    assert all(R[n].grid_only for n in R if n[0] in "ABCDEM") and not R["G_flow"].grid_only and not R["H_scan_fused"].grid_only
    assert all(R["D_ramp"].specs[i].expected == "resident_created" for i in (0, 16, 32))  # the first pair of each piece
    assert all(R["D_ramp"].specs[i].sized for i in (15, 16, 31, 32, 63)) and R["D_ramp"].specs[17].init
    assert R["D_ramp"].specs[3].identical and R["D_ramp"].pieces() == [16, 16, 32]
    assert not any(s.ignore or CC.decoded(s) for s in R["D_ramp"].specs)
    assert sum(s.ignore for s in R["D_masked"].specs) == 1 and not R["D_masked"].ramp
    assert all(s.expected != "device" for i, s in enumerate(R["D_ramp"].specs) if i in (15, 31))  # (the ramp's marks: host pairs)
    for r in R.values():
        assert len(r.specs) <= r.slots, r.name
        # (a batch's first filtered image is its largest: a larger one later would start another batch)
        assert r.specs[0].expected == "rgba_rows" or not any("rgba_rows" in (s.expected, s.target) for s in r.specs), r.name


# ---- the reference builder ---------------------------------------------------------------------------------------------
def test_reference_of_an_unmodified_pair_is_the_pair(oracle, golden):
    case = next(c for c in golden.values() if c["expect_img"].shape == (117, 180) and c["vector"])
    a, b = np.ascontiguousarray(case["expect_img"]), np.ascontiguousarray(case["target_img"])
    import twflow as T
    gray_of = {"rgba_rows": lambda g: as_rgba(T, g)[1], "pal4_rows": lambda g: as_pal4(T, g)[1],
               "jpeg_coef": lambda g: as_jpeg(T, g)[1]}
    keeper = CC.Pair(oracle, P(keep=True), a, b)
    n = 0
    for ex in CC.EXPECTED_FORMS:
        for tg in CC.TARGET_FORMS:
            s = P(ex, tg)
            if CC.why_refused(s):
                continue
            ra, rb, rects, init = CC.reference(CC.Pair(oracle, s, a, b, prev=keeper))
            want_a = b if ex == "resident_kept_target" else gray_of.get(ex, lambda g: g)(a)
            assert np.array_equal(ra, want_a) and np.array_equal(rb, gray_of.get(tg, lambda g: g)(b)), s
            assert rects == [] and init is None and ra.dtype == np.uint8 and ra.shape == (117, 180)
            n += 1
    assert n == 32
    # lossy means lossy: the decoded grays are not the picture, the plain forms are
    assert not np.array_equal(gray_of["pal4_rows"](a), a) and not np.array_equal(gray_of["jpeg_coef"](a), a)
    # the modifiers: a sized target is the oracle's reconcile of it, the mask comes after the resize, a kept target is masked
    p = CC.Pair(oracle, P("pageable_gray", "pal4_rows", sized=True, ignore=True, keep=True), a, b, seed=1)
    assert p.size == (180 - 4, 117 - 5) and p.t_gray.shape == (112, 176)
    resized = oracle.reconcile_target(p.t_gray, 180, 117)
    inside = np.zeros((117, 180), bool)
    for x0, y0, x1, y1 in CC.reference(p)[2]:
        inside[y0:y1, x0:x1] = True
    assert np.array_equal(p.b[inside], a[inside]) and np.array_equal(p.b[~inside], resized[~inside]) and inside.any()
    assert not np.array_equal(p.b, resized)
    nxt = CC.Pair(oracle, P("resident_kept_target", "pageable_gray", identical=True), a, b, prev=p)
    assert np.array_equal(nxt.a, p.b) and np.array_equal(nxt.b, p.b) and nxt.same == 1
    patched = CC.Pair(oracle, P(ignore=True, patch=True), a, b)
    assert patched.same == 1 and not np.array_equal(patched.t_gray, a)  # identical only after masking
    f = CC.Pair(oracle, P(init=True), a, b, seed=2).init
    assert f.shape == (2, 117, 180) and f.dtype == np.float32 and np.abs(f).max() <= 2 and f.std() > 0.5


def test_the_rectangles_are_the_ones_the_recipes_need():
    for w, h in ((397, 99), (333, 41), (640, 480)):
        rects = CC.rects_for(w, h)
        cl = CC.clip(rects, w, h)
        assert len(cl) == 4
        assert any(y + rh > h or x + rw > w for x, y, rw, rh in rects)          # one clipped by the right or bottom edge
        assert any(rw == 1 and rh == 1 and all(x % s == 0 and y % s == 0 for s in (5, 7, 10)) for x, y, rw, rh in rects)
        for span in (5, 7, 10):
            last = (w - 1) // span * span
            assert any(x0 <= last < x1 and any(y0 <= gy * span < y1 for gy in range(-(-h // span))) for x0, y0, x1, y1 in cl)


# ---- the recipes' inputs -----------------------------------------------------------------------------------------------
def hits_share(oracle, pair, span, thr):
    f = pair.field(oracle)
    G = -(-pair.h // span) * -(-pair.w // span)
    return len(oracle.span_scan(f[0], f[1], span, thr)) / G


@pytest.mark.parametrize("name", [n for n in CC.RECIPES if not n.startswith("M_")] +
                         ["M_span5_gap1_lanes2", "M_span7_gap3_lanes2", "M_span10_gap0_lanes1"])  # (M: once per span)
def test_recipe_inputs_are_not_degenerate(oracle, name):
    """On the reference alone.  Threshold 1: a pair with hits at 10 - 90 % of its grid points and at least two regions at gap
    1; threshold 0: at least 95 % of the grid points of every pair that is not identical are hits.  (Measured for the
    unmodified synth pairs of kinds 0 and 1: 39 - 61 % and 2 - 9 regions at 397 x 99, 24 - 41 % and 4 - 11 at 333 x 41.)"""
    r = CC.RECIPES[name]
    pairs = r.pairs(oracle)
    good = 0
    for i, p in enumerate(pairs):
        if p.same:
            assert p.spec.identical or p.spec.patch, (name, i)
            continue
        assert p.spec.expected == "resident_kept_target" or not (p.spec.identical or p.spec.patch)
        full = hits_share(oracle, p, r.span, 0.0)
        share = hits_share(oracle, p, r.span, 1.0)
        nreg = len(p.regions(oracle, r.span, 1.0, 1)[0])
        print("%s pair %d %s -> %s: hits at threshold 0: %.1f %%, at 1: %.1f %%, regions (gap 1): %d" % (
            name, i, p.spec.expected, p.spec.target, 100 * full, 100 * share, nreg))
        assert full >= 0.95, (name, i, full)
        good += 0.10 <= share <= 0.90 and nreg >= 2
    assert good >= 1, name
    assert any(p.same for p in pairs), name
    for p in pairs:
        if p.rects:  # the filter is exercised: vectors inside the rectangles exist
            f = p.field(oracle)
            assert len(p.vectors(oracle, r.span, 0.0)) < len(oracle.span_scan(f[0], f[1], r.span, 0.0))


def test_counts_that_follow_from_the_specs(oracle):
    """decode_launches on the written-out recipes, by hand from flush_ctx's steps."""
    A = CC.decode_launches(CC.RECIPES["A"].pairs(oracle))
    # pal4 target of another size: the batch-wide tw_png_unfilter and one at its size; its resize and the JPEG target's share
    # the batch's one tw_resize_u8 launch; three masked pairs, none behind a masked kept target: one round
    assert A == {"tw_jpeg_idct": 1, "tw_png_unfilter": 2, "tw_resize_u8": 1, "tw_mask_rects": 1}
    Ad = CC.decode_launches(CC.RECIPES["A_device"].pairs(oracle))
    assert Ad == dict(A, tw_resize_u8=2)  # ... and the device targets' launch
    C = CC.decode_launches(CC.RECIPES["C_lanes2"].pairs(oracle))
    # the sized page-locked gray pair resizes at submit time; pair 6 reads the kept masked target of pair 5: a second round
    assert C == {"tw_jpeg_idct": 1, "tw_png_unfilter": 2, "tw_resize_u8": 2, "tw_mask_rects": 2}
    D = CC.decode_launches(CC.RECIPES["D_ramp"].pairs(oracle))
    assert D["tw_jpeg_idct"] == 0 and D["tw_png_unfilter"] == 0 and D["tw_mask_rects"] == 0 and D["tw_resize_u8"] >= 5
    assert CC.decode_launches(CC.RECIPES["D_masked"].pairs(oracle))["tw_mask_rects"] == 1
    pairs = CC.RECIPES["C_lanes2"].pairs(oracle)
    assert [p.same for p in pairs] == [0, 0, 1, 1, 0, 0, 0, 0]  # pair 2 is identical only after masking


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [
    P("device", "device", ignore=True),
    P("pageable_gray", "resident_created"),
    P("pageable_gray", "resident_kept_target"),
    P("rgba_rows", "rgba_rows", png8=True, ignore=True),
    P("device", "pageable_gray"),
    P("resident_created", "device"),
    P("jpeg_coef", "pal4_rows"),
    P("rgba_rows", "jpeg_coef"),
    P("pal4_rows", "pal4_rows", png8=True),
    P("pageable_gray", "pageable_gray", identical=True, sized=True),
    P("pageable_gray", "pal4_rows", identical=True),
    P("pageable_gray", "pageable_gray", patch=True),
    P("device", "device", sized=True, keep=True),
    P("bmp", "pageable_gray"),
], ids=str)
def test_builder_refuses_what_the_abi_does_not_have(oracle, spec):
    a, b = CC.frames(333, 41)[0]
    assert CC.why_refused(spec)
    with pytest.raises(ValueError):
        CC.Pair(oracle, spec, a, b)
    with pytest.raises(ValueError):
        CC.check(spec)


def test_builder_refuses_a_kept_target_nobody_kept(oracle):
    a, b = CC.frames(333, 41)[0]
    with pytest.raises(ValueError):
        CC.Pair(oracle, P("resident_kept_target", "pageable_gray"), a, b)
    with pytest.raises(ValueError):
        CC.Pair(oracle, P("resident_kept_target", "pageable_gray"), a, b, prev=CC.Pair(oracle, P(), a, b))
    nxt = CC.frames(333, 41)[1][1]
    assert CC.Pair(oracle, P("resident_kept_target", "pageable_gray"), a, nxt, prev=CC.Pair(oracle, P(keep=True), a, b)).same == 0
    assert dataclasses.is_dataclass(P)
