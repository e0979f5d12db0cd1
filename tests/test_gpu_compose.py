"""Feature combinations on the schedule production runs, against the CPU oracle (DESIGN.md §3 "Composition").

Device JPEG, PNG kinds, size reconcile, resident images, ignore rectangles, hit regions, initial fields and kept targets, mixed
in one batch that ends in the grid-only iteration (tw_flow_iter<15, 3>: no tw_span_gather) — the recipes of
tests/compose_cases.py.  Every recipe runs at threshold 0 (every grid point with a non-zero flow) and at threshold 1
(scattered hits, several regions), and once more under TW_GRID_FINAL=0, which must change the launches and nothing else.

Values are compared bit for bit with the oracle's answer on the CPU-prepared images (compose_cases.reference): vectors,
regions (regions_ref), dense fields where a pair asks for one, and kept images (a follow-up pair of the kept image against
the reference's bytes must be flagged identical by tw_pair_same).  The path is asserted from the launch counters: what the
level plan says about level 0, and what the specs say about the decode, resize and mask launches.  After every batch the
same engine runs a plain pair and answers the oracle: no table of the batch is left behind.
"""
import numpy as np
import pytest

import compose_cases as CC
import regions_ref as R
from compose_cases import PairSpec as P
from test_gpu_level_plan import SWITCHES
from test_gpu_stages_f64 import same_bits, same_vectors

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.0, 1.0)
MODES = [True, False]
MODE_IDS = ["grid_final", "TW_GRID_FINAL=0"]


def set_env(monkeypatch, env, grid_final):
    for name in SWITCHES + ("TW_RAMP",):
        monkeypatch.delenv(name, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if not grid_final:
        monkeypatch.setenv("TW_GRID_FINAL", "0")


def check_wait(e, oracle, pair, ticket, span, thr, gap, what):
    """One ticket against the oracle: tw_wait_regions where the batch has regions (gap > 0), tw_wait otherwise."""
    want = pair.vectors(oracle, span, thr)
    if gap:
        status, vecs, rof, regs, nreg = e.wait_regions(ticket)
        records, region_of = pair.regions(oracle, span, thr, gap)
        assert nreg == len(records), "%s: %d regions, want %d" % (what, nreg, len(records))
        assert rof == region_of, what
        assert len(regs) == min(len(records), R.MAX_REGIONS), what
        for got, rec in zip(regs, records):
            assert R.same_record(got, rec), (what, got, rec)
    else:
        res = e.wait(ticket)
        status, vecs = res["status"], res["vector"]
    same_vectors(vecs, want, what)
    assert status == ("SUSPICIOUS" if want else "OK"), what
    return len(want)


def level0(e, r, n, any_fout, any_init):
    """(level-0 launches, their pairs, the plans) of the batch: one plan per piece of the ramp, one part per lane."""
    plans = [e.level_plan(r.w, r.h, r.span, m, any_fout=any_fout, any_init=any_init) for m in (r.pieces() if r.ramp else [n])]
    rows = [part[0] for pl in plans for part in pl.parts]
    assert [row.pairs for row in rows] == r.pieces(), (r.name, rows)
    for row in rows:
        assert row.flow_iter and row.flow_iter_last, (r.name, row)  # level 0 runs tw_flow_iter: the path is reached
    return sum(row.launches for row in rows), {row.tail for row in rows} | {row.per for row in rows}, plans


_PLAIN = {}


def plain_pairs(oracle, w, h):
    """a plain pair, and an identical one (two pairs: the batch schedule, whose tw_pair_same flags are what is read)"""
    if (w, h) not in _PLAIN:
        a, b = CC.frames(w, h)[1]
        _PLAIN[(w, h)] = [CC.Pair(oracle, P(), a, b), CC.Pair(oracle, P(identical=True), a, b)]
    return _PLAIN[(w, h)]


def run_batch(e, oracle, r, pairs, thr, grid_final, plain_wait=False):
    n = len(pairs)
    gap = 0 if plain_wait else r.gap
    live, kept_images, kept = [], [], None
    any_fout = any(p.spec.flow for p in pairs)
    out = None
    if any_fout:
        out = e.host_array((n, 2, r.h, r.w), np.float32)
        out[...] = np.nan
    created = {i: e.image(p.a) for i, p in enumerate(pairs) if p.spec.expected == "resident_created"}
    e.launch_counts(reset=True)
    tickets = []
    for i, p in enumerate(pairs):
        res = created.get(i, kept if p.spec.expected == "resident_kept_target" else None)
        tickets.append(CC.submit(e, p, r.span, thr, resident=res, flow=out[i] if p.spec.flow else None, live=live))
        if p.spec.keep:
            kept = e.keep(tickets[-1], "target")
            kept_images.append((kept, p))
    assert [t[0] for t in tickets] == list(range(tickets[0][0], tickets[0][0] + n)), "tickets are not consecutive"
    hits = [check_wait(e, oracle, p, tk, r.span, thr, gap, "%s thr %g pair %d (%s -> %s)" % (r.name, thr, i, p.spec.expected, p.spec.target))
            for i, (p, tk) in enumerate(zip(pairs, tickets))]
    flags = e.same_flags()
    cnt = e.launch_counts(reset=True)
    print("compose %s thr %g grid_final %d: hits %s launches %s" % (r.name, thr, grid_final, hits, {k: v for k, v in cnt.items() if v}))
    assert sum(hits) > 0

    # ---- values beyond the vectors
    assert flags == [p.same for p in pairs], (r.name, flags)
    for i, p in enumerate(pairs):
        if p.spec.flow:
            same_bits(np.array(out[i]), p.field(oracle), "%s: dense field of pair %d" % (r.name, i))

    # ---- the path
    chunks, zs, plans = level0(e, r, n, any_fout, any(p.init is not None for p in pairs))
    assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1, cnt  # one batch
    assert cnt["tw_hit_regions"] == (1 if r.gap else 0), cnt
    assert cnt["tw_pair_same"] == len(r.pieces()), cnt               # a launch per part: the ramp's three pieces, a lane's half
    for fam, want in CC.decode_launches(pairs).items():
        assert cnt[fam] == want, (r.name, fam, cnt[fam], want)
    assert cnt["tw_flow_export"] >= 1 if any_fout else cnt["tw_flow_export"] == 0
    on = r.grid_only and grid_final
    assert all(pl.kind == "batch" and pl.grid_final == on and pl.fused_final == r.scan_fused for pl in plans), plans
    if r.scan_fused:
        assert cnt["tw_blur_grid"] == chunks == 1 and cnt["tw_flow_iter_grid"] == 0 and cnt["tw_span_gather"] == 0, cnt
    elif on:
        assert cnt["tw_flow_iter_grid"] == chunks and cnt["tw_span_gather"] == 0 and cnt["tw_blur_grid"] == 0, (cnt, chunks)
        assert cnt.last_z["tw_flow_iter_grid"] in zs, (cnt.last_z, zs)
    else:
        assert cnt["tw_flow_iter_grid"] == 0 and cnt["tw_span_gather"] == chunks and cnt["tw_blur_grid"] == 0, (cnt, chunks)

    # ---- isolation: a plain pair on the same engine, and every kept image against the reference's bytes
    follow = plain_pairs(oracle, r.w, r.h)
    tks = [CC.submit(e, p, r.span, thr, live=live) for p in follow]
    tks += [e.submit_image(img, p.b, r.span, thr) for img, p in kept_images]
    for p, tk in zip(follow, tks):
        check_wait(e, oracle, p, tk, r.span, thr, gap, "%s thr %g: the plain pair behind the batch" % (r.name, thr))
    for tk in tks[2:]:
        e.wait(tk)
    assert e.same_flags() == [0, 1] + [1] * len(kept_images), "a kept image is not the reference's prepared target"
    cnt = e.launch_counts(reset=True)
    assert cnt["tw_mask_rects"] == 0 and cnt["tw_jpeg_idct"] == 0 and cnt["tw_png_unfilter"] == 0 and cnt["tw_resize_u8"] == 0, cnt
    for img in [im for im, _ in kept_images] + list(created.values()):
        img.release()
    assert e.resident()["images"] == 0 and e.resident()["bytes_in_use"] == 0


@pytest.mark.parametrize("grid_final", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(CC.RECIPES))
def test_recipe_against_the_oracle(twflow, oracle, monkeypatch, name, grid_final):
    r = CC.RECIPES[name]
    pairs = r.pairs(oracle)
    set_env(monkeypatch, r.env, grid_final)
    with twflow.Engine(0, twflow.default_params(), slots=r.slots) as e:
        if r.scan_fused:
            e.set_option(twflow.OPT_SCAN_FUSED_FINAL, 1)
        e.set_regions(r.gap)
        for thr in THRESHOLDS:
            run_batch(e, oracle, r, pairs, thr, grid_final)
        if r.gap:  # a plain tw_wait on a regions batch returns the same vectors
            run_batch(e, oracle, r, pairs, 1.0, grid_final, plain_wait=True)


# ---- F: one pair on a slots = 1 engine — the twin schedule, which is not grid-only ------------------------------------
@pytest.mark.parametrize("grid_final", MODES, ids=MODE_IDS)
def test_single_pair_twin_schedule(twflow, oracle, monkeypatch, grid_final):
    """No call takes coefficients for one image and PNG rows for the other, so the recipe is three batches of one pair:
    JPEG expected image -> sized gray target; RGBA -> sized palette target; and the first pair's expected image, kept as the
    device decoded it, -> sized palette target.  Each with rectangles, a field and regions."""
    set_env(monkeypatch, (), grid_final)
    w, h, span, gap = 640, 480, 10, 1
    fr = CC.frames(w, h)
    first = CC.Pair(oracle, P("jpeg_coef", "pageable_gray", sized=True, ignore=True, init=True), fr[0][0], fr[0][1], seed=0)
    second = CC.Pair(oracle, P("rgba_rows", "pal4_rows", sized=True, ignore=True, init=True), fr[1][0], fr[1][1], seed=1)
    third = CC.Pair(oracle, P("resident_created", "pal4_rows", sized=True, ignore=True, init=True), first.a, fr[0][1], seed=1)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        e.set_regions(gap)
        plan = e.level_plan(w, h, span, 1, any_init=True)
        assert plan.kind == "twin" and not plan.grid_final, plan
        for thr in THRESHOLDS:
            kept = None
            for k, p in enumerate((first, second, third)):
                live = []
                e.launch_counts(reset=True)
                tk = CC.submit(e, p, span, thr, resident=kept, live=live)
                if k == 0:
                    kept = e.keep(tk, "expect")
                assert check_wait(e, oracle, p, tk, span, thr, gap, "F thr %g pair %d" % (thr, k)) > 0
                cnt = e.launch_counts(reset=True)
                print("compose F thr %g pair %d: %s" % (thr, k, {f: v for f, v in cnt.items() if v}))
                assert cnt["tw_twin"] > 0 and cnt["tw_pair_same"] == 0, cnt
                # not grid-only: no tw_flow_iter launch of any kind, the window kernels run level 0 — and the pair's last window
                # launch stores the span-grid samples itself (enqueue_update_blur_chain), so no tw_span_gather either
                assert cnt["tw_flow_iter_grid"] == 0 and cnt.flow_iter() == 0 and cnt["tw_blur_grid"] == 0, cnt
                assert cnt["tw_span_gather"] == 0 and cnt["tw_hit_regions"] == 1, cnt
                assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1, cnt
                for fam, want in CC.decode_launches([p]).items():
                    assert cnt[fam] == want, (k, fam, cnt[fam], want)
            kept.release()
            # no table left behind: a plain pair
            p = plain_pairs(oracle, w, h)[0]
            check_wait(e, oracle, p, CC.submit(e, p, span, thr), span, thr, gap, "F thr %g: the plain pair" % thr)
            assert e.resident()["images"] == 0
