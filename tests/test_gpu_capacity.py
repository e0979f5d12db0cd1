"""Every slot of full-capacity batches, past 4 GiB of workspace, against the CPU oracle (DESIGN.md §3 "Capacity").

A kernel of a batch finds its pair at base + z * (bytes per pair); at 1920 x 1080 a pair's polynomial expansions are 83 MB,
so z * bytes passes 2^32 at slot 52 and 2^33 at slot 104 of the level-0 launch, and the staging arrays pass 2^32 within 256
slots from 1936 x 1089 on.  The other batch tests stop at 64 pairs of 640 x 480 or 16 pairs of 1080p.

Every test first asserts the regime it is there for — from tests/capacity_cases.byte_table (which arrays pass which power of
two), from the launch counters (how many pairs the level-0 launches covered) and from Engine.level_chunk — then compares
EVERY slot with the oracle, bit for bit, and names the first wrong slot.  A batch holds K distinct pairs, slot s holding pair
s % K; capacity_cases.assert_wrap_cannot_hide proves on the table that no offset which lost a power of two finds the same
pair again.  The oracle's answers are computed once per module (`refs`).

Level-0 launches are balanced (choose_level_schedule: balanced_launch_pairs): 256 pairs against a chunk of 139 go out as
128 + 128, not 139 + 117, so a launch index above 127 needs a batch of 129 .. 139 pairs (the second batch of case b).
"""
import time

import numpy as np
import pytest

import capacity_cases as CAP
from capacity_cases import Form, P31, P32, P33

pytestmark = pytest.mark.gpu
F32 = np.float32
K = 5
SPAN = 10
HD = (1920, 1080)
BIG = CAP.smallest_shape_past_2_32()  # the smallest 16:9 size whose d_filt and d_fstage pass 2^32 within 256 slots
HUGE = CAP.smallest_shape_for_images_past_2_32()  # ... and the smallest whose gray images (d_img) do: 3872 x 2178
SWITCHES = ("TW_LANES", "TW_RAMP", "TW_MFREE", "TW_LATENCY_STREAMS", "TW_GRID_FINAL", "TW_CHUNK_TILES", "TW_SAME_IMAGE",
            "TW_PYR_FUSED")


def clean_env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- the oracle's answers, once per module ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(oracle):
    """refs(w, h, K, **params) -> (pairs, fields [K] of (2, h, w), vectors [K] at SPAN / threshold 0): one oracle.farneback
    and one oracle.span_scan per distinct pair; read-only.  refs.seconds: the oracle's time so far."""
    cache = {}

    def get(w, h, k=K, images=None, **params):
        key = (w, h, k, tuple(sorted(params.items())), images is not None and id(images))
        if key not in cache:
            pairs = images if images is not None else CAP.distinct_pairs(w, h, k)
            t0 = time.time()
            op = oracle.default_params(**params)
            fields = CAP.in_threads(lambda ab: np.stack(oracle.farneback(ab[0], ab[1], op)), pairs)
            vecs = [CAP.vectors_array(oracle.span_scan(f[0], f[1], SPAN, 0.0)) for f in fields]
            for x in fields + vecs:
                x.flags.writeable = False
            get.seconds += time.time() - t0
            print("oracle: %d pairs of %dx%d %r in %.1f s" % (len(pairs), w, h, params, time.time() - t0))
            cache[key] = (pairs, fields, vecs)
        return cache[key]

    get.seconds = 0.0
    yield get
    cache.clear()        # the fields, and the images of capacity_cases' cache: nothing of this module stays resident
    CAP._PAIRS.clear()


def level_sizes(oracle, e, w, h):
    return [(lv.width, lv.height) for lv in oracle.level_plan(w, h, e.params.pyrScale, e.params.pyrLevels)]


def regime(e, oracle, name, w, h, n, form, expect, k=K, span=SPAN):
    """The byte table of the batch; the wrap-cannot-hide proof; `expect`: {row name: the power of two its largest offset
    must have reached}.  Returns (rows, parts)."""
    sizes = level_sizes(oracle, e, w, h)
    rows = CAP.byte_table(e, w, h, span, n, form, sizes)
    CAP.assert_wrap_cannot_hide(rows, k)
    print(CAP.format_table(rows, "\ncase %s: %d pairs of %dx%d, slots %d, level-0 chunk %d" % (name, n, w, h, e.slots, e.level_chunk(w, h, 0))))
    by = {r.name: r for r in rows}
    for rn, p in expect.items():
        assert rn in by, "case %s: the batch has no %s (rows %s)" % (name, rn, sorted(by))
        assert by[rn].max_offset >= p, "case %s is out of its regime: %s reaches %d < 2^%d" % (name, rn, by[rn].max_offset, p.bit_length() - 1)
    return rows, CAP.batch_parts(e, w, h, span, n, form)


def assert_launches(cnt, parts, n, levels):
    """The launch counters against the plan: one tw_polyexp per launch of every level and part; level 0's launches, the pairs
    of the last one, and that together they covered the batch."""
    l0 = [nc for part in parts for _, nc in CAP.level_launches(part, 0)]
    assert sum(l0) == n
    every = sum(part.rows[k].launches for part in parts for k in range(levels + 1))
    assert cnt["tw_polyexp"] == every and cnt.last_z["tw_polyexp"] == 2 * l0[-1], (cnt["tw_polyexp"], cnt.last_z["tw_polyexp"], every, l0)
    row0, plan = parts[-1].rows[0], parts[-1].plan
    if row0.flow_iter:
        assert cnt["tw_update_matrices"] == sum(part.rows[k].launches for part in parts for k in range(levels + 1)
                                                if not part.rows[k].flow_iter), cnt
        assert cnt.last_z["tw_flow_iter"] == l0[-1], cnt.last_z
    fam = "tw_flow_iter_grid" if plan.grid_final and row0.flow_iter else "tw_span_gather"
    assert cnt[fam] == len(l0) and cnt.last_z[fam] == l0[-1], (fam, cnt[fam], cnt.last_z[fam], l0)
    per = parts[-1].rows[0].per
    assert all(nc == per for nc in l0[:-1]) or len(parts) > 1
    assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1, cnt  # one batch
    return l0


def reconcile_memory(e, oracle, rows, w, h, name, extra=0):
    """Engine.memory() against the table's allocations + the single-pair buffers: the rest is the job, count, flag and plan
    tables and the region records (d_regs: 256 x 36 bytes a slot), none indexed by z * (a pair's bytes) — 0.4 to 3.3 MB as
    measured; 4 MiB is the bound, so that no array of a pair's size goes unlisted."""
    mem = e.memory()["device_bytes"]
    mine = CAP.table_alloc_bytes(rows) + CAP.single_pair_buffers(e, level_sizes(oracle, e, w, h)) + extra
    print("case %s: Engine.memory() device bytes %d (%.2f GB), the table's arrays %d, rest %d" % (name, mem, mem / 1e9, mine, mem - mine))
    assert 0 <= mem - mine < 4 << 20, (mem, mine)


def collect_vectors(e, tickets):
    buf = np.zeros(max(CAP.T.grid_capacity(tickets[0][1], tickets[0][2], tickets[0][3]), 1), CAP.VEC)
    return [CAP.wait_array(e, t, buf).copy() for t in tickets]


# ---- a. host pairs, 128 slots, 1080p: the bench's engine ------------------------------------------------------------------
def run_host_pairs(twflow, oracle, refs, monkeypatch, lanes, n):
    w, h = HD
    clean_env(monkeypatch, **({"TW_LANES": "2"} if lanes == 2 else {}))
    pairs, _, want = refs(w, h)
    assert all(len(v) > 1000 for i, v in enumerate(want) if i != 3)
    name = "a lanes %d" % lanes + (", %d slots" % n if n != 128 else "")
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_chunk(w, h, 0) == min(n, 139)  # (min(139, slots))
        form = Form(images="host", ramp=lanes == 1)
        pieces = [n // 4, n // 4, n // 2] if lanes == 1 else [n // 2, n // 2]
        expect = ({"R@L0": P32} if lanes == 1 else {"R@L0": P33, "I@L0": P31, "flow[0]": P31} if n == 128 else
                  {"R@L0": P33, "I@L0": P32, "flow[0]": P32})
        rows, parts = regime(e, oracle, name, w, h, n, form, expect)
        assert [p.hi - p.lo for p in parts] == pieces
        levels = e.num_levels(w, h)
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[s % K], SPAN, 0.0) for s in range(n)]
        got = collect_vectors(e, tk)
        cnt = e.launch_counts()
        l0 = assert_launches(cnt, parts, n, levels)
        assert l0 == pieces
        if lanes == 1:  # the ramp's three pieces, as test_cold_start_ramp asserts them
            assert cnt["tw_polyexp"] == 3 * (levels + 1) and cnt.last_z["tw_polyexp"] == 2 * pieces[-1], (cnt, cnt.last_z)
        assert cnt.last_z["tw_flow_iter"] == pieces[-1], cnt.last_z
        CAP.first_wrong_slot(got, lambda s: want[s % K], "case " + name)
        reconcile_memory(e, oracle, rows, w, h, name)
    print("case %s: %.1f s" % (name, time.time() - t0))


@pytest.mark.parametrize("lanes", [1, 2])
def test_a_host_pairs_128_slots_1080p(twflow, oracle, refs, monkeypatch, lanes):
    """Pageable gray pairs into an idle engine: the cold-start ramp's pieces of 32, 32 and 64 pairs (R past 2^32 in the
    last), and with TW_LANES=2 two halves of 64, the second lane's workspace behind the first's (R past 2^33)."""
    run_host_pairs(twflow, oracle, refs, monkeypatch, lanes, 128)


def test_a_two_lanes_256_slots_1080p(twflow, oracle, refs, monkeypatch):
    """TW_LANES=2 with 256 slots: two halves of 128; the second lane's base (make_chunk, added on the host) plus the index
    inside its launch takes I and flow[0] past 2^32 — the index alone cannot (the chunk rule: about 2.3 GB a launch)."""
    run_host_pairs(twflow, oracle, refs, monkeypatch, 2, 256)


# ---- b. 256 slots, 1080p, device-resident pairs ---------------------------------------------------------------------------
def test_b_device_pairs_256_slots_1080p(twflow, oracle, refs, monkeypatch):
    """No ramp (nothing to upload).  Level 0 runs as two launches of 128, the second reusing the chunk buffers (R past
    2^33 in both); levels 1 to 3 cover all 256 pairs in one launch (R of level 1 past 2^32).  Then a batch of exactly
    level_chunk pairs on the same engine: ONE level-0 launch, whose indices 130 .. 138 take I, flow[0] and the flow
    iterations' ping-pong buffer past 2^31."""
    w, h = HD
    n = 256
    clean_env(monkeypatch)
    pairs, _, want = refs(w, h)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        chunk = e.level_chunk(w, h, 0)
        assert chunk == 139  # 300 000 tiles / (8 x 135 x 2) tiles of a pair
        dev = [(e.upload(a), e.upload(b)) for a, b in pairs]
        levels = e.num_levels(w, h)
        for m, expect in ((n, {"R@L0": P33, "R@L1": P32}),
                          (chunk, {"R@L0": P33, "I@L0": P31, "flow[0]": P31, "M[0] as flow@L0": P31})):
            rows, parts = regime(e, oracle, "b %d pairs" % m, w, h, m, Form(images="device"), expect)
            assert [part.rows[k].launches for part in parts for k in range(levels + 1)] == [2 if m == n else 1] + [1] * levels
            e.launch_counts(reset=True)
            tk = [e.submit_dev(dev[s % K][0], dev[s % K][1], w, h, w, SPAN, 0.0) for s in range(m)]
            got = collect_vectors(e, tk)
            cnt = e.launch_counts()
            l0 = assert_launches(cnt, parts, m, levels)
            assert l0 == ([128, 128] if m == n else [chunk]), l0
            assert cnt["tw_flow_iter_grid"] == len(l0) and cnt.last_z["tw_flow_iter_grid"] == l0[-1], (cnt, cnt.last_z)
            assert cnt.last_z["tw_flow_iter_ups"] == l0[-1] and cnt["tw_pair_same"] == 1, (cnt, cnt.last_z)
            CAP.first_wrong_slot(got, lambda s: want[s % K], "case b, %d pairs" % m)
        reconcile_memory(e, oracle, rows, w, h, "b")  # (the caller's own device images are not the engine's)
    print("case b: %.1f s" % (time.time() - t0))


# ---- c. dense fields -------------------------------------------------------------------------------------------------------
def test_c_dense_fields_1080p(twflow, oracle, refs, monkeypatch):
    """level_chunk + 5 pairs with a page-locked flow= destination each (2.4 GB): two level-0 launches, the second reusing
    flow[0]; every pixel of every slot.  d_fstage passes 2^31 (it cannot pass 2^32 at this size: 256 slots end 48 MB short).
    TW_RAMP=0: the whole batch is one part, so that level 0 is split by the chunk rule alone."""
    w, h = HD
    clean_env(monkeypatch, TW_RAMP="0")
    pairs, fields, _ = refs(w, h)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=256) as e:
        chunk = e.level_chunk(w, h, 0)
        n = chunk + 5
        assert chunk == 139
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        rows, parts = regime(e, oracle, "c 1080p", w, h, n, Form(images="host", flow_out=True), {"d_fstage": P31, "R@L0": P32})
        assert not parts[0].plan.grid_final
        out = e.host_array((n, 2, h, w), F32)
        out[...] = np.nan
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[s % K], SPAN, 1e9, flow=out[s]) for s in range(n)]
        for t in tk:
            assert e.wait_count(t)[0] == 0
        cnt = e.launch_counts()
        l0 = assert_launches(cnt, parts, n, e.num_levels(w, h))
        assert l0 == [72, 72] and cnt["tw_flow_export"] >= 2, (l0, cnt)
        CAP.first_wrong_slot([out[s] for s in range(n)], lambda s: fields[s % K], "case c, 1080p")
        reconcile_memory(e, oracle, rows, w, h, "c 1080p")
    print("case c 1080p: %.1f s" % (time.time() - t0))


def test_c_dense_fields_and_initial_fields_256_slots(twflow, oracle, refs, monkeypatch):
    """256 slots of the second shape, every pair with a page-locked destination (d_fstage past 2^32), every fourth pair
    (slots 3, 7, .. 255) with a pageable initial field of its own (d_istage past 2^32); the fields and their references are
    built as tests/test_gpu_flow_init.py builds its own."""
    from test_gpu_flow_init import _field, _want
    w, h = BIG
    n = 256
    clean_env(monkeypatch, TW_RAMP="0")
    pairs, fields, _ = refs(w, h)
    inits = [_field(k, h, w, "interleaved") for k in range(K)]  # (the view the submit takes, the field the reference takes)
    t1 = time.time()
    with_init = CAP.in_threads(lambda k: _want(oracle, pairs[k], inits[k][1]), range(K))
    refs.seconds += time.time() - t1
    print("oracle: %d pairs of %dx%d from an initial field in %.1f s" % (K, w, h, time.time() - t1))
    want = lambda s: with_init[s % K] if s % 4 == 3 else fields[s % K]  # noqa: E731
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_chunk(w, h, 0) < n
        form = Form(images="host", flow_out=True, init=True)
        rows, parts = regime(e, oracle, "c second shape", w, h, n, form, {"d_fstage": P32, "d_istage": P32, "R@L0": P32})
        out = e.host_array((n, 2, h, w), F32)
        out[...] = np.nan
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[s % K], SPAN, 1e9, flow=out[s], init=inits[s % K][0] if s % 4 == 3 else None) for s in range(n)]
        for t in tk:
            e.wait_count(t)
        cnt = e.launch_counts()
        l0 = assert_launches(cnt, parts, n, e.num_levels(w, h))
        assert len(l0) >= 2 and cnt["tw_flow_export"] >= len(l0), (l0, cnt)
        assert cnt["tw_flow_area_init"] >= 1 and cnt.last_z["tw_flow_area_init"] == parts[-1].rows[-1].tail, (cnt, cnt.last_z)
        CAP.first_wrong_slot([out[s] for s in range(n)], want, "case c, %dx%d" % (w, h))
        reconcile_memory(e, oracle, rows, w, h, "c second shape")
    print("case c second shape: %.1f s" % (time.time() - t0))


# ---- d. filtered RGBA rows, 256 slots, second shape -------------------------------------------------------------------------
def test_d_filtered_rgba_rows_256_slots(twflow, oracle, refs, monkeypatch):
    """tw_submit_png8 with the K pairs' RGBA rows as reused host buffers: 512 images of filtered rows (d_filt past 2^32), one
    tw_png_unfilter launch of 512 jobs; vectors against the oracle on gray15 of the images."""
    from test_gpu_resident import as_rgba
    w, h = BIG
    n = 256
    clean_env(monkeypatch)
    rgba = [[as_rgba(twflow, g)[:2] for g in pr] for pr in CAP.distinct_pairs(w, h, K)]
    gray = [(a[1], b[1]) for a, b in rgba]
    assert np.array_equal(gray[3][0], gray[3][1])
    _, _, want = refs(w, h, images=gray)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_chunk(w, h, 0) < n
        rows, parts = regime(e, oracle, "d", w, h, n, Form(images="host", rows_ch=4), {"d_filt": P32, "R@L0": P32})
        e.launch_counts(reset=True)
        tk = [e.submit_png8(rgba[s % K][0][0]._rows, 4, rgba[s % K][1][0]._rows, 4, w, h, SPAN, 0.0) for s in range(n)]
        assert [t[0] for t in tk] == list(range(tk[0][0], tk[0][0] + n))  # one batch: no slot was too small for its rows
        got = collect_vectors(e, tk)
        cnt = e.launch_counts()
        assert_launches(cnt, parts, n, e.num_levels(w, h))
        # one batch of n consecutive tickets and ONE tw_png_unfilter launch: flush_ctx gives it 2 n jobs, job 511 the last
        # (its grid is dim3(2 n): last_z, the grid's z, is 1)
        assert cnt["tw_png_unfilter"] == 1 and len(tk) == n and 2 * n - 1 == 511 and cnt.last_z["tw_png_unfilter"] == 1, (cnt, cnt.last_z)
        CAP.first_wrong_slot(got, lambda s: want[s % K], "case d")
        reconcile_memory(e, oracle, rows, w, h, "d")
    print("case d: %.1f s" % (time.time() - t0))


# ---- e. one mixed batch at capacity ---------------------------------------------------------------------------------------
def test_e_mixed_batch_256_slots_1080p(twflow, oracle, monkeypatch):
    """K specs of tests/compose_cases.py cycled over 256 slots at 1080p: RGBA rows (first: the batch's largest filtered
    image), JPEG coefficients, sized targets (gray: d_tsrc and a tw_resize_u8 launch per pair; coefficients: the batch's
    resize jobs), ignore rectangles, a resident expected image, an identical pair; regions at gap 2.  Vectors, regions and
    region_of of every slot against the CPU reference of compose_cases."""
    import compose_cases as CC
    from compose_cases import PairSpec as S
    from regions_ref import same_record
    from test_gpu_stages_f64 import same_vectors
    w, h = HD
    n, gap, thr = 256, 2, 1.0
    clean_env(monkeypatch)
    specs = (S("rgba_rows", "pageable_gray", ignore=True), S("jpeg_coef", "pageable_gray", sized=True),
             S("resident_created", "rgba_rows"), S("pageable_gray", "jpeg_coef", sized=True, ignore=True),
             S("pageable_gray", "pageable_gray", identical=True))
    assert len(specs) == K
    fr = CAP.distinct_pairs(w, h, K)
    t1 = time.time()
    cp = [CC.Pair(oracle, s, fr[k][0], fr[k][1], seed=k) for k, s in enumerate(specs)]
    CAP.in_threads(lambda p: p.field(oracle), cp)
    want = [(p.vectors(oracle, SPAN, thr), p.regions(oracle, SPAN, thr, gap)) for p in cp]
    print("oracle: the %d composed pairs of %dx%d in %.1f s; hits %s, regions %s" %
          (K, w, h, time.time() - t1, [len(v) for v, _ in want], [len(r[0]) for _, r in want]))
    assert sum(len(v) > 0 for v, _ in want) >= 3
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        e.set_regions(gap)
        form = Form(images="host", sized=True, regions=True, filt_slot=CAP.filtered_rows_slot(w, h, 4))
        rows, parts = regime(e, oracle, "e", w, h, n, form, {"R@L0": P33, "d_filt": P31})
        created = e.image(cp[2].a)
        live = []
        e.launch_counts(reset=True)
        tk = [CC.submit(e, cp[s % K], SPAN, thr, resident=created if s % K == 2 else None, live=live) for s in range(n)]
        assert [t[0] for t in tk] == list(range(tk[0][0], tk[0][0] + n)), "the batch was split"
        got = [e.wait_regions(t) for t in tk]
        cnt = e.launch_counts()
        assert_launches(cnt, parts, n, e.num_levels(w, h))
        assert cnt["tw_hit_regions"] == 1, cnt  # (one launch, a workgroup per pair: region_of + z * G up to z = 255)
        for fam, launches in CC.decode_launches([cp[s % K] for s in range(n)]).items():
            assert cnt[fam] == launches, (fam, cnt[fam], launches)
        for s, (status, vecs, rof, regs, nreg) in enumerate(got):
            wv, (records, region_of) = want[s % K]
            what = "case e: slot %d is the first that differs from the reference (%s -> %s)" % (s, specs[s % K].expected, specs[s % K].target)
            same_vectors(vecs, wv, what)
            assert status == ("SUSPICIOUS" if wv else "OK"), what
            assert nreg == len(records) and rof == region_of, what
            assert len(regs) == min(len(records), CC.R.MAX_REGIONS) and all(same_record(g, r) for g, r in zip(regs, records)), what
        created.release()
    print("case e: %.1f s" % (time.time() - t0))


# ---- f. M through HBM ---------------------------------------------------------------------------------------------------------
def smallest_window_without_flow_iter(twflow, w, h, n):
    for win in range(2, 65):
        with twflow.Engine(0, twflow.default_params(winSize=win), slots=n) as e:
            if not e.level_runs_flow_iter(w, h, 0, n):
                return win
    raise AssertionError("every window runs tw_flow_iter")


@pytest.mark.parametrize("window", ["box", "gaussian"])
def test_f_matrices_through_memory_1080p(twflow, oracle, refs, monkeypatch, window):
    """A batch of level_chunk pairs (one level-0 launch, indices up to 138) on the schedules that keep M in memory: the box
    window (flags 0: tw_box's column sums in Vd past 2^33, M past 2^32) and the smallest Gaussian window tw_flow_iter refuses
    (tw_update_matrices + the window kernels, M[0] / M[1] past 2^32).  Three distinct pairs."""
    w, h = HD
    k3 = 3
    clean_env(monkeypatch)
    with twflow.Engine(0, twflow.default_params(), slots=256) as e:
        n = e.level_chunk(w, h, 0)
    assert n == 139
    kw = dict(flags=0) if window == "box" else dict(winSize=smallest_window_without_flow_iter(twflow, w, h, n))
    pairs, _, want = refs(w, h, k3, **kw)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(**kw), slots=n) as e:
        assert not e.level_runs_flow_iter(w, h, 0, n) and e.level_chunk(w, h, 0) == n
        expect = {"M[0]@L0": P32, "M[1]@L0": P32, "R@L0": P33}
        if window == "box":
            expect["Vd@L0"] = P33
        rows, parts = regime(e, oracle, "f %s %r" % (window, kw), w, h, n, Form(images="device"), expect, k=k3)
        dev = [(e.upload(a), e.upload(b)) for a, b in pairs]
        levels = e.num_levels(w, h)
        e.launch_counts(reset=True)
        tk = [e.submit_dev(dev[s % k3][0], dev[s % k3][1], w, h, w, SPAN, 0.0) for s in range(n)]
        got = collect_vectors(e, tk)
        cnt = e.launch_counts()
        l0 = assert_launches(cnt, parts, n, levels)
        # (at least one tw_update_matrices per level; the box window has no fused refresh and launches one per iteration)
        assert l0 == [n] and cnt.flow_iter() == 0 and cnt["tw_update_matrices"] >= levels + 1, (l0, cnt)
        assert cnt.last_z["tw_update_matrices"] == n, cnt.last_z
        if window == "box":
            assert cnt["tw_box"] >= 1 and cnt.last_z["tw_box"] == n, (cnt, cnt.last_z)
        print("case f %s: launches %s" % (window, {f: v for f, v in cnt.items() if v}))
        CAP.first_wrong_slot(got, lambda s: want[s % k3], "case f, %s window" % window)
        reconcile_memory(e, oracle, rows, w, h, "f " + window)
    print("case f %s: %.1f s" % (window, time.time() - t0))


# ---- g. span 1: the dense grid, the records and the region arrays ------------------------------------------------------------
def test_g_span_1_grid_records_and_regions_256_slots(twflow, oracle, refs, monkeypatch):
    """Span 1 makes every pixel a grid point: at the second shape a pair's samples are 16.9 MB of d_grid (past 2^32 within
    256 slots), its records 33.7 MB of d_rec (past 2^33), its region_of and label plane 8.4 MB each (d_regof, d_lab: past
    2^31; the grid is far beyond the label planes that fit LDS).  Threshold 5: 87 to 35 000 hits a pair, so both the eager
    copy of a pair's first 1024 records and the late read of the rest run.  Vectors, region_of and regions of every slot."""
    import regions_ref as R
    w, h = BIG
    n, span, thr, gap = 256, 1, 5.0, 2
    clean_env(monkeypatch)
    pairs, fields, _ = refs(w, h)
    t1 = time.time()
    hits = [oracle.span_scan(f[0], f[1], span, thr) for f in fields]
    want = [(CAP.vectors_array(v),) + CAP.regions_arrays(*R.regions(v, gap, span, w, h)) for v in hits]
    nregs = [len(R.regions(v, gap, span, w, h)[0]) for v in hits]
    refs.seconds += time.time() - t1
    print("reference: span-1 hits %s, regions %s in %.1f s" % ([len(v) for v in hits], nregs, time.time() - t1))
    assert min(len(v) for v in hits) > 0 and max(len(v) for v in hits) > 1024 > min(len(v) for v in hits)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        e.set_regions(gap)
        G = twflow.grid_capacity(w, h, span)
        assert G == w * h > CAP.RGN_LDS_POINTS and e.level_chunk(w, h, 0) < n
        form = Form(images="device", regions=True)
        rows, parts = regime(e, oracle, "g", w, h, n, form, {"d_grid": P32, "d_rec": P33, "d_regof": P31, "d_lab": P31}, span=span)
        assert not parts[0].plan.grid_final  # (span below 5: tw_span_gather fills d_grid)
        dev = [(e.upload(a), e.upload(b)) for a, b in pairs]
        e.launch_counts(reset=True)
        tk = [e.submit_dev(dev[s % K][0], dev[s % K][1], w, h, w, span, thr) for s in range(n)]
        buf, rof_buf, regs_buf = np.zeros(G, CAP.VEC), np.zeros(G, np.int32), np.zeros(twflow.MAX_REGIONS, twflow.REGION_DTYPE)
        for s, t in enumerate(tk):
            vec, rof, regs, nreg = CAP.wait_regions_arrays(e, t, buf, rof_buf, regs_buf)
            wv, wregs, wrof = want[s % K]
            what = "case g: slot %d is the first that differs from the reference" % s
            CAP.first_wrong_slot([vec], lambda _: wv, what)
            assert nreg == nregs[s % K] and np.array_equal(rof, wrof), what
            assert regs.tobytes() == wregs.tobytes(), what
        cnt = e.launch_counts()
        assert_launches(cnt, parts, n, e.num_levels(w, h))
        assert cnt["tw_hit_regions"] == 1, cnt
        reconcile_memory(e, oracle, rows, w, h, "g")
    print("case g: %.1f s" % (time.time() - t0))


# ---- h. 8.4 Mpixel: the gray images, the coarser levels' flow and the region arrays ------------------------------------------
def test_h_gray_images_and_span_1_regions_at_8_megapixels_256_slots(twflow, oracle, refs, monkeypatch):
    """256 pageable gray pairs of 3872 x 2178, the smallest 16:9 size at which d_img passes 2^32; flow[1] (indexed by the
    batch slot, not by the launch) passes it too, and at span 1 d_regof and d_lab pass 2^33 (d_grid 2^34, d_rec 2^35).
    Level 0 runs as eight launches of 32.  Three distinct pairs; TW_RAMP=0, so that the batch is one part."""
    import regions_ref as R
    w, h = HUGE
    n, span, thr, gap, k3 = 256, 1, 6.0, 2, 3
    clean_env(monkeypatch, TW_RAMP="0")
    pairs, fields, _ = refs(w, h, k3)
    t1 = time.time()
    hits = [oracle.span_scan(f[0], f[1], span, thr) for f in fields]
    ref = CAP.in_threads(lambda v: R.regions(v, gap, span, w, h), hits)
    want = [(CAP.vectors_array(v),) + CAP.regions_arrays(*r) for v, r in zip(hits, ref)]
    refs.seconds += time.time() - t1
    print("reference: span-1 hits %s, regions %s in %.1f s" % ([len(v) for v in hits], [len(r[0]) for r in ref], time.time() - t1))
    assert min(len(v) for v in hits) > 0 and max(len(v) for v in hits) > 1024  # (the eager copy and the late read of the records)
    t0 = time.time()
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        e.set_regions(gap)
        G = twflow.grid_capacity(w, h, span)
        form = Form(images="host", regions=True)
        expect = {"d_img": P32, "flow[1]": P32, "d_regof": P33, "d_lab": P33, "d_grid": P33, "d_rec": P33, "R@L0": P33}
        rows, parts = regime(e, oracle, "h", w, h, n, form, expect, k=k3, span=span)
        assert len(parts) == 1 and parts[0].rows[0].launches == 8 and parts[0].rows[0].per == 32, parts[0].rows[0]
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[s % k3], span, thr) for s in range(n)]
        buf, rof_buf, regs_buf = np.zeros(G, CAP.VEC), np.zeros(G, np.int32), np.zeros(twflow.MAX_REGIONS, twflow.REGION_DTYPE)
        for s, t in enumerate(tk):
            vec, rof, regs, nreg = CAP.wait_regions_arrays(e, t, buf, rof_buf, regs_buf)
            wv, wregs, wrof = want[s % k3]
            what = "case h: slot %d is the first that differs from the reference" % s
            CAP.first_wrong_slot([vec], lambda _: wv, what)
            assert nreg == len(ref[s % k3][0]) and np.array_equal(rof, wrof), what
            assert regs.tobytes() == wregs.tobytes(), what
        cnt = e.launch_counts()
        l0 = assert_launches(cnt, parts, n, e.num_levels(w, h))
        assert l0 == [32] * 8 and cnt["tw_hit_regions"] == 1, (l0, cnt)
        reconcile_memory(e, oracle, rows, w, h, "h")
    print("case h: %.1f s" % (time.time() - t0))


# ---- i. 16.8 Mpixel: the sized targets' staging -----------------------------------------------------------------------------
def test_i_sized_gray_targets_at_16_megapixels_256_slots(twflow, oracle, monkeypatch):
    """A pageable gray target of another size in every slot (tw_submit_u8_sized: d_tsrc + tsrc_slot * j, one tw_resize_u8
    launch per pair at submit time) at the smallest 16:9 size at which 256 slots of (w + 5) x (h + 5) bytes pass 2^32.
    d_img passes 2^32 too, flow[1] 2^33; level 0 runs in launches of at most 17 pairs.  Three distinct pairs; the reference
    is the oracle on oracle.reconcile_target of the target.  TW_RAMP=0, so that the batch is one part."""
    w, h = CAP.smallest_shape_for_sized_targets_past_2_32()
    n, k3, (dw, dh) = 256, 3, (3, -2)
    clean_env(monkeypatch, TW_RAMP="0")
    src = CAP.distinct_pairs(w, h, k3)
    t1 = time.time()
    targets = CAP.in_threads(lambda ab: oracle.resize_u8_linear(ab[1], w + dw, h + dh), src)

    def reference(i):
        fx, fy = oracle.farneback(src[i][0], oracle.reconcile_target(targets[i], w, h))
        return CAP.vectors_array(oracle.span_scan(fx, fy, SPAN, 0.0))
    want = CAP.in_threads(reference, range(k3))
    print("oracle: %d sized pairs of %dx%d in %.1f s; vectors %s" % (k3, w, h, time.time() - t1, [len(v) for v in want]))
    assert all(len(v) > 1000 for v in want)
    t0 = time.time()
    try:
        with twflow.Engine(0, twflow.default_params(), slots=n) as e:
            form = Form(images="host", sized=True)
            rows, parts = regime(e, oracle, "i", w, h, n, form, {"d_tsrc": P32, "d_img": P32, "flow[1]": P33, "R@L0": P33}, k=k3)
            assert len(parts) == 1 and parts[0].rows[0].launches >= 15
            e.launch_counts(reset=True)
            tk = [e.submit(src[s % k3][0], targets[s % k3], SPAN, 0.0, reconcile=True) for s in range(n)]
            assert [t[0] for t in tk] == list(range(tk[0][0], tk[0][0] + n))
            got = collect_vectors(e, tk)
            cnt = e.launch_counts()
            assert_launches(cnt, parts, n, e.num_levels(w, h))
            assert cnt["tw_resize_u8"] == n, cnt  # a gray host target is resized by a launch of its own, from its d_tsrc slot
            CAP.first_wrong_slot(got, lambda s: want[s % k3], "case i")
            reconcile_memory(e, oracle, rows, w, h, "i")
    finally:
        CAP._PAIRS.clear()
    print("case i: %.1f s" % (time.time() - t0))
