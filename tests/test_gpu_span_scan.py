"""The span scan and the hit read-back on chosen fields, value by value: tw_span_gather, tw_span_scan<false> and
tw_span_scan_seg through tw_stage_span_scan against the plain numpy reference of tests/span_scan_cases.py (which
tests/test_span_scan_reference.py holds against the oracle's loop), the eager 1 024-record copy and tw_wait's late fetch
through the real entry points against the oracle.  Every comparison is on ints and on float BITS; grids, segments and
seams come from Engine.scan_plan, the function the launch itself takes its kernel from (choose_scan)."""
import ctypes as C

import numpy as np
import pytest

import span_scan_cases as S

pytestmark = pytest.mark.gpu

U32 = np.uint32


@pytest.fixture(scope="module")
def eng(twflow):
    e = twflow.Engine(0, twflow.default_params(), slots=1)
    yield e
    e.close()


def run_stage(e, fields, span, thr, single_pair, what):
    """One tw_stage_span_scan call checked against the reference: the counts, the first `count` records in order, the 0xff
    fill from `count` to G, and the launch counters against the kernel scan_plan named.  Returns (plan, [hit indices])."""
    fields = np.ascontiguousarray(fields, np.float32)
    n, _, h, w = fields.shape
    plan = e.scan_plan(w, h, span, n, single_pair)
    e.launch_counts(reset=True)
    counts, xy, dxy = e.stage_span_scan(fields, span, thr, single_pair)
    cnt = e.launch_counts(reset=True)
    other = "tw_span_scan" if plan.kernel == "tw_span_scan_seg" else "tw_span_scan_seg"
    assert (cnt["tw_span_gather"], cnt[plan.kernel], cnt[other], sum(cnt.values())) == (1, 1, 0, 2), (what, plan, cnt)
    assert xy.shape == dxy.shape == (n, plan.G, 2)
    hits = []
    for j in range(n):
        want_n, want_xy, want_dxy = S.ref_scan(fields[j, 0], fields[j, 1], span, thr)
        k = int(counts[j])
        assert k == want_n, (what, j, plan)
        bad = np.flatnonzero((xy[j, :k] != want_xy).any(1) | (dxy[j, :k].view(U32) != want_dxy.view(U32)).any(1))
        assert bad.size == 0, (what, j, plan, "record %d of %d: got %s %s, want %s %s" % (
            bad[0], k, xy[j, bad[0]], dxy[j, bad[0]], want_xy[bad[0]], want_dxy[bad[0]]))
        stray = np.flatnonzero((xy[j, k:].view(U32) != S.FILL).any(1) | (dxy[j, k:].view(U32) != S.FILL).any(1))
        assert stray.size == 0, (what, j, plan, "record %d beyond the count %d was written" % (k + stray[0], k))
        hits.append(want_xy[:, 1].astype(np.int64) // span * plan.gw + want_xy[:, 0] // span)
    return plan, hits


# ---- value cases ----------------------------------------------------------------------------------------------------

def wrong_cases(e, fields, thr, single_pair, where):
    """The names of the value cases of one field (where: [(pair, grid index, case)]) that the kernels get wrong, every one of
    them: the cases whose point is a hit when it must not be or the reverse, or — when the launch differs from the reference
    in anything else, a record's bits, the order, the fill — the whole field's."""
    fields = np.ascontiguousarray(fields, np.float32)
    counts, xy, dxy = e.stage_span_scan(fields, 1, thr, single_pair)
    bad = []
    for j, i, c in where:
        k = max(int(counts[j]), 0)
        got = set((xy[j, :k, 1].astype(np.int64) * S.VALUE_W + xy[j, :k, 0]).tolist())
        if (i in got) != c.hit:
            bad.append((c.name, "pair %d" % j, "hit" if i in got else "no hit"))
    try:
        run_stage(e, fields, 1, thr, single_pair, thr)
    except AssertionError as err:
        bad.append(("threshold %r" % thr, str(err)[:300]))
    return bad


@pytest.mark.parametrize("single_pair", [False, True], ids=["one_workgroup", "segments"])
def test_value_cases(eng, single_pair):
    """Every value case at a grid point of its own (span_scan_cases.value_cases: the strict compare at 25, the compare in
    double, both contractions, denormal and underflowing len, signed zeros, NaN, infinities, overflow, thresholds whose square
    is beyond float or infinite, a negative threshold), through both kernels."""
    assert eng.scan_plan(S.VALUE_W, S.VALUE_H, 1, 1, single_pair).kernel == ("tw_span_scan_seg" if single_pair else "tw_span_scan")
    wrong = []
    for thr, where, f in S.value_fields():
        wrong += wrong_cases(eng, f[None], thr, single_pair, [(0, i, c) for c, i in where])
    assert not wrong, "\n".join(map(str, wrong))  # (a string: pytest abridges a list)


def test_value_cases_inside_a_batch(eng):
    """The value fields as the middle pair of three, between a pair whose every point is a hit and their own mirror image."""
    G = S.VALUE_W * S.VALUE_H
    full = S.pattern_field(S.VALUE_W, S.VALUE_H, 1, np.ones(G, bool))
    wrong = []
    for thr, where, f in S.value_fields():
        wrong += wrong_cases(eng, np.stack([full, f, f[:, ::-1, ::-1]]), thr, False,
                             [(1, i, c) for c, i in where] + [(2, G - 1 - i, c) for c, i in where])
    assert not wrong, "\n".join(map(str, wrong))  # (a string: pytest abridges a list)


# ---- position patterns ----------------------------------------------------------------------------------------------

def test_the_grids_reach_what_they_are_there_for(eng):
    """The plans of the chosen sizes, from the function the launches use: which kernel a single pair and a batch take, the
    segment size, a last segment of one point, second rounds of one point and of four iterations, 17 rounds."""
    single = [eng.scan_plan(w, h, s, 1, True) for w, h, s in S.GRIDS]
    batch = [eng.scan_plan(w, h, s, 1, False) for w, h, s in S.GRIDS]
    assert [p.G for p in single[:12]] == [5, 1024, 1025, 2048, 2049, 16384, 16385, 32768, 32769, 35845, 524288, 524290]
    assert all(p.kernel == "tw_span_scan" and p.S == 0 and p.segments == 0 for p in batch)
    assert [p.kernel == "tw_span_scan_seg" for p in single[:12]] == [False] * 4 + [True] * 7 + [False]
    seg = {p.G: (p.S, p.segments) for p in single if p.kernel == "tw_span_scan_seg"}
    assert seg[2049][1] == 3 and 2049 - 2 * seg[2049][0] == 1            # the last segment holds one point
    assert seg[16384][1] == 16 and 16 * seg[16384][0] == 16384           # sixteen full segments
    assert seg[16385][1] == 9 and seg[16385][0] == 2 * seg[16384][0]
    assert seg[524288][1] == 16 and 16 * seg[524288][0] == 524288
    assert all(p.rounds == 1 for p in single if p.kernel == "tw_span_scan_seg")
    rounds = {p.G: p.rounds for p in batch}
    per_round = 524288 // 16  # the points of a round: the largest segment
    assert seg[524288][0] == per_round
    assert (rounds[32768], rounds[32769], rounds[35845], rounds[524288], rounds[524290]) == (1, 2, 2, 16, 17)
    assert 32769 - per_round == 1 and 524290 - 16 * per_round == 2
    it = seg[2049][0]  # the points of an iteration: the smallest segment
    assert -(-(35845 - per_round) // it) == 4                            # four iterations: half an unroll group of eight
    odd = [p for p in single if p.gw == 157]
    assert len(odd) == 3 and all(p.kernel == "tw_span_scan_seg" for p in odd)
    assert eng.scan_plan(S.VALUE_W, S.VALUE_H, 1, 1, True).kernel == "tw_span_scan_seg"
    assert eng.scan_plan(S.VALUE_W, S.VALUE_H, 1, 3, False).kernel == "tw_span_scan"


@pytest.mark.parametrize("grid", S.GRIDS, ids=lambda g: "%dx%d_span%d" % g)
def test_hit_patterns(eng, grid):
    """No hit, every point, every second point, hits in the first / the last segment only and a single hit at every seam
    (span_scan_cases.seam_indices with the single pair's S), through the one-workgroup kernel and, where a single pair takes
    it, through the segments."""
    w, h, span = grid
    sp = eng.scan_plan(w, h, span, 1, True)
    modes = [False] + ([True] if sp.kernel == "tw_span_scan_seg" else [])
    pats = S.patterns(sp.G, sp.S, sp.segments)
    assert len(pats) >= 7
    for name, hits in pats:
        f = S.pattern_field(w, h, span, hits)[None]
        for single_pair in modes:
            plan, got = run_stage(eng, f, span, S.PATTERN_THRESHOLD, single_pair, (name, single_pair))
            assert plan.kernel == ("tw_span_scan_seg" if single_pair else "tw_span_scan")
            assert np.array_equal(got[0], np.flatnonzero(hits)), name


@pytest.mark.parametrize("grid", [(41, 25, 1), (145, 113, 1), (335, 107, 1), (1093, 98, 7)], ids=lambda g: "%dx%d_span%d" % g)
def test_batch_of_five_keeps_each_pairs_region(eng, grid):
    """Five pairs in one tw_span_scan<false> launch — all, none, sparse, all, a single last point: every pair's region holds its
    own records and the fill behind them (a pair's records spilling into its neighbour's region would overwrite either)."""
    w, h, span = grid
    G = eng.scan_plan(w, h, span, 5, False).G
    i = np.arange(G)
    pats = [np.ones(G, bool), np.zeros(G, bool), i % 7 == 3, np.ones(G, bool), i == G - 1]
    f = np.stack([S.pattern_field(w, h, span, p) for p in pats])
    for j in range(5):
        f[j, :, ::span, ::span] += np.where(f[j, :, ::span, ::span] != 0, np.float32(j * 2 ** 20), 0)  # the pair's mark, exact
    plan, got = run_stage(eng, f, span, S.PATTERN_THRESHOLD, False, grid)
    assert plan.kernel == "tw_span_scan"
    for j in range(5):
        assert np.array_equal(got[j], np.flatnonzero(pats[j])), j


def test_stage_refuses_a_single_pair_of_several(eng, twflow):
    f = np.zeros((2, 2, 8, 8), np.float32)
    with pytest.raises(twflow.TwError) as ei:
        eng.stage_span_scan(f, 1, 1.0, True)
    assert ei.value.code == twflow.TW_E_BAD_PARAMETER
    with pytest.raises(twflow.TwError) as ei:
        eng.stage_span_scan(f, 0, 1.0, False)
    assert ei.value.code == twflow.TW_E_BAD_PARAMETER


# ---- the read-back, through the real entry points -------------------------------------------------------------------

@pytest.fixture(scope="module")
def readback(oracle):
    pairs = S.readback_pairs()
    return [(a, b) + tuple(oracle.farneback(a, b)) for a, b in pairs]


def test_counts_around_the_eager_copy(twflow, oracle, readback):
    """Hit counts of exactly 0, 1, 1 023, 1 024, 1 025 and every point (the thresholds from the oracle's field, the counts
    asserted from the oracle): a single pair, and one pair of a 4-pair batch (tw_span_scan<false> over four record regions)."""
    (a, b, wx, wy), (a2, b2, wx2, wy2) = readback
    lens = S.ref_len(wx, wy)
    cases = [(k, S.threshold_for_count(lens, k)) for k in S.READBACK_COUNTS] + [(int((lens > 0).sum()), 0.0)]
    with twflow.Engine(0, twflow.default_params(), slots=1) as e1, twflow.Engine(0, twflow.default_params(), slots=4) as e4:
        for k, thr in cases:
            want = oracle.span_scan(wx, wy, 1, thr)
            assert len(want) == k, (k, thr)
            assert e1.diff(a, b, 1, thr)["vector"] == want, k
            e4.launch_counts(reset=True)
            tk = [e4.submit(p, q, 1, thr) for p, q in ((a2, b2), (a, b), (a2, b2), (a, b))]
            got = [e4.wait(t)["vector"] for t in tk]
            cnt = e4.launch_counts(reset=True)
            assert (cnt["tw_span_scan"], cnt["tw_span_scan_seg"]) == (1, 0), cnt
            want2 = oracle.span_scan(wx2, wy2, 1, thr)
            assert got[1] == want and got[3] == want and got[0] == want2 and got[2] == want2, k


def test_tw_wait_caps(twflow, oracle, readback):
    """tw_wait with cap below, at and above the count and the eager copy's 1 024 records, and without a buffer: *n is the
    full count, exactly min(count, cap) records are written, the caller's buffer beyond them keeps its bytes."""
    a, b, wx, wy = readback[0]
    count, thr = S.wait_threshold(S.ref_len(wx, wy))
    want = oracle.span_scan(wx, wy, 1, thr)
    assert len(want) == count >= 1500
    L = twflow.lib()
    room = count + 8
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        for cap in (0, 1, 1023, 1024, 1025, count - 1, count, count + 1, None):
            buf = (twflow.Vector * room)()
            C.memset(buf, 0xAB, C.sizeof(buf))
            n = C.c_int(-7)
            tk = e.submit(a, b, 1, thr)
            rc = L.tw_wait(e._h, tk[0], None if cap is None else buf, count if cap is None else cap, C.byref(n), None)
            assert rc == twflow.TW_OK and n.value == count, (cap, rc, n.value)
            k = 0 if cap is None else min(count, cap)
            assert [(buf[i].x, buf[i].y, buf[i].dx, buf[i].dy) for i in range(k)] == want[:k], cap
            raw = np.frombuffer(buf, np.uint8)
            assert (raw[k * C.sizeof(twflow.Vector):] == 0xAB).all(), cap
