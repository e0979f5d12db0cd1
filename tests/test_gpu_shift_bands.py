"""The shift bands (TW_OPT_SHIFT_BANDS) on the GPU.

Part 1: the global estimation and the three band kernels alone (Engine.stage_shift_bands) against tests/band_ref.py, value by
value: both signatures, the global record, every band record — at both strides, through LDS and through device memory.
Part 2: batches.  A batch with TW_OPT_SHIFT and TW_OPT_SHIFT_BANDS on must equal, bit for bit in the dense field and vector for
vector, the same pairs submitted with both options off and the explicit field of Engine.shift_bands(ticket) as their init — and
at sizes the oracle handles both must equal farneback_with_init of tests/test_flow_init_abi.py and the oracle's span scan.
Engine.shift_bands(ticket) equals band_ref on the images as the batch sees them.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_ref as BR  # noqa: E402
import shift_ref as S  # noqa: E402
from test_flow_init_abi import farneback_with_init  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
RADIUS = 100
H, W = 240, 320
FAMILIES = ("tw_band_rows", "tw_band_search", "tw_band_verify", "tw_flow_band_init")


# ---- part 1: the stage ------------------------------------------------------------------------------------

def _halves_pair(rng, h, w, sx, sy1, sy2):
    """Noise whose halves move differently: rows above h // 2 of E are T's at (sx, sy1), the rows from h // 2 on at (sx, sy2),
    wherever those exist; everything else independent noise."""
    P = max(abs(sx), abs(sy1), abs(sy2), 1)
    base = rng.integers(0, 256, (h + 2 * P, w + 2 * P)).astype(np.uint8)
    T = base[P:P + h, P:P + w].copy()
    E = np.empty_like(T)
    E[:h // 2] = base[P + sy1:P + sy1 + h, P + sx:P + sx + w][:h // 2]
    E[h // 2:] = base[P + sy2:P + sy2 + h, P + sx:P + sx + w][h // 2:]
    return E, T


def _check_stage(e, E, T, radius, band, want=None):
    """Both strides (padding 0xEE, never read) and both search paths against the reference; the call itself checks the 0xff
    guards behind the pair's share.  Returns the reference (global record, band records)."""
    h, w = E.shape
    if want is None:
        want = BR.estimate(E, T, radius, band)
    g, bands = want
    sE, sT = BR.signatures(E, T, g.dx)
    for stride in (None, w + 13):
        for force_global in (False, True):
            (gE, gT), grec, brec = e.stage_shift_bands(E, T, radius, band, stride=stride, force_global=force_global)
            ctx = (E.shape, radius, band, stride, force_global)
            assert grec == tuple(g), (ctx, grec, g)
            assert gE.shape == sE.shape and np.array_equal(gE, sE) and np.array_equal(gT, sT), ctx
            assert brec == [tuple(b) for b in bands], (ctx, brec, bands)
    return want


@pytest.mark.parametrize("wh", [(1, 33), (63, 40), (64, 64), (65, 97), (129, 130), (257, 130), (320, 240)])
def test_stage_equals_the_reference_value_by_value(engine, wh):
    """Every size, band height and radius; a global move of 0, +r and -r columns; the upper half moved by +ry rows and the
    lower by -(ry // 2).  (1, 33): h < B at B = 48 and 64, h == B + 1 at B = 32 — a last band of one row.  R = 100 is larger
    than every band."""
    w, h = wh
    rng = np.random.default_rng(w * 1000 + h)
    for band in (32, 48, 64):
        for radius in (1, 8, 100):
            rx, ry = min(radius, w // 2), min(radius, h // 2)
            for sx in sorted({0, rx, -rx}):
                E, T = _halves_pair(rng, h, w, sx, ry, -(ry // 2))
                g, bands = _check_stage(engine, E, T, radius, band)
                assert len(bands) == -(-h // band) and bands[-1].rows == h - bands[-1].y
    if wh == (1, 33):
        assert [(b.y, b.rows) for b in BR.estimate(E, T, 8, 32)[1]] == [(0, 32), (32, 1)]
        assert [(b.y, b.rows) for b in BR.estimate(E, T, 8, 48)[1]] == [(0, 33)]


def test_stage_halves_come_back_per_band(engine):
    """The pair the stage test is built from, at a size where the answer is known: bands wholly in the upper half answer its
    move, bands wholly in the lower half theirs, and all are applied."""
    rng = np.random.default_rng(5)
    E, T = _halves_pair(rng, 256, 200, -7, 20, -11)
    g, bands = _check_stage(engine, E, T, 32, 32)
    assert g.dx == -7
    assert [(b.dy, b.applied) for b in bands] == [(20, 1)] * 4 + [(-11, 1)] * 4


def test_stage_on_an_inserted_page(engine):
    """One page of the CPU test: the records equal the reference, and the reference meets the CPU test's expectation."""
    from test_band_ref import expected_bands, inserted
    at, ins, sx = 100, 40, 25
    E, T = inserted(20, at, ins, sx)
    for band in (32, 48, 64):
        g, bands = _check_stage(engine, E, T, RADIUS, band)
        assert g.dx == sx
        for i, want in expected_bands(H, band, at, ins, sx).items():
            assert (bands[i].dy, bands[i].applied) == want, (band, i, bands[i])


def test_stage_products_past_32_bits_at_4096_by_128(engine):
    from test_band_ref import products_pair
    E, T = products_pair()
    g, bands = _check_stage(engine, E, T, 1024, 128)
    assert (bands[0].dy, bands[0].applied) == (40, 1)


def test_stage_a_size_whose_search_reads_device_memory(engine):
    """A wide, short image at R = 1024: the plan says the band's signatures do not fit LDS.  Against its neighbour that stays."""
    h, band, radius = 160, 64, 1024
    # 2 * nblk * (64 + min(160, 64 + 160)) = 448 nblk bytes against the budget
    budget = engine.band_plan(64, h, radius, band).lds_budget
    nblk = budget // 448
    for w, lds in ((64 * nblk, True), (64 * nblk + 1, False)):
        plan = engine.band_plan(w, h, radius, band)
        assert plan.lds == lds and plan.nblk == nblk + (0 if lds else 1) and plan.r == 80 and plan.nb == 3, plan
        assert plan.lds_bytes == 448 * plan.nblk
        rng = np.random.default_rng(w)
        E, T = _halves_pair(rng, h, w, 0, 30, -9)
        g, bands = _check_stage(engine, E, T, radius, band)
        assert [(b.dy, b.applied) for b in bands] == [(30, 1), (bands[1].dy, bands[1].applied), (-9, 1)]


# ---- part 2: batches ---------------------------------------------------------------------------------------

def _planar_out(e, n, h, w):
    arr = e.host_array((n, 2, h, w), np.float32)
    arr[...] = np.nan
    return arr


_WANT = {}


def _want(oracle, E, T, start, params=None, key=None):
    """The oracle's field of (E, T) from `start` (None: zero), computed once per distinct pair, start and parameter set."""
    k = (hash(E.tobytes()), hash(T.tobytes()), E.shape, None if start is None else hash(start.tobytes()), key)
    if k not in _WANT:
        if start is None:
            fx, fy = oracle.farneback(E, T) if params is None else oracle.farneback(E, T, params)
        else:
            fx, fy = farneback_with_init(oracle, E, T, start, params)
        _WANT[k] = np.stack([fx, fy])
    return _WANT[k]


def _run(e, oracle, subs, seen, span, thr, band, radius=RADIUS, inits=None, check_oracle=True, oparams=None, okey=None):
    """subs[i](flow, init) -> the ticket of pair i; seen[i] = (E, T) as the batch sees the pair; inits[i]: a field of the
    pair's own, or None.  One batch with both options on, one with both off in which every seeded pair gets its explicit field;
    returns (band records, fields, results, launch counts) of the batch with the options on."""
    n = len(subs)
    h, w = seen[0][0].shape
    inits = inits or [None] * n
    e.set_shift(radius)
    e.set_shift_bands(band)
    on = _planar_out(e, n, h, w)
    e.launch_counts(reset=True)
    tk = [subs[i](on[i], inits[i]) for i in range(n)]
    sh = [e.shift(t) for t in tk]
    bd = [e.shift_bands(t) for t in tk]
    assert bd == [e.shift_bands(t) for t in tk]  # (the ticket is not consumed, and the answer does not change)
    res = [e.wait(t) for t in tk]
    counts = e.launch_counts(reset=True)
    e.set_shift(0)
    e.set_shift_bands(0)
    starts = []
    for i in range(n):
        if inits[i] is not None:
            starts.append(inits[i])
        else:
            starts.append(BR.field((h, w), sh[i][0], bd[i]) if any(b[3] for b in bd[i]) else None)
    off = _planar_out(e, n, h, w)
    tk = [subs[i](off[i], starts[i]) for i in range(n)]
    res_off = [e.wait(t) for t in tk]
    after = e.launch_counts()
    assert all(after[f] == 0 for f in FAMILIES)
    assert counts["tw_flow_shift_init"] == 0
    for i in range(n):
        g, ref = BR.estimate(seen[i][0], seen[i][1], radius, band, own_field=inits[i] is not None)
        assert sh[i] == tuple(g), (i, sh[i], g)
        assert bd[i] == [tuple(b) for b in ref], (i, bd[i], ref)
        assert np.array_equal(on[i], off[i]), "pair %d: options on against the explicit field" % i
        assert res[i]["vector"] == res_off[i]["vector"], i
        if check_oracle:
            want = _want(oracle, seen[i][0], seen[i][1], starts[i], oparams, okey)
            assert np.array_equal(on[i], want), "pair %d against the oracle" % i
            if span > 0:
                assert res[i]["vector"] == oracle.span_scan(want[0], want[1], span, thr), i
    return bd, on, res, counts


def _host_sub(e, E, T, span, thr):
    return lambda flow, init: e.submit(E, T, span, thr, flow=flow, init=init)


INSERTS = [(100, 40, 0), (64, 32, 25), (130, 24, -30), (96, 48, 0)]


def _pages(n, h=H, w=W, seed=40, scale=1):
    """n inserted-block pairs; returns (pairs, [(at, ins, sx)])."""
    rng = np.random.default_rng(seed)
    what = [(at * scale, ins, sx) for at, ins, sx in INSERTS]
    return [BR.inserted_pair(rng, h, w, *what[i % 4]) for i in range(n)], [what[i % 4] for i in range(n)]


def _promised(bd, what, h, band):
    """The bands the definition promises of pair records `bd` answer their insertion."""
    at, ins, sx = what
    for b in bd:
        y, rows, dy, applied = b[:4]
        if y + rows <= at:
            assert (dy, applied) == (0, 1 if sx else 0), b
        elif y >= at and y + rows + ins <= h:
            assert (dy, applied) == (ins, 1), b


def test_single_pair_schedule_with_area_tables(twflow, oracle):
    """A slots=1 engine at 641 x 481: one pair on two streams, and the coarsest level is not an integer fraction of the image —
    the start comes through the area tables (mode 2), whose source rows fall inside bands."""
    h, w, band = 481, 641, 64
    (pair,), (what,) = _pages(1, h, w, scale=2)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        plan = e.level_plan(w, h, 10, 1, any_fout=True, shift=True)
        assert plan.kind == "two_stream" and plan.parts[0][plan.levels].init
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *pair, 10, 1.0)], [pair], 10, 1.0, band)
        _promised(bd[0], what, h, band)
        assert any(b[3] for b in bd[0])
        assert [cnt[f] for f in FAMILIES] == [1, 1, 2, 1] and cnt["tw_flow_area_init"] == 0


def test_three_pair_batch_on_integer_ratios(twflow, oracle):
    """320 x 240 at the default parameters: the coarsest level is an eighth (mode 1)."""
    band = 32
    pairs, what = _pages(3)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        plan = e.level_plan(W, H, 10, 3, any_fout=True, shift=True)
        assert plan.kind == "batch" and plan.parts[0][plan.levels].launches == 1
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0, band)
        for i in range(3):
            _promised(bd[i], what[i], H, band)
        assert [cnt[f] for f in FAMILIES] == [1, 1, 2, 1] and cnt["tw_flow_area_init"] == 0
        assert cnt.last_z["tw_band_rows"] == 6 and cnt.last_z["tw_flow_band_init"] == 3
        assert cnt["tw_shift_profiles"] == 1 and cnt["tw_shift_verify"] == 2


@pytest.mark.parametrize("kw,band,hw", [(dict(pyrLevels=1), 32, (H, W)), (dict(pyrLevels=0), 32, (H, W)),
                                        (dict(pyrLevels=5), 48, (1024, 1024))])
def test_parameter_sets(twflow, oracle, kw, band, hw):
    """pyrLevels 1 and 0 (0: the start is a copy at scale 1, mode 0); pyrLevels 5 at 1024 x 1024: the coarsest ratio is 32, and with B = 48 the
    32-row area blocks straddle band edges (48, 144, ...), so a block sums rows of two bands."""
    h, w = hw
    pairs, what = _pages(2, h, w, scale=h // H)
    p, op = twflow.default_params(**kw), oracle.default_params(**kw)
    with twflow.Engine(0, p, slots=2) as e:
        assert e.num_levels(w, h) == kw["pyrLevels"]
        # (1024 x 1024, the smallest size with a level at a 32nd: against the explicit field only)
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *q, 10, 1.0) for q in pairs], pairs, 10, 1.0, band, oparams=op,
                             okey=tuple(kw.items()), check_oracle=h < 1000)
        assert all(any(b[3] for b in r) for r in bd)
        if band == 48:
            # a seeded band edge inside an area block: band edges at multiples of 48 that are no multiples of 32
            assert any(b[3] and b[0] % 32 for r in bd for b in r)
        assert cnt["tw_flow_band_init"] >= 1


def test_two_lanes(twflow, oracle, monkeypatch):
    monkeypatch.setenv("TW_LANES", "2")
    pairs, what = _pages(4)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0, 48)
        for i in range(4):
            _promised(bd[i], what[i], H, 48)
        assert [cnt[f] for f in FAMILIES] == [2, 2, 4, 2]  # (each lane's half on its own stream)


def test_one_band_init_per_chunk(twflow, oracle, monkeypatch):
    monkeypatch.setenv("TW_CHUNK_TILES", "1")
    pairs, what = _pages(3)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        plan = e.level_plan(W, H, 10, 3, any_fout=True, shift=True)
        chunks = plan.parts[0][plan.levels].launches
        assert chunks == 3
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0, 64)
        assert [cnt[f] for f in FAMILIES] == [1, 1, 2, chunks] and cnt["tw_flow_area_init"] == 0


def test_ramp_pieces(twflow, oracle):
    """A 64-slot engine fed host pairs from idle: every piece of the cold-start ramp estimates its own pairs behind its own
    uploads."""
    n = 64
    pairs, what = _pages(4)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        for t in [e.submit(*pairs[i % 4], 0, 5.0) for i in range(n)]:  # (buffers and plans exist; the engine is idle again)
            e.wait(t)
        subs = [_host_sub(e, *pairs[i % 4], 0, 5.0) for i in range(n)]
        bd, _, _, cnt = _run(e, oracle, subs, [pairs[i % 4] for i in range(n)], 0, 5.0, 32)
        assert all(bd[i] == bd[i % 4] for i in range(n))
        assert cnt["tw_band_rows"] >= 3 and cnt["tw_band_rows"] == cnt["tw_band_search"] == cnt["tw_flow_band_init"]
        assert cnt["tw_band_verify"] == 2 * cnt["tw_band_rows"] and cnt["tw_band_rows"] == cnt["tw_shift_profiles"]


def test_coarsest_level_on_tw_flow_iter(twflow, oracle, monkeypatch):
    """TW_MFREE=2, TW_MFREE_MIN_W=64: the coarsest level of 640 x 480 is M-free, and its first iteration reads the bands' start."""
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_MFREE_MIN_W", "64")
    h, w, n = 480, 640, 2
    pairs, what = _pages(n, h, w, scale=2)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plan = e.level_plan(w, h, 0, n, any_fout=True, shift=True)
        row = plan.parts[0][plan.levels]
        assert row.init and row.flow_iter and e.level_runs_flow_iter(w, h, plan.levels, n)
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 0, 5.0) for p in pairs], pairs, 0, 5.0, 64)
        for i in range(n):
            _promised(bd[i], what[i], h, 64)
        assert cnt["tw_flow_iter_zero"] == 0 and cnt["tw_flow_band_init"] == row.launches


@pytest.mark.parametrize("env", [dict(), dict(TW_CHUNK_TILES="1")])
def test_mixed_batch(twflow, oracle, env, monkeypatch):
    """An inserted page, an identical pair, an unrelated pair and a pair with its own field in one batch: every pair equals its
    own expectation, the last one's bands all answer applied = 0 and its field is kept, and each coarsest-level chunk has one
    tw_flow_area_init and one tw_flow_band_init launch."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    band = 32
    pairs, what = _pages(2)
    rng = np.random.default_rng(9)
    same = (pairs[0][0], pairs[0][0].copy())
    unrelated = (pairs[0][0], S.page(rng, H + 200, W + 200)[100:100 + H, 100:100 + W].copy())
    seen = [pairs[0], same, unrelated, pairs[1]]
    own = (rng.standard_normal((H, W, 2)) * 2.0).astype(F32)
    inits = [None, None, None, own]
    n = len(seen)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plan = e.level_plan(W, H, 10, n, any_fout=True, shift=True)
        chunks = plan.parts[0][plan.levels].launches
        assert chunks == (n if env else 1)
        bd, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in seen], seen, 10, 1.0, band, inits=inits)
        _promised(bd[0], what[0], H, band)
        assert any(b[3] for b in bd[0])
        assert [b[2:] for b in bd[1]] == [(0, 0, b[1] * W, b[1] * W, 0, 0) for b in bd[1]]
        assert not any(b[3] for b in bd[3]) and any(b[2] for b in bd[3])  # (measured, never applied)
        assert cnt["tw_flow_area_init"] == chunks and cnt["tw_flow_band_init"] == chunks
        assert [cnt[f] for f in FAMILIES[:3]] == [1, 1, 2]


def test_every_kind_of_pair(twflow, oracle):
    """One device pair with a stride, one PNG pair, one reconciled pair (target 3 px wider), one pair with an ignore rectangle
    (estimated after the mask), one resident expected image: each sees the images its batch sees."""
    band = 32
    (pair,), (what,) = _pages(1)
    E, T = pair
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        stride = W + 13
        pe = np.full((H, stride), 0xEE, np.uint8)
        pt = np.full((H, stride), 0xEE, np.uint8)
        pe[:, :W] = E
        pt[:, :W] = T
        dE, dT = e.upload(pe), e.upload(pt)
        bd, *_ = _run(e, oracle, [lambda flow, init: e.submit_dev(dE, dT, W, H, stride, 10, 1.0, flow=flow, init=init)],
                      [pair], 10, 1.0, band)
        _promised(bd[0], what, H, band)

        def rows(img):
            r = np.zeros((H, 1 + W), np.uint8)
            r[:, 1:] = img
            return twflow.PngRows(r, W, H, color_type=0, bit_depth=8)
        pa, pb = rows(E), rows(T)
        bd, *_ = _run(e, oracle, [lambda flow, init: e.submit_png(pa, pb, 10, 1.0, flow=flow, init=init)], [pair], 10, 1.0, band)
        _promised(bd[0], what, H, band)
        # a target 3 px wider: reconciled on the device first
        T2 = np.concatenate([T, T[:, -3:]], axis=1)
        seen = (E, e.stage_resize_u8(T2, W, H))
        bd, *_ = _run(e, oracle, [lambda flow, init: e.submit(E, T2, 10, 1.0, flow=flow, init=init, reconcile=True)],
                      [seen], 10, 1.0, band)
        # an ignore rectangle over a repainted block: the mask copies the expected pixels in before the estimation
        T3 = T.copy()
        T3[10:40, 60:200] = 30
        rects = [(60, 10, 140, 30)]
        seen = (E, e.stage_mask_rects(E, T3, rects))
        assert not np.array_equal(seen[1], T3)
        bd, *_ = _run(e, oracle, [lambda flow, init: e.submit(E, T3, 10, 1.0, flow=flow, init=init, ignore=rects)],
                      [seen], 10, 1.0, band, check_oracle=False)  # (the ignore rule filters vectors: against the explicit field)
        _promised(bd[0], what, H, band)
        img = e.image(E)
        bd, *_ = _run(e, oracle, [lambda flow, init: e.submit_image(img, T, 10, 1.0, flow=flow, init=init)], [pair], 10, 1.0, band)
        _promised(bd[0], what, H, band)
        img.release()


def test_with_the_residual(twflow, oracle):
    """An inserted page: tw_ticket_changes is residual_ref on the oracle's band-seeded flow, and fewer pixels stay unexplained
    than from a zero start.  Measured with the oracle on the CPU for this page (40 rows inserted at row 100, B = 32, span 10,
    tolerance 16; the two bands wholly below the insertion whose content stays are seeded, rows 128 .. 191): 17 825 unexplained
    pixels from a zero start, 12 809 from the bands, a ratio of 0.72 — the inserted rows, the straddling band and the 48 rows
    whose content left the image stay unexplained either way.  The device's records equal the reference's exactly, so the ratio
    here is that one; asserted below 0.8."""
    import residual_ref as RR
    (pair,), (what,) = _pages(1)
    E, T = pair
    span, tol, band = 10, 16, 32
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(tol)
        e.set_shift(RADIUS)
        e.set_shift_bands(band)
        tk = e.submit(E, T, span, 1.0)
        bd = e.shift_bands(tk)
        got, cnt = e.changes(tk)
        res = e.wait(tk)
        g, ref = BR.estimate(E, T, RADIUS, band)
        assert bd == [tuple(b) for b in ref]
        want = _want(oracle, E, T, BR.field((H, W), g.dx, ref))
        _, rec = RR.residual_ref(E, T, (want[0], want[1]), span, tol)
        assert got == rec and cnt == len(rec)
        assert res["vector"] == oracle.span_scan(want[0], want[1], span, 1.0)
        zero = _want(oracle, E, T, None)
        _, rec0 = RR.residual_ref(E, T, (zero[0], zero[1]), span, tol)
        n1, n0 = sum(r[3] for r in rec), sum(r[3] for r in rec0)
        print("unexplained pixels: zero start %d, bands %d" % (n0, n1))
        assert n1 * 5 < n0 * 4


def test_option_off_launches_copies_and_holds_what_it_did(twflow):
    pairs, _ = _pages(3)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        def run():
            e.launch_counts(reset=True)
            tk = [e.submit(*p, 10, 1.0) for p in pairs]
            with pytest.raises(twflow.TwError) as ei:
                e.shift_bands(tk[1])
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
            res = [e.wait(t) for t in tk]  # (the tickets are still waitable)
            return e.launch_counts(reset=True), res, e.memory()
        c0, r0, m0 = run()
        assert all(c0[f] == 0 for f in FAMILIES)
        e.set_shift_bands(64)
        e.set_shift_bands(0)
        c1, r1, m1 = run()
        assert c1 == c0 and m1 == m0 and [r["vector"] for r in r1] == [r["vector"] for r in r0]
        # the bands option without TW_OPT_SHIFT: ignored — no launch, no buffer, no records
        e.set_shift_bands(64)
        c2, r2, m2 = run()
        assert c2 == c0 and m2 == m0 and [r["vector"] for r in r2] == [r["vector"] for r in r0]
        # shift alone: its buffers, none of the bands'
        e.set_shift_bands(0)
        e.set_shift(64)
        for t in [e.submit(*p, 10, 1.0) for p in pairs]:
            e.wait(t)
        ms = e.memory()
        # with both on the feature's buffers appear once and stay
        e.set_shift_bands(64)
        for t in [e.submit(*p, 10, 1.0) for p in pairs]:
            e.wait(t)
        m3 = e.memory()
        assert m3["device_bytes"] > ms["device_bytes"] and m3["pinned_host_bytes"] > ms["pinned_host_bytes"]
        for _ in range(2):
            for t in [e.submit(*p, 10, 1.0) for p in pairs]:
                e.wait(t)
        assert e.memory() == m3
        e.set_shift(0)
        e.set_shift_bands(0)
        c4, r4, _ = run()
        assert c4 == c0 and [r["vector"] for r in r4] == [r["vector"] for r in r0]


def test_refusals(twflow):
    (pair,), _ = _pages(1)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_shift(RADIUS)
        e.set_shift_bands(48)
        for v in (16, 33, 1040, -1):
            with pytest.raises(twflow.TwError) as ei:
                e.set_shift_bands(v)
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        tk = e.submit(*pair, 10, 1.0)
        L = twflow.lib()
        bad = twflow.TW_E_BAD_PARAMETER
        n = C.c_int(-7)
        recs = (twflow.ShiftBand * 8)()
        assert L.tw_ticket_shift_bands(e._h, tk[0], recs, 8, None) == bad             # a null n
        assert L.tw_ticket_shift_bands(e._h, tk[0], None, 8, C.byref(n)) == bad       # a null out with cap > 0
        assert L.tw_ticket_shift_bands(e._h, tk[0] + 1000, recs, 8, C.byref(n)) == bad  # an unknown ticket
        assert n.value == -7
        want = [tuple(b) for b in BR.estimate(*pair, RADIUS, 48)[1]]  # (the refused values left the band height at 48)
        assert len(want) == 5 and e.shift_bands(tk) == want
        # cap smaller than nb: cap records written, nb reported
        for i in range(8):
            recs[i].y = -1
        assert L.tw_ticket_shift_bands(e._h, tk[0], recs, 2, C.byref(n)) == 0 and n.value == 5
        assert [recs[i].as_tuple() for i in range(2)] == want[:2] and recs[2].y == -1
        e.wait(tk)
        assert L.tw_ticket_shift_bands(e._h, tk[0], recs, 8, C.byref(n)) == bad       # a waited ticket
