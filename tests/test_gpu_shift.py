"""The shift (TW_OPT_SHIFT) on the GPU.

Part 1: the three estimation kernels alone (Engine.stage_shift) against tests/shift_ref.py, value by value: the four profiles,
dx, dy, both sums, both areas, `applied`.
Part 2: batches.  A pair whose shift was applied must equal, bit for bit, the same pair submitted with the option off and the
constant field (dx, dy) as its init — and both must equal farneback_with_init of tests/test_flow_init_abi.py and the oracle's
span scan.  Every other pair equals its plain submission.  Engine.shift(ticket) equals shift_ref on the images as the batch
sees them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shift_ref as S  # noqa: E402
from test_flow_init_abi import farneback_with_init  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
RADIUS = 100
H, W = 240, 320
FAMILIES = ("tw_shift_profiles", "tw_shift_search", "tw_shift_verify", "tw_flow_shift_init")


# ---- part 1: the stage ------------------------------------------------------------------------------------

def _noise_pair(rng, h, w, sx, sy):
    """E[y][x] = T[y + sy][x + sx] wherever both exist; everything else independent noise."""
    P = max(abs(sx), abs(sy), 1)
    base = rng.integers(0, 256, (h + 2 * P, w + 2 * P)).astype(np.uint8)
    return base[P:P + h, P:P + w].copy(), base[P - sy:P - sy + h, P - sx:P - sx + w].copy()


def _check_stage(e, E, T, radius, stride=None, force_global=False):
    prof, rec = e.stage_shift(E, T, radius, stride=stride, force_global=force_global)
    for got, want, name in zip(prof, S.profiles(E, T), ("colE", "colT", "rowE", "rowT")):
        assert np.array_equal(got, want), (name, E.shape, radius, stride)
    want = tuple(S.estimate(E, T, radius))
    assert rec == want, (E.shape, radius, stride, force_global, rec, want)
    return rec


@pytest.mark.parametrize("wh", [(1, 1), (1, 9), (9, 1), (3, 3), (63, 5), (65, 33), (257, 130), (320, 240)])
def test_stage_equals_the_reference_value_by_value(engine, wh):
    """Every size, both strides (padding 0xEE, never read), every radius; shifts at 0, at +r and -r of each axis, and one
    beyond r, which must answer the best within reach — whatever the reference says that is.  The call itself checks the
    0xff guards behind the pair's share."""
    w, h = wh
    rng = np.random.default_rng(w * 1000 + h)
    for radius in (1, 8, 100, 1024):
        rx, ry = min(radius, w // 2), min(radius, h // 2)
        for sx, sy in ((0, 0), (rx, ry), (-rx, -ry), (rx + 1, -(ry + 1))):
            E, T = _noise_pair(rng, h, w, sx, sy)
            for stride in (None, w + 13):
                _check_stage(engine, E, T, radius, stride)


def test_stage_on_pages_constant_images_and_the_device_memory_path(engine):
    rng = np.random.default_rng(11)
    E, T = S.shifted_pair(rng, H, W, 25, 60)
    assert _check_stage(engine, E, T, RADIUS)[:3] == (25, 60, 1)
    assert _check_stage(engine, E, T, RADIUS, stride=W + 13)[:3] == (25, 60, 1)
    # force_global on a small size: the device-memory path must equal the LDS path
    plan = engine.shift_plan(W, H, RADIUS)
    assert plan.lds_x and plan.lds_y
    assert _check_stage(engine, E, T, RADIUS, force_global=True)[:3] == (25, 60, 1)
    assert _check_stage(engine, E, T, 24, force_global=True) == _check_stage(engine, E, T, 24)  # (beyond r: the best in reach)
    # constant images: every cost is 0, d = 0 stays
    c = np.full((33, 65), 77, np.uint8)
    assert _check_stage(engine, c, c, 8)[:3] == (0, 0, 0)
    assert _check_stage(engine, c, np.full_like(c, 78), 8)[:3] == (0, 0, 0)


def test_stage_products_past_32_bits_at_4096_by_128(engine):
    w, h = 4096, 128
    E = np.zeros((h, w), np.uint8)
    E[:, w // 2:] = 255
    T = np.zeros((h, w), np.uint8)
    T[:, w // 2 + 300:] = 255
    assert _check_stage(engine, E, T, 1024)[:3] == (300, 0, 1)
    assert _check_stage(engine, E.T.copy(), T.T.copy(), 1024)[:3] == (0, 300, 1)


@pytest.mark.parametrize("wh", [(32768, 4), (4, 32768)])
def test_stage_one_axis_above_the_lds_limit(engine, wh):
    w, h = wh
    plan = engine.shift_plan(w, h, 1024)
    assert (plan.lds_x, plan.lds_y) == (w < h, h < w)  # (the long axis reads its profiles from device memory)
    rng = np.random.default_rng(w)
    long_shift = 777
    E, T = _noise_pair(rng, h, w, long_shift if w > h else 0, long_shift if h > w else 0)
    rec = _check_stage(engine, E, T, 1024)
    assert (rec[0] if w > h else rec[1]) == long_shift
    # the last axis length that stays in LDS and the first that does not, against each other's reference
    edge = plan.lds_budget // 8
    for L in (edge, edge + 1):
        p = engine.shift_plan(L, 4, 64)
        assert p.lds_x == (L == edge)
        E, T = _noise_pair(rng, 4, L, -37, 0)
        assert _check_stage(engine, E, T, 64)[0] == -37


# ---- part 2: batches ---------------------------------------------------------------------------------------

def _planar_out(e, n, h, w):
    arr = e.host_array((n, 2, h, w), np.float32)
    arr[...] = np.nan
    return arr


def _const(h, w, dx, dy):
    f = np.empty((h, w, 2), F32)
    f[..., 0] = dx
    f[..., 1] = dy
    return f


_WANT = {}


def _want(oracle, E, T, start):
    """The oracle's field of (E, T) from `start` (None: zero), computed once per distinct pair and start."""
    key = (hash(E.tobytes()), hash(T.tobytes()), E.shape, None if start is None else hash(start.tobytes()))
    if key not in _WANT:
        fx, fy = oracle.farneback(E, T) if start is None else farneback_with_init(oracle, E, T, start)
        _WANT[key] = np.stack([fx, fy])
    return _WANT[key]


def _run(e, oracle, subs, seen, span, thr, radius=RADIUS, inits=None, check_oracle=True):
    """subs[i](flow, init) -> the ticket of pair i; seen[i] = (E, T) as the batch sees the pair; inits[i]: a field of the
    pair's own, or None.  One batch with the option on, one with it off in which every applied pair gets its constant field;
    returns (shift records, fields, results, launch counts) of the batch with the option on."""
    n = len(subs)
    h, w = seen[0][0].shape
    inits = inits or [None] * n
    e.set_shift(radius)
    on = _planar_out(e, n, h, w)
    e.launch_counts(reset=True)
    tk = [subs[i](on[i], inits[i]) for i in range(n)]
    sh = [e.shift(t) for t in tk]
    assert sh == [e.shift(t) for t in tk]  # (the ticket is not consumed, and the answer does not change)
    res = [e.wait(t) for t in tk]
    counts = e.launch_counts(reset=True)
    e.set_shift(0)
    starts = [inits[i] if inits[i] is not None else (_const(h, w, sh[i][0], sh[i][1]) if sh[i][2] else None) for i in range(n)]
    off = _planar_out(e, n, h, w)
    tk = [subs[i](off[i], starts[i]) for i in range(n)]
    res_off = [e.wait(t) for t in tk]
    assert all(e.launch_counts()[f] == 0 for f in FAMILIES)
    for i in range(n):
        ref = S.estimate(seen[i][0], seen[i][1], radius)
        if inits[i] is not None:
            ref = ref._replace(applied=0)  # (a pair with a field of its own keeps it; the shift is still measured)
        assert sh[i] == tuple(ref), (i, sh[i], ref)
        assert np.array_equal(on[i], off[i]), "pair %d: option on against the constant field" % i
        assert res[i]["vector"] == res_off[i]["vector"], i
        if check_oracle:
            want = _want(oracle, seen[i][0], seen[i][1], starts[i])
            assert np.array_equal(on[i], want), "pair %d against the oracle" % i
            if span > 0:
                assert res[i]["vector"] == oracle.span_scan(want[0], want[1], span, thr), i
    return sh, on, res, counts


def _host_sub(e, E, T, span, thr):
    return lambda flow, init: e.submit(E, T, span, thr, flow=flow, init=init)


def _pages(n, h=H, w=W, seed=40):
    rng = np.random.default_rng(seed)
    shifts = [(0, 40), (25, 60), (-30, 7), (60, 60)]
    return [S.shifted_pair(rng, h, w, *shifts[i % 4]) for i in range(n)], [shifts[i % 4] for i in range(n)]


@pytest.mark.parametrize("hw", [(481, 641), (1080, 1920)])
def test_single_pair_schedules(twflow, oracle, hw):
    """A slots=1 engine: one pair on two streams (641 x 481: an odd size does not halve exactly) and the twin launches
    (1080p); the estimation runs on the flow chain's stream in front of the coarsest level.  (1080p: against the constant
    field only; the oracle has 641 x 481.)"""
    h, w = hw
    (pair,), (shift,) = _pages(1, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        plan = e.level_plan(w, h, 10, 1, any_fout=True, shift=True)
        assert plan.kind == ("twin" if w == 1920 else "two_stream") and plan.parts[0][plan.levels].init
        sh, _, _, cnt = _run(e, oracle, [_host_sub(e, *pair, 10, 1.0)], [pair], 10, 1.0, check_oracle=w < 1000)
        assert sh[0][:3] == shift + (1,)
        assert [cnt[f] for f in FAMILIES] == [1, 1, 2, 1] and cnt["tw_flow_area_init"] == 0


def test_three_pair_batch_on_the_tile_path(twflow, oracle):
    pairs, shifts = _pages(3)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        plan = e.level_plan(W, H, 10, 3, any_fout=True, shift=True)
        row = plan.parts[0][plan.levels]
        assert plan.kind == "batch" and row.init and not row.flow_iter and row.launches == 1
        out = _planar_out(e, 3, H, W)
        e.launch_counts(reset=True)
        for t in [e.submit(*pairs[i], 10, 1.0, flow=out[i]) for i in range(3)]:
            e.wait(t)
        plain = e.launch_counts(reset=True)
        sh, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0)
        assert [s[:3] for s in sh] == [s + (1,) for s in shifts]
        assert [cnt[f] for f in FAMILIES] == [1, 1, 2, 1] and cnt["tw_flow_area_init"] == 0
        assert cnt.last_z["tw_shift_profiles"] == 6 and cnt.last_z["tw_flow_shift_init"] == 3
        # the coarsest level's tw_update_matrices reads the start (the launch count is the plain batch's)
        assert cnt["tw_update_matrices"] == plain["tw_update_matrices"] and cnt["tw_flow_iter_zero"] == 0


def test_coarsest_level_on_tw_flow_iter(twflow, oracle, monkeypatch):
    """TW_MFREE=2, TW_MFREE_MIN_W=64: the coarsest level of 640 x 480 is M-free, and a shift batch's first iteration there is
    tw_flow_iter<15, 0> reading the start instead of <15, 2>."""
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_MFREE_MIN_W", "64")
    h, w, n = 480, 640, 2
    pairs, shifts = _pages(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plan = e.level_plan(w, h, 0, n, any_fout=True, shift=True)
        row = plan.parts[0][plan.levels]
        assert row.init and row.flow_iter and e.level_runs_flow_iter(w, h, plan.levels, n)
        out = _planar_out(e, n, h, w)
        e.launch_counts(reset=True)
        for t in [e.submit(*pairs[i], 0, 5.0, flow=out[i]) for i in range(n)]:
            e.wait(t)
        plain = e.launch_counts(reset=True)
        sh, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 0, 5.0) for p in pairs], pairs, 0, 5.0)
        assert [s[:3] for s in sh] == [s + (1,) for s in shifts]
        assert plain["tw_flow_iter_zero"] == row.launches and cnt["tw_flow_iter_zero"] == 0
        assert cnt["tw_flow_iter"] == plain["tw_flow_iter"] + row.launches
        assert cnt["tw_flow_shift_init"] == row.launches


def test_two_lanes(twflow, oracle, monkeypatch):
    monkeypatch.setenv("TW_LANES", "2")
    pairs, shifts = _pages(4)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        sh, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0)
        assert [s[:3] for s in sh] == [s + (1,) for s in shifts]
        assert [cnt[f] for f in FAMILIES] == [2, 2, 4, 2]  # (each lane's half on its own stream)


def test_ramp_pieces(twflow, oracle):
    """A 64-slot engine fed host pairs from idle: every piece of the cold-start ramp estimates its own pairs behind its
    own uploads."""
    n = 64
    pairs, shifts = _pages(4)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        for t in [e.submit(*pairs[i % 4], 0, 5.0) for i in range(n)]:  # (buffers and plans exist; the engine is idle again)
            e.wait(t)
        subs = [_host_sub(e, *pairs[i % 4], 0, 5.0) for i in range(n)]
        sh, _, _, cnt = _run(e, oracle, subs, [pairs[i % 4] for i in range(n)], 0, 5.0)
        assert [s[:3] for s in sh] == [shifts[i % 4] + (1,) for i in range(n)]
        assert cnt["tw_shift_profiles"] >= 3 and cnt["tw_shift_profiles"] == cnt["tw_shift_search"] == cnt["tw_flow_shift_init"]


def test_every_kind_of_pair(twflow, oracle):
    """One device pair with a stride, one PNG pair, one reconciled pair (target 3 px wider), one pair with an ignore rectangle
    (estimated after the mask), one resident expected image: each sees the images its batch sees."""
    (pair,), (shift,) = _pages(1)
    E, T = pair
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        # device images, rows 13 bytes of 0xEE apart from the next
        stride = W + 13
        pe = np.full((H, stride), 0xEE, np.uint8)
        pt = np.full((H, stride), 0xEE, np.uint8)
        pe[:, :W] = E
        pt[:, :W] = T
        dE, dT = e.upload(pe), e.upload(pt)
        sh, *_ = _run(e, oracle, [lambda flow, init: e.submit_dev(dE, dT, W, H, stride, 10, 1.0, flow=flow, init=init)],
                      [pair], 10, 1.0)
        assert sh[0][:3] == shift + (1,)
        # PNG rows with filter type 0: the estimation runs behind the device's decode
        def rows(img):
            r = np.zeros((H, 1 + W), np.uint8)
            r[:, 1:] = img
            return twflow.PngRows(r, W, H, color_type=0, bit_depth=8)
        pa, pb = rows(E), rows(T)
        sh, *_ = _run(e, oracle, [lambda flow, init: e.submit_png(pa, pb, 10, 1.0, flow=flow, init=init)], [pair], 10, 1.0)
        assert sh[0][:3] == shift + (1,)
        # a target 3 px wider: reconciled on the device first
        rng = np.random.default_rng(77)
        P = S.page(rng, H + 200, W + 203)
        E2, T2 = P[100:100 + H, 100:100 + W].copy(), P[60:60 + H, 100:100 + W + 3].copy()  # moved by (0, 40)
        seen = (E2, e.stage_resize_u8(T2, W, H))
        sh, *_ = _run(e, oracle, [lambda flow, init: e.submit(E2, T2, 10, 1.0, flow=flow, init=init, reconcile=True)],
                      [seen], 10, 1.0)
        assert sh[0][2] == 1 and sh[0][1] == 40, sh[0]
        # an ignore rectangle over a repainted block: the mask copies the expected pixels in before the estimation
        T3 = T.copy()
        T3[100:140, 60:200] = 30
        rects = [(60, 100, 140, 40)]
        seen = (E, e.stage_mask_rects(E, T3, rects))
        assert not np.array_equal(seen[1], T3)
        sh, *_ = _run(e, oracle, [lambda flow, init: e.submit(E, T3, 10, 1.0, flow=flow, init=init, ignore=rects)],
                      [seen], 10, 1.0, check_oracle=False)  # (the ignore rule filters vectors: against the constant field)
        assert sh[0][:3] == shift + (1,)
        # a resident expected image
        img = e.image(E)
        sh, *_ = _run(e, oracle, [lambda flow, init: e.submit_image(img, T, 10, 1.0, flow=flow, init=init)], [pair], 10, 1.0)
        assert sh[0][:3] == shift + (1,)
        img.release()


@pytest.mark.parametrize("env", [dict(), dict(TW_CHUNK_TILES="1")])
def test_mixed_batch(twflow, oracle, env, monkeypatch):
    """Shifted pairs, an identical pair, an unrelated pair and a pair with its own field in one batch: every pair equals its
    own expectation, and each coarsest-level chunk has one tw_flow_area_init and one tw_flow_shift_init launch."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pairs, shifts = _pages(3)
    rng = np.random.default_rng(9)
    same = (pairs[0][0], pairs[0][0].copy())
    unrelated = (pairs[0][0], S.page(rng, H + 200, W + 200)[100:100 + H, 100:100 + W].copy())
    seen = [pairs[0], same, unrelated, pairs[1], pairs[2]]
    own = (rng.standard_normal((H, W, 2)) * 2.0).astype(F32)
    inits = [None, None, None, own, None]
    n = len(seen)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plan = e.level_plan(W, H, 10, n, any_fout=True, shift=True)
        chunks = plan.parts[0][plan.levels].launches
        assert chunks == (n if env else 1)  # (TW_CHUNK_TILES=1: one pair per launch at every level)
        sh, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in seen], seen, 10, 1.0, inits=inits)
        assert [s[:3] for s in sh] == [shifts[0] + (1,), (0, 0, 0), sh[2][:2] + (0,), shifts[1] + (0,), shifts[2] + (1,)]
        assert cnt["tw_flow_area_init"] == chunks and cnt["tw_flow_shift_init"] == chunks
        assert [cnt[f] for f in FAMILIES[:3]] == [1, 1, 2]
        # a batch of shifted pairs alone launches no tw_flow_area_init
        _, _, _, cnt = _run(e, oracle, [_host_sub(e, *p, 10, 1.0) for p in pairs], pairs, 10, 1.0)
        plan3 = e.level_plan(W, H, 10, 3, any_fout=True, shift=True)
        assert cnt["tw_flow_area_init"] == 0 and cnt["tw_flow_shift_init"] == plan3.parts[0][plan3.levels].launches == (3 if env else 1)


def test_with_the_residual(twflow, oracle):
    """A shifted page with one repainted block: once the move is explained, tw_ticket_changes is residual_ref on the oracle's
    seeded flow — and the whole page is not 'unexplained'."""
    import residual_ref as RR
    (pair,), (shift,) = _pages(1)
    E, T = pair[0], pair[1].copy()
    T[150:190, 80:220] = 30
    span, tol = 10, 16
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_residual(tol)
        e.set_shift(RADIUS)
        tk = e.submit(E, T, span, 1.0)
        sh = e.shift(tk)
        got, cnt = e.changes(tk)
        res = e.wait(tk)
        assert sh == tuple(S.estimate(E, T, RADIUS)) and sh[:3] == shift + (1,)
        want = _want(oracle, E, T, _const(H, W, *shift))
        _, rec = RR.residual_ref(E, T, (want[0], want[1]), span, tol)
        assert got == rec and cnt == len(rec)
        assert res["vector"] == oracle.span_scan(want[0], want[1], span, 1.0)
        # what the start is for: seeded, only the block and the 40 rows that left the image stay unexplained, under a third of
        # the page; from a zero start the flow explains next to nothing of a page moved by 40 px
        zero = _want(oracle, E, T, None)
        _, rec0 = RR.residual_ref(E, T, (zero[0], zero[1]), span, tol)
        assert sum(r[3] for r in rec) * 2 < sum(r[3] for r in rec0)


def test_option_off_launches_copies_and_holds_what_it_did(twflow):
    pairs, _ = _pages(3)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        def run():
            e.launch_counts(reset=True)
            tk = [e.submit(*p, 10, 1.0) for p in pairs]
            with pytest.raises(twflow.TwError) as ei:
                e.shift(tk[1])
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
            res = [e.wait(t) for t in tk]  # (the tickets are still waitable)
            return e.launch_counts(reset=True), res, e.memory()
        c0, r0, m0 = run()
        assert all(c0[f] == 0 for f in FAMILIES)
        e.set_shift(64)
        e.set_shift(0)
        c1, r1, m1 = run()
        assert c1 == c0 and m1 == m0 and [r["vector"] for r in r1] == [r["vector"] for r in r0]
        # with the option on the feature's buffers appear once, and going back off launches what it did before
        e.set_shift(64)
        for t in [e.submit(*p, 10, 1.0) for p in pairs]:
            e.wait(t)
        m2 = e.memory()
        assert m2["device_bytes"] > m0["device_bytes"] and m2["pinned_host_bytes"] > m0["pinned_host_bytes"]
        for t in [e.submit(*p, 10, 1.0) for p in pairs]:
            e.wait(t)
        assert e.memory() == m2
        e.set_shift(0)
        c3, r3, _ = run()
        assert c3 == c0 and [r["vector"] for r in r3] == [r["vector"] for r in r0]


def test_refusals(twflow):
    import ctypes as C
    (pair,), _ = _pages(1)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_shift(7)
        for v in (-1, 1025):
            with pytest.raises(twflow.TwError) as ei:
                e.set_shift(v)
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        tk = e.submit(*pair, 10, 1.0)
        L = twflow.lib()
        rec = twflow.Shift()
        assert L.tw_ticket_shift(e._h, tk[0], None) == twflow.TW_E_BAD_PARAMETER          # a null out
        assert L.tw_ticket_shift(e._h, tk[0] + 1000, C.byref(rec)) == twflow.TW_E_BAD_PARAMETER  # an unknown ticket
        assert e.shift(tk) == tuple(S.estimate(*pair, 7))  # (the refused values left the radius at 7)
        e.wait(tk)
        assert L.tw_ticket_shift(e._h, tk[0], C.byref(rec)) == twflow.TW_E_BAD_PARAMETER  # a waited ticket
