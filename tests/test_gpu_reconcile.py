"""Pairs of unequal size through the batch path (tw_submit_u8_sized / tw_submit_png8_sized / tw_submit_dev_sized):
OpticalFlow::calculate's <= 5 px reconcile (src/opticalflow.cpp:52-68) on the device.

Every expected result is oracle.span_scan(*oracle.farneback(a, oracle.reconcile_target(b, w, h))) and that dense field;
every comparison is exact (np.array_equal, list equality): the feature has no tolerance.  The kernel alone is
tests/test_gpu_resize_u8.py.
"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_init_abi import farneback_with_init  # noqa: E402
from test_gpu_png import gray15, png_filter  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
ADDON = os.path.join(HOST, "build", "Release", "tidalwave.node")

W, H, SPAN, THR = 180, 117, 10, 1.0
OFFSETS = [(0, 0), (3, 0), (0, -5), (-5, 5), (5, 5), (-1, -1), (0, 0), (2, -4)]  # (dx, dy) of the target's size


def _target(oracle, b, dx, dy):
    """The pair's second image at another size: what a page that grew or shrank by a few pixels looks like."""
    h, w = b.shape
    return b if (dx, dy) == (0, 0) else oracle.resize_u8_linear(b, w + dx, h + dy)


@pytest.fixture(scope="module")
def mixed(oracle):
    """The mixed batch and its expected results, computed once: [(a, target, want field [2, H, W], want vectors)]."""
    import synth
    out = []
    for i, (dx, dy) in enumerate(OFFSETS):
        a, b = synth.make_pair(i, H, W)
        t = _target(oracle, b, dx, dy)
        fx, fy = oracle.farneback(a, oracle.reconcile_target(t, W, H))
        out.append((a, t, np.stack([fx, fy]), oracle.span_scan(fx, fy, SPAN, THR)))
    return out


def _planar_out(e, n, h, w):
    arr = e.host_array((n, 2, h, w), np.float32)
    arr[...] = np.nan
    return arr


def _pinned(e, img):
    p = e.host_array(img.shape)
    p[...] = img
    return p


def _check(e, tickets, out, mixed):
    for i, t in enumerate(tickets):
        res = e.wait(t)
        assert (res["width"], res["height"]) == (W, H)
        assert res["vector"] == mixed[i][3], "pair %d (offset %s)" % (i, OFFSETS[i])
        assert np.array_equal(out[i], mixed[i][2]), "pair %d (offset %s): field" % (i, OFFSETS[i])


def _plain_results(twflow, mixed, idx):
    """The equal pairs through the plain call on an engine of their own."""
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out = _planar_out(e, len(idx), H, W)
        tk = [e.submit(mixed[i][0], mixed[i][1], SPAN, THR, flow=out[k]) for k, i in enumerate(idx)]
        return [(e.wait(t)["vector"], out[k].copy()) for k, t in enumerate(tk)]


def test_mixed_batch_of_gray_host_pairs(twflow, mixed):
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        out = _planar_out(e, 8, H, W)
        tickets = []
        for i, (a, t, _, _) in enumerate(mixed):
            if i % 2:  # page-locked: DMA-ed in place
                a, t = _pinned(e, a), _pinned(e, t)
            tickets.append(e.submit(a, t, SPAN, THR, flow=out[i], reconcile=True))
        assert [t[0] for t in tickets] == list(range(1, 9))  # one batch, tickets in order
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 6, cnt  # one per reconciled pair, launched at submit time
        _check(e, tickets, out, mixed)
        plain = _plain_results(twflow, mixed, [0, 6])
        for k, i in enumerate((0, 6)):
            assert plain[k][0] == mixed[i][3] and np.array_equal(plain[k][1], out[i])


def _png_images(mixed):
    """The mixed batch as filtered PNG rows: channels 1-4 mixed, every filter type on the target's rows, one expected
    image handed over as gray (ch 0).  Returns [(expect, cha, target, chb, tw, th)] whose gray conversions are the
    mixed batch's own images."""
    def colour(g, ch, seed):
        # r == g == b pixels take libpng's shortcut: the gray conversion of these images is g itself
        if ch == 1:
            return g[..., None]
        alpha = np.random.default_rng(seed).integers(0, 256, g.shape, dtype=np.uint8)
        if ch == 2:
            return np.stack([g, alpha], -1)
        return np.stack([g, g, g] + ([alpha] if ch == 4 else []), -1)
    out = []
    for i, (a, t, _, _) in enumerate(mixed):
        # (the first pair has the batch's largest rows: a batch's d_filt slots are sized by its first filtered image, and
        # a larger one would start a new batch — four channels only on targets no larger than the pair's size)
        cha, chb = (4, 1, 2, 3, 3, 2, 1, 3)[i], (4, 3, 4, 2, 1, 4, 3, 4)[i]
        ra, rt = colour(a, cha, i), colour(t, chb, 100 + i)
        assert np.array_equal(gray15(ra), a) and np.array_equal(gray15(rt), t)
        rows_a = png_filter(ra, np.random.default_rng(i).integers(0, 5, a.shape[0]))
        rows_t = png_filter(rt, np.arange(t.shape[0]) % 5)
        if i == 3:  # a reconciled pair whose expected image the host decoded
            rows_a, cha = a, 0
        out.append((rows_a, cha, rows_t, chb, t.shape[1], t.shape[0]))
    return out


def test_mixed_batch_of_filtered_png_rows(twflow, mixed):
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        out = _planar_out(e, 8, H, W)
        tickets = []
        for i, (ra, cha, rt, chb, tw_, th_) in enumerate(_png_images(mixed)):
            if i % 2:
                ra, rt = _pinned(e, ra), _pinned(e, rt)
            tickets.append(e.submit_png8(ra, cha, rt, chb, W, H, SPAN, THR, flow=out[i], target_size=(tw_, th_)))
        assert [t[0] for t in tickets] == list(range(1, 9))
        _check(e, tickets, out, mixed)
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 1 and cnt.last_z["tw_resize_u8"] == 8, cnt  # one launch for the batch's targets
        assert cnt["tw_png_unfilter"] == 1 + 6, cnt  # the batch-wide launch and one per reconciled target
        assert cnt["tw_pair_same"] == 1, cnt  # (one batch)
        plain = _plain_results(twflow, mixed, [0, 6])
        for k, i in enumerate((0, 6)):
            assert plain[k][0] == mixed[i][3] and np.array_equal(plain[k][1], out[i])


def test_png_targets_of_one_size_share_a_launch(twflow, oracle):
    """Every target 3 px narrower (a page that shrank between two runs): one more tw_png_unfilter launch for all of them."""
    import synth
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        tickets, want = [], []
        for i in range(4):
            a, b = synth.make_pair(30 + i, H, W)
            t = np.ascontiguousarray(b[:, :W - 3])
            fx, fy = oracle.farneback(a, oracle.reconcile_target(t, W, H))
            want.append(oracle.span_scan(fx, fy, SPAN, THR))
            ra = png_filter(np.stack([a, a, a], -1), np.arange(H) % 5)
            rt = png_filter(np.stack([t, t, t], -1), (np.arange(H) + i) % 5)
            tickets.append(e.submit_png8(ra, 3, rt, 3, W, H, SPAN, THR, target_size=(W - 3, H)))
        assert [e.wait(t)["vector"] for t in tickets] == want
        cnt = e.launch_counts()
        assert cnt["tw_png_unfilter"] == 2 and cnt.last_z["tw_png_unfilter"] == 1, cnt
        assert cnt["tw_resize_u8"] == 1 and cnt.last_z["tw_resize_u8"] == 4, cnt


def test_mixed_batch_from_device_memory(twflow, mixed):
    """Row strides that differ from the widths (and the target's from the expected image's); the caller's target
    buffers are not written."""
    stride = W + 12
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        out = _planar_out(e, 8, H, W)
        tickets, kept = [], []
        for i, (a, t, _, _) in enumerate(mixed):
            pa = np.full((H, stride), 0xA5, np.uint8)
            pa[:, :W] = a
            tstride = t.shape[1] + 7 + i  # (pair 6: an equal-size target at another row pitch)
            if i == 0:
                tstride = stride
            pt = np.full((t.shape[0], tstride), 0x5A, np.uint8)
            pt[:, :t.shape[1]] = t
            da, dt = e.upload(pa), e.upload(pt)
            kept.append((dt, pt))
            tickets.append(e.submit_dev(da, dt, W, H, stride, SPAN, THR, flow=out[i],
                                        target_size=(t.shape[1], t.shape[0]), target_stride=tstride))
        assert [t[0] for t in tickets] == list(range(1, 9))
        _check(e, tickets, out, mixed)
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 1 and cnt.last_z["tw_resize_u8"] == 8, cnt  # one launch, grid z = the batch
        for dt, pt in kept:
            assert np.array_equal(e.dev_download(dt, pt.size), pt.ravel())


def _equal_batch(twflow, kind, sized):
    """Four equal-size pairs through the _sized calls (sized) or the calls they must equal; (results, counts, memory)."""
    import synth
    pairs = [synth.make_pair(20 + i, H, W) for i in range(4)]
    L = twflow.lib()
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        tickets = []
        for a, b in pairs:
            tk = C.c_int64()
            pa, pb = twflow._u8(a), twflow._u8(b)
            if kind == "u8":
                if sized:
                    e._check(L.tw_submit_u8_sized(e._h, pa, W, H, W, pb, W, H, W, SPAN, THR, None, None, C.byref(tk)))
                    tickets.append((tk.value, W, H, SPAN, THR))
                else:
                    tickets.append(e.submit(a, b, SPAN, THR))
            elif kind == "png8":
                ra = png_filter(a[..., None], np.arange(H) % 5)
                rb = png_filter(np.stack([b, b, b], -1), np.arange(H) % 5)
                if sized:
                    tickets.append(e.submit_png8(ra, 1, rb, 3, W, H, SPAN, THR, target_size=(W, H)))
                else:
                    tickets.append(e.submit_png8(ra, 1, rb, 3, W, H, SPAN, THR))
            else:
                da, db = e.upload(a), e.upload(b)
                if sized:
                    tickets.append(e.submit_dev(da, db, W, H, W, SPAN, THR, target_size=(W, H), target_stride=W))
                else:
                    tickets.append(e.submit_dev(da, db, W, H, W, SPAN, THR))
        res = [e.wait(t)["vector"] for t in tickets]
        return res, dict(e.launch_counts()), e.memory()


@pytest.mark.parametrize("kind", ["u8", "png8", "dev"])
def test_equal_sizes_are_the_plain_call(twflow, kind):
    """Launch for launch and byte for byte of the engine's own memory: no tw_resize_u8, no staging."""
    got, cnt, mem = _equal_batch(twflow, kind, True)
    want, cnt0, mem0 = _equal_batch(twflow, kind, False)
    assert got == want
    assert cnt == cnt0, {k: (cnt[k], cnt0[k]) for k in cnt if cnt[k] != cnt0[k]}
    assert cnt["tw_resize_u8"] == 0
    assert mem == mem0


def test_refusals_leave_the_open_batch_as_it_was(twflow, oracle, mixed):
    L = twflow.lib()
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        out = _planar_out(e, 4, H, W)
        tickets = [e.submit(mixed[i][0], mixed[i][1], SPAN, THR, flow=out[i], reconcile=True) for i in range(2)]
        a = mixed[0][0]
        for dx, dy in ((6, 0), (0, -6), (5, 6)):
            t = np.zeros((H + dy, W + dx), np.uint8)
            with pytest.raises(twflow.TwError) as ei:
                e.submit(a, t, SPAN, THR, reconcile=True)
            assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
            with pytest.raises(twflow.TwError) as ei:
                e.submit_png8(a, 0, png_filter(t[..., None], np.zeros(H + dy, int)), 1, W, H, SPAN, THR,
                              target_size=(W + dx, H + dy))
            assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
            with pytest.raises(twflow.TwError) as ei:
                e.submit_dev(e.upload(a), e.upload(t), W, H, W, SPAN, THR, target_size=(W + dx, H + dy), target_stride=W + dx)
            assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
        # a target stride below the target's width
        t = np.zeros((H, W + 3), np.uint8)
        tk = C.c_int64()
        rc = L.tw_submit_u8_sized(e._h, twflow._u8(a), W, H, W, twflow._u8(t), W + 3, H, W + 2, SPAN, THR, None, None, C.byref(tk))
        assert rc == twflow.TW_E_BAD_PARAMETER
        # a filter type above 4 on a row that only the TARGET's row length finds (row 50 of 1 + (W + 3) bytes)
        rows = png_filter(np.zeros((H, W + 3, 1), np.uint8), np.zeros(H, int))
        rows[50, 0] = 5
        assert rows.ravel()[50 * (1 + W)] == 0  # (the pair's row length would have read a sample there)
        with pytest.raises(twflow.TwError) as ei:
            e.submit_png8(a, 0, rows, 1, W, H, SPAN, THR, target_size=(W + 3, H))
        assert ei.value.code == twflow.TW_E_BAD_IMAGE_FORMAT
        # the open batch is as it was: the next tickets are the next ones, and the batch completes
        tickets += [e.submit(mixed[i][0], mixed[i][1], SPAN, THR, flow=out[i], reconcile=True) for i in range(2, 4)]
        assert [t[0] for t in tickets] == [1, 2, 3, 4]
        for i, t in enumerate(tickets):
            res = e.wait(t)
            assert res["vector"] == mixed[i][3] and np.array_equal(out[i], mixed[i][2])


# 320 x 240 is below the engine's single-pair threshold (TW_LATENCY_MIN_PX, 100 000 px): it is lowered there, so that the
# single-pair schedules are what runs; 640 x 480 takes them by itself
SINGLE = [(240, 320, "0"), (480, 640, None)]


@pytest.mark.parametrize("h,w,min_px", SINGLE, ids=["320x240", "640x480"])
@pytest.mark.parametrize("lat_fused", [None, "0"])
def test_single_pair_engine(twflow, oracle, monkeypatch, lat_fused, h, w, min_px):
    """slots = 1, offsets (+4, -3): the twin-launch schedule (the default where it applies: 640 x 480) and the two-stream
    schedule (TW_LAT_FUSED=0, and 320 x 240 under both settings) — proven by the launch counters: tw_twin launches under
    the first only, and no tw_pair_same (the batch schedule's) under either."""
    import synth
    if lat_fused is not None:
        monkeypatch.setenv("TW_LAT_FUSED", lat_fused)
    if min_px is not None:
        monkeypatch.setenv("TW_LATENCY_MIN_PX", min_px)
    a, b = synth.make_pair(5, h, w)
    t = _target(oracle, b, 4, -3)
    fx, fy = oracle.farneback(a, oracle.reconcile_target(t, w, h))
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        out = _planar_out(e, 1, h, w)
        for k in range(2):  # pageable, then page-locked
            out[...] = np.nan
            res = e.wait(e.submit(a if k == 0 else _pinned(e, a), t if k == 0 else _pinned(e, t), SPAN, THR,
                                  flow=out[0], reconcile=True))
            assert res["vector"] == oracle.span_scan(fx, fy, SPAN, THR)
            assert np.array_equal(out[0], np.stack([fx, fy]))
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 2
        assert cnt["tw_pair_same"] == 0, cnt  # a single-pair schedule ran, not the batch schedule with one pair
        # (320 x 240 does not meet the twin schedule's conditions — no tw_twin launch there on an MI355X — so the
        # two-stream schedule runs under both settings)
        assert (cnt["tw_twin"] > 0) == (lat_fused is None and (h, w) == (480, 640)), cnt


def test_single_pair_never_takes_the_captured_graph(twflow, oracle, monkeypatch):
    """TW_LAT_GRAPH=1 on a slots = 1 engine at 640 x 480: an equal-size pair captures and replays a graph, a reconciled
    pair before and after it never does (and never replays the equal pair's graph: its result is its own)."""
    import synth
    monkeypatch.setenv("TW_LAT_GRAPH", "1")
    h, w = 480, 640
    a, b = synth.make_pair(5, h, w)
    t = _target(oracle, b, 4, -3)
    fx, fy = oracle.farneback(a, oracle.reconcile_target(t, w, h))
    ex, ey = oracle.farneback(a, b)
    assert oracle.span_scan(fx, fy, SPAN, THR) != oracle.span_scan(ex, ey, SPAN, THR)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        assert e.wait(e.submit(a, t, SPAN, THR, reconcile=True))["vector"] == oracle.span_scan(fx, fy, SPAN, THR)
        assert e.memory()["graphs"] == 0
        assert e.wait(e.submit(a, b, SPAN, THR))["vector"] == oracle.span_scan(ex, ey, SPAN, THR)
        assert e.memory()["graphs"] == 1  # (the switch is on and the schedule is capturable: the guard is what held above)
        assert e.wait(e.submit(a, t, SPAN, THR, reconcile=True))["vector"] == oracle.span_scan(fx, fy, SPAN, THR)
        assert e.wait(e.submit(a, b, SPAN, THR))["vector"] == oracle.span_scan(ex, ey, SPAN, THR)
        assert e.memory()["graphs"] == 1
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 2 and cnt["tw_pair_same"] == 0, cnt


def test_cold_start_ramp(twflow, oracle):
    """One full batch of a 64-slot engine from page-locked memory into an idle stream: it goes out in three pieces, each
    behind its own mark on the copy stream — reconciled pairs at the pieces' edges must be finished behind those marks."""
    import synth
    h, w, n = 64, 96, 64
    recon = {3: (2, -1), 15: (-5, 5), 16: (5, -5), 31: (1, 0), 32: (0, 3), 63: (-3, -4)}
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        imgs, want = [], []
        for i in range(n):
            a, b = synth.make_pair(40 + i, h, w)
            t = _target(oracle, b, *recon.get(i, (0, 0)))
            fx, fy = oracle.farneback(a, oracle.reconcile_target(t, w, h))
            want.append((np.stack([fx, fy]), oracle.span_scan(fx, fy, SPAN, THR)))
            imgs.append((_pinned(e, a), _pinned(e, t)))
        out = _planar_out(e, n, h, w)
        e.launch_counts(reset=True)
        tickets = [e.submit(a, t, SPAN, THR, flow=out[i], reconcile=True) for i, (a, t) in enumerate(imgs)]
        for i, tk in enumerate(tickets):
            res = e.wait(tk)
            assert res["vector"] == want[i][1], i
            assert np.array_equal(out[i], want[i][0]), i
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == len(recon)
        assert cnt["tw_pair_same"] == 3, cnt  # the ramp's three pieces ran


def test_with_init_and_flow_together(twflow, oracle):
    import synth
    h, w = 480, 640
    a, b = synth.make_pair(3, h, w)
    t = _target(oracle, b, -4, 5)
    f0 = (np.random.default_rng(9).standard_normal((h, w, 2)) * 2.0).astype(F32)
    bt = oracle.reconcile_target(t, w, h)
    fx, fy = farneback_with_init(oracle, a, bt, f0)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out = _planar_out(e, 1, h, w)
        res = e.wait(e.submit(a, t, SPAN, THR, flow=out[0], init=f0, reconcile=True))
        assert np.array_equal(out[0], np.stack([fx, fy]))
        assert res["vector"] == oracle.span_scan(fx, fy, SPAN, THR)
        cnt = e.launch_counts()
        assert cnt["tw_resize_u8"] == 1 and cnt["tw_flow_area_init"] >= 1


NODE_JS = """
var T=require('./index'); var t=new T.TidalWave({span:6, threshold:0.25}); var res=[]; var n=0; var pairs=process.argv.slice(1);
function done(){ if(++n===pairs.length/2) t.dispose(); }
t.on('data',function(d){res.push({t:d.target_image,h:d.height,w:d.width,s:d.status,v:d.vector}); done();});
t.on('error',function(e){res.push({e:e.reason}); done();});
t.on('finish',function(){console.log(JSON.stringify(res));});
for (var i=0;i<pairs.length;i+=2) t.calc(pairs[i],pairs[i+1]);
"""


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the built addon is not available")
def test_host_layer_through_node_device_and_host_reconcile_agree(oracle, tmp_path):
    """120 x 90 against 117 x 94, as RGBA PNG files (filtered rows all the way to the device) and as PGM files (gray
    pixels): TW_DEVICE_RECONCILE=1 and =0 answer the same JSON, the oracle's vectors."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:90, 0:120]
    a = ((np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128 + rng.integers(-6, 7, (90, 120))).clip(0, 255).astype(np.uint8)
    b = oracle.resize_u8_linear(a, 117, 94)
    b[20:40, 30:70] = np.roll(b[20:40, 30:70], 3, axis=1)
    fx, fy = oracle.farneback(a, oracle.reconcile_target(b, 120, 90))
    want = oracle.span_scan(fx, fy, 6, 0.25)
    assert want
    files = []
    for name, img in (("a", a), ("b", b)):
        Image.fromarray(np.dstack([img] * 3 + [np.full_like(img, 255)])).save(tmp_path / (name + ".png"))
        with open(tmp_path / (name + ".pgm"), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    for ext in (".png", ".pgm"):
        files += [str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))]
    answers = []
    for sw in ("1", "0"):
        r = subprocess.run(["node", "-e", NODE_JS] + files, cwd=HOST, capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, TW_DEVICE_RECONCILE=sw))
        assert r.returncode == 0, r.stderr[-400:]
        res = sorted(json.loads(r.stdout.strip().splitlines()[-1]), key=lambda d: d.get("t", ""))
        assert len(res) == 2 and all("t" in d for d in res), res
        for d in res:
            assert (d["w"], d["h"], d["s"]) == (120, 90, "SUSPICIOUS")
            assert [(v["x"], v["y"], v["dx"], v["dy"]) for v in d["v"]] == want
        answers.append(res)
    assert answers[0] == answers[1]
