"""Dense flow fields from batched submissions (tw_submit_*_flow) on the GPU.

Every field is compared bit for bit (np.array_equal on float32) with the CPU oracle or with tw_flow_u8 of the same pair;
every vector list with the same batch submitted without destinations.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


def _pairs(n_distinct, h, w):
    import synth
    return [synth.make_pair(i, h, w) for i in range(n_distinct)]


def _oracle_fields(oracle, pairs, params=None):
    out = []
    for a, b in pairs:
        fx, fy = oracle.farneback(a, b, params) if params is not None else oracle.farneback(a, b)
        out.append(np.stack([fx, fy]))  # planar (2, h, w)
    return out


def _planar(f, layout):
    return f if layout == "planar" else np.moveaxis(f, 2, 0)


def _dest(e, n, h, w, layout, pad=0):
    """Page-locked destinations with `pad` padding floats per row, filled with the sentinel: (whole array, views)."""
    if layout == "planar":
        arr = e.host_array((n, 2, h, w + pad), np.float32)
        arr[...] = SENTINEL
        return arr, [arr[i][:, :, :w] for i in range(n)]
    arr = e.host_array((n, h, w + pad, 2), np.float32)
    arr[...] = SENTINEL
    return arr, [arr[i][:, :w, :] for i in range(n)]


def _padding_untouched(arr, w, layout):
    pad = arr[:, :, :, w:] if layout == "planar" else arr[:, :, w:, :]
    return bool(np.all(pad == SENTINEL))


def _run(e, pairs, n, span, thr, dests=None):
    tk = [e.submit(*pairs[i % len(pairs)], span, thr, flow=None if dests is None else dests[i]) for i in range(n)]
    return [e.wait(t) for t in tk]


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_host_batch_640x480_both_layouts(twflow, oracle, layout):
    h, w, n = 480, 640, 24
    pairs = _pairs(4, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain = _run(e, pairs, n, 10, 0.0)
        arr, views = _dest(e, n, h, w, layout, pad=12)
        e.launch_counts(reset=True)
        got = _run(e, pairs, n, 10, 0.0, views)
        assert e.launch_counts()["tw_flow_export"] >= 1
        for i in range(n):
            assert np.array_equal(_planar(views[i], layout), want[i % 4]), "pair %d" % i
            assert got[i]["vector"] == plain[i]["vector"] and len(got[i]["vector"]) > 1000
        assert _padding_untouched(arr, w, layout)


def test_headline_shape_1080p(twflow, oracle):
    """16 pairs of 1080p in one host batch (span 10, threshold 5) through the batched tw_flow_iter launch shape: every
    field equals tw_flow_u8 of the same pair (a single pair: other kernels), two of them the oracle's."""
    h, w, n = 1080, 1920, 16
    pairs = _pairs(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_runs_flow_iter(w, h, 0, n)
        plain = _run(e, pairs, n, 10, 5.0)
        arr, views = _dest(e, n, h, w, "interleaved")
        e.launch_counts(reset=True)
        got = _run(e, pairs, n, 10, 5.0, views)
        cnt = e.launch_counts()
        chunk0 = e.level_chunk(w, h, 0)
        launches0 = -(-n // chunk0)
        assert cnt.last_z["tw_flow_iter"] == n, cnt.last_z
        assert cnt["tw_flow_export"] == launches0 and cnt.last_z["tw_flow_export"] == n // launches0, cnt
        assert [g["vector"] for g in got] == [p["vector"] for p in plain]
        for i in range(n):
            gx, gy, _ = e.calculate_internal(*pairs[i])
            assert np.array_equal(views[i][:, :, 0], gx) and np.array_equal(views[i][:, :, 1], gy), "pair %d" % i
        for i, f in zip((0, 1), _oracle_fields(oracle, pairs[:2])):
            assert np.array_equal(_planar(views[i], "interleaved"), f), "pair %d vs oracle" % i


@pytest.mark.parametrize("env", [dict(TW_CHUNK_TILES="100"), dict(TW_CHUNK_TILES="100", TW_LANES="2")])
def test_level0_in_several_launches(twflow, oracle, env, monkeypatch):
    """Level 0 in one launch per pair: each chunk's flow is exported before the next chunk overwrites the buffer."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w, n = 480, 640, 8
    pairs = _pairs(4, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_chunk(w, h, 0) * 3 <= n
        arr, views = _dest(e, n, h, w, "planar", pad=3)
        e.launch_counts(reset=True)
        _run(e, pairs, n, 10, 0.0, views)
        assert e.launch_counts()["tw_flow_export"] >= 3
        for i in range(n):
            assert np.array_equal(views[i], want[i % 4]), "pair %d" % i
        assert _padding_untouched(arr, w, "planar")


def test_mixed_batch(twflow, oracle):
    h, w, n = 480, 640, 8
    pairs = _pairs(4, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain = _run(e, pairs, n, 10, 0.0)
        arr, views = _dest(e, n, h, w, "interleaved")
        got = _run(e, pairs, n, 10, 0.0, [views[i] if i % 3 == 0 else None for i in range(n)])
        assert [g["vector"] for g in got] == [p["vector"] for p in plain]
        for i in range(n):
            if i % 3 == 0:
                assert np.array_equal(_planar(views[i], "interleaved"), want[i % 4]), "pair %d" % i
            else:
                assert np.all(arr[i] == SENTINEL), "pair %d without a destination was written" % i


def test_device_destinations_and_inputs(twflow, oracle):
    import ctypes as C
    h, w, n = 480, 640, 6
    pairs = _pairs(3, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        L = e._L
        # raw device memory (tw_dev_alloc) with a padded pitch, read back with tw_dev_download
        pitch = w * 4 + 64
        nbytes = pitch * 2 * h
        d = C.c_void_p()
        assert L.tw_dev_alloc(e._h, nbytes, C.byref(d)) == twflow.TW_OK
        try:
            sentinel = np.full(nbytes // 4, SENTINEL, np.float32)
            assert L.tw_dev_upload(e._h, d, sentinel.ctypes.data_as(C.c_void_p), nbytes) == twflow.TW_OK
            t = e.submit(*pairs[1], 10, 0.0, flow=(d.value, pitch, twflow.FLOW_PLANAR))
            e.wait(t)
            got = e.dev_download(d, nbytes).view(np.float32).reshape(2, h, pitch // 4)
            assert np.array_equal(got[:, :, :w], want[1])
            assert np.all(got[:, :, w:] == SENTINEL)
            # a field that would not fit the allocation, a bad pitch or layout: refused
            for bad in ((d.value, pitch, 7), (d.value, w * 4 - 4, twflow.FLOW_PLANAR), (d.value, w * 4 + 2, twflow.FLOW_PLANAR),
                        (d.value + 8192, pitch, twflow.FLOW_PLANAR), (0, pitch, twflow.FLOW_PLANAR)):
                with pytest.raises(twflow.TwError) as ei:
                    e.submit(*pairs[0], 10, 0.0, flow=bad)
                assert ei.value.code == twflow.TW_E_BAD_PARAMETER, bad
        finally:
            L.tw_dev_free(e._h, d)
        # pinned host destinations through flow_batch (numpy)
        out, res = e.flow_batch([p[0] for p in pairs] * 2, [p[1] for p in pairs] * 2, layout="planar")
        assert out.shape == (n, 2, h, w) and len(res) == n
        for i in range(n):
            assert np.array_equal(out[i], want[i % 3]), "numpy pair %d" % i
        # a pageable destination is refused, and the engine still works afterwards
        with pytest.raises(twflow.TwError) as ei:
            e.submit(*pairs[0], 10, 0.0, flow=np.empty((h, w, 2), np.float32))
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        assert e.diff(*pairs[0], 10, 0.0)["vector"] == oracle.span_scan(want[0][0], want[0][1], 10, 0.0)


_TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # before the library: torch's HIP runtime must be the one the process loads first (as in bench.py)
torch.cuda.init()
sys.path[:0] = sys.argv[1:]
import oracle, synth, twflow
h, w = 480, 640
pairs = [synth.make_pair(i, h, w) for i in range(3)]
want = [np.stack(oracle.farneback(a, b)) for a, b in pairs]
dev = torch.device("cuda", 0)
ta = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
tb = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
with twflow.Engine(0, twflow.default_params(), slots=4) as e:
    for layout in ("interleaved", "planar"):
        out, res = e.flow_batch(ta, tb, layout=layout, span=10, threshold=0.0)
        assert out.device == dev and out.dtype == torch.float32
        host = out.cpu().numpy()
        for i in range(3):
            got = host[i] if layout == "planar" else np.moveaxis(host[i], 2, 0)
            assert np.array_equal(got, want[i]), (layout, i)
            assert res[i]["vector"] == oracle.span_scan(want[i][0], want[i][1], 10, 0.0)
print("torch ok")
"""


def test_torch_tensors_in_and_out():
    """Engine.flow_batch on torch uint8 tensors in HBM: tw_submit_dev_flow into a float32 tensor on the device.  In a
    child process, so that torch is imported before the library as a torch program does it."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, os.path.join(root, "tidal-wave_amd"), os.path.join(root, "oracle")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_cold_start_ramp_pieces(twflow, oracle):
    """64 host pairs into an idle 64-slot engine go out in three pieces (16, 16, 32): each piece's level-0 launch is
    exported before the next piece reuses the level-0 buffer."""
    assert "TW_RAMP" not in os.environ
    h, w, n = 480, 640, 64
    pairs = _pairs(4, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        levels = e.num_levels(w, h)
        arr, views = _dest(e, n, h, w, "interleaved")
        e.launch_counts(reset=True)
        _run(e, pairs, n, 10, 0.0, views)
        cnt = e.launch_counts()
        assert cnt["tw_polyexp"] == 3 * (levels + 1) and cnt.last_z["tw_polyexp"] == 2 * 32, (cnt, cnt.last_z)
        assert cnt["tw_flow_export"] == 3 and cnt.last_z["tw_flow_export"] == 32, (cnt, cnt.last_z)
        for i in range(n):
            assert np.array_equal(_planar(views[i], "interleaved"), want[i % 4]), "pair %d" % i


def test_scan_fused_option_takes_the_full_path(twflow, oracle):
    h, w, n = 480, 640, 24
    pairs = _pairs(4, h, w)
    want = _oracle_fields(oracle, pairs)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain = _run(e, pairs, n, 10, 0.0)
        e.set_option(twflow.OPT_SCAN_FUSED_FINAL, 1)
        e.launch_counts(reset=True)
        fused = _run(e, pairs, n, 10, 0.0)
        assert e.launch_counts()["tw_blur_grid"] >= 1  # (the option is really on)
        arr, views = _dest(e, n, h, w, "planar")
        e.launch_counts(reset=True)
        got = _run(e, pairs, n, 10, 0.0, views)
        cnt = e.launch_counts()
        assert cnt["tw_blur_grid"] == 0 and cnt["tw_flow_export"] >= 1, cnt
        assert [g["vector"] for g in got] == [p["vector"] for p in plain] == [f["vector"] for f in fused]
        for i in range(n):
            assert np.array_equal(views[i], want[i % 4]), "pair %d" % i


@pytest.mark.parametrize("hw,env", [((480, 640), {}), ((1080, 1920), {}), ((480, 640), dict(TW_LAT_GRAPH="1"))])
def test_single_pair_schedule(twflow, oracle, hw, env, monkeypatch):
    """A slots=1 engine: the single-pair latency schedule (twin launches at 1080p); with TW_LAT_GRAPH=1 a batch with a
    destination is not captured into a graph."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w = hw
    pairs = _pairs(1, h, w)
    want = _oracle_fields(oracle, pairs)[0]
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        plain = e.diff(*pairs[0], 10, 0.0)
        graphs = e._L.tw_debug_graphs(e._h)
        arr, views = _dest(e, 1, h, w, "interleaved", pad=1)
        e.launch_counts(reset=True)
        got = e.wait(e.submit(*pairs[0], 10, 0.0, flow=views[0]))
        assert e.launch_counts()["tw_flow_export"] == 1
        assert e._L.tw_debug_graphs(e._h) == graphs  # (no schedule with a destination in it was captured)
        assert got["vector"] == plain["vector"]
        assert np.array_equal(_planar(views[0], "interleaved"), want)
        assert _padding_untouched(arr, w, "interleaved")


def test_png8_flow_on_golden_fixture(twflow, oracle, golden):
    from test_gpu_png import GOLDEN, read_png_rows
    case = golden["revision2_capture2"]
    ra, w, h, cha = read_png_rows(os.path.join(GOLDEN, "tree", "expected", "scenario2", "capture2.png"))
    rb, _, _, chb = read_png_rows(os.path.join(GOLDEN, "tree", "revision2", "scenario2", "capture2.png"))
    fx, fy = oracle.farneback(case["expect_img"], case["target_img"])
    want_vec = [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        arr, views = _dest(e, 2, h, w, "planar")
        t1 = e.submit_png8(ra, cha, rb, chb, w, h, case["span"], float(case["threshold"]), flow=views[0])
        t2 = e.submit_png8(case["expect_img"], 0, rb, chb, w, h, case["span"], float(case["threshold"]), flow=views[1])
        assert e.wait(t1)["vector"] == want_vec and e.wait(t2)["vector"] == want_vec
        for v in views:
            assert np.array_equal(v, np.stack([fx, fy]))


@pytest.mark.parametrize("kw", [dict(flags=0), dict(winSize=50)])
def test_m_through_hbm_paths(twflow, oracle, kw):
    """Box window / a 51-tap window: level 0 runs update + window launches with M in HBM."""
    h, w, n = 117, 180, 4
    pairs = _pairs(2, h, w)
    want = _oracle_fields(oracle, pairs, oracle.default_params(**kw))
    with twflow.Engine(0, twflow.default_params(**kw), slots=n) as e:
        arr, views = _dest(e, n, h, w, "interleaved", pad=5)
        e.launch_counts(reset=True)
        _run(e, pairs, n, 10, 0.0, views)
        cnt = e.launch_counts()
        assert cnt.flow_iter() == 0 and cnt["tw_flow_export"] >= 1, cnt
        for i in range(n):
            assert np.array_equal(_planar(views[i], "interleaved"), want[i % 2]), "pair %d" % i
        assert _padding_untouched(arr, w, "interleaved")


def test_staging_memory(twflow):
    """The first host destination adds one context's staging (slots x the field) and the destination table to the
    engine's device bytes; 20 more batches add nothing."""
    h, w, n = 480, 640, 8
    pairs = _pairs(2, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        _run(e, pairs, n, 10, 0.0)
        arr, views = _dest(e, n, h, w, "interleaved")
        m0 = e.memory()
        _run(e, pairs, n, 10, 0.0, views)
        m1 = e.memory()
        slot = (w * h * 8 + 255) // 256 * 256
        assert m1["device_bytes"] - m0["device_bytes"] == slot * n + 256 + 24 * n + 256, (m0, m1)
        for _ in range(20):
            _run(e, pairs, n, 10, 0.0, views)
        assert e.memory() == m1
