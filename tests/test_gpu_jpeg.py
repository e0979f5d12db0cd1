"""JPEG on the device: tw_jpeg_idct alone (tw_stage_jpeg_idct) against the host's jpeg_luma_to_gray and a numpy int64
jidctint, byte for byte, with the bytes around the image untouched; tw_submit_jpeg against tw_submit_u8 on the
host-decoded images, the oracle and tw_flow_u8.  Only the committed fixtures and numpy: no PIL, no node (the host decoder
is compiled at test time, tests/jpeg_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J

pytestmark = pytest.mark.gpu
ROOT = J.ROOT
SPAN, THR = 10, 1.0


def wg_blocks():
    """Blocks a workgroup of tw_jpeg_idct takes along x (it takes one block row), from the launch's own constant."""
    src = open(os.path.join(ROOT, "tidal-wave_amd", "csrc", "twflow_kernels.hip.h")).read()
    return int(re.search(r"constexpr int JPEG_WG_BLOCKS = (\d+);", src).group(1))


# (w, h, blocks_w, blocks_h): one block; one whole block; a partial block on either axis; the 4:2:0 MCU padding (a whole
# column and a whole row of blocks that are never computed); 1031 px = 129 blocks crosses every workgroup boundary along x
# (workgroups of JPEG_WG_BLOCKS = 32 blocks = 256 px: 4 full ones and one with a single 7-px block), 9 x 1031 every one
# along y (a workgroup per block row: 129 rows, the last 7 px high); the reference's own fixture size
SIZES = [(1, 1, 1, 1), (8, 8, 1, 1), (9, 7, 2, 1), (7, 9, 1, 2), (17, 15, 4, 2), (33, 31, 6, 4), (1031, 9, 130, 2),
         (9, 1031, 2, 130), (280, 279, 36, 36)]


def test_the_wide_sizes_cross_every_workgroup_boundary():
    nb = wg_blocks()
    assert (1031 + 7) // 8 > 4 * nb and (1031 + 7) // 8 % nb != 0 and 1031 % 8 != 0


@pytest.fixture(scope="module")
def host():
    if J.host_lib() is None:
        pytest.fail("no g++: the host decoder cannot be built")
    return J


@pytest.mark.parametrize("full_range", [True, False], ids=["full_range", "valid_range"])
@pytest.mark.parametrize("w,h,bw,bh", SIZES, ids=["%dx%d" % s[:2] for s in SIZES])
def test_stage_jpeg_idct_equals_the_host_idct(twflow, engine, host, w, h, bw, bh, full_range):
    coef, quant = J.random_blocks(bw * bh, 1000 + w + (7 if full_range else 0), full_range)
    luma = J.Luma(w, h, coef.reshape(bh, bw, 64), quant)
    want = J.luma_to_gray(luma)
    assert np.array_equal(want, J.blocks_to_image(J.idct_reference(coef, quant), bw, bh, w, h))
    before = engine.launch_counts()["tw_jpeg_idct"]
    got, guard = engine.stage_jpeg_idct(twflow.JpegLuma(luma.coef, luma.quant, w, h), guard=True)
    assert engine.launch_counts()["tw_jpeg_idct"] == before + 1
    assert np.array_equal(got, want)
    assert guard.shape == (512,) and np.all(guard == 0xA5)


@pytest.mark.parametrize("name", J.fixture_names() + ["capture1_expected", "capture1_revision1", "capture1_revision2"])
def test_fixture_files_on_the_device_equal_libjpeg(twflow, engine, host, name):
    data, want = J.capture1(name[9:]) if name.startswith("capture1_") else J.fixture(name)
    luma, _ = J.decode_luma(data)
    got, guard = engine.stage_jpeg_idct(twflow.JpegLuma(luma.coef, luma.quant, luma.w, luma.h), guard=True)
    assert np.array_equal(got, want) and np.all(guard == 0xA5)


def test_stage_refuses_what_it_cannot_run(twflow, engine):
    L = twflow.lib()
    out = (C.c_uint8 * 4096)()
    ok = twflow.JpegLuma(np.zeros((2, 3, 64), np.int16), np.ones(64, np.uint16), 17, 15)
    assert L.tw_stage_jpeg_idct(engine._h, C.byref(ok), out, None) == 0
    for bw, bh in ((2, 2), (7, 2), (3, 1), (3, 6)):
        bad = twflow.JpegLuma(np.zeros((bh, bw, 64), np.int16), np.ones(64, np.uint16), 17, 15)
        assert L.tw_stage_jpeg_idct(engine._h, C.byref(bad), out, None) == twflow.TW_E_BAD_PARAMETER
    gray = twflow.JpegLuma.from_gray(np.zeros((15, 17), np.uint8))
    assert L.tw_stage_jpeg_idct(engine._h, C.byref(gray), out, None) == twflow.TW_E_BAD_PARAMETER
    assert L.tw_stage_jpeg_idct(engine._h, C.byref(ok), None, None) == twflow.TW_E_BAD_PARAMETER


# ---- tw_submit_jpeg ---------------------------------------------------------------------------------------------------
def _luma(twflow, name, e=None):
    """(JpegLuma of a fixture file, its host decode); e: the coefficients in page-locked memory (DMA-ed in place)"""
    data, want = J.fixture(name)
    luma, _ = J.decode_luma(data)
    gray = J.luma_to_gray(luma)
    assert np.array_equal(gray, want)
    coef = luma.coef
    if e is not None:
        coef = e.host_array(luma.coef.shape, np.int16)
        coef[...] = luma.coef
    return twflow.JpegLuma(coef, luma.quant, luma.w, luma.h), gray


def _planar_out(e, n, h, w):
    arr = e.host_array((n, 2, h, w), np.float32)
    arr[...] = np.nan
    return arr


def _reference(twflow, oracle, a, b):
    """vectors of submit_u8 and of the oracle, and the dense field of tw_flow_u8 and of the oracle, for one gray pair"""
    fx, fy = oracle.farneback(a, b)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        plain = e.wait(e.submit(a, b, SPAN, THR))
        gx, gy, _ = e.calculate_internal(a, b)
    assert np.array_equal(gx, fx) and np.array_equal(gy, fy)
    assert plain["vector"] == oracle.span_scan(fx, fy, SPAN, THR)
    return plain, np.stack([gx, gy])


@pytest.fixture(scope="module")
def golden_pair(twflow, oracle, host):
    a, b = J.fixture("golden_expected")[1], J.fixture("golden_revision2")[1]
    plain, field = _reference(twflow, oracle, a, b)
    assert len(plain["vector"]) > 0  # (a pair with vectors)
    swapped, field_s = _reference(twflow, oracle, b, a)
    return {"ab": (plain, field), "ba": (swapped, field_s)}


@pytest.mark.parametrize("pair", [("progressive_420_33x31", "baseline_gray_33x31"), ("golden_expected", "golden_revision2")],
                         ids=["33x31", "golden"])
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page_locked"])
def test_submit_jpeg_equals_submit_u8_on_the_host_decode(twflow, oracle, host, pair, pinned):
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        la, a = _luma(twflow, pair[0], e if pinned else None)
        lb, b = _luma(twflow, pair[1], e if pinned else None)
        h, w = a.shape
        out = _planar_out(e, 1, h, w)
        res = e.wait(e.submit_jpeg(la, lb, SPAN, THR, out=out[0]))
        cnt = e.launch_counts()
        assert cnt["tw_jpeg_idct"] == 1 and cnt.last_z["tw_jpeg_idct"] == 2 and cnt["tw_png_unfilter"] == 0
        assert cnt["tw_resize_u8"] == 0
        got = out[0].copy()  # (page-locked memory goes with the engine)
    plain, field = _reference(twflow, oracle, a, b)
    assert res["status"] == plain["status"] and res["vector"] == plain["vector"]
    assert (res["width"], res["height"]) == (w, h)
    assert np.array_equal(got, field)


def test_mixed_batch_of_five_pairs(twflow, oracle, host, golden_pair):
    """JPEG + JPEG (pageable and page-locked), JPEG + plain gray, plain gray + JPEG and a gray pair in one batch: tickets in
    order, one tw_jpeg_idct launch for the batch, every pair's vectors and field those of the gray pair."""
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        la, a = _luma(twflow, "golden_expected")
        lb, b = _luma(twflow, "golden_revision2")
        pa, _ = _luma(twflow, "golden_expected", e)
        pb, _ = _luma(twflow, "golden_revision2", e)
        h, w = a.shape
        out = _planar_out(e, 5, h, w)
        pairs = [(la, lb, "ab"), (pb, pa, "ba"), (la, b, "ab"), (b, pa, "ba"), (a, b, "ab")]
        tickets = [e.submit_jpeg(x, y, SPAN, THR, out=out[i]) for i, (x, y, _) in enumerate(pairs)]
        assert [t[0] for t in tickets] == [1, 2, 3, 4, 5]
        assert e.launch_counts()["tw_jpeg_idct"] == 0  # (nothing before the batch is launched)
        e.flush()
        cnt = e.launch_counts()
        assert cnt["tw_jpeg_idct"] == 1 and cnt.last_z["tw_jpeg_idct"] == 10 and cnt["tw_png_unfilter"] == 0
        for i, t in enumerate(tickets):
            res = e.wait(t)
            plain, field = golden_pair[pairs[i][2]]
            assert res["status"] == plain["status"] and res["vector"] == plain["vector"], i
            assert np.array_equal(out[i], field), i
        assert e.launch_counts()["tw_jpeg_idct"] == 1


def test_an_all_gray_batch_is_submit_u8_sized(twflow, oracle, host, golden_pair):
    a, b = J.fixture("golden_expected")[1], J.fixture("golden_revision2")[1]

    def run(call):
        with twflow.Engine(0, twflow.default_params(), slots=4) as e:
            out = _planar_out(e, 3, *a.shape)
            tickets = [call(e, x, y, out[i]) for i, (x, y) in enumerate(((a, b), (b, a), (a, b)))]
            e.flush()
            res = [e.wait(t) for t in tickets]
            return res, out.copy(), dict(e.launch_counts())

    res_j, out_j, cnt_j = run(lambda e, x, y, o: e.submit_jpeg(x, y, SPAN, THR, out=o))
    res_u, out_u, cnt_u = run(lambda e, x, y, o: e.submit(x, y, SPAN, THR, flow=o, reconcile=True))
    assert cnt_j["tw_jpeg_idct"] == 0 and cnt_j == cnt_u  # the same launches
    assert [r["vector"] for r in res_j] == [r["vector"] for r in res_u] and np.array_equal(out_j, out_u)
    for i, key in enumerate(("ab", "ba", "ab")):
        assert res_j[i]["vector"] == golden_pair[key][0]["vector"] and np.array_equal(out_j[i], golden_pair[key][1])


@pytest.mark.parametrize("target_is_coef", [True, False], ids=["coefficients", "gray"])
def test_a_target_of_another_size_is_reconciled_on_the_device(twflow, oracle, host, target_is_coef):
    """33 x 31 expected, 30 x 35 target: the inverse DCT writes the target at its own size, one tw_resize_u8 launch takes it
    to the pair's size; the result is submit_u8_sized's on the decoded grays."""
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        la, a = _luma(twflow, "progressive_420_33x31")
        lt, t = _luma(twflow, "restart_420_30x35")
        out = _planar_out(e, 1, 31, 33)
        res = e.wait(e.submit_jpeg(la, lt if target_is_coef else t, SPAN, THR, out=out[0]))
        cnt = e.launch_counts()
        assert cnt["tw_jpeg_idct"] == 1 and cnt["tw_resize_u8"] == 1
        got = out[0].copy()  # (page-locked memory goes with the engine)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out_u = _planar_out(e, 1, 31, 33)
        res_u = e.wait(e.submit(a, t, SPAN, THR, flow=out_u[0], reconcile=True))
        got_u = out_u[0].copy()
    assert res["vector"] == res_u["vector"] and res["status"] == res_u["status"]
    assert np.array_equal(got, got_u)
    fx, fy = oracle.farneback(a, oracle.reconcile_target(t, 33, 31))
    assert np.array_equal(got, np.stack([fx, fy]))


def test_refusals_leave_the_open_batch_as_it_was(twflow, oracle, host, golden_pair):
    L = twflow.lib()
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        la, a = _luma(twflow, "golden_expected")
        lb, b = _luma(twflow, "golden_revision2")
        h, w = a.shape
        out = _planar_out(e, 2, h, w)
        tickets = [e.submit_jpeg(la, lb, SPAN, THR, out=out[0])]
        # a target 6 px off, as coefficients and as gray
        for dw, dh in ((6, 0), (0, -6), (-5, 6)):
            tw_, th_ = w + dw, h + dh
            far = twflow.JpegLuma(np.zeros(((th_ + 7) // 8, (tw_ + 7) // 8, 64), np.int16), np.ones(64, np.uint16), tw_, th_)
            for t in (far, np.zeros((th_, tw_), np.uint8)):
                with pytest.raises(twflow.TwError) as ei:
                    e.submit_jpeg(la, t, SPAN, THR)
                assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
        # block counts outside ceil(size / 8) .. + 3; an image with neither pointer
        nbx, nby = (w + 7) // 8, (h + 7) // 8
        for bw, bh in ((nbx - 1, nby), (nbx + 4, nby), (nbx, nby - 1), (nbx, nby + 4)):
            bad = twflow.JpegLuma(np.zeros((bh, bw, 64), np.int16), np.ones(64, np.uint16), w, h)
            for x, y in ((la, bad), (bad, lb)):
                with pytest.raises(twflow.TwError) as ei:
                    e.submit_jpeg(x, y, SPAN, THR)
                assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        empty = twflow.JpegLuma.from_gray(a)
        empty.gray = None
        tk = C.c_int64(-1)
        assert L.tw_submit_jpeg(e._h, C.byref(la), C.byref(empty), SPAN, THR, None, None, C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
        assert L.tw_submit_jpeg(e._h, None, C.byref(lb), SPAN, THR, None, None, C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
        assert tk.value == -1
        # the open batch is as it was: the next ticket is the next one, and the batch completes in one launch
        tickets.append(e.submit_jpeg(lb, la, SPAN, THR, out=out[1]))
        assert [t[0] for t in tickets] == [1, 2]
        for i, key in enumerate(("ab", "ba")):
            res = e.wait(tickets[i])
            assert res["vector"] == golden_pair[key][0]["vector"] and np.array_equal(out[i], golden_pair[key][1])
        cnt = e.launch_counts()
        assert cnt["tw_jpeg_idct"] == 1 and cnt.last_z["tw_jpeg_idct"] == 4


HOST_DIR = os.path.join(ROOT, "tidal-wave_amd", "host")
ADDON = os.path.join(HOST_DIR, "build", "Release", "tidalwave.node")


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the built addon is not available")
@pytest.mark.parametrize("device_jpeg", ["0", "1"])
def test_reference_mocha_suite_in_node_with_the_switch_either_way(device_jpeg):
    """The golden tree (half of it JPEG) through create() -> addon -> libtwflow.so: the reference's mocha expectations hold
    with the inverse DCT on the host and on the device."""
    r = subprocess.run(["node", "test_reference.js"], cwd=HOST_DIR, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TW_DEVICE_JPEG=device_jpeg))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all 4 reference tests passed" in r.stdout
