"""Initial flow fields (tw_submit_*_flow_init, OPTFLOW_USE_INITIAL_FLOW): the ABI side and the CPU restatement, no GPU.

The restatement below is what the GPU is pinned against (tests/test_gpu_flow_init.py): OpenCV 2.4.9's
resize(flow0, coarsest size, INTER_AREA) on CV_32FC2 followed by flow *= scale, written again in numpy with float32
operations in OpenCV's order, and composed with the oracle's own stages (level plan, pyramid, polynomial expansion,
FarnebackUpdateMatrices, the window update, the upsample) in orc_farneback's loop.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tw_submit_u8_flow_init", "tw_submit_png8_flow_init", "tw_submit_dev_flow_init")
F32 = np.float32
DBL_EPSILON = np.finfo(np.float64).eps


# ---- INTER_AREA on CV_32FC2 (imgwarp.cpp, 2.4.9), restated ------------------------------------------------------------
def area_tab(ssize, dsize, scale):
    """computeResizeAreaTab in double: per output index, the list of (source index, float alpha) in table order."""
    tab = []
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        ent = []
        if sx1 - fsx1 > 1e-3:
            ent.append((sx1 - 1, F32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            ent.append((sx, F32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            ent.append((sx2, F32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        tab.append(ent)
    return tab


def area_scales(w0, h0, w, h):
    sx, sy = 1.0 / (w / w0), 1.0 / (h / h0)
    ix, iy = int(round(sx)), int(round(sy))  # saturate_cast<int>: round half to even, as Python's round
    fast = abs(sx - ix) < DBL_EPSILON and abs(sy - iy) < DBL_EPSILON
    return sx, sy, ix, iy, fast


def area_fast(f, w, h, ix, iy):
    """resizeAreaFast_Invoker<float, float>: the block's offsets row-major, sum += ((S0+S1)+S2)+S3 per group of four,
    then the rest, then sum * (1.f/area)."""
    area = ix * iy
    blk = f.reshape(h, iy, w, ix, 2).transpose(0, 2, 1, 3, 4).reshape(h, w, area, 2)
    s = np.zeros((h, w, 2), F32)
    k = 0
    while k <= area - 4:
        s = s + (((blk[:, :, k] + blk[:, :, k + 1]) + blk[:, :, k + 2]) + blk[:, :, k + 3])
        k += 4
    while k < area:
        s = s + blk[:, :, k]
        k += 1
    return s * (F32(1) / F32(area))


def area_generic(f, w, h, xtab, ytab):
    """ResizeArea_Invoker with the tables: per row entry buf = buf + S*alpha in column-table order (from 0), then per
    output row sum = beta_0*buf_0, sum += beta_j*buf_j.  Vectorised over outputs, entry by entry in table order."""
    def by_position(tab):
        n = max(len(t) for t in tab)
        idx = np.zeros((len(tab), n), np.int64)
        wt = np.zeros((len(tab), n), F32)
        has = np.zeros((len(tab), n), bool)
        for d, ent in enumerate(tab):
            for m, (si, a) in enumerate(ent):
                idx[d, m], wt[d, m], has[d, m] = si, a, True
        return idx, wt, has
    xi, xa, xh = by_position(xtab)
    yi, yb, yh = by_position(ytab)
    out = np.zeros((h, w, 2), F32)
    for m in range(yi.shape[1]):
        rows = f[yi[:, m]]  # (h, w0, 2): this row entry of every output row
        buf = np.zeros((h, w, 2), F32)
        for q in range(xi.shape[1]):
            t = rows[:, xi[:, q]] * xa[:, q][None, :, None]
            buf = np.where(xh[:, q][None, :, None], buf + t, buf)
        t = yb[:, m][:, None, None] * buf
        out = np.where(yh[:, m][:, None, None], t if m == 0 else out + t, out)
    return out


def area_resize(flow0, w, h, force_generic=False):
    """resize(flow0, Size(w, h), 0, 0, INTER_AREA) for a (h0, w0, 2) float32 field."""
    f = np.ascontiguousarray(flow0, F32)
    h0, w0, _ = f.shape
    if (w0, h0) == (w, h):
        return f.copy()
    sx, sy, ix, iy, fast = area_scales(w0, h0, w, h)
    if fast and not force_generic:
        return area_fast(f, w, h, ix, iy)
    return area_generic(f, w, h, area_tab(w0, w, sx), area_tab(h0, h, sy))


def init_level_flow(flow0, w, h, scale):
    """resize(flow0, ..., INTER_AREA); flow *= scale (convertTo: v * (float)scale + 0.f; a plain copy at scale 1)."""
    f = area_resize(flow0, w, h)
    if abs(scale - 1.0) < DBL_EPSILON:
        return f
    return f * F32(scale) + F32(0)


def farneback_with_init(oracle, prev, nxt, flow0, params=None):
    """orc_farneback's loop with OPTFLOW_USE_INITIAL_FLOW: the coarsest level starts from flow0 (h0, w0, 2) or planar
    (2, h0, w0); flow0 None: zero.  Returns (flowx, flowy)."""
    p = params or oracle.default_params()
    h0, w0 = prev.shape
    if flow0 is not None and flow0.shape == (2, h0, w0):
        flow0 = np.moveaxis(flow0, 0, 2)
    lv = oracle.level_plan(w0, h0, p.pyrScale, p.pyrLevels)
    flow = None
    for k in range(len(lv) - 1, -1, -1):
        L = lv[k]
        if flow is None:
            flow = (np.zeros((L.height, L.width, 2), F32) if flow0 is None else
                    init_level_flow(flow0, L.width, L.height, L.scale))
        else:
            flow = oracle.flow_upsample(flow, L.width, L.height, p.pyrScale)
        R0 = oracle.polyexp(oracle.pyr_level(prev, L), p.polyN, p.polySigma)
        R1 = oracle.polyexp(oracle.pyr_level(nxt, L), p.polyN, p.polySigma)
        M = oracle.update_matrices(R0, R1, flow)
        for i in range(p.pyrIterations):
            flow, M = oracle.update_flow(R0, R1, flow, M, p.winSize, i < p.pyrIterations - 1,
                                         gaussian=bool(p.flags & 256))
    return flow[..., 0].copy(), flow[..., 1].copy()


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def _declared():
    syms = set()
    for fn in ("twflow.h", "twflow_debug.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fn)).read(), flags=re.S)
        syms |= set(re.findall(r"\b(tw_[a-z0-9_]+)\s*\(", txt))
    return syms


def test_new_symbols_declared_exported_and_bound(twflow):
    L = twflow.lib()
    decl = _declared()
    for s in NEW_SYMBOLS:
        assert s in decl, s
        assert hasattr(L, s), s
        assert s in twflow.SYMBOLS, s
    assert set(twflow.SYMBOLS) == decl


def test_flow_init_family_unique_and_export_still_last(twflow):
    dbg = open(os.path.join(ROOT, "include", "twflow_debug.h")).read()
    fams = re.findall(r"^\s+(TW_DF_[A-Z0-9_]+)", dbg.split("enum tw_debug_family")[1].split("};")[0], flags=re.M)
    assert fams[-3:] == ["TW_DF_FLOW_INIT", "TW_DF_FLOW_EXPORT", "TW_DF_COUNT"]
    L = twflow.lib()
    names = [L.tw_debug_family_name(i) for i in range(len(fams) - 1)]
    assert names[fams.index("TW_DF_FLOW_INIT")] == b"tw_flow_area_init"
    assert names.count(b"tw_flow_area_init") == 1
    assert names[fams.index("TW_DF_FLOW_EXPORT")] == b"tw_flow_export"
    assert len(set(names)) == len(names)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   "int f(tw_engine* e, const tw_flow_in* i, const tw_flow_out* o, tw_ticket* t) {\n"
                   "  tw_flow_in in = {0, 8, TW_FLOW_INTERLEAVED}; (void)in;\n"
                   "  return tw_submit_dev_flow_init(e, 0, 0, 1, 1, 1, 0, 0.0, i, o, t); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])


def test_null_engine_is_refused(twflow):
    L = twflow.lib()
    img = (C.c_uint8 * 64)()
    buf = (C.c_float * 128)()
    fi = twflow.FlowIn(C.cast(buf, C.c_void_p), 64, twflow.FLOW_INTERLEAVED)
    tk = C.c_int64()
    bad = twflow.TW_E_BAD_PARAMETER
    assert L.tw_submit_u8_flow_init(None, img, img, 8, 8, 8, 0, 0.0, C.byref(fi), None, C.byref(tk)) == bad
    assert L.tw_submit_png8_flow_init(None, img, 0, img, 0, 8, 8, 0, 0.0, C.byref(fi), None, C.byref(tk)) == bad
    assert L.tw_submit_dev_flow_init(None, img, img, 8, 8, 8, 0, 0.0, C.byref(fi), None, C.byref(tk)) == bad


def test_python_init_argument_shapes(twflow):
    h, w = 6, 10
    fi, _ = twflow._flow_in(np.zeros((h, w + 3, 2), F32)[:, :w], w, h)
    assert (fi.pitch, fi.layout) == ((w + 3) * 8, twflow.FLOW_INTERLEAVED)
    fi, _ = twflow._flow_in(np.zeros((2, h, w + 2), F32)[:, :, :w], w, h)
    assert (fi.pitch, fi.layout) == ((w + 2) * 4, twflow.FLOW_PLANAR)
    assert twflow._flow_in(None, w, h) == (None, None)
    with pytest.raises(twflow.TwError):
        twflow._flow_in(np.zeros((h, w, 2), np.float64), w, h)
    with pytest.raises(twflow.TwError):
        twflow._flow_in(np.zeros((h, w + 1, 2), F32), w, h)


# ---- self-checks of the restatement -----------------------------------------------------------------------------------
def _pair(h, w, seed=0):
    import synth
    return synth.make_pair(seed, h, w)


@pytest.mark.parametrize("hw", [(117, 180), (480, 640)])
@pytest.mark.parametrize("flags", [256, 0])
def test_zero_init_equals_oracle(oracle, hw, flags):
    """flow0 = 0 through the init path (resize, then * scale) gives exactly orc_farneback's zero start."""
    h, w = hw
    a, b = _pair(h, w)
    p = oracle.default_params(flags=flags)
    fx, fy = farneback_with_init(oracle, a, b, np.zeros((h, w, 2), F32), p)
    wx, wy = oracle.farneback(a, b, p)
    assert np.array_equal(fx, wx) and np.array_equal(fy, wy)


@pytest.mark.parametrize("hw,levels,scale", [((480, 640), 3, 0.5), ((117, 180), 3, 0.5), ((1079, 1917), 3, 0.5),
                                              ((200, 300), 2, 0.6), ((64, 96), 0, 0.5)])
def test_constant_field_resizes_to_constant_times_scale(oracle, hw, levels, scale):
    h0, w0 = hw
    L = oracle.level_plan(w0, h0, scale, levels)[-1]
    f0 = np.empty((h0, w0, 2), F32)
    f0[..., 0], f0[..., 1] = 1.5, -0.75
    got = init_level_flow(f0, L.width, L.height, L.scale)
    assert got.shape == (L.height, L.width, 2)
    s = F32(1) if abs(L.scale - 1) < DBL_EPSILON else F32(L.scale)
    want = np.empty_like(got)
    want[..., 0], want[..., 1] = F32(1.5) * s + F32(0), F32(-0.75) * s + F32(0)
    if (L.width, L.height) == (w0, h0) or area_scales(w0, h0, L.width, L.height)[4]:
        assert np.array_equal(got, want)  # a copy, or the block mean of a constant: exact
    else:
        # the generic tables' float alphas need not sum to exactly one: within a few ulp of the constant
        np.testing.assert_allclose(got, want, rtol=4e-7, atol=0)


def test_fast_and_generic_tables_agree_on_an_integer_ratio():
    """At ratio 2 every alpha is 0.5 and every sum of small integers is exact: both paths give the block mean."""
    rng = np.random.default_rng(5)
    f0 = rng.integers(-8, 8, size=(64, 96, 2)).astype(F32)
    _, _, ix, iy, fast = area_scales(96, 64, 48, 32)
    assert fast and (ix, iy) == (2, 2)
    a = area_resize(f0, 48, 32)
    g = area_resize(f0, 48, 32, force_generic=True)
    assert np.array_equal(a, g)
    assert np.array_equal(a, f0.reshape(32, 2, 48, 2, 2).mean(axis=(1, 3), dtype=np.float64).astype(F32))


def test_generic_path_is_taken_where_opencv_takes_it():
    assert not area_scales(180, 117, 90, 58)[4]      # x 2, y 2.017
    assert not area_scales(1917, 1079, 240, 135)[4]
    for w0, h0, w, h in ((640, 480, 80, 60), (1920, 1080, 240, 135), (3840, 2160, 480, 270)):
        assert area_scales(w0, h0, w, h)[2:] == (8, 8, True)


def test_generic_weights_sum_to_one_per_output():
    for s, d in ((117, 58), (1079, 135), (1917, 240), (180, 90)):
        tab = area_tab(s, d, 1.0 / (d / s))
        for ent in tab:
            assert abs(sum(float(a) for _, a in ent) - 1.0) < 1e-5
            assert all(0 <= si < s for si, _ in ent)
