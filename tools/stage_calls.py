#!/usr/bin/env python3
"""The per-stage entry points, call by call: a fixed tour through every tw_stage_* entry point (and
tw_debug_png_kernel_time) on seeded inputs, through twflow.Engine.  Needs a GPU.

    TWFLOW_LIB=<a build of libtwflow.so> stage_calls.py [OUT.json]     (prints the steps as one JSON document)

After every call a step records the returned status, Engine.launch_counts(reset=True) — per family that launched, the
number of launches and the grid z of its last launch — and a SHA-256 of everything the call returned.  A refused call
records its status and the tw_last_error text instead of a hash (the text is read as it stands after the call: an entry
point that refuses without setting one leaves the previous text there, and the tour's order is fixed).  Two builds of
the library that check, launch and compute alike print the same document, byte for byte:
tests/golden/stage_calls_parent.json is this tool's output for the library before the entry points moved onto one stage
scaffold in csrc/twflow_stage.hip.h (profiles/stage_scaffold.md), and tests/test_gpu_stage_calls.py holds the tree's
library to it.  The time tw_debug_png_kernel_time measures is not recorded.

Sizes are the smallest at which the code under an entry point still branches: per-level stages at 37x29 (one partial
tile, odd row padding) and 333x37; tw_flow_iter from 320x20 up; the span scan on 61x47 at span 4; tw_hit_regions below
and just above RGN_LDS_POINTS (256x129 at span 1 is 33 024 points); the pyramid stages at 64x48 and 61x47 (one level
with the default parameters: the fused kernels refuse both) and at 256x256, where they run; tw_png_unfilter at every
wave count on a 40-pixel-wide image.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tidal-wave_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

P = object()  # in a refused call's arguments: a valid pointer of the parameter's type (64 KB of zeros)


def _digest(x, h):
    if isinstance(x, (tuple, list)):
        h.update(b"(%d" % len(x))
        for v in x:
            _digest(v, h)
    elif isinstance(x, np.ndarray):
        h.update(("%s%r" % (x.dtype.str, x.shape)).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    else:
        h.update(repr(x).encode())


class Tour:
    def __init__(self, T):
        self.T = T
        self.steps = []
        self.zeros = (C.c_uint8 * 65536)()

    def _launches(self, e):
        lc = e.launch_counts(reset=True)
        return {k: [lc[k], lc.last_z[k]] for k in sorted(lc) if lc[k]}

    def call(self, e, name, fn, *args, keep=lambda r: r, **kw):
        """One call through the Engine's method; returns what it returned (None when the library refused)."""
        e.launch_counts(reset=True)
        try:
            ret = fn(*args, **kw)
        except self.T.TwError as err:
            self.steps.append([name, {"status": err.code, "error": str(err), "launches": self._launches(e)}])
            return None
        h = hashlib.sha256()
        _digest(keep(ret), h)
        self.steps.append([name, {"status": 0, "launches": self._launches(e), "sha256": h.hexdigest()}])
        return ret

    def refused(self, e, name, sym, *args):
        """One call of the library's own symbol that it must refuse: status and tw_last_error."""
        f = getattr(e._L, sym)
        raw = [C.cast(self.zeros, t) if a is P else a for a, t in zip(args, f.argtypes[1:])]
        assert len(raw) == len(f.argtypes) - 1, sym
        e.launch_counts(reset=True)
        rc = f(e._h, *raw)
        self.steps.append(["%s refused: %s" % (sym, name),
                           {"status": rc, "error": e._L.tw_last_error(e._h).decode(), "launches": self._launches(e)}])


def level_inputs(seed, w, h):
    rng = np.random.default_rng(seed)
    I0 = rng.integers(0, 256, (h, w)).astype(np.float32)
    I1 = np.roll(I0, 1, axis=1) + rng.integers(-3, 4, (h, w)).astype(np.float32)
    flow = rng.normal(0, 1.5, (2, h, w)).astype(np.float32)
    return I0, I1, flow


def level_stages(t, e, w, h, pw, ph):
    """polyexp, update_matrices, flow_upsample_update and blur_solve at one level size; returns (R0, R1, M)."""
    tag = "%dx%d" % (w, h)
    I0, I1, flow = level_inputs(1000 + w, w, h)
    R0 = t.call(e, "polyexp %s" % tag, e.stage_polyexp, I0)
    R1 = t.call(e, "polyexp %s second image" % tag, e.stage_polyexp, I1)
    M = t.call(e, "update_matrices %s" % tag, e.stage_update_matrices, R0, R1, flow)
    prev = np.random.default_rng(2000 + w).normal(0, 1.0, (2, ph, pw)).astype(np.float32)
    t.call(e, "flow_upsample_update %s from %dx%d" % (tag, pw, ph), e.stage_flow_upsample_update, R0, R1, prev)
    for upd in (0, 1):
        t.call(e, "blur_solve %s update_matrices=%d" % (tag, upd), e.stage_blur_solve, R0, R1, M, upd)
    return R0, R1, M


def level_refusals(t, e):
    R = t.refused
    R(e, "null output", "tw_stage_polyexp", P, 37, 29, None)
    R(e, "width 0", "tw_stage_polyexp", P, 0, 29, P)
    R(e, "too large", "tw_stage_polyexp", P, 32768, 32768, P)
    R(e, "null output", "tw_stage_update_matrices", P, P, P, 37, 29, None)
    R(e, "width 0", "tw_stage_update_matrices", P, P, P, 0, 29, P)
    R(e, "too large", "tw_stage_update_matrices", P, P, P, 32768, 32768, P)
    R(e, "null output", "tw_stage_flow_upsample_update", P, P, P, 19, 15, 37, 29, P, None)
    R(e, "width 0", "tw_stage_flow_upsample_update", P, P, P, 19, 15, 0, 29, P, P)
    R(e, "coarser width 0", "tw_stage_flow_upsample_update", P, P, P, 0, 15, 37, 29, P, P)
    R(e, "null output", "tw_stage_blur_solve", P, P, P, 37, 29, 0, None, P)
    R(e, "update_matrices without Mout", "tw_stage_blur_solve", P, P, P, 37, 29, 1, P, None)
    R(e, "width 0", "tw_stage_blur_solve", P, P, P, 0, 29, 0, P, P)


def flow_iter_stages(t, e):
    for w, h, pw, ph in ((320, 20, 160, 10), (333, 37, 167, 19)):
        tag = "%dx%d" % (w, h)
        I0, I1, flow = level_inputs(3000 + w, w, h)
        R0, R1 = e.stage_polyexp(I0), e.stage_polyexp(I1)
        prev = np.random.default_rng(4000 + w).normal(0, 1.0, (2, ph, pw)).astype(np.float32)
        t.call(e, "flow_iter %s with flow_in" % tag, e.stage_flow_iter, R0, R1, flow=flow)
        t.call(e, "flow_iter %s with prev %dx%d" % (tag, pw, ph), e.stage_flow_iter, R0, R1, prev=prev)
        t.call(e, "flow_iter %s from zero" % tag, e.stage_flow_iter, R0, R1)
        if (w, h) == (333, 37):
            for span in (5, 10):
                t.call(e, "flow_iter_grid %s span %d" % (tag, span), e.stage_flow_iter_grid, R0, R1, flow, span)
    R = t.refused
    R(e, "null output", "tw_stage_flow_iter", P, P, P, None, 0, 0, 320, 20, None)
    R(e, "flow_in and prev", "tw_stage_flow_iter", P, P, P, P, 160, 10, 320, 20, P)
    R(e, "width 0", "tw_stage_flow_iter", P, P, P, None, 0, 0, 0, 20, P)
    R(e, "coarser width 0", "tw_stage_flow_iter", P, P, None, P, 0, 10, 320, 20, P)
    R(e, "level too small", "tw_stage_flow_iter", P, P, P, None, 0, 0, 37, 29, P)
    R(e, "null output", "tw_stage_flow_iter_grid", P, P, P, 333, 37, 5, None)
    R(e, "span 1", "tw_stage_flow_iter_grid", P, P, P, 333, 37, 1, P)
    R(e, "width 0", "tw_stage_flow_iter_grid", P, P, P, 0, 37, 5, P)
    R(e, "level too small", "tw_stage_flow_iter_grid", P, P, P, 37, 29, 5, P)


def hit_fields(seed, npairs, w, h, share):
    """Fields of small vectors with `share` of the points displaced by a few pixels, in runs along a row."""
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 0.05, (npairs, 2, h, w)).astype(np.float32)
    on = rng.random((npairs, 1, h, w)) < share
    on |= np.roll(on, 1, axis=3)
    return np.where(on, f + rng.normal(0, 3.0, f.shape).astype(np.float32), f).astype(np.float32)


def scan_stages(t, e):
    w, h, span, thr = 61, 47, 4, 0.5
    t.call(e, "span_scan 61x47 3 pairs", e.stage_span_scan, hit_fields(11, 3, w, h, 0.2), span, thr, False)
    t.call(e, "span_scan 61x47 single pair", e.stage_span_scan, hit_fields(12, 1, w, h, 0.2), span, thr, True)
    R = t.refused
    R(e, "null output", "tw_stage_span_scan", P, 3, w, h, span, thr, 0, None, P, P)
    R(e, "single_pair with 3 pairs", "tw_stage_span_scan", P, 3, w, h, span, thr, 1, P, P, P)
    R(e, "span 0", "tw_stage_span_scan", P, 3, w, h, 0, thr, 0, P, P, P)
    R(e, "width 0", "tw_stage_span_scan", P, 3, 0, h, span, thr, 0, P, P, P)
    rects = [[(5, 7, 20, 10)], [], [(0, 0, 8, 8), (30, 20, 40, 40), (10, 40, 5, 3)]]
    f = hit_fields(13, 3, w, h, 0.1)
    t.call(e, "hit_regions 61x47 span 4 with rectangles", e.stage_hit_regions, f, span, thr, 2, rects)
    t.call(e, "hit_regions 61x47 span 4 n_ignore null", e.stage_hit_regions, f, span, thr, 2, None)
    f = hit_fields(14, 1, 256, 129, 0.02)
    t.call(e, "hit_regions 256x129 span 1 with rectangles", e.stage_hit_regions, f, 1, thr, 1, [[(100, 50, 60, 30)]])
    t.call(e, "hit_regions 256x129 span 1 n_ignore null", e.stage_hit_regions, f, 1, thr, 1, None)
    R(e, "null output", "tw_stage_hit_regions", P, 3, w, h, span, thr, 2, None, None, P, None, P)
    R(e, "gap 9", "tw_stage_hit_regions", P, 3, w, h, span, thr, 9, None, None, P, P, P)
    R(e, "n_ignore without rectangles", "tw_stage_hit_regions", P, 3, w, h, span, thr, 2, None, P, P, P, P)
    R(e, "width 0", "tw_stage_hit_regions", P, 3, 0, h, span, thr, 2, None, None, P, P, P)
    bad = (t.T.Rect * (t.T.MAX_IGNORE * 1))()
    bad[0] = t.T.Rect(0, 0, -1, 2)
    one = (C.c_int * 1)(1)
    R(e, "rectangle of negative width", "tw_stage_hit_regions", P, 1, w, h, span, thr, 2, bad, one, P, P, P)


def pyramid_stages(t, e):
    for w, h in ((64, 48), (61, 47), (256, 256)):  # (256x256: the smallest size with levels 2 and 3, where the fused kernels run)
        tag = "%dx%d" % (w, h)
        img = np.random.default_rng(20 + w).integers(0, 256, (h, w)).astype(np.uint8)
        for level in range(e.num_levels(w, h) + 1):
            t.call(e, "pyr_level %s level %d" % (tag, level), e.stage_pyr_level, img, level)
        t.call(e, "pyr_fused01 %s" % tag, e.stage_pyr_fused01, img)
        t.call(e, "pyr_fused23 %s" % tag, e.stage_pyr_fused23, img)
    R = t.refused
    R(e, "null output", "tw_stage_pyr_level", P, 64, 48, 0, None, P, P)
    R(e, "width 0", "tw_stage_pyr_level", P, 0, 48, 0, P, P, P)
    R(e, "level 99", "tw_stage_pyr_level", P, 64, 48, 99, P, P, P)
    R(e, "level -1", "tw_stage_pyr_level", P, 64, 48, -1, P, P, P)
    for sym in ("tw_stage_pyr_fused01", "tw_stage_pyr_fused23"):
        R(e, "null output", sym, P, 64, 48, P, None)
        R(e, "width 0", sym, P, 0, 48, P, P)
        R(e, "61x47", sym, P, 61, 47, P, P)


def png_rows(rng, w, h, bpp):
    """h rows of 1 + w * bpp bytes: filter type y % 5, then random bytes."""
    rows = rng.integers(0, 256, (h, 1 + w * bpp)).astype(np.uint8)
    rows[:, 0] = np.arange(h) % 5
    return rows


def image_stages(t, e):
    T = t.T
    rng = np.random.default_rng(31)
    w, h = 40, 13
    rgb = png_rows(rng, w, h, 3)
    pal = T.PngRows(png_rows(rng, w, h, 1), w, h, 3, 8, rng.integers(0, 256, (256, 3)).astype(np.uint8))
    for waves in (0, 1, 4, 16):
        t.call(e, "png_unfilter RGB 40x13 waves %d" % waves, e.stage_png_unfilter, rgb, 3, w, h, waves)
        t.call(e, "png_decode palette 40x13 waves %d" % waves, e.stage_png_decode, pal, waves)
    t.call(e, "png_kernel_time palette 40x13", e.png_kernel_time, pal, 2, 0, keep=lambda us: None)
    R = t.refused
    R(e, "null output", "tw_stage_png_unfilter", P, 3, w, h, 0, None)
    R(e, "width 0", "tw_stage_png_unfilter", P, 3, 0, h, 0, P)
    R(e, "5 channels", "tw_stage_png_unfilter", P, 5, w, h, 0, P)
    R(e, "waves 2", "tw_stage_png_unfilter", P, 3, w, h, 2, P)
    bad = rgb.copy()
    bad[3, 0] = 5
    R(e, "filter type 5", "tw_stage_png_unfilter", bad.ctypes.data_as(C.POINTER(C.c_uint8)), 3, w, h, 0, P)
    R(e, "null output", "tw_stage_png_decode", C.byref(pal), 0, None)
    R(e, "waves 2", "tw_stage_png_decode", C.byref(pal), 2, P)
    gray = T.PngRows(np.zeros((h, w), np.uint8), w, h)
    R(e, "plain gray", "tw_stage_png_decode", C.byref(gray), 0, P)
    nopal = T.PngRows(png_rows(rng, w, h, 1), w, h, 3, 8)
    R(e, "palette image without PLTE", "tw_stage_png_decode", C.byref(nopal), 0, P)
    R(e, "null time", "tw_debug_png_kernel_time", C.byref(pal), 0, 2, None)
    R(e, "0 iterations", "tw_debug_png_kernel_time", C.byref(pal), 0, 0, P)
    R(e, "waves 2", "tw_debug_png_kernel_time", C.byref(pal), 2, 2, P)

    src = rng.integers(0, 256, (30, 40)).astype(np.uint8)
    t.call(e, "resize_u8 40x30 to 43x28", e.stage_resize_u8, src, 43, 28)
    R(e, "null output", "tw_stage_resize_u8", P, 40, 30, None, 43, 28)
    R(e, "width 0", "tw_stage_resize_u8", P, 0, 30, P, 43, 28)
    R(e, "target width 0", "tw_stage_resize_u8", P, 40, 30, P, 0, 28)
    R(e, "10 pixels apart", "tw_stage_resize_u8", P, 40, 30, P, 50, 30)

    import jpeg_cases as J
    coef, quant = J.random_blocks(3 * 2, 1017, False)
    luma = T.JpegLuma(coef.reshape(2, 3, 64), quant, 17, 9)
    t.call(e, "jpeg_idct 17x9", e.stage_jpeg_idct, luma, guard=True)
    R(e, "null output", "tw_stage_jpeg_idct", C.byref(luma), None, None)
    R(e, "plain gray", "tw_stage_jpeg_idct", C.byref(T.JpegLuma.from_gray(np.zeros((9, 17), np.uint8))), P, None)
    R(e, "too few blocks", "tw_stage_jpeg_idct", C.byref(T.JpegLuma(np.zeros((2, 2, 64), np.int16), np.ones(64, np.uint16), 17, 9)),
      P, None)
    R(e, "width 0", "tw_stage_jpeg_idct", C.byref(T.JpegLuma(np.zeros((2, 3, 64), np.int16), np.ones(64, np.uint16), 0, 9)), P, None)

    a = rng.integers(0, 256, (30, 40)).astype(np.uint8)
    b = rng.integers(0, 256, (30, 40)).astype(np.uint8)
    t.call(e, "mask_rects 40x30 no rectangle", e.stage_mask_rects, a, b, [], guard=True)
    t.call(e, "mask_rects 40x30 3 rectangles", e.stage_mask_rects, a, b, [(3, 4, 10, 5), (30, 20, 40, 40), (0, 29, 40, 1)], guard=True)
    R(e, "null output", "tw_stage_mask_rects", P, P, 40, 30, None, 0, None, None)
    R(e, "width 0", "tw_stage_mask_rects", P, P, 0, 30, None, 0, P, None)
    one = (T.Rect * 1)(T.Rect(0, 0, -1, 2))
    R(e, "rectangle of negative width", "tw_stage_mask_rects", P, P, 40, 30, one, 1, P, None)
    R(e, "too many rectangles", "tw_stage_mask_rects", P, P, 40, 30, C.cast(t.zeros, C.POINTER(T.Rect)), T.MAX_IGNORE + 1, P, None)


def pair_stages(t, e):
    import synth
    R = t.refused
    w, h = 128, 96
    a, _ = synth.make_pair(3, h, w)
    b = np.roll(a, (2, -3), axis=(0, 1))
    b[40:] = np.roll(b[40:], 3, axis=0)
    t.call(e, "shift 128x96 stride 133", e.stage_shift, a, b, 8, stride=w + 5)
    t.call(e, "shift 128x96 stride 133 force_global", e.stage_shift, a, b, 8, stride=w + 5, force_global=True)
    t.call(e, "shift_bands 128x96 band 32 stride 133", e.stage_shift_bands, a, b, 8, 32, stride=w + 5)
    R(e, "null output", "tw_stage_shift", P, P, w, w, h, 8, 0, P, None)
    R(e, "radius 0", "tw_stage_shift", P, P, w, w, h, 0, 0, P, P)
    R(e, "width 0", "tw_stage_shift", P, P, w, 0, h, 8, 0, P, P)
    R(e, "stride below the width", "tw_stage_shift", P, P, w - 1, w, h, 8, 0, P, P)
    R(e, "null output", "tw_stage_shift_bands", P, P, w, w, h, 8, 32, 0, P, P, None, P)
    R(e, "band 40", "tw_stage_shift_bands", P, P, w, w, h, 8, 40, 0, P, P, P, P)
    R(e, "width 0", "tw_stage_shift_bands", P, P, w, 0, h, 8, 32, 0, P, P, P, P)
    R(e, "stride below the width", "tw_stage_shift_bands", P, P, w - 1, w, h, 8, 32, 0, P, P, P, P)

    w, h = 61, 47
    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    b = np.roll(a, 1, axis=1)
    b[10:20, 30:45] = rng.integers(0, 256, (10, 15))
    flow = np.zeros((2, h, w), np.float32)
    flow[0] = 1.0
    flow += rng.normal(0, 0.2, flow.shape).astype(np.float32)
    t.call(e, "warp_residual 61x47 span 4", e.stage_warp_residual, a, b, flow, 4, 16)
    t.call(e, "warp_residual 61x47 span 4 stride 64", e.stage_warp_residual, a, b, flow, 4, 16, stride=64)
    R(e, "null output", "tw_stage_warp_residual", P, P, w, w, h, P, 4, 16, None, P, P)
    R(e, "tolerance 255", "tw_stage_warp_residual", P, P, w, w, h, P, 4, 255, P, P, P)
    R(e, "width 0", "tw_stage_warp_residual", P, P, w, 0, h, P, 4, 16, P, P, P)
    R(e, "stride below the width", "tw_stage_warp_residual", P, P, w - 1, w, h, P, 4, 16, P, P, P)

    w, h = 40, 30
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    b = a.copy()
    b[5:12, 8:30] = rng.integers(0, 256, (7, 22))
    rects, hits = [(2, 3, 6, 5), (35, 25, 10, 10)], [(8, 8, 3.5, -2.25), (20, 12, -6.0, 0.5), (39, 29, 1.0, 1.0)]
    regions = [(8, 5, 22, 7), (0, 0, 40, 30)]
    for mis in (0, 1):
        t.call(e, "overlay 40x30 misalign %d" % mis, e.stage_overlay, a, b, rects, hits, regions, 16, pitch=3 * w + 7,
               stride=w + 4, misalign=mis)
    R(e, "null output", "tw_stage_overlay", P, P, w, h, w, 0, None, 0, None, 0, None, 0, 16, None, 3 * w, P)
    R(e, "width 0", "tw_stage_overlay", P, P, 0, h, w, 0, None, 0, None, 0, None, 0, 16, P, 3 * w, P)
    R(e, "misalign 4", "tw_stage_overlay", P, P, w, h, w, 4, None, 0, None, 0, None, 0, 16, P, 3 * w, P)
    R(e, "pitch below three bytes a pixel", "tw_stage_overlay", P, P, w, h, w, 0, None, 0, None, 0, None, 0, 16, P, 3 * w - 1, P)


def tour(T):
    """[[step name, record]] of the whole tour, in order."""
    t = Tour(T)
    levels = {}
    with T.Engine(0, T.default_params(), slots=1) as e:
        for w, h, pw, ph in ((37, 29, 19, 15), (333, 37, 167, 19)):
            levels[(w, h)] = level_stages(t, e, w, h, pw, ph)
        level_refusals(t, e)
        flow_iter_stages(t, e)
        scan_stages(t, e)
        pyramid_stages(t, e)
        image_stages(t, e)
        pair_stages(t, e)
    # tw_blur_solve's other windows: a Gaussian window of 50 and the box window (double running sums, Vbox)
    for what, params in (("winSize 50", T.default_params(winSize=50)), ("box window", T.default_params(flags=0))):
        with T.Engine(0, params, slots=1) as e:
            for (w, h), (R0, R1, M) in levels.items():
                for upd in (0, 1):
                    t.call(e, "%s: blur_solve %dx%d update_matrices=%d" % (what, w, h, upd), e.stage_blur_solve, R0, R1, M, upd)
    return t.steps


def main():
    import twflow as T
    doc = json.dumps(tour(T), indent=1)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
