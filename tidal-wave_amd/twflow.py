"""ctypes binding of libtwflow.so (include/twflow.h) — test / bench plumbing.

The product is the C-ABI HIP library; this module only marshals numpy arrays into it.  There is no
fallback of any kind: if the library is missing or no HIP device is usable, calls raise.

Names follow the reference: `Engine.calculate_internal` is OpticalFlow::calculateInternal
(/root/reference/src/opticalflow.h:49), `Engine.diff` is the flow + span-grid scan of
Consumer::run (/root/reference/src/consumer.cpp:54-84) and returns the fields of `Response`
(/root/reference/src/message_queue.h:27-42).
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtwflow.so")

TW_OK, TW_E_BAD_PARAMETER, TW_E_BAD_IMAGE_FORMAT, TW_E_DONT_MATCH_SIZE = 0, 1, 2, 3
TW_E_DEVICE, TW_E_NOMEM, TW_E_UNSUPPORTED, TW_E_BUSY = 4, 5, 6, 7
K_PYR, K_POLYEXP, K_UPDATE_MATRICES, K_BLUR_SOLVE, K_SCAN = 0, 1, 2, 3, 4
KERNEL_NAMES = {K_PYR: "tw_pyr_level", K_POLYEXP: "tw_polyexp", K_UPDATE_MATRICES: "tw_update_matrices",
                K_BLUR_SOLVE: "tw_blur_solve", K_SCAN: "tw_span_scan"}


class Params(C.Structure):
    # tw_params == struct OpticalFlowParameter, /root/reference/src/opticalflow.h:28-36
    _fields_ = [("pyrScale", C.c_double), ("pyrLevels", C.c_int), ("winSize", C.c_int),
                ("pyrIterations", C.c_int), ("polyN", C.c_int), ("polySigma", C.c_double),
                ("flags", C.c_int)]


class Vector(C.Structure):
    # tw_vector == struct Vector, /root/reference/src/message_queue.h:20-25
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("dx", C.c_double), ("dy", C.c_double)]


class FlowOut(C.Structure):
    # tw_flow_out (include/twflow.h): destination of a pair's final flow for the tw_submit_*_flow calls
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_ssize_t), ("layout", C.c_int)]


class FlowIn(C.Structure):
    # tw_flow_in (include/twflow.h): a pair's initial flow field for the tw_submit_*_flow_init calls
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_ssize_t), ("layout", C.c_int)]


class Rect(C.Structure):
    # tw_rect (include/twflow.h): an ignore rectangle of the tw_submit_*_ignore calls, in pair coordinates
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class Region(C.Structure):
    # tw_region (include/twflow.h): one connected component of a pair's hits (TW_OPT_REGIONS / tw_wait_regions), 36 bytes
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int), ("count", C.c_int),
                ("peak_x", C.c_int), ("peak_y", C.c_int), ("peak_dx", C.c_float), ("peak_dy", C.c_float)]

    def as_tuple(self):
        return (self.x, self.y, self.width, self.height, self.count, self.peak_x, self.peak_y, self.peak_dx, self.peak_dy)


class Change(C.Structure):
    # tw_change (include/twflow.h): one span-grid cell with a differing pixel (TW_OPT_RESIDUAL / tw_ticket_changes), 24 bytes
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("n_diff", C.c_int), ("n_unexplained", C.c_int), ("max_diff", C.c_int),
                ("max_unexplained", C.c_int)]

    def as_tuple(self):
        return (self.x, self.y, self.n_diff, self.n_unexplained, self.max_diff, self.max_unexplained)


class Shift(C.Structure):
    # tw_shift (include/twflow.h): a pair's estimated translation and its acceptance check (TW_OPT_SHIFT / tw_ticket_shift), 40 bytes
    _fields_ = [("dx", C.c_int), ("dy", C.c_int), ("applied", C.c_int), ("n_shift", C.c_int), ("n_zero", C.c_int),
                ("sad_shift", C.c_uint64), ("sad_zero", C.c_uint64)]

    def as_tuple(self):
        return (self.dx, self.dy, self.applied, self.n_shift, self.n_zero, self.sad_shift, self.sad_zero)


class OverlayOut(C.Structure):
    # tw_overlay_out (include/twflow.h): destination of a pair's diff image (tw_ticket_overlay)
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_ssize_t), ("format", C.c_int)]


OVERLAY_RGB8 = 0
OVERLAY_MAX_LEN = 1024
# tw_overlay_hit (include/twflow_debug.h): a hit record as the ordered scan leaves it (16 bytes)
OVERLAY_HIT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("dx", "<f4"), ("dy", "<f4")])
class ShiftBand(C.Structure):
    # tw_shift_band (include/twflow.h): one band's vertical shift and its acceptance check (TW_OPT_SHIFT_BANDS / tw_ticket_shift_bands), 40 bytes
    _fields_ = [("y", C.c_int), ("rows", C.c_int), ("dy", C.c_int), ("applied", C.c_int), ("n_shift", C.c_int), ("n_zero", C.c_int),
                ("sad_shift", C.c_uint64), ("sad_zero", C.c_uint64)]

    def as_tuple(self):
        return (self.y, self.rows, self.dy, self.applied, self.n_shift, self.n_zero, self.sad_shift, self.sad_zero)


MAX_IGNORE = 32
MAX_REGIONS = 256
FLOW_PLANAR, FLOW_INTERLEAVED = 0, 1
# tw_region as a numpy record (36 bytes, no padding)
REGION_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("count", "<i4"),
                         ("peak_x", "<i4"), ("peak_y", "<i4"), ("peak_dx", "<f4"), ("peak_dy", "<f4")])


class TwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("twflow status %d: %s" % (code, msg))
        self.code = code


_lib = None

# every symbol include/twflow.h and include/twflow_debug.h (diagnostics, not part of the boundary) declare
OPT_SCAN_FUSED_FINAL = 1
OPT_POLYEXP_F32 = 2
OPT_REGIONS = 3
OPT_RESIDUAL = 4
OPT_SHIFT = 5
OPT_SHIFT_BANDS = 6

SYMBOLS = [
    "tw_default_params", "tw_abi_version", "tw_has_variants", "tw_device_count", "tw_device_pci_bus_id", "tw_engine_create", "tw_engine_destroy", "tw_strerror",
    "tw_last_error", "tw_flow_u8", "tw_diff_u8", "tw_submit_u8", "tw_submit_png8", "tw_submit_dev", "tw_flush", "tw_wait",
    "tw_submit_u8_flow", "tw_submit_png8_flow", "tw_submit_dev_flow",
    "tw_submit_u8_flow_init", "tw_submit_png8_flow_init", "tw_submit_dev_flow_init",
    "tw_submit_u8_sized", "tw_submit_png8_sized", "tw_submit_dev_sized", "tw_stage_resize_u8",
    "tw_png_on_device", "tw_submit_png", "tw_stage_png_decode", "tw_submit_jpeg", "tw_stage_jpeg_idct",
    "tw_image_keep", "tw_image_create_u8", "tw_image_release", "tw_image_size", "tw_submit_image_png", "tw_submit_image_jpeg",
    "tw_debug_resident",
    "tw_submit_u8_ignore", "tw_submit_png_ignore", "tw_submit_jpeg_ignore", "tw_submit_image_png_ignore",
    "tw_submit_image_jpeg_ignore", "tw_stage_mask_rects",
    "tw_grid_capacity", "tw_dev_alloc", "tw_dev_free", "tw_dev_upload", "tw_dev_download", "tw_host_alloc", "tw_host_free", "tw_host_register", "tw_host_unregister", "tw_set_option",
    "tw_prof_select", "tw_prof_read",
    "tw_algorithmic_bytes", "tw_algorithmic_bytes_launch", "tw_level_runs_flow_iter", "tw_algorithmic_bytes_pair", "tw_min_traffic_bytes_pair", "tw_num_levels", "tw_level_chunk", "tw_bench_stage", "tw_stage_pyr_level", "tw_stage_pyr_fused23", "tw_stage_pyr_fused01",
    "tw_stage_png_unfilter", "tw_stage_polyexp", "tw_stage_update_matrices", "tw_stage_flow_upsample_update", "tw_stage_blur_solve", "tw_stage_flow_iter",
    "tw_stage_flow_iter_grid", "tw_stage_span_scan",
    "tw_wait_regions", "tw_stage_hit_regions",
    "tw_ticket_changes", "tw_stage_warp_residual",
    "tw_ticket_shift", "tw_stage_shift", "tw_debug_shift_plan",
    "tw_ticket_shift_bands", "tw_stage_shift_bands", "tw_debug_band_plan",
    "tw_ticket_hits", "tw_ticket_overlay", "tw_stage_overlay", "tw_debug_overlay_plan",
    "tw_debug_graphs", "tw_debug_occupancy", "tw_debug_stamps", "tw_debug_stamps_ex", "tw_debug_copy_rate",
    "tw_debug_launch_counts", "tw_debug_family_name", "tw_debug_memory", "tw_debug_check_size", "tw_debug_flow_iter_plan",
    "tw_debug_blur_plan", "tw_debug_same_flags", "tw_debug_png_kernel_time", "tw_debug_scan_plan", "tw_debug_level_plan",
    "tw_debug_pyr_plan",
]


PNG_PLAIN_GRAY = -1


class PngRows(C.Structure):
    """tw_png_rows: one image of submit_png / stage_png_decode as its IHDR describes it.  rows: the inflated IDAT stream
    (height rows of 1 + ceil(width * channels * bit_depth / 8) bytes, filter type first) or, with color_type
    PNG_PLAIN_GRAY, a gray image of shape (height, width).  palette: the PLTE body (colour type 3), r g b per entry;
    palette_entries defaults to its length / 3.  The arrays stay alive with the structure."""
    _fields_ = [("rows", C.POINTER(C.c_uint8)), ("width", C.c_int), ("height", C.c_int), ("color_type", C.c_int),
                ("bit_depth", C.c_int), ("palette", C.POINTER(C.c_uint8)), ("palette_entries", C.c_int)]

    def __init__(self, rows, width, height, color_type=PNG_PLAIN_GRAY, bit_depth=8, palette=None, palette_entries=None):
        super().__init__()
        self._rows = np.ascontiguousarray(rows, np.uint8)
        self._palette = None if palette is None else np.ascontiguousarray(palette, np.uint8)
        self.rows = _u8(self._rows)
        self.width, self.height, self.color_type, self.bit_depth = width, height, color_type, bit_depth
        if self._palette is not None:
            self.palette = _u8(self._palette)
        n = 0 if self._palette is None else self._palette.size // 3
        self.palette_entries = n if palette_entries is None else palette_entries


class JpegLuma(C.Structure):
    """tw_jpeg_luma: one image of submit_jpeg / stage_jpeg_idct.  coef: the quantised luma coefficients after the entropy
    decode, an int16 array [bh, bw, 64] (bh x bw stored blocks — whole MCUs — of 64 coefficients in natural order);
    quant: the 64 entries of the luma table, natural order; w, h: the image's own size.  JpegLuma.from_gray(img) is a plain
    gray image instead (coef NULL).  The arrays stay alive with the structure."""
    _fields_ = [("coef", C.POINTER(C.c_int16)), ("gray", C.POINTER(C.c_uint8)), ("width", C.c_int), ("height", C.c_int),
                ("blocks_w", C.c_int), ("blocks_h", C.c_int), ("quant", C.c_uint16 * 64)]

    def __init__(self, coef, quant, w, h):
        super().__init__()
        self._coef = np.ascontiguousarray(coef, np.int16)
        if self._coef.ndim != 3 or self._coef.shape[2] != 64:
            raise ValueError("coef must have shape [bh, bw, 64]")
        self._gray = None
        self.coef = self._coef.ctypes.data_as(C.POINTER(C.c_int16))
        self.width, self.height = w, h
        self.blocks_h, self.blocks_w = self._coef.shape[:2]
        q = np.ascontiguousarray(quant, np.uint16).reshape(64)
        C.memmove(self.quant, q.ctypes.data, 128)

    @classmethod
    def from_gray(cls, img):
        self = cls.__new__(cls)
        C.Structure.__init__(self)
        self._coef = None
        self._gray = np.ascontiguousarray(_gray(img))
        self.gray = _u8(self._gray)
        self.height, self.width = self._gray.shape
        return self

    @property
    def w(self):
        return self.width

    @property
    def h(self):
        return self.height


def png_on_device(color_type, bit_depth, interlace=0):
    """tw_png_on_device: does submit_png take rows of this IHDR colour type, bit depth and interlace method?"""
    return bool(lib().tw_png_on_device(color_type, bit_depth, interlace))


VARIANTS_LIB_PATH = os.path.join(_HERE, "libtwflow_variants.so")
_variants = None


def lib():
    """Load libtwflow.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if os.environ.get("TWFLOW_VARIANTS") == "1":
        path = VARIANTS_LIB_PATH  # tools/ A/B runs (kbench, sq_probe) of the kernels the product library leaves out
    if os.environ.get("TWFLOW_LIB"):
        path = os.environ["TWFLOW_LIB"]  # tools/ A/B runs of another BUILD of the library (e.g. make NT=<bits>)
    if not os.path.exists(path):
        raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % os.path.basename(path))
    _lib = _bind(path)
    return _lib


class use_variants_library:
    """Context manager: engines created inside use libtwflow_variants.so (`make VARIANTS=1`: the product library plus
    the measured-slower A/B kernels behind TW_BLUR_VARIANT / TW_POLY_VARIANT / TW_BLUR_SMALL / TW_UPD_NY).  Tests and
    tools only; the product library refuses those switches."""

    def __enter__(self):
        global _lib, _variants
        if _variants is None:
            if not os.path.exists(VARIANTS_LIB_PATH):
                raise ImportError("libtwflow_variants.so not built: make -C tidal-wave_amd/csrc VARIANTS=1")
            _variants = _bind(VARIANTS_LIB_PATH)
        self._saved = lib()
        _lib = _variants
        return _variants

    def __exit__(self, *a):
        global _lib
        _lib = self._saved


def _bind(path):
    L = C.CDLL(path)
    vp, fp, u8p, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    L.tw_default_params.argtypes = [C.POINTER(Params)]
    L.tw_default_params.restype = None
    L.tw_device_count.restype = C.c_int
    L.tw_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.tw_engine_create.argtypes = [C.c_int, C.POINTER(Params), C.c_int, C.POINTER(vp)]
    L.tw_engine_destroy.argtypes = [vp]
    L.tw_engine_destroy.restype = None
    L.tw_strerror.argtypes = [C.c_int]
    L.tw_strerror.restype = C.c_char_p
    L.tw_last_error.argtypes = [vp]
    L.tw_last_error.restype = C.c_char_p
    L.tw_flow_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, fp, fp, fp]
    L.tw_diff_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double,
                             C.POINTER(Vector), C.c_int, ip, fp]
    L.tw_submit_u8.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double,
                               C.POINTER(C.c_int64)]
    L.tw_submit_png8.argtypes = [vp, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int64)]
    L.tw_stage_png_unfilter.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, u8p]
    L.tw_submit_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double,
                                C.POINTER(C.c_int64)]
    fop, tkp = C.POINTER(FlowOut), C.POINTER(C.c_int64)
    L.tw_submit_u8_flow.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double, fop, tkp]
    L.tw_submit_png8_flow.argtypes = [vp, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, fop, tkp]
    L.tw_submit_dev_flow.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double, fop, tkp]
    fip = C.POINTER(FlowIn)
    L.tw_submit_u8_flow_init.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double, fip, fop, tkp]
    L.tw_submit_png8_flow_init.argtypes = [vp, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, fip,
                                           fop, tkp]
    L.tw_submit_dev_flow_init.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_double, fip, fop, tkp]
    L.tw_submit_u8_sized.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_ssize_t, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int,
                                     C.c_double, fip, fop, tkp]
    L.tw_submit_png8_sized.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_double, fip, fop, tkp]
    L.tw_submit_dev_sized.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int,
                                      C.c_double, fip, fop, tkp]
    L.tw_stage_resize_u8.argtypes = [vp, u8p, C.c_int, C.c_int, u8p, C.c_int, C.c_int]
    L.tw_png_on_device.argtypes = [C.c_int, C.c_int, C.c_int]
    L.tw_png_on_device.restype = C.c_int
    L.tw_submit_png.argtypes = [vp, C.POINTER(PngRows), C.POINTER(PngRows), C.c_int, C.c_double, fip, fop, tkp]
    L.tw_stage_png_decode.argtypes = [vp, C.POINTER(PngRows), C.c_int, u8p]
    L.tw_submit_jpeg.argtypes = [vp, C.POINTER(JpegLuma), C.POINTER(JpegLuma), C.c_int, C.c_double, fip, fop, tkp]
    L.tw_stage_jpeg_idct.argtypes = [vp, C.POINTER(JpegLuma), u8p, u8p]
    L.tw_debug_png_kernel_time.argtypes = [vp, C.POINTER(PngRows), C.c_int, C.c_int, fp]
    L.tw_image_keep.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(vp)]
    L.tw_image_create_u8.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_ssize_t, C.POINTER(vp)]
    L.tw_image_release.argtypes = [vp, vp]
    L.tw_image_size.argtypes = [vp, vp, ip, ip]
    L.tw_submit_image_png.argtypes = [vp, vp, C.POINTER(PngRows), C.c_int, C.c_double, fip, fop, tkp]
    L.tw_submit_image_jpeg.argtypes = [vp, vp, C.POINTER(JpegLuma), C.c_int, C.c_double, fip, fop, tkp]
    rp = C.POINTER(Rect)
    L.tw_submit_u8_ignore.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_ssize_t, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int,
                                      C.c_double, fip, fop, rp, C.c_int, tkp]
    L.tw_submit_png_ignore.argtypes = [vp, C.POINTER(PngRows), C.POINTER(PngRows), C.c_int, C.c_double, fip, fop, rp,
                                       C.c_int, tkp]
    L.tw_submit_jpeg_ignore.argtypes = [vp, C.POINTER(JpegLuma), C.POINTER(JpegLuma), C.c_int, C.c_double, fip, fop, rp,
                                        C.c_int, tkp]
    L.tw_submit_image_png_ignore.argtypes = [vp, vp, C.POINTER(PngRows), C.c_int, C.c_double, fip, fop, rp, C.c_int, tkp]
    L.tw_submit_image_jpeg_ignore.argtypes = [vp, vp, C.POINTER(JpegLuma), C.c_int, C.c_double, fip, fop, rp, C.c_int, tkp]
    L.tw_stage_mask_rects.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, rp, C.c_int, u8p, u8p]
    L.tw_debug_resident.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.tw_debug_resident.restype = C.c_int
    L.tw_wait.argtypes = [vp, C.c_int64, C.POINTER(Vector), C.c_int, ip, fp]
    L.tw_wait_regions.argtypes = [vp, C.c_int64, C.POINTER(Vector), C.c_int, ip, ip, C.POINTER(Region), C.c_int, ip, fp]
    L.tw_stage_hit_regions.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, rp, ip, ip,
                                       C.POINTER(Region), ip]
    L.tw_ticket_changes.argtypes = [vp, C.c_int64, C.POINTER(Change), C.c_int, ip]
    L.tw_stage_warp_residual.argtypes = [vp, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, fp, C.c_int, C.c_int, ip, ip,
                                         C.POINTER(Change)]
    L.tw_ticket_shift.argtypes = [vp, C.c_int64, C.POINTER(Shift)]
    L.tw_stage_shift.argtypes = [vp, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                 C.POINTER(Shift)]
    L.tw_debug_shift_plan.argtypes = [C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_ticket_shift_bands.argtypes = [vp, C.c_int64, C.POINTER(ShiftBand), C.c_int, ip]
    L.tw_stage_shift_bands.argtypes = [vp, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_uint16), C.POINTER(Shift), C.POINTER(ShiftBand), ip]
    L.tw_debug_band_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_ticket_hits.argtypes = [vp, C.c_int64, ip]
    L.tw_ticket_overlay.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(OverlayOut)]
    L.tw_stage_overlay.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int, rp, C.c_int, vp, C.c_int,
                                   C.POINTER(Region), C.c_int, C.c_int, u8p, C.c_ssize_t, ip]
    L.tw_debug_overlay_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_longlong, C.c_uint64, C.c_longlong, C.c_int, C.c_int, ip,
                                        C.c_int]
    L.tw_flush.argtypes = [vp]
    L.tw_bench_stage.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]
    L.tw_level_chunk.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.tw_grid_capacity.argtypes = [C.c_int, C.c_int, C.c_int]
    L.tw_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.tw_dev_free.argtypes = [vp, vp]
    L.tw_dev_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.tw_dev_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.tw_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.tw_host_free.argtypes = [vp, vp]
    L.tw_host_register.argtypes = [vp, vp, C.c_size_t]
    L.tw_host_unregister.argtypes = [vp, vp]
    L.tw_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.tw_prof_select.argtypes = [vp, C.c_int, C.c_int]
    L.tw_prof_read.argtypes = [vp, C.c_int, C.POINTER(C.c_double), ip]
    L.tw_algorithmic_bytes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.tw_algorithmic_bytes.restype = C.c_double
    L.tw_algorithmic_bytes_pair.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.tw_algorithmic_bytes_pair.restype = C.c_double
    L.tw_min_traffic_bytes_pair.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.tw_min_traffic_bytes_pair.restype = C.c_double
    L.tw_num_levels.argtypes = [vp, C.c_int, C.c_int]
    L.tw_stage_pyr_level.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, fp, ip, ip]
    L.tw_stage_pyr_fused23.argtypes = [vp, u8p, C.c_int, C.c_int, fp, fp]
    L.tw_stage_pyr_fused01.argtypes = [vp, u8p, C.c_int, C.c_int, fp, fp]
    L.tw_stage_flow_iter.argtypes = [vp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp]
    L.tw_stage_flow_iter_grid.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, fp]
    L.tw_stage_span_scan.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, ip, ip, fp]
    L.tw_stage_polyexp.argtypes = [vp, fp, C.c_int, C.c_int, fp]
    L.tw_stage_update_matrices.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, fp]
    L.tw_stage_flow_upsample_update.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]
    L.tw_stage_blur_solve.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp]
    L.tw_has_variants.restype = C.c_int
    L.tw_debug_copy_rate.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.tw_debug_graphs.argtypes = [vp]
    L.tw_debug_graphs.restype = C.c_int
    L.tw_abi_version.restype = C.c_int
    L.tw_algorithmic_bytes_launch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.tw_algorithmic_bytes_launch.restype = C.c_double
    L.tw_level_runs_flow_iter.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.tw_level_runs_flow_iter.restype = C.c_int
    u64p = C.POINTER(C.c_uint64)
    L.tw_debug_launch_counts.argtypes = [vp, u64p, u64p, C.c_int, C.c_int]
    L.tw_debug_launch_counts.restype = C.c_int
    L.tw_debug_family_name.argtypes = [C.c_int]
    L.tw_debug_family_name.restype = C.c_char_p
    L.tw_debug_memory.argtypes = [vp, u64p, C.c_int]
    L.tw_debug_memory.restype = C.c_int
    L.tw_debug_check_size.argtypes = [C.c_int, C.c_int]
    L.tw_debug_check_size.restype = C.c_int
    L.tw_debug_flow_iter_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_debug_flow_iter_plan.restype = C.c_int
    L.tw_debug_blur_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_debug_blur_plan.restype = C.c_int
    L.tw_debug_pyr_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_longlong, ip, C.c_int]
    L.tw_debug_pyr_plan.restype = C.c_int
    L.tw_debug_scan_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_debug_scan_plan.restype = C.c_int
    L.tw_debug_level_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
    L.tw_debug_level_plan.restype = C.c_int
    L.tw_debug_same_flags.argtypes = [vp, C.POINTER(C.c_uint), C.c_int]
    L.tw_debug_same_flags.restype = C.c_int
    return L


FlowIterPlan = collections.namedtuple("FlowIterPlan", "strips segments nt nt_last")
ShiftPlan = collections.namedtuple("ShiftPlan", "lds_x lds_y rx ry grid_x block lds_budget prof_grid_x prof_grid_y verify_grid_x")
BandPlan = collections.namedtuple("BandPlan", "nb nblk lds lds_bytes lds_budget r rows_grid_x block verify_grid_x")
BlurPlan = collections.namedtuple("BlurPlan", "family block tile_cols rows xsh grid_x grid_y small forced")
PYR_KERNELS = ("tw_pyr_k3", "tw_pyr_k3f", "tw_pyr_23", "tw_pyr_taps", "tw_pyr_level_lds", "tw_pyr_level")
PyrPlan = collections.namedtuple("PyrPlan", "kernel targ family block tile_cols rows grid_x grid_y lds pitch aligned4 w h ksize mode xmax "
                                 "nrows_max fused23 fused01 threads23_pair threads23_batch levels yclip")
ScanPlan = collections.namedtuple("ScanPlan", "kernel gw gh G S segments rounds")
# images: 0 a pyramid launch of its own, 1 written by the coarser level's launch, 2 its launch writes the next finer level's too
LevelPlanRow = collections.namedtuple("LevelPlanRow", "pairs per launches tail images init flow_iter same flow_iter_last same_last same01")
LevelPlanView = collections.namedtuple("LevelPlanView", "kind nlanes levels lat_quads fused_final grid_final parts")


class LaunchCounts(dict):
    """Engine.launch_counts(): family -> launches; .last_z: family -> grid z (pairs / images) of its latest launch."""

    def flow_iter(self):
        return self["tw_flow_iter"] + self["tw_flow_iter_ups"] + self["tw_flow_iter_zero"]


def abi_version():
    return lib().tw_abi_version()


def default_params(**kw):
    p = Params()
    lib().tw_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def device_count():
    return lib().tw_device_count()


def device_pci_bus_id(device):
    buf = C.create_string_buffer(32)
    rc = lib().tw_device_pci_bus_id(device, buf, 32)
    if rc != TW_OK:
        raise TwError(rc, "no such device")
    return buf.value.decode()


def grid_capacity(w, h, span):
    return lib().tw_grid_capacity(w, h, span)


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _flow_out(flow, w, h):
    """A submit's `flow=` argument -> FlowOut (None: no destination).  Accepted: a float32 numpy array in page-locked
    memory (Engine.host_array) or a float32 torch tensor on the engine's device, shaped (2, h, w) planar or (h, w, 2)
    interleaved (rows may be padded: any row stride, unit stride within a row), or a raw (pointer, pitch, layout) tuple.
    The library itself refuses pageable host memory and memory of another device."""
    if flow is None:
        return None
    if isinstance(flow, tuple):
        ptr, pitch, layout = flow
        return FlowOut(ptr, pitch, layout)
    if isinstance(flow, np.ndarray):
        if flow.dtype != np.float32:
            raise TwError(TW_E_BAD_PARAMETER, "flow destination must be float32")
        shape, strides, ptr = flow.shape, flow.strides, flow.ctypes.data
    elif type(flow).__module__.startswith("torch"):
        import torch
        if flow.dtype != torch.float32 or not flow.is_cuda:
            raise TwError(TW_E_BAD_PARAMETER, "flow destination tensor must be float32 on the GPU")
        shape, strides, ptr = tuple(flow.shape), tuple(s * 4 for s in flow.stride()), flow.data_ptr()
    else:
        raise TwError(TW_E_BAD_PARAMETER, "unsupported flow destination %r" % type(flow))
    if shape == (2, h, w) and strides[2] == 4 and strides[0] == strides[1] * h:
        return FlowOut(ptr, strides[1], FLOW_PLANAR)
    if shape == (h, w, 2) and strides[2] == 4 and strides[1] == 8:
        return FlowOut(ptr, strides[0], FLOW_INTERLEAVED)
    raise TwError(TW_E_BAD_PARAMETER, "flow destination must be (2, %d, %d) planar or (%d, %d, 2) interleaved with "
                  "unit-stride rows, got shape %r strides %r" % (h, w, h, w, shape, strides))


def _flow_in(init, w, h):
    """A submit's `init=` argument -> (FlowIn, the object to keep alive) (None: zero start).  Accepted: a float32 numpy
    array in any host memory (page-locked memory of Engine.host_array is DMA-ed in place, any other is copied by the
    library before the submit returns), a float32 torch tensor on the engine's device, shaped (2, h, w) planar or
    (h, w, 2) interleaved (rows may be padded), or a raw (pointer, pitch, layout) tuple (a device pointer, say)."""
    if init is None:
        return None, None
    if isinstance(init, tuple):
        ptr, pitch, layout = init
        return FlowIn(ptr, pitch, layout), None
    if isinstance(init, np.ndarray):
        if init.dtype != np.float32:
            raise TwError(TW_E_BAD_PARAMETER, "initial flow must be float32")
        if init.ndim == 3 and init.strides[-1] != 4:
            init = np.ascontiguousarray(init)
        shape, strides, ptr = init.shape, init.strides, init.ctypes.data
    elif type(init).__module__.startswith("torch"):
        import torch
        if init.dtype != torch.float32 or not init.is_cuda:
            raise TwError(TW_E_BAD_PARAMETER, "initial flow tensor must be float32 on the GPU")
        shape, strides, ptr = tuple(init.shape), tuple(s * 4 for s in init.stride()), init.data_ptr()
    else:
        raise TwError(TW_E_BAD_PARAMETER, "unsupported initial flow %r" % type(init))
    if shape == (2, h, w) and strides[2] == 4 and strides[0] == strides[1] * h:
        return FlowIn(ptr, strides[1], FLOW_PLANAR), init
    if shape == (h, w, 2) and strides[2] == 4 and strides[1] == 8:
        return FlowIn(ptr, strides[0], FLOW_INTERLEAVED), init
    raise TwError(TW_E_BAD_PARAMETER, "initial flow must be (2, %d, %d) planar or (%d, %d, 2) interleaved with "
                  "unit-stride rows, got shape %r strides %r" % (h, w, h, w, shape, strides))


def _rects(ignore):
    """A list of (x, y, w, h) as (tw_rect array or None, count) for the tw_submit_*_ignore calls; the library reads the
    rectangles before the call returns."""
    rs = [tuple(int(v) for v in r) for r in ignore]
    if not rs:
        return None, 0
    arr = (Rect * len(rs))()
    for i, (x, y, w, h) in enumerate(rs):
        arr[i] = Rect(x, y, w, h)
    return arr, len(rs)


def _gray(a):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise TwError(TW_E_BAD_IMAGE_FORMAT, "expected a 2-D uint8 image")
    if a.strides[1] != 1:
        a = np.ascontiguousarray(a)
    return a


KEEP_EXPECT, KEEP_TARGET = 0, 1


class Image:
    """tw_image: a gray image resident in the engine's device memory (Engine.image / Engine.keep).  The engine looks the
    handle up in its own registry, so a released or foreign Image is refused (TW_E_BAD_PARAMETER), never dereferenced."""

    def __init__(self, engine, handle):
        self._e, self._h = engine, handle

    @property
    def size(self):
        """(width, height)"""
        w, h = C.c_int(), C.c_int()
        self._e._check(self._e._L.tw_image_size(self._e._h, self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def release(self):
        """tw_image_release: the block returns to the engine's store once every batch that reads it has been collected."""
        self._e._check(self._e._L.tw_image_release(self._e._h, self._h))


class Engine:
    """One worker's engine on one GPU (OpticalFlowByGPU of the reference, src/opticalflow.h:62-70)."""

    def __init__(self, device=0, params=None, slots=1):
        self._L = lib()
        self._h = C.c_void_p()
        self.params = params or default_params()
        rc = self._L.tw_engine_create(device, C.byref(self.params), slots, C.byref(self._h))
        if rc != TW_OK:
            self._h = C.c_void_p()
            raise TwError(rc, self._L.tw_strerror(rc).decode())
        self.device = device
        self.slots = slots
        self._devbufs = []
        self._hostbufs = []

    def close(self):
        if self._h:
            for d in self._devbufs:
                self._L.tw_dev_free(self._h, d)
            self._devbufs = []
            for hb in self._hostbufs:
                self._L.tw_host_free(self._h, hb)
            self._hostbufs = []
            self._L.tw_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != TW_OK:
            msg = self._L.tw_last_error(self._h).decode() or self._L.tw_strerror(rc).decode()
            raise TwError(rc, msg)

    # ---- OpticalFlow::calculateInternal -------------------------------------------------------------
    def calculate_internal(self, expect, target):
        """Returns (flowx, flowy, seconds)."""
        a, b = _gray(expect), _gray(target)
        if a.shape != b.shape:
            raise TwError(TW_E_DONT_MATCH_SIZE, "Don't match image size")
        h, w = a.shape
        fx = np.empty((h, w), np.float32)
        fy = np.empty((h, w), np.float32)
        sec = C.c_float()
        if a.strides[0] != b.strides[0]:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        self._check(self._L.tw_flow_u8(self._h, _u8(a), _u8(b), w, h, a.strides[0], _f(fx), _f(fy), C.byref(sec)))
        return fx, fy, sec.value

    # ---- flow + span-grid scan ---------------------------------------------------------------------
    def diff(self, expect, target, span=10, threshold=5.0):
        """Returns dict(status, vector=[(x,y,dx,dy)...], time, height, width) like Response."""
        t = self.submit(expect, target, span, threshold)
        return self.wait(t)

    def submit(self, expect, target, span=10, threshold=5.0, *, flow=None, init=None, reconcile=False, ignore=None):
        """ignore: a list of (x, y, w, h) rectangles of the pair that may differ (tw_submit_u8_ignore; None: the plain calls).
        flow: where the pair's final flow goes (tw_submit_u8_flow; see _flow_out), kept alive by the caller until wait().
        init: the pair's initial flow field (tw_submit_u8_flow_init; see _flow_in), unchanged until wait().
        reconcile: a target of another shape goes to tw_submit_u8_sized, which resizes one within 5 px to the expected
        image's size on the device and refuses any other (the default refuses every shape mismatch here)."""
        a, b = _gray(expect), _gray(target)
        if ignore is not None:
            if a.shape != b.shape and not reconcile:
                raise TwError(TW_E_DONT_MATCH_SIZE, "Don't match image size")
            h, w = a.shape
            tk = C.c_int64()
            fo = _flow_out(flow, w, h)
            fi, _keep = _flow_in(init, w, h)
            rs, nr = _rects(ignore)
            self._check(self._L.tw_submit_u8_ignore(self._h, _u8(a), w, h, a.strides[0], _u8(b), b.shape[1], b.shape[0],
                                                    b.strides[0], span, threshold,
                                                    C.byref(fi) if fi is not None else None,
                                                    C.byref(fo) if fo is not None else None, rs, nr, C.byref(tk)))
            return (tk.value, w, h, span, threshold)
        if a.shape != b.shape and reconcile:
            h, w = a.shape
            tk = C.c_int64()
            fo = _flow_out(flow, w, h)
            fi, _keep = _flow_in(init, w, h)
            self._check(self._L.tw_submit_u8_sized(self._h, _u8(a), w, h, a.strides[0], _u8(b), b.shape[1], b.shape[0],
                                                   b.strides[0], span, threshold,
                                                   C.byref(fi) if fi is not None else None,
                                                   C.byref(fo) if fo is not None else None, C.byref(tk)))
            return (tk.value, w, h, span, threshold)
        if a.shape != b.shape:
            raise TwError(TW_E_DONT_MATCH_SIZE, "Don't match image size")
        if a.strides[0] != b.strides[0]:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        h, w = a.shape
        tk = C.c_int64()
        fo = _flow_out(flow, w, h)
        fi, _keep = _flow_in(init, w, h)
        if fi is not None:
            self._check(self._L.tw_submit_u8_flow_init(self._h, _u8(a), _u8(b), w, h, a.strides[0], span, threshold,
                                                       C.byref(fi), C.byref(fo) if fo is not None else None, C.byref(tk)))
        elif fo is None:
            self._check(self._L.tw_submit_u8(self._h, _u8(a), _u8(b), w, h, a.strides[0], span, threshold, C.byref(tk)))
        else:
            self._check(self._L.tw_submit_u8_flow(self._h, _u8(a), _u8(b), w, h, a.strides[0], span, threshold,
                                                  C.byref(fo), C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    def submit_ptr(self, p_expect, p_target, w, h, stride, span=10, threshold=5.0):
        """tw_submit_u8 on raw HOST pointers (ctypes POINTER(c_uint8)) the caller keeps alive — the bench's inner loop:
        no numpy marshalling per pair.  Page-locked memory (host_array) is DMAed in place."""
        tk = C.c_int64()
        self._check(self._L.tw_submit_u8(self._h, p_expect, p_target, w, h, stride, span, threshold, C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    def submit_png8(self, expect, ch_a, target, ch_b, w, h, span=10, threshold=5.0, *, flow=None, init=None,
                    target_size=None):
        """tw_submit_png8: each image is either filtered PNG rows (uint8 array of h * (1 + w * ch) bytes, ch 1-4) or a
        plain gray image (ch 0, shape (h, w)).  flow, init: as for submit (tw_submit_png8_flow[_init]).
        target_size: (width, height) of the target's own rows (tw_submit_png8_sized; None: the pair's size)."""
        a = np.ascontiguousarray(expect, np.uint8)
        b = np.ascontiguousarray(target, np.uint8)
        tk = C.c_int64()
        fo = _flow_out(flow, w, h)
        fi, _keep = _flow_in(init, w, h)
        if target_size is not None:
            self._check(self._L.tw_submit_png8_sized(self._h, _u8(a), ch_a, w, h, _u8(b), ch_b, target_size[0],
                                                     target_size[1], span, threshold,
                                                     C.byref(fi) if fi is not None else None,
                                                     C.byref(fo) if fo is not None else None, C.byref(tk)))
        elif fi is not None:
            self._check(self._L.tw_submit_png8_flow_init(self._h, _u8(a), ch_a, _u8(b), ch_b, w, h, span, threshold,
                                                         C.byref(fi), C.byref(fo) if fo is not None else None, C.byref(tk)))
        elif fo is None:
            self._check(self._L.tw_submit_png8(self._h, _u8(a), ch_a, _u8(b), ch_b, w, h, span, threshold, C.byref(tk)))
        else:
            self._check(self._L.tw_submit_png8_flow(self._h, _u8(a), ch_a, _u8(b), ch_b, w, h, span, threshold,
                                                    C.byref(fo), C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    def stage_png_unfilter(self, rows, ch, w, h, waves=0):
        rows = np.ascontiguousarray(rows, np.uint8)
        assert rows.size == h * (1 + w * ch)
        out = np.empty((h, w), np.uint8)
        self._check(self._L.tw_stage_png_unfilter(self._h, _u8(rows), ch, w, h, waves, _u8(out)))
        return out

    def submit_png(self, expect, target, span=10, threshold=5.0, *, flow=None, init=None, ignore=None):
        """tw_submit_png: expect, target are PngRows (any kind png_on_device admits, or PNG_PLAIN_GRAY), each at its own
        size; the pair's size is the expected image's.  flow, init, ignore (tw_submit_png_ignore): as for submit."""
        w, h = expect.width, expect.height
        tk = C.c_int64()
        fo = _flow_out(flow, w, h)
        fi, _keep = _flow_in(init, w, h)
        if ignore is not None:
            rs, nr = _rects(ignore)
            self._check(self._L.tw_submit_png_ignore(self._h, C.byref(expect), C.byref(target), span, threshold,
                                                     C.byref(fi) if fi is not None else None,
                                                     C.byref(fo) if fo is not None else None, rs, nr, C.byref(tk)))
            return (tk.value, w, h, span, threshold)
        self._check(self._L.tw_submit_png(self._h, C.byref(expect), C.byref(target), span, threshold,
                                          C.byref(fi) if fi is not None else None,
                                          C.byref(fo) if fo is not None else None, C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    def stage_png_decode(self, img, waves=0):
        """tw_png_unfilter alone on one PngRows image of any admitted kind: the (height, width) gray image."""
        out = np.empty((img.height, img.width), np.uint8)
        self._check(self._L.tw_stage_png_decode(self._h, C.byref(img), waves, _u8(out)))
        return out

    def submit_jpeg(self, expect, target, span=10, threshold=5.0, init=None, out=None, ignore=None):
        """tw_submit_jpeg: expect, target are JpegLuma (coefficients, or JpegLuma.from_gray) or 2-D uint8 gray images, each
        at its own size; the pair's size is the expected image's.  init, out: the initial field and the destination of
        the final flow, as submit's init and flow; ignore (tw_submit_jpeg_ignore): as for submit."""
        a = expect if isinstance(expect, JpegLuma) else JpegLuma.from_gray(expect)
        b = target if isinstance(target, JpegLuma) else JpegLuma.from_gray(target)
        w, h = a.width, a.height
        tk = C.c_int64()
        fo = _flow_out(out, w, h)
        fi, _keep = _flow_in(init, w, h)
        if ignore is not None:
            rs, nr = _rects(ignore)
            self._check(self._L.tw_submit_jpeg_ignore(self._h, C.byref(a), C.byref(b), span, threshold,
                                                      C.byref(fi) if fi is not None else None,
                                                      C.byref(fo) if fo is not None else None, rs, nr, C.byref(tk)))
            return (tk.value, w, h, span, threshold)
        self._check(self._L.tw_submit_jpeg(self._h, C.byref(a), C.byref(b), span, threshold,
                                           C.byref(fi) if fi is not None else None,
                                           C.byref(fo) if fo is not None else None, C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    # ---- resident images ------------------------------------------------------------------------------
    def image(self, gray):
        """tw_image_create_u8: a 2-D uint8 image made resident."""
        a = _gray(gray)
        h, w = a.shape
        out = C.c_void_p()
        self._check(self._L.tw_image_create_u8(self._h, _u8(a), w, h, a.strides[0], C.byref(out)))
        return Image(self, out)

    def keep(self, ticket, which="expect"):
        """tw_image_keep: the expected ("expect") or target ("target") image of a submitted, not yet waited pair, as its
        batch sees it; `which` may also be the raw integer."""
        k = {"expect": KEEP_EXPECT, "target": KEEP_TARGET}.get(which, which)
        out = C.c_void_p()
        self._check(self._L.tw_image_keep(self._h, ticket[0], int(k), C.byref(out)))
        return Image(self, out)

    def submit_image(self, img, target, span=10, threshold=5.0, *, flow=None, init=None, ignore=None):
        """tw_submit_image_png / tw_submit_image_jpeg: the expected image is the resident `img`; target is a 2-D uint8 gray
        image or a PngRows (tw_submit_image_png), or a JpegLuma (tw_submit_image_jpeg), at its own size.  flow, init,
        ignore (the tw_submit_image_*_ignore calls): as for submit."""
        w, h = img.size if img is not None else (0, 0)
        tk = C.c_int64()
        fo = _flow_out(flow, w, h) if img is not None else None
        fi, _keep = _flow_in(init, w, h) if img is not None else (None, None)
        args = (span, threshold, C.byref(fi) if fi is not None else None, C.byref(fo) if fo is not None else None,
                C.byref(tk))
        ih = img._h if img is not None else None
        if ignore is not None:
            args = args[:-1] + _rects(ignore) + args[-1:]
        if isinstance(target, JpegLuma):
            call = self._L.tw_submit_image_jpeg if ignore is None else self._L.tw_submit_image_jpeg_ignore
            self._check(call(self._h, ih, C.byref(target), *args))
        else:
            if not isinstance(target, PngRows):
                b = np.ascontiguousarray(_gray(target))
                target = PngRows(b, b.shape[1], b.shape[0])
            call = self._L.tw_submit_image_png if ignore is None else self._L.tw_submit_image_png_ignore
            self._check(call(self._h, ih, C.byref(target), *args))
        return (tk.value, w, h, span, threshold)

    def resident(self):
        """The resident store (twflow_debug.h: tw_debug_resident)."""
        v = (C.c_uint64 * 4)()
        if self._L.tw_debug_resident(self._h, v) != 4:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_resident failed")
        return {"images": int(v[0]), "bytes_in_use": int(v[1]), "bytes_reserved": int(v[2]), "chunk_allocs": int(v[3])}

    def stage_jpeg_idct(self, luma, guard=False):
        """tw_jpeg_idct alone on one JpegLuma with coefficients: the (h, w) gray image; guard=True: also the 512 device
        bytes around it (256 in front, 256 behind), which were 0xA5 before the launch."""
        out = np.empty((luma.height, luma.width), np.uint8)
        g = np.empty(512, np.uint8) if guard else None
        self._check(self._L.tw_stage_jpeg_idct(self._h, C.byref(luma), _u8(out), _u8(g) if guard else None))
        return (out, g) if guard else out

    def stage_mask_rects(self, expect, target, rects, guard=False):
        """tw_mask_rects alone on two 2-D uint8 images of one shape and a list of (x, y, w, h): the edited target;
        guard=True: also the 512 device bytes around the target's slot (256 in front, 256 behind), 0xA5 before the launch."""
        a, b = np.ascontiguousarray(_gray(expect)), np.ascontiguousarray(_gray(target))
        if a.shape != b.shape:
            raise TwError(TW_E_DONT_MATCH_SIZE, "Don't match image size")
        h, w = a.shape
        out = np.empty((h, w), np.uint8)
        g = np.empty(512, np.uint8) if guard else None
        rs, nr = _rects(rects)
        self._check(self._L.tw_stage_mask_rects(self._h, _u8(a), _u8(b), w, h, rs, nr, _u8(out), _u8(g) if guard else None))
        return (out, g) if guard else out

    def png_kernel_time(self, img, iters=20, waves=0):
        """tw_debug_png_kernel_time: microseconds of one tw_png_unfilter launch on this PngRows image (event-timed)."""
        us = C.c_float()
        self._check(self._L.tw_debug_png_kernel_time(self._h, C.byref(img), waves, iters, C.byref(us)))
        return us.value

    def stage_resize_u8(self, img, dw, dh):
        """The size reconcile's kernel alone (tw_resize_u8): a 2-D uint8 image -> (dh, dw), cv::resize's INTER_LINEAR."""
        img = np.ascontiguousarray(_gray(img))
        sh, sw = img.shape
        out = np.empty((dh, dw), np.uint8)
        self._check(self._L.tw_stage_resize_u8(self._h, _u8(img), sw, sh, _u8(out), dw, dh))
        return out

    def submit_dev(self, d_expect, d_target, w, h, stride, span=10, threshold=5.0, *, flow=None, init=None,
                   target_size=None, target_stride=None):
        """flow, init: as for submit (tw_submit_dev_flow[_init]).  target_size, target_stride: (width, height) and row
        stride of the target's own memory (tw_submit_dev_sized; None: the pair's)."""
        tk = C.c_int64()
        fo = _flow_out(flow, w, h)
        fi, _keep = _flow_in(init, w, h)
        if target_size is not None or target_stride is not None:
            tw_, th_ = target_size if target_size is not None else (w, h)
            self._check(self._L.tw_submit_dev_sized(self._h, d_expect, w, h, stride, d_target, tw_, th_,
                                                    stride if target_stride is None else target_stride, span, threshold,
                                                    C.byref(fi) if fi is not None else None,
                                                    C.byref(fo) if fo is not None else None, C.byref(tk)))
        elif fi is not None:
            self._check(self._L.tw_submit_dev_flow_init(self._h, d_expect, d_target, w, h, stride, span, threshold,
                                                        C.byref(fi), C.byref(fo) if fo is not None else None, C.byref(tk)))
        elif fo is None:
            self._check(self._L.tw_submit_dev(self._h, d_expect, d_target, w, h, stride, span, threshold, C.byref(tk)))
        else:
            self._check(self._L.tw_submit_dev_flow(self._h, d_expect, d_target, w, h, stride, span, threshold,
                                                   C.byref(fo), C.byref(tk)))
        return (tk.value, w, h, span, threshold)

    def flow_batch(self, expects, targets, layout="interleaved", span=0, threshold=5.0, init=None):
        """Dense flow fields of N pairs through the batched API.  numpy inputs (N 2-D uint8 images each): returns a
        page-locked float32 array [N, H, W, 2] ("interleaved") or [N, 2, H, W] ("planar") — freed with the engine —
        and the per-pair result dicts of wait().  torch uint8 tensors [N, H, W] on the engine's device: submitted in place
        (tw_submit_dev_flow), the fields come back as a float32 tensor on that device (a torch program imports torch before
        this module loads the library, as bench.py does: the process's HIP runtime must be torch's).
        init: the pairs' initial flow fields (tw_submit_*_flow_init) — a sequence of N fields (None: that pair starts from
        zero) or one stacked array / tensor [N, ...], each field as submit's init= takes it."""
        if layout not in ("interleaved", "planar"):
            raise TwError(TW_E_BAD_PARAMETER, "layout must be 'interleaved' or 'planar'")
        inter = layout == "interleaved"
        if type(expects).__module__.startswith("torch"):
            import torch
            if expects.shape != targets.shape or expects.dim() != 3 or expects.dtype != torch.uint8:
                raise TwError(TW_E_BAD_IMAGE_FORMAT, "expected two uint8 tensors [N, H, W] of one shape")
            if expects.stride(2) != 1 or targets.stride() != expects.stride():
                expects, targets = expects.contiguous(), targets.contiguous()
            n, h, w = expects.shape
            out = torch.empty((n, h, w, 2) if inter else (n, 2, h, w), dtype=torch.float32, device=expects.device)
            # the ABI takes no stream: the inputs and `out` may still be in flight on torch's stream
            torch.cuda.current_stream(expects.device).synchronize()
            sub = lambda i: self.submit_dev(expects[i].data_ptr(), targets[i].data_ptr(), w, h, expects.stride(1),  # noqa: E731
                                            span, threshold, flow=out[i], init=None if init is None else init[i])
        else:
            a0 = _gray(expects[0])
            n, (h, w) = len(expects), a0.shape
            out = self.host_array((n, h, w, 2) if inter else (n, 2, h, w), np.float32)
            sub = lambda i: self.submit(expects[i], targets[i], span, threshold, flow=out[i],  # noqa: E731
                                        init=None if init is None else init[i])
        if init is not None and len(init) != n:
            raise TwError(TW_E_BAD_PARAMETER, "init: %d fields for %d pairs" % (len(init), n))
        res, pending = [None] * n, []
        for i in range(n):
            if len(pending) >= 2 * self.slots:  # (at most NCTX batches in flight: collect the oldest first)
                j, t = pending.pop(0)
                res[j] = self.wait(t)
            pending.append((i, sub(i)))
        for j, t in pending:
            res[j] = self.wait(t)
        return out, res

    def bench_stage(self, kclass, w, h, level, npairs=1, iters=20, flags=0):
        """Average microseconds per launch of one kernel class on synthetic resident data."""
        us = C.c_float()
        self._check(self._L.tw_bench_stage(self._h, kclass, w, h, level, npairs, iters, flags, C.byref(us)))
        return us.value

    def flush(self):
        self._check(self._L.tw_flush(self._h))

    def level_chunk(self, w, h, level):
        return self._L.tw_level_chunk(self._h, w, h, level)

    def wait(self, ticket, cap=None):
        """cap: room for that many vectors only (None: a grid's worth, which cannot overflow); the result then has "count",
        what tw_wait found, and "vector" holds the first min(count, cap)."""
        tk, w, h, span, threshold = ticket
        given = cap is not None
        if not given:
            cap = max(self._L.tw_grid_capacity(w, h, span), 1)
        out = (Vector * max(cap, 1))()
        n = C.c_int()
        sec = C.c_float()
        self._check(self._L.tw_wait(self._h, tk, out, cap, C.byref(n), C.byref(sec)))
        vec = [(out[i].x, out[i].y, out[i].dx, out[i].dy) for i in range(min(n.value, cap))]
        res = {"status": "OK" if n.value == 0 else "SUSPICIOUS", "span": span, "threshold": threshold,
               "time": sec.value, "height": h, "width": w, "vector": vec}
        if given:
            res["count"] = n.value
        return res

    def set_regions(self, gap):
        """TW_OPT_REGIONS: 0 turns hit regions off (the default), 1 .. 8 is the gap; batches opened from now on take it."""
        self.set_option(OPT_REGIONS, gap)

    def wait_regions(self, ticket, cap=None, region_cap=MAX_REGIONS):
        """tw_wait_regions: (status, vectors, region_of, regions, n_regions) — vectors as wait() returns them (the first
        min(count, cap)), region_of parallel to them, regions the kept records as Region.as_tuple() tuples (x, y, width,
        height, count, peak_x, peak_y, peak_dx, peak_dy), n_regions the pair's true number of regions."""
        tk, w, h, span, threshold = ticket
        if cap is None:
            cap = max(self._L.tw_grid_capacity(w, h, span), 1)
        out = (Vector * max(cap, 1))()
        rof = (C.c_int * max(cap, 1))()
        regs = (Region * max(region_cap, 1))()
        n, nreg, sec = C.c_int(), C.c_int(), C.c_float()
        self._check(self._L.tw_wait_regions(self._h, tk, out, cap, C.byref(n), rof, regs, region_cap, C.byref(nreg),
                                            C.byref(sec)))
        m = min(n.value, cap)
        vec = [(out[i].x, out[i].y, out[i].dx, out[i].dy) for i in range(m)]
        kept = max(0, min(nreg.value, region_cap, MAX_REGIONS))
        return ("OK" if n.value == 0 else "SUSPICIOUS", vec, [int(rof[i]) for i in range(m)],
                [regs[i].as_tuple() for i in range(kept)], nreg.value)

    def set_residual(self, tol):
        """TW_OPT_RESIDUAL: 0 turns the residual off (the default), 1 .. 254 is the tolerance; batches opened from now on
        take it."""
        self.set_option(OPT_RESIDUAL, tol)

    def changes(self, ticket, cap=None):
        """tw_ticket_changes, before the wait that collects the ticket: (records, count) — the first min(count, cap) cells
        with a differing pixel as Change.as_tuple() tuples (x, y, n_diff, n_unexplained, max_diff, max_unexplained) in
        row-major order, and the pair's true count (cap None: a grid's worth, which cannot overflow)."""
        tk, w, h, span, threshold = ticket
        if cap is None:
            cap = max(self._L.tw_grid_capacity(w, h, span), 1)
        out = (Change * max(cap, 1))()
        n = C.c_int()
        self._check(self._L.tw_ticket_changes(self._h, tk, out, cap, C.byref(n)))
        return [out[i].as_tuple() for i in range(max(0, min(n.value, cap)))], n.value

    def set_shift(self, radius):
        """TW_OPT_SHIFT: 0 turns the shift estimation off (the default), 1 .. 1024 is the search radius in pixels; batches
        opened from now on take it."""
        self.set_option(OPT_SHIFT, radius)

    def set_shift_bands(self, band):
        """TW_OPT_SHIFT_BANDS: 0 turns the per-band shifts off (the default), 32 .. 1024 (a multiple of 16) is the band height
        in rows; batches opened from now on take it, and it takes effect in a batch that also has TW_OPT_SHIFT on."""
        self.set_option(OPT_SHIFT_BANDS, band)

    def shift_bands(self, ticket):
        """tw_ticket_shift_bands, before the wait that collects the ticket: the pair's ShiftBand.as_tuple() per band — (y, rows,
        dy, applied, n_shift, n_zero, sad_shift, sad_zero)."""
        n = C.c_int(0)
        self._check(self._L.tw_ticket_shift_bands(self._h, ticket[0], None, 0, C.byref(n)))
        out = (ShiftBand * max(1, n.value))()
        self._check(self._L.tw_ticket_shift_bands(self._h, ticket[0], out, n.value, C.byref(n)))
        return [out[i].as_tuple() for i in range(n.value)]

    def shift(self, ticket):
        """tw_ticket_shift, before the wait that collects the ticket: the pair's Shift.as_tuple() — (dx, dy, applied, n_shift,
        n_zero, sad_shift, sad_zero)."""
        out = Shift()
        self._check(self._L.tw_ticket_shift(self._h, ticket[0], C.byref(out)))
        return out.as_tuple()

    def hits(self, ticket):
        """tw_ticket_hits, before the wait that collects the ticket: the count tw_wait will report for the pair (after the
        ignore rule).  Does not consume the ticket."""
        n = C.c_int(0)
        self._check(self._L.tw_ticket_hits(self._h, ticket[0], C.byref(n)))
        return n.value

    def overlay(self, ticket, tol, out=None, pitch=None):
        """tw_ticket_overlay, before the wait that collects the ticket: the pair's diff image (include/twflow.h, "Diff image")
        as an (h, w, 3) uint8 array.  out None: a fresh numpy array (pageable memory: through the bounce buffer); a uint8
        numpy array of at least pitch * (h - 1) + 3 * w bytes: rendered into it with rows `pitch` bytes apart (default
        3 * w) and returned as a view of its pixels; a raw address (int / c_void_p: device memory, or a tw_host_alloc
        block): rendered there, returns None.  Does not consume the ticket."""
        tk, w, h = ticket[0], ticket[1], ticket[2]
        pitch = 3 * w if pitch is None else int(pitch)
        view = None
        if out is None:
            out = np.empty(pitch * h, np.uint8)
        if isinstance(out, np.ndarray):
            assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= pitch * (h - 1) + 3 * w
            flat = out.reshape(-1)
            view = np.lib.stride_tricks.as_strided(flat, (h, w, 3), (pitch, 3, 1), writeable=False)
            addr = flat.ctypes.data
        else:
            addr = out.value if isinstance(out, C.c_void_p) else int(out)
        oo = OverlayOut(addr, pitch, OVERLAY_RGB8)
        self._check(self._L.tw_ticket_overlay(self._h, tk, int(tol), C.byref(oo)))
        return view

    def overlay_plan(self, expect_addr, target_addr, stride, dst_addr, pitch, w, h):
        """How tw_overlay_base runs for these addresses, strides and size (twflow_debug.h: tw_debug_overlay_plan), a pure host
        function: (vec4, pixels per lane, threads, grid x, grid y)."""
        v = (C.c_int * 5)()
        if self._L.tw_debug_overlay_plan(int(expect_addr), int(target_addr), int(stride), int(dst_addr), int(pitch), int(w),
                                         int(h), v, 5) != 5:
            raise ValueError("no overlay plan for %dx%d" % (w, h))
        return tuple(v)

    def stage_overlay(self, expect, target, rects, hits, regions, tol, pitch=None, stride=None, misalign=0, fill=0xA5):
        """tw_overlay_base and tw_overlay_marks alone: expect / target (h, w) uint8 — with `stride` both are copied into rows
        that far apart first — at device addresses `misalign` bytes off a 256-byte boundary; rects: (x, y, w, h) tuples;
        hits: (x, y, dx, dy) rows (a float32-exact array or tuples); regions: (x, y, width, height) boxes.  Returns (buf,
        path): buf [h, pitch] uint8, pre-filled with `fill` — the picture is buf[:, :3 * w] — and the base kernel's path
        (1: dwords, 0: bytes)."""
        expect = np.ascontiguousarray(expect, np.uint8)
        target = np.ascontiguousarray(target, np.uint8)
        h, w = expect.shape
        assert target.shape == (h, w)
        if stride is None:
            stride = w
        else:
            pe = np.full((h, stride), 0xEE, np.uint8)
            pt = np.full((h, stride), 0xEE, np.uint8)
            pe[:, :w] = expect
            pt[:, :w] = target
            expect, target = pe, pt
        pitch = 3 * w if pitch is None else int(pitch)
        rs = (Rect * max(len(rects), 1))(*[Rect(*(int(v) for v in r)) for r in rects])
        hrec = np.zeros(max(len(hits), 1), OVERLAY_HIT_DTYPE)
        for i, hrow in enumerate(hits):
            hrec[i] = (int(hrow[0]), int(hrow[1]), np.float32(hrow[2]), np.float32(hrow[3]))
        regs = (Region * max(len(regions), 1))()
        for i, r in enumerate(regions):
            regs[i].x, regs[i].y, regs[i].width, regs[i].height = (int(v) for v in r[:4])
        buf = np.full((h, max(pitch, 0)), fill, np.uint8)
        path = C.c_int(-1)
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.tw_stage_overlay(self._h, expect.ctypes.data_as(u8p), target.ctypes.data_as(u8p), w, h, stride,
                                             int(misalign), rs, len(rects), hrec.ctypes.data_as(C.c_void_p), len(hits), regs,
                                             len(regions), int(tol), buf.ctypes.data_as(u8p), pitch, C.byref(path)))
        return buf, path.value

    def wait_count(self, ticket):
        """tw_wait without materialising the vectors (bench inner loop). Returns (n, seconds)."""
        tk = ticket[0]
        n = C.c_int()
        sec = C.c_float()
        self._check(self._L.tw_wait(self._h, tk, None, 0, C.byref(n), C.byref(sec)))
        return n.value, sec.value

    # ---- device memory --------------------------------------------------------------------------------
    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        d = C.c_void_p()
        self._check(self._L.tw_dev_alloc(self._h, arr.nbytes, C.byref(d)))
        self._devbufs.append(d)
        self._check(self._L.tw_dev_upload(self._h, d, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return d

    def set_option(self, option, value):
        self._check(self._L.tw_set_option(self._h, option, int(value)))

    def host_array(self, shape, dtype=np.uint8):
        """Array in page-locked memory (tw_host_alloc): submit() DMAs straight from it, without staging, and it can take
        a flow field (dtype float32).  Freed with the engine."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        h = C.c_void_p()
        self._check(self._L.tw_host_alloc(self._h, n, C.byref(h)))
        self._hostbufs.append(h)
        return np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_uint8)), shape=(n,)).view(dt).reshape(shape)

    def dev_download(self, dptr, nbytes):
        """tw_dev_download: nbytes of device memory as a uint8 numpy array."""
        out = np.empty(nbytes, np.uint8)
        self._check(self._L.tw_dev_download(self._h, out.ctypes.data_as(C.c_void_p), dptr, nbytes))
        return out

    # ---- instrumentation -------------------------------------------------------------------------------
    def prof_select(self, kclass, level=-1):
        self._check(self._L.tw_prof_select(self._h, kclass, level))

    def copy_rate_gbps(self, nbytes=1 << 30, reps=10):
        """The yardstick: GB/s (read + write) of a float4 device copy kernel on this engine's stream (twflow_debug.h)."""
        g = C.c_double()
        self._check(self._L.tw_debug_copy_rate(self._h, nbytes, reps, C.byref(g)))
        return g.value

    def prof_read(self, kclass):
        ms = C.c_double()
        n = C.c_int()
        self._check(self._L.tw_prof_read(self._h, kclass, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def algorithmic_bytes(self, kclass, level, w, h, npairs=None):
        """Bytes one launch of `kclass` at `level` must move per pair; npairs: the batch (default: the engine's slots)."""
        if npairs is None:
            return self._L.tw_algorithmic_bytes(self._h, kclass, level, w, h)
        return self._L.tw_algorithmic_bytes_launch(self._h, kclass, level, w, h, npairs)

    def level_runs_flow_iter(self, w, h, level, npairs):
        """Does `level` of a batch of npairs pairs run tw_flow_iter (the schedule's own predicate)?"""
        return self._L.tw_level_runs_flow_iter(self._h, w, h, level, npairs) == 1

    def flow_iter_plan(self, w, h, npairs=1):
        """Geometry of a tw_flow_iter launch of npairs pairs at a level of w x h pixels, from the function the launch
        itself uses (twflow_debug.h: tw_debug_flow_iter_plan): strips, segments per strip, steps of 5 rows per segment,
        steps of the last segment."""
        v = (C.c_int * 4)()
        n = self._L.tw_debug_flow_iter_plan(self._h, w, h, npairs, v, 4)
        if n != 4:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_flow_iter_plan(%d, %d, %d) returned %d" % (w, h, npairs, n))
        return FlowIterPlan(*v)

    def blur_plan(self, w, h, level=-1, npairs=1, update=False, quads=False):
        """The choice of one window average + solve launch at a level of w x h pixels, from the function the launch itself
        uses (twflow_debug.h: tw_debug_blur_plan): the kernel's family name, threads, tile columns, rows per workgroup, xsh,
        grid x / y, the small-grid class and whether TW_BLUR_SMALL / TW_BLUR_SMALL_LEVELS forced it."""
        v = (C.c_int * 9)()
        n = self._L.tw_debug_blur_plan(self._h, w, h, level, npairs, int(bool(update)), int(bool(quads)), v, 9)
        if n != 9:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_blur_plan(%d, %d, %d, %d) returned %d" % (w, h, level, npairs, n))
        return BlurPlan(self._L.tw_debug_family_name(v[0]).decode(), *v[1:8], bool(v[8]))

    def pyr_plan(self, w, h, level, stride=None):
        """The choice of one pyramid level's launch at `level` of a w x h image (rows `stride` bytes apart, default w), from
        the function the launch itself uses (twflow_debug.h: tw_debug_pyr_plan): the kernel's name and template argument,
        its launch-count family, threads, output-tile columns and rows, grid x / y, dynamic LDS bytes, staged-row pitch,
        aligned4 (whole-dword loads of the source rows: answered for images at 4-byte-aligned addresses, so the stride alone
        decides, and nothing the engine ran before changes it), the level's width, height, taps, resize mode, xmax and
        row-buffer height, whether the size is eligible
        for tw_pyr_23 / tw_pyr_k3f, tw_pyr_23's threads for one pair / a batch, the coarsest level's index, the output rows
        whose lower source row is clipped to the image's last row."""
        v = (C.c_int * 23)()
        n = self._L.tw_debug_pyr_plan(self._h, w, h, level, w if stride is None else stride, v, 23)
        if n != 23:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_pyr_plan(%d, %d, %d) returned %d" % (w, h, level, n))
        return PyrPlan(PYR_KERNELS[v[0]], v[1], self._L.tw_debug_family_name(v[2]).decode(), *v[3:10], bool(v[10]), *v[11:17],
                       bool(v[17]), bool(v[18]), *v[19:23])

    def scan_plan(self, w, h, span, npairs=1, single_pair=False):
        """The choice of the ordered scan's launch for npairs pairs of w x h pixels at `span`, from the function the launch
        itself uses (twflow_debug.h: tw_debug_scan_plan): the kernel's family name, the grid's width, height and points G,
        the points S of a segment and the segments (0 for tw_span_scan), the rounds of 32 768 points a workgroup runs."""
        v = (C.c_int * 7)()
        n = self._L.tw_debug_scan_plan(self._h, w, h, int(span), npairs, int(bool(single_pair)), v, 7)
        if n != 7:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_scan_plan(%d, %d, %d, %d) returned %d" % (w, h, span, npairs, n))
        return ScanPlan(("tw_span_scan", "tw_span_scan_seg")[v[0]], *v[1:7])

    def level_plan(self, w, h, span, npairs, any_fout=False, any_init=False, prof_on=False, residual=False, shift=False):
        """What a batch of npairs pairs of w x h pixels at `span` launches for each pyramid level, from the function the
        enqueue itself executes (twflow_debug.h: tw_debug_level_plan): a LevelPlanView whose `parts` (a lane's share of the
        batch each) hold one LevelPlanRow per level, level 0 first."""
        cap = 8 + 2 * 61 * 11
        v = (C.c_int * cap)()
        # (a batch opened with TW_OPT_SHIFT on takes the schedule a batch with an initial field takes)
        traits = (1 if any_fout else 0) | (2 if any_init or shift else 0) | (4 if prof_on else 0) | (16 if residual else 0)
        n = self._L.tw_debug_level_plan(self._h, w, h, int(span), npairs, traits, v, cap)
        if n < 8 or v[7] != 11 or n != 8 + v[6] * (v[2] + 1) * 11:
            raise TwError(TW_E_BAD_PARAMETER, "tw_debug_level_plan(%d, %d, %d, %d) returned %d" % (w, h, span, npairs, n))
        rows = [LevelPlanRow(*(v[8 + 11 * i + j] if j < 5 else bool(v[8 + 11 * i + j]) for j in range(11)))
                for i in range(v[6] * (v[2] + 1))]
        parts = [rows[p * (v[2] + 1):(p + 1) * (v[2] + 1)] for p in range(v[6])]
        return LevelPlanView(("batch", "two_stream", "twin")[v[0]], v[1], v[2], bool(v[3]), bool(v[4]), bool(v[5]), parts)

    def same_flags(self):
        """tw_pair_same's flags of the batch enqueued last, one per pair: 1 where the pair's second image is byte for byte
        its first (twflow_debug.h: tw_debug_same_flags); all 0 when no tw_pair_same ran (TW_SAME_IMAGE=0, a single pair).
        A debug hook on engine-level state: it describes whichever batch the engine enqueued LAST (a full batch, or the
        one a wait() flushed), not a ticket — ask before the next submit fills another batch.  Waits for that batch."""
        v = (C.c_uint * self.slots)()
        n = self._L.tw_debug_same_flags(self._h, v, self.slots)
        if n < 0:
            raise TwError(TW_E_DEVICE, "tw_debug_same_flags returned %d" % n)
        return [int(v[i]) for i in range(n)]

    def launch_counts(self, reset=False):
        """{family name: launches} since creation / the last reset, every family (twflow_debug.h)."""
        n = self._L.tw_debug_launch_counts(self._h, None, None, 0, 0)
        cnt = (C.c_uint64 * n)()
        z = (C.c_uint64 * n)()
        self._L.tw_debug_launch_counts(self._h, cnt, z, n, 1 if reset else 0)
        out = LaunchCounts((self._L.tw_debug_family_name(i).decode(), int(cnt[i])) for i in range(n))
        out.last_z = {self._L.tw_debug_family_name(i).decode(): int(z[i]) for i in range(n)}
        return out

    def memory(self):
        """The library's own byte accounting of this engine (twflow_debug.h: tw_debug_memory)."""
        v = (C.c_uint64 * 8)()
        n = self._L.tw_debug_memory(self._h, v, 8)
        keys = ("device_bytes", "pinned_host_bytes", "plans", "bounce_bytes", "pagelock_entries", "pagelock_bytes",
                "prof_events", "graphs")
        return {k: int(v[i]) for i, k in enumerate(keys[:n])}

    def algorithmic_bytes_pair(self, w, h, span):
        return self._L.tw_algorithmic_bytes_pair(self._h, w, h, span)

    def min_traffic_bytes_pair(self, w, h, span):
        return self._L.tw_min_traffic_bytes_pair(self._h, w, h, span)

    def num_levels(self, w, h):
        return self._L.tw_num_levels(self._h, w, h)

    # ---- per-stage entry points (planar layouts) ----------------------------------------------------
    def stage_pyr_level(self, img, level):
        img = np.ascontiguousarray(_gray(img))
        h0, w0 = img.shape
        buf = np.empty(h0 * w0, np.float32)
        w, h = C.c_int(), C.c_int()
        self._check(self._L.tw_stage_pyr_level(self._h, _u8(img), w0, h0, level, _f(buf), C.byref(w), C.byref(h)))
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def stage_pyr_fused23(self, img):
        """Levels 3 and 2 from the one-read kernel (tw_pyr_23); raises TwError(TW_E_UNSUPPORTED) for sizes without exact
        reductions by 4 and 8."""
        img = np.ascontiguousarray(_gray(img))
        h0, w0 = img.shape
        I3 = np.empty((h0 // 8, w0 // 8), np.float32)
        I2 = np.empty((h0 // 4, w0 // 4), np.float32)
        self._check(self._L.tw_stage_pyr_fused23(self._h, _u8(img), w0, h0, _f(I3), _f(I2)))
        return I3, I2

    def stage_pyr_fused01(self, img):
        """Levels 0 and 1 from one read of the image (tw_pyr_k3f); TwError(TW_E_UNSUPPORTED) unless level 1 is an exact halving."""
        img = np.ascontiguousarray(_gray(img))
        h0, w0 = img.shape
        I0 = np.empty((h0, w0), np.float32)
        I1 = np.empty((h0 // 2, w0 // 2), np.float32)
        self._check(self._L.tw_stage_pyr_fused01(self._h, _u8(img), w0, h0, _f(I0), _f(I1)))
        return I0, I1

    def stage_polyexp(self, I):
        I = np.ascontiguousarray(I, np.float32)
        h, w = I.shape
        R = np.empty((5, h, w), np.float32)
        self._check(self._L.tw_stage_polyexp(self._h, _f(I), w, h, _f(R)))
        return R

    def stage_update_matrices(self, R0, R1, flow):
        R0 = np.ascontiguousarray(R0, np.float32)
        R1 = np.ascontiguousarray(R1, np.float32)
        flow = np.ascontiguousarray(flow, np.float32)
        _, h, w = R0.shape
        M = np.empty((5, h, w), np.float32)
        self._check(self._L.tw_stage_update_matrices(self._h, _f(R0), _f(R1), _f(flow), w, h, _f(M)))
        return M

    def stage_flow_upsample_update(self, R0, R1, prevflow):
        R0 = np.ascontiguousarray(R0, np.float32)
        R1 = np.ascontiguousarray(R1, np.float32)
        prevflow = np.ascontiguousarray(prevflow, np.float32)
        _, h, w = R0.shape
        _, ph, pw = prevflow.shape
        flow = np.empty((2, h, w), np.float32)
        M = np.empty((5, h, w), np.float32)
        self._check(self._L.tw_stage_flow_upsample_update(self._h, _f(R0), _f(R1), _f(prevflow), pw, ph, w, h,
                                                          _f(flow), _f(M)))
        return flow, M

    def stage_flow_iter(self, R0, R1, flow=None, prev=None):
        """One whole iteration without M in memory (tw_flow_iter): input flow = `flow` (2, h, w), or the coarser level's
        flow `prev` (2, ph, pw) upsampled, or zero."""
        R0 = np.ascontiguousarray(R0, np.float32)
        R1 = np.ascontiguousarray(R1, np.float32)
        _, h, w = R0.shape
        out = np.empty((2, h, w), np.float32)
        fin = None if flow is None else np.ascontiguousarray(flow, np.float32)
        pv = None if prev is None else np.ascontiguousarray(prev, np.float32)
        ph, pw = (pv.shape[1], pv.shape[2]) if pv is not None else (0, 0)
        null = C.POINTER(C.c_float)()
        self._check(self._L.tw_stage_flow_iter(self._h, _f(R0), _f(R1), _f(fin) if fin is not None else null,
                                               _f(pv) if pv is not None else null, pw, ph, w, h, _f(out)))
        return out

    def stage_flow_iter_grid(self, R0, R1, flow, span):
        """The same iteration from `flow` (2, h, w), evaluated at the span-grid points only (tw_flow_iter's grid-only mode):
        (ceil(h / span), ceil(w / span), 2) — (dx, dy) of the points (gx * span, gy * span)."""
        R0 = np.ascontiguousarray(R0, np.float32)
        R1 = np.ascontiguousarray(R1, np.float32)
        flow = np.ascontiguousarray(flow, np.float32)
        _, h, w = R0.shape
        out = np.empty((-(-h // span), -(-w // span), 2), np.float32)
        self._check(self._L.tw_stage_flow_iter_grid(self._h, _f(R0), _f(R1), _f(flow), w, h, int(span), _f(out)))
        return out

    def stage_span_scan(self, fields, span, threshold, single_pair=False):
        """The span-grid scan alone (tw_span_gather + the ordered scan scan_plan names) on `fields` (npairs, 2, h, w):
        (counts [npairs] int32, xy [npairs, G, 2] int32, dxy [npairs, G, 2] float32) — every pair's whole record region;
        what the kernels did not write holds 0xff bytes (a count of -1)."""
        fields = np.ascontiguousarray(fields, np.float32)
        npairs, two, h, w = fields.shape
        assert two == 2
        sp = max(int(span), 1)  # (a span below 1 is the library's to refuse)
        G = (-(-h // sp)) * (-(-w // sp))
        counts = np.zeros(npairs, np.int32)
        xy = np.zeros((npairs, G, 2), np.int32)
        dxy = np.zeros((npairs, G, 2), np.float32)
        self._check(self._L.tw_stage_span_scan(self._h, _f(fields), npairs, w, h, int(span), float(threshold),
                                               int(bool(single_pair)), counts.ctypes.data_as(C.POINTER(C.c_int)),
                                               xy.ctypes.data_as(C.POINTER(C.c_int)), _f(dxy)))
        return counts, xy, dxy

    def stage_warp_residual(self, expect, target, flow2, span, tol, stride=None):
        """tw_warp_residual and tw_change_scan alone: expect / target (h, w) uint8 — with `stride` both are copied into
        rows that far apart first — flow2 (2, h, w) float32.  (cells [G, 4] int32, n_changes, changes [G, 6] int32: x, y,
        n_diff, n_unexplained, max_diff, max_unexplained); what the launches did not write holds 0xff bytes."""
        expect = np.ascontiguousarray(expect, np.uint8)
        target = np.ascontiguousarray(target, np.uint8)
        flow2 = np.ascontiguousarray(flow2, np.float32)
        h, w = expect.shape
        assert target.shape == (h, w) and flow2.shape == (2, h, w)
        if stride is None:
            stride = w
        else:
            pe = np.full((h, stride), 0xA5, np.uint8)
            pt = np.full((h, stride), 0x5A, np.uint8)
            pe[:, :w] = expect
            pt[:, :w] = target
            expect, target = pe, pt
        sp = max(int(span), 1)
        G = (-(-h // sp)) * (-(-w // sp))
        cells = np.zeros((G, 4), np.int32)
        chg = np.zeros((G, 6), np.int32)
        n = C.c_int(0)
        u8p, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int)
        self._check(self._L.tw_stage_warp_residual(self._h, expect.ctypes.data_as(u8p), target.ctypes.data_as(u8p), stride, w, h,
                                                   _f(flow2), int(span), int(tol), cells.ctypes.data_as(ip), C.byref(n),
                                                   chg.ctypes.data_as(C.POINTER(Change))))
        return cells, n.value, chg

    def stage_shift(self, expect, target, radius, stride=None, force_global=False, pad=0xEE):
        """tw_shift_profiles, tw_shift_search and tw_shift_verify alone: expect / target (h, w) uint8 — with `stride` both are
        copied into rows that far apart first, the padding filled with `pad`.  (profiles: (colE [w], colT [w], rowE [h], rowT [h])
        uint32, the record as Shift.as_tuple()).  The call itself answers a device error when a launch wrote beyond the pair's
        share of the 0xff-filled outputs."""
        expect = np.ascontiguousarray(expect, np.uint8)
        target = np.ascontiguousarray(target, np.uint8)
        h, w = expect.shape
        assert target.shape == (h, w)
        if stride is None:
            stride = w
        else:
            pe = np.full((h, stride), pad, np.uint8)
            pt = np.full((h, stride), pad, np.uint8)
            pe[:, :w] = expect
            pt[:, :w] = target
            expect, target = pe, pt
        prof = np.zeros(2 * (w + h), np.uint32)
        out = Shift()
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.tw_stage_shift(self._h, expect.ctypes.data_as(u8p), target.ctypes.data_as(u8p), stride, w, h,
                                           int(radius), int(bool(force_global)), prof.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           C.byref(out)))
        return (prof[:w], prof[w:2 * w], prof[2 * w:2 * w + h], prof[2 * w + h:]), out.as_tuple()

    def stage_shift_bands(self, expect, target, radius, band, stride=None, force_global=False, pad=0xEE):
        """The global estimation, then tw_band_rows, tw_band_search and tw_band_verify alone (tw_stage_shift_bands): expect /
        target (h, w) uint8, strided as in stage_shift.  ((sigE, sigT) each (h, nblk) uint16 at the pair's dx, the global record
        as Shift.as_tuple(), the band records as ShiftBand.as_tuple() each).  The call itself answers a device error when a
        launch wrote beyond the pair's share of the 0xff-filled outputs."""
        expect = np.ascontiguousarray(expect, np.uint8)
        target = np.ascontiguousarray(target, np.uint8)
        h, w = expect.shape
        assert target.shape == (h, w)
        if stride is None:
            stride = w
        else:
            pe = np.full((h, stride), pad, np.uint8)
            pt = np.full((h, stride), pad, np.uint8)
            pe[:, :w] = expect
            pt[:, :w] = target
            expect, target = pe, pt
        nblk0, nb = (w + 63) // 64, (h + int(band) - 1) // int(band)
        sig = np.zeros(2 * h * nblk0, np.uint16)
        glob = Shift()
        bands = (ShiftBand * nb)()
        n = C.c_int(0)
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.tw_stage_shift_bands(self._h, expect.ctypes.data_as(u8p), target.ctypes.data_as(u8p), stride, w, h,
                                                 int(radius), int(band), int(bool(force_global)),
                                                 sig.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(glob), bands, C.byref(n)))
        assert n.value == nb
        dx = glob.dx
        nblk = (min(w, w - dx) - max(0, -dx) + 63) // 64
        sig = sig[:2 * h * nblk].reshape(2, h, nblk)
        return (sig[0], sig[1]), glob.as_tuple(), [bands[i].as_tuple() for i in range(nb)]

    def band_plan(self, w, h, radius, band):
        """How the band launches run for a w x h pair at `radius` and band height `band` (twflow_debug.h: tw_debug_band_plan), a
        pure host function."""
        v = (C.c_int * 9)()
        if self._L.tw_debug_band_plan(int(w), int(h), int(radius), int(band), v, 9) != 9:
            raise ValueError("no band plan for %dx%d at radius %d, band %d" % (w, h, radius, band))
        return BandPlan(v[0], v[1], bool(v[2]), *v[3:9])

    def shift_plan(self, w, h, radius):
        """How tw_shift_search runs for a w x h pair at `radius` (twflow_debug.h: tw_debug_shift_plan), a pure host function."""
        v = (C.c_int * 10)()
        if self._L.tw_debug_shift_plan(int(w), int(h), int(radius), v, 10) != 10:
            raise ValueError("no shift plan for %dx%d at radius %d" % (w, h, radius))
        return ShiftPlan(bool(v[0]), bool(v[1]), *v[2:10])

    def stage_hit_regions(self, fields, span, threshold, gap, ignore=None):
        """tw_hit_regions alone behind the gather and the ordered scan on `fields` (npairs, 2, h, w); ignore: per pair a
        list of (x, y, w, h), or None.  (n_regions [npairs] int32, regions [npairs, MAX_REGIONS] structured (the fields of
        tw_region), region_of [npairs, G] int32); what the launch did not write holds 0xff bytes."""
        fields = np.ascontiguousarray(fields, np.float32)
        npairs, two, h, w = fields.shape
        assert two == 2
        sp = max(int(span), 1)
        G = (-(-h // sp)) * (-(-w // sp))
        nreg = np.zeros(npairs, np.int32)
        regs = np.zeros((npairs, MAX_REGIONS), REGION_DTYPE)
        rof = np.zeros((npairs, G), np.int32)
        rects, nign = None, None
        if ignore is not None:
            assert len(ignore) == npairs
            rects = (Rect * (MAX_IGNORE * npairs))()
            nign = (C.c_int * npairs)()
            for j, rs in enumerate(ignore):
                nign[j] = len(rs)
                for i, r in enumerate(rs[:MAX_IGNORE]):
                    rects[j * MAX_IGNORE + i] = Rect(*(int(v) for v in r))
        ip = C.POINTER(C.c_int)
        self._check(self._L.tw_stage_hit_regions(self._h, _f(fields), npairs, w, h, int(span), float(threshold), int(gap),
                                                 rects, nign, nreg.ctypes.data_as(ip),
                                                 regs.ctypes.data_as(C.POINTER(Region)), rof.ctypes.data_as(ip)))
        return nreg, regs, rof

    def stage_blur_solve(self, R0, R1, M, update_matrices):
        R0 = np.ascontiguousarray(R0, np.float32)
        R1 = np.ascontiguousarray(R1, np.float32)
        M = np.ascontiguousarray(M, np.float32)
        _, h, w = R0.shape
        flow = np.empty((2, h, w), np.float32)
        Mo = np.empty((5, h, w), np.float32)
        self._check(self._L.tw_stage_blur_solve(self._h, _f(R0), _f(R1), _f(M), w, h, int(bool(update_matrices)),
                                                _f(flow), _f(Mo)))
        return flow, (Mo if update_matrices else None)
