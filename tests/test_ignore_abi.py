"""Ignore regions (tw_rect, the tw_submit_*_ignore calls, tw_stage_mask_rects, TW_DF_MASK_RECTS): the ABI side, no GPU.
The device side is tests/test_gpu_ignore.py, the host layer tests/test_host_ignore.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tw_submit_u8_ignore", "tw_submit_png_ignore", "tw_submit_jpeg_ignore", "tw_submit_image_png_ignore",
               "tw_submit_image_jpeg_ignore", "tw_stage_mask_rects")


def _cc():
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    return cc


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
    assert callable(twflow.Engine.stage_mask_rects)
    assert twflow.MAX_IGNORE == 32


def test_abi_version_is_unchanged(twflow):
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr)
    assert twflow.abi_version() == 4  # additive within ABI 4: detected by the symbols


def test_header_compiles_as_c99_and_tw_rect_is_16_bytes(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, const unsigned char* a, unsigned char* out, const tw_png_rows* p, const tw_jpeg_luma* j,\n"
                   "      const tw_image* img, const tw_flow_in* i, const tw_flow_out* o, tw_ticket* t) {\n"
                   "  tw_rect r[TW_MAX_IGNORE];\n"
                   "  int n;\n"
                   "  r[0].x = r[0].y = -1; r[0].width = r[0].height = 4; r[1] = r[0];\n"
                   "  n = tw_submit_u8_ignore(e, a, 8, 8, 8, a, 8, 8, 8, 10, 5.0, i, o, r, 2, t);\n"
                   "  n += tw_submit_png_ignore(e, p, p, 10, 5.0, i, o, r, 2, t);\n"
                   "  n += tw_submit_jpeg_ignore(e, j, j, 10, 5.0, i, o, r, 2, t);\n"
                   "  n += tw_submit_image_png_ignore(e, img, p, 10, 5.0, i, o, r, 2, t);\n"
                   "  n += tw_submit_image_jpeg_ignore(e, img, j, 10, 5.0, i, o, 0, 0, t);\n"
                   "  return n + tw_stage_mask_rects(e, a, a, 8, 8, r, 1, out, 0); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(tw_rect), offsetof(tw_rect, x), offsetof(tw_rect, y),\n'
                   "         offsetof(tw_rect, width), offsetof(tw_rect, height), (int)TW_MAX_IGNORE, (int)TW_DF_MASK_RECTS,\n"
                   "         (int)TW_DF_JPEG_IDCT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:6] == [16, 0, 4, 8, 12, 32]
    assert got[6] == got[7] + 1  # TW_DF_MASK_RECTS sits directly after TW_DF_JPEG_IDCT
    assert C.sizeof(twflow.Rect) == 16
    assert [(f, getattr(twflow.Rect, f).offset) for f in ("x", "y", "width", "height")] == \
        [("x", 0), ("y", 4), ("width", 8), ("height", 12)]
    # ... and the library's family table agrees with the header
    L = twflow.lib()
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert names[got[7]] == "tw_jpeg_idct" and names[got[6]] == "tw_mask_rects"
    assert len(set(names)) == len(names)  # every family has a name of its own
    assert names.index("tw_pair_same") == got[6] + 1  # (and the families behind it follow as before)
    assert names[-3:] == ["tw_resize_u8", "tw_flow_area_init", "tw_flow_export"]


def test_null_engine_is_refused_by_every_new_call(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    img = (C.c_uint8 * 64)()
    out = (C.c_uint8 * 64)()
    handle = C.c_void_p(0x1234)
    tk = C.c_int64(77)
    rects = (twflow.Rect * 1)(twflow.Rect(1, 1, 2, 2))
    rows = twflow.PngRows(img, 8, 8)
    luma = twflow.JpegLuma.from_gray(np.zeros((8, 8), np.uint8))
    for rs, n in ((rects, 1), (None, 0)):
        assert L.tw_submit_u8_ignore(None, img, 8, 8, 8, img, 8, 8, 8, 4, 0.0, None, None, rs, n, C.byref(tk)) == bad
        assert L.tw_submit_png_ignore(None, C.byref(rows), C.byref(rows), 4, 0.0, None, None, rs, n, C.byref(tk)) == bad
        assert L.tw_submit_jpeg_ignore(None, C.byref(luma), C.byref(luma), 4, 0.0, None, None, rs, n, C.byref(tk)) == bad
        assert L.tw_submit_image_png_ignore(None, handle, C.byref(rows), 4, 0.0, None, None, rs, n, C.byref(tk)) == bad
        assert L.tw_submit_image_jpeg_ignore(None, handle, C.byref(luma), 4, 0.0, None, None, rs, n, C.byref(tk)) == bad
        assert L.tw_stage_mask_rects(None, img, img, 8, 8, rs, n, out, None) == bad
    assert tk.value == 77  # (no ticket written)
