"""Resident images (tw_image_*, tw_submit_image_png / _jpeg, tw_debug_resident): the ABI side, no GPU.
The device side is tests/test_gpu_resident.py, the host layer tests/test_host_resident.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tw_image_keep", "tw_image_create_u8", "tw_image_release", "tw_image_size", "tw_submit_image_png",
               "tw_submit_image_jpeg", "tw_debug_resident")


def _declared():
    syms = set()
    for fn in ("twflow.h", "twflow_debug.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fn)).read(), flags=re.S)
        syms |= set(re.findall(r"\b(tw_[a-z0-9_]+)\s*\(", txt))
    return syms


def _cc():
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    return cc


def test_new_symbols_declared_exported_and_bound(twflow):
    L = twflow.lib()
    decl = _declared()
    for s in NEW_SYMBOLS:
        assert s in decl, s
        assert hasattr(L, s), s
        assert s in twflow.SYMBOLS, s
    assert set(twflow.SYMBOLS) == decl
    for name in ("image", "keep", "submit_image", "resident"):
        assert callable(getattr(twflow.Engine, name)), name
    assert callable(twflow.Image.release) and isinstance(twflow.Image.size, property)
    assert (twflow.KEEP_EXPECT, twflow.KEEP_TARGET) == (0, 1)


def test_abi_version_is_unchanged(twflow):
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr)
    assert twflow.abi_version() == 4  # additive within ABI 4: detected by the symbols


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, const unsigned char* a, const tw_png_rows* p, const tw_jpeg_luma* j,\n"
                   "      const tw_flow_in* i, const tw_flow_out* o, tw_ticket* t) {\n"
                   "  tw_image* img = 0;\n"
                   "  int w, h;\n"
                   "  unsigned long long r4[4];\n"
                   "  int r = tw_image_create_u8(e, a, 8, 8, 8, &img);\n"
                   "  r += tw_image_keep(e, *t, TW_KEEP_EXPECT, &img) + tw_image_keep(e, *t, TW_KEEP_TARGET, &img);\n"
                   "  r += tw_image_size(e, img, &w, &h);\n"
                   "  r += tw_submit_image_png(e, img, p, 10, 5.0, i, o, t);\n"
                   "  r += tw_submit_image_jpeg(e, img, j, 10, 5.0, i, o, t);\n"
                   "  r += tw_debug_resident(e, r4);\n"
                   "  return r + tw_image_release(e, img); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])


# sizeof, then the offset of every field, as the header of ABI 4 has laid them out on LP64 since each struct was added
LAYOUTS = {
    "tw_params": (40, ("pyrScale", 0), ("pyrLevels", 8), ("winSize", 12), ("pyrIterations", 16), ("polyN", 20),
                  ("polySigma", 24), ("flags", 32)),
    "tw_vector": (24, ("x", 0), ("y", 4), ("dx", 8), ("dy", 16)),
    "tw_flow_out": (24, ("data", 0), ("pitch", 8), ("layout", 16)),
    "tw_flow_in": (24, ("data", 0), ("pitch", 8), ("layout", 16)),
    "tw_png_rows": (40, ("rows", 0), ("width", 8), ("height", 12), ("color_type", 16), ("bit_depth", 20), ("palette", 24),
                    ("palette_entries", 32)),
    "tw_jpeg_luma": (160, ("coef", 0), ("gray", 8), ("width", 16), ("height", 20), ("blocks_w", 24), ("blocks_h", 28),
                     ("quant", 32)),
}


def test_existing_structs_keep_their_layout(tmp_path, twflow):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "twflow.h"', "int main(void) {"]
    for name, (size, *fields) in LAYOUTS.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in fields:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (name, f))
        lines.append('  printf("\\n");')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe], text=True).splitlines():
        name, *nums = ln.split()
        got[name] = [int(v) for v in nums]
    for name, (size, *fields) in LAYOUTS.items():
        assert got[name] == [size] + [off for _, off in fields], name
    # ... and the binding's structures are those
    for cls, name in ((twflow.Params, "tw_params"), (twflow.Vector, "tw_vector"), (twflow.FlowOut, "tw_flow_out"),
                      (twflow.FlowIn, "tw_flow_in"), (twflow.PngRows, "tw_png_rows"), (twflow.JpegLuma, "tw_jpeg_luma")):
        size, *fields = LAYOUTS[name]
        assert C.sizeof(cls) == size, name
        assert [(f, getattr(cls, f).offset) for f, _ in fields] == list(fields), name


def test_null_arguments_are_refused_without_a_device(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    img = (C.c_uint8 * 64)()
    out = C.c_void_p(0x1234)
    tk = C.c_int64(77)
    w, h = C.c_int(-1), C.c_int(-1)
    assert L.tw_image_keep(None, 1, 0, C.byref(out)) == bad
    assert L.tw_image_create_u8(None, img, 8, 8, 8, C.byref(out)) == bad
    assert L.tw_image_release(None, None) == bad
    assert L.tw_image_release(None, out) == bad
    assert L.tw_image_size(None, out, C.byref(w), C.byref(h)) == bad
    assert (w.value, h.value) == (-1, -1)
    rows = twflow.PngRows(img, 8, 8)
    assert L.tw_submit_image_png(None, out, C.byref(rows), 4, 0.0, None, None, C.byref(tk)) == bad
    luma = twflow.JpegLuma.from_gray(np.zeros((8, 8), np.uint8))
    assert L.tw_submit_image_jpeg(None, out, C.byref(luma), 4, 0.0, None, None, C.byref(tk)) == bad
    assert tk.value == 77  # (no ticket written)
    v = (C.c_uint64 * 4)()
    assert L.tw_debug_resident(None, v) == -1
