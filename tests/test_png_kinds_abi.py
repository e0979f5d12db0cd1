"""PNG kinds on the device (tw_png_on_device, tw_submit_png, tw_stage_png_decode): the ABI side, no GPU.  The device side
is tests/test_gpu_png_kinds.py, the host layer on the stub backend tests/test_host_png_kinds.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tw_png_on_device", "tw_submit_png", "tw_stage_png_decode")


def on_device(color_type, depth, interlace):
    """The table of the issue: non-interlaced; gray 1/2/4/8/16, palette 1/2/4/8, gray + alpha 8/16, RGB and RGBA 8."""
    if interlace != 0:
        return False
    return depth in {0: (1, 2, 4, 8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 2: (8,), 6: (8,)}.get(color_type, ())


def test_png_on_device_over_every_triple(twflow):
    L = twflow.lib()
    for ct in range(8):
        for depth in range(18):
            for il in range(3):
                want = on_device(ct, depth, il)
                assert bool(L.tw_png_on_device(ct, depth, il)) == want, (ct, depth, il)
                assert twflow.png_on_device(ct, depth, il) == want
    assert twflow.png_on_device(3, 4) and not twflow.png_on_device(2, 16)
    assert not twflow.png_on_device(twflow.PNG_PLAIN_GRAY, 8)


def test_new_symbols_declared_exported_and_bound(twflow):
    L = twflow.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "twflow.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(tw_[a-z0-9_]+)\s*\(", txt))
    for s in NEW_SYMBOLS:
        assert s in decl, s
        assert hasattr(L, s), s
        assert s in twflow.SYMBOLS, s
    assert twflow.abi_version() == 4  # additive within ABI 4
    assert C.sizeof(twflow.PngRows) == 40 and twflow.PngRows.palette.offset == 24  # tw_png_rows on LP64


def test_header_with_png_rows_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   "int f(tw_engine* e, const unsigned char* rows, const unsigned char* plte, unsigned char* gray, tw_ticket* t) {\n"
                   "  tw_png_rows a, b;\n"
                   "  a.rows = rows; a.width = 8; a.height = 8; a.color_type = 3; a.bit_depth = 2; a.palette = plte;\n"
                   "  a.palette_entries = 4;\n"
                   "  b.rows = rows; b.width = 5; b.height = 11; b.color_type = TW_PNG_PLAIN_GRAY; b.bit_depth = 8;\n"
                   "  b.palette = 0; b.palette_entries = 0;\n"
                   "  if (!tw_png_on_device(a.color_type, a.bit_depth, 0)) return -1;\n"
                   "  return (int)tw_submit_png(e, &a, &b, 10, 5.0, 0, 0, t) + (int)tw_stage_png_decode(e, &a, 0, gray); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])


def test_null_arguments_are_refused(twflow):
    L = twflow.lib()
    tk = C.c_int64()
    assert L.tw_submit_png(None, None, None, 10, 5.0, None, None, C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
    assert L.tw_stage_png_decode(None, None, 0, None) == twflow.TW_E_BAD_PARAMETER
