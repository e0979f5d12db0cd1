"""tw_submit_jpeg / tw_stage_jpeg_idct: the ABI side, no GPU.  The device side is tests/test_gpu_jpeg.py, the host layer
tests/test_host_jpeg.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
NEW_SYMBOLS = ("tw_submit_jpeg", "tw_stage_jpeg_idct")


def test_new_symbols_declared_exported_and_bound(twflow):
    L = twflow.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "twflow.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(tw_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in decl and hasattr(L, s) and s in twflow.SYMBOLS, s
    assert twflow.abi_version() == 4  # additive within ABI 4


def test_launch_family_has_a_unique_name(twflow):
    dbg = open(os.path.join(ROOT, "include", "twflow_debug.h")).read()
    fams = re.findall(r"^\s+(TW_DF_[A-Z0-9_]+)", dbg.split("enum tw_debug_family")[1].split("};")[0], flags=re.M)
    assert fams.index("TW_DF_JPEG_IDCT") < fams.index("TW_DF_COUNT") == len(fams) - 1
    L = twflow.lib()
    names = [L.tw_debug_family_name(i) for i in range(len(fams) - 1)]
    assert names[fams.index("TW_DF_JPEG_IDCT")] == b"tw_jpeg_idct" and names.count(b"tw_jpeg_idct") == 1


def test_struct_layout_matches_the_python_mirror(twflow, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    T = twflow.JpegLuma
    lines = ['#include <stddef.h>', '#include "twflow.h"',
             "_Static_assert(sizeof(tw_jpeg_luma) == %d, \"size\");" % C.sizeof(T)]
    for name, _ in T._fields_:
        lines.append("_Static_assert(offsetof(tw_jpeg_luma, %s) == %d, \"%s\");" % (name, getattr(T, name).offset, name))
    lines.append("int f(tw_engine* e, const tw_jpeg_luma* a, unsigned char* g, tw_ticket* t) {\n"
                 "  return tw_submit_jpeg(e, a, a, 10, 5.0, 0, 0, t) + tw_stage_jpeg_idct(e, a, g, g); }")
    src = tmp_path / "t.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "t.o")])


def test_python_mirror_takes_coefficients_or_a_gray_image(twflow):
    coef = np.arange(2 * 3 * 64, dtype=np.int16).reshape(2, 3, 64)
    l = twflow.JpegLuma(coef, np.arange(64), 17, 15)
    assert (l.width, l.height, l.blocks_w, l.blocks_h, l.w, l.h) == (17, 15, 3, 2, 17, 15)
    assert l.coef[64] == 64 and list(l.quant) == list(range(64)) and not l.gray
    g = twflow.JpegLuma.from_gray(np.full((5, 7), 9, np.uint8))
    assert (g.width, g.height) == (7, 5) and not g.coef and g.gray[0] == 9
    with pytest.raises(ValueError):
        twflow.JpegLuma(np.zeros((2, 3, 63), np.int16), np.arange(64), 17, 15)


def _luma(twflow, w=17, h=15, bw=None, bh=None):
    bw = (w + 7) // 8 if bw is None else bw
    bh = (h + 7) // 8 if bh is None else bh
    return twflow.JpegLuma(np.zeros((bh, bw, 64), np.int16), np.ones(64, np.uint16), w, h)


def test_null_arguments_are_refused_without_a_device(twflow):
    L = twflow.lib()
    ok = _luma(twflow)
    tk = C.c_int64(-1)
    out = (C.c_uint8 * 1024)()
    bad = twflow.TW_E_BAD_PARAMETER
    assert L.tw_submit_jpeg(None, C.byref(ok), C.byref(ok), 10, 5.0, None, None, C.byref(tk)) == bad
    assert L.tw_stage_jpeg_idct(None, C.byref(ok), out, None) == bad
    assert tk.value == -1


def _stub(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path / "libstub.so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HOST, "stub_twflow.cpp"),
                        os.path.join(HOST, "jpeg_gray.cpp"), "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return C.CDLL(so)


def test_stub_library_applies_tw_submit_jpegs_argument_rules(twflow, tmp_path):
    """The stub answers as the library does for what needs no device: an image with both pointers null and block counts
    outside ceil(size / 8) .. + 3 are TW_E_BAD_PARAMETER, a target 6 px off is TW_E_DONT_MATCH_SIZE, and a refusal
    consumes no ticket."""
    S = _stub(tmp_path)
    assert hasattr(S, "tw_submit_jpeg") and hasattr(S, "tw_stub_jpeg_calls")
    vp, lp = C.c_void_p, C.POINTER(twflow.JpegLuma)
    S.tw_submit_jpeg.argtypes = [vp, lp, lp, C.c_int, C.c_double, vp, vp, C.POINTER(C.c_int64)]
    S.tw_engine_create.argtypes = [C.c_int, vp, C.c_int, C.POINTER(vp)]
    S.tw_engine_destroy.argtypes = [vp]
    S.tw_engine_destroy.restype = None
    eng = vp()
    assert S.tw_engine_create(0, None, 4, C.byref(eng)) == 0
    tk = C.c_int64()
    ok = _luma(twflow)
    sub = lambda a, b: S.tw_submit_jpeg(eng, C.byref(a), C.byref(b), 10, 5.0, None, None, C.byref(tk))  # noqa: E731
    assert sub(ok, ok) == 0 and tk.value == 1
    empty = twflow.JpegLuma.from_gray(np.zeros((15, 17), np.uint8))
    empty.gray = None
    assert sub(ok, empty) == 1 and sub(empty, ok) == 1
    for bw, bh in ((2, 2), (7, 2), (3, 1), (3, 6)):  # 17 x 15: 3 .. 6 blocks across, 2 .. 5 down
        assert sub(ok, _luma(twflow, bw=bw, bh=bh)) == 1, (bw, bh)
    assert sub(ok, _luma(twflow, bw=6, bh=5)) == 0 and tk.value == 2
    assert sub(ok, _luma(twflow, w=23, h=15)) == 3 and sub(ok, _luma(twflow, w=17, h=9)) == 3
    assert sub(ok, _luma(twflow, w=14, h=20)) == 0 and tk.value == 3  # within 5 px: handed over with its own size
    assert sub(ok, twflow.JpegLuma.from_gray(np.zeros((15, 17), np.uint8))) == 0 and tk.value == 4
    pairs, coefs = C.c_long(), C.c_long()
    S.tw_stub_jpeg_calls(C.byref(pairs), C.byref(coefs))
    assert (pairs.value, coefs.value) == (4, 7)
    S.tw_engine_destroy(eng)
