"""The diff image (tw_overlay_out, tw_ticket_hits, tw_ticket_overlay, tw_stage_overlay, tw_debug_overlay_plan,
TW_DF_OVERLAY_BASE / TW_DF_OVERLAY_MARKS): the ABI side, no GPU.  The device side is tests/test_gpu_overlay.py, the reference
tests/overlay_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
PKG = os.path.join(ROOT, "tidal-wave_amd")
NEW_SYMBOLS = ("tw_ticket_hits", "tw_ticket_overlay", "tw_stage_overlay", "tw_debug_overlay_plan")


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


def test_new_symbols_declared_exported_by_both_libraries_and_bound(twflow):
    decl = _declared()
    libs = [twflow.lib(), C.CDLL(os.path.join(PKG, "libtwflow_variants.so"))]
    for s in NEW_SYMBOLS:
        assert s in decl, s
        assert s in twflow.SYMBOLS, s
        for L in libs:
            assert hasattr(L, s), s
    for m in ("hits", "overlay", "stage_overlay", "overlay_plan"):
        assert callable(getattr(twflow.Engine, m))
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr) and twflow.abi_version() == 4  # additive within ABI 4
    assert re.search(r"#define TW_OVERLAY_MAX_LEN 1024\b", hdr) and twflow.OVERLAY_MAX_LEN == 1024


def test_header_compiles_as_c99_and_tw_overlay_out_layout(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, tw_ticket t, const uint8_t* a, uint8_t* px, const tw_rect* r, const tw_region* g) {\n"
                   "  tw_overlay_out o;\n"
                   "  tw_overlay_hit h[1];\n"
                   "  int n = 0, plan[5], path = 0;\n"
                   "  o.data = px; o.pitch = 24; o.format = TW_OVERLAY_RGB8;\n"
                   "  h[0].x = 1; h[0].y = 1; h[0].dx = 2.5f; h[0].dy = 0.f;\n"
                   "  n += tw_ticket_hits(e, t, &n);\n"
                   "  n += tw_ticket_overlay(e, t, 16, &o);\n"
                   "  n += tw_debug_overlay_plan(0, 0, 8, 0, 24, 8, 8, plan, 5);\n"
                   "  return n + tw_stage_overlay(e, a, a, 8, 8, 8, 0, r, 1, h, 1, g, 1, 16, px, 24, &path) + TW_OVERLAY_MAX_LEN; }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu ", sizeof(tw_overlay_out), offsetof(tw_overlay_out, data),\n'
                   "         offsetof(tw_overlay_out, pitch), offsetof(tw_overlay_out, format));\n"
                   '  printf("%zu %zu ", sizeof(tw_overlay_hit), offsetof(tw_overlay_hit, dx));\n'
                   '  printf("%d %d %d %d %d %d\\n", (int)TW_OVERLAY_RGB8, (int)TW_DF_BLUR_SOLVE4Q, (int)TW_DF_OVERLAY_BASE,\n'
                   "         (int)TW_DF_OVERLAY_MARKS, (int)TW_DF_PYR_LEVEL_LDS, (int)TW_DF_COUNT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:6] == [24, 0, 8, 16, 16, 8]
    rgb8, s4q, base, marks, lds, count = got[6:]
    assert rgb8 == 0
    # the two families sit directly in front of TW_DF_PYR_LEVEL_LDS: every neighbourhood the other ABI tests pin lies behind it
    assert base == s4q + 1 and marks == base + 1 and lds == marks + 1
    assert C.sizeof(twflow.OverlayOut) == 24
    assert [(f, getattr(twflow.OverlayOut, f).offset) for f in ("data", "pitch", "format")] == [("data", 0), ("pitch", 8), ("format", 16)]
    assert twflow.OVERLAY_HIT_DTYPE.itemsize == 16 and twflow.OVERLAY_HIT_DTYPE.fields["dx"][1] == 8
    L = twflow.lib()
    L.tw_debug_family_name.restype = C.c_char_p
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert len(names) == count and names[base] == "tw_overlay_base" and names[marks] == "tw_overlay_marks"
    assert names[lds] == "tw_pyr_level_lds" and len(set(names)) == len(names)


def test_null_engine_is_refused_by_every_new_call(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    n = C.c_int(7)
    path = C.c_int(7)
    img = np.zeros((4, 4), np.uint8)
    px = np.full(48, 0xA5, np.uint8)
    u8p = C.POINTER(C.c_uint8)
    oo = twflow.OverlayOut(px.ctypes.data, 12, 0)
    assert L.tw_ticket_hits(None, 1, C.byref(n)) == bad
    assert L.tw_ticket_overlay(None, 1, 16, C.byref(oo)) == bad
    assert L.tw_stage_overlay(None, img.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 4, 4, 4, 0, None, 0, None, 0, None, 0, 16,
                              px.ctypes.data_as(u8p), 12, C.byref(path)) == bad
    assert n.value == 7 and path.value == 7 and (px == 0xA5).all()


def test_overlay_plan_is_a_pure_host_function_that_flips_at_the_alignment_edges(twflow):
    L = twflow.lib()

    def plan(e, t, stride, d, pitch, w=397, h=99):
        v = (C.c_int * 5)()
        assert L.tw_debug_overlay_plan(e, t, stride, d, pitch, w, h, v, 5) == 5
        return list(v)

    base = (0x7f0000001000, 0x7f0000101000, 400, 0x7f0000201000, 1192)
    assert plan(*base) == [1, 4, 256, 2, 25]  # ceil(397 / 256) columns of workgroups, ceil(99 / 4) rows
    for i in range(5):
        for off in (1, 2, 3):
            a = list(base)
            a[i] += off
            assert plan(*a)[0] == 0, (i, off)  # any one of the five off a multiple of 4: the byte path
        a = list(base)
        a[i] += 4
        assert plan(*a)[0] == 1, i
    assert plan(*base, w=256, h=4)[3:] == [1, 1] and plan(*base, w=257, h=5)[3:] == [2, 2] and plan(*base, w=1, h=1)[3:] == [1, 1]
    v = (C.c_int * 5)(9, 9, 9, 9, 9)
    assert L.tw_debug_overlay_plan(0, 0, 4, 0, 12, 4, 4, v, 2) == 2 and list(v) == [1, 4, 9, 9, 9]
    assert L.tw_debug_overlay_plan(0, 0, 4, 0, 12, 0, 4, v, 5) == 0 and L.tw_debug_overlay_plan(0, 0, 4, 0, 12, 4, 4, None, 5) == 0


def test_the_stub_exports_both_calls(tmp_path):
    """tw_ticket_hits echoes the count the ticket's tw_wait will give and tw_ticket_overlay writes pixel (x & 255, y & 255, tol),
    nothing behind a row; neither consumes the ticket, both refuse a waited one."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "ovl.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include <string.h>\n'
                   '#include "twflow.h"\n'
                   "int main() {\n"
                   "  tw_params p; tw_default_params(&p);\n"
                   "  tw_engine* e = nullptr;\n"
                   "  if (tw_engine_create(0, &p, 2, &e) != TW_OK) return 2;\n"
                   "  unsigned char a[64] = {10}, b[64] = {40}, px[8 * 30];\n"
                   "  memset(px, 0xA5, sizeof px);\n"
                   "  tw_overlay_out o = {px, 30, TW_OVERLAY_RGB8}, shortp = {px, 23, TW_OVERLAY_RGB8}, fmt = {px, 30, 1};\n"
                   "  tw_ticket t; tw_vector out[4]; int n = 0, nh = -1; float s;\n"
                   "  tw_submit_u8(e, a, b, 8, 8, 8, 4, 0.0, &t);\n"
                   '  printf("%d ", (int)tw_ticket_hits(e, t, &nh));\n'
                   '  printf("%d %d %d %d %d ", (int)tw_ticket_overlay(e, t, 256, &o), (int)tw_ticket_overlay(e, t, -1, &o),\n'
                   "         (int)tw_ticket_overlay(e, t, 16, &shortp), (int)tw_ticket_overlay(e, t, 16, &fmt),\n"
                   "         (int)tw_ticket_overlay(e, t, 16, nullptr));\n"
                   "  int clean = 1; for (unsigned char c : px) clean &= c == 0xA5;\n"
                   '  printf("%d ", clean);\n'
                   '  printf("%d %d ", (int)tw_ticket_overlay(e, t, 77, &o), (int)tw_ticket_overlay(e, t, 77, &o));\n'
                   '  printf("%d ", (int)tw_wait(e, t, out, 4, &n, &s));\n'
                   '  printf("%d %d ", (int)tw_ticket_hits(e, t, &nh), (int)tw_ticket_overlay(e, t, 77, &o));\n'
                   '  printf("%d %d\\n", n, nh);\n'
                   "  int ok = 1;\n"
                   "  for (int y = 0; y < 8; y++) for (int x = 0; x < 30; x++) {\n"
                   "    const int want = x >= 24 ? 0xA5 : x % 3 == 0 ? x / 3 : x % 3 == 1 ? y : 77;\n"
                   "    ok &= px[y * 30 + x] == want; }\n"
                   '  printf("%d\\n", ok);\n'
                   "  tw_engine_destroy(e);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "ovl")
    srcs = [str(src)] + [os.path.join(HOST, f) for f in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe] + srcs +
                          ["-lpthread"])
    env = dict(os.environ, TW_STUB_DEVICES="1")
    env.pop("TW_STUB_TRACE", None)
    lines = subprocess.check_output([exe], text=True, env=env).splitlines()
    # hits; five refused overlays that wrote nothing; two overlays; the wait; both calls on the waited ticket; n == hits
    assert lines[0].split() == ["0", "1", "1", "1", "1", "1", "1", "0", "0", "0", "1", "1"] + lines[0].split()[12:]
    n, nh = lines[0].split()[12:]
    assert n == nh
    assert lines[1] == "1"
