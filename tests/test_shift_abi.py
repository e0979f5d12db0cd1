"""The shift (tw_shift, TW_OPT_SHIFT, tw_ticket_shift, tw_stage_shift, tw_debug_shift_plan, TW_DF_SHIFT_* and
TW_DF_FLOW_SHIFT_INIT): the ABI side, no GPU.  The device side is tests/test_gpu_shift.py, the host layer
tests/test_host_shift.py, the reference tests/shift_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shift_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
PKG = os.path.join(ROOT, "tidal-wave_amd")
NEW_SYMBOLS = ("tw_ticket_shift", "tw_stage_shift", "tw_debug_shift_plan")
FIELDS = ["dx", "dy", "applied", "n_shift", "n_zero", "sad_shift", "sad_zero"]
OFFSETS = [0, 4, 8, 12, 16, 24, 32]
FAMILIES = ["tw_shift_profiles", "tw_shift_search", "tw_shift_verify", "tw_flow_shift_init"]


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
    for m in ("set_shift", "shift", "stage_shift", "shift_plan"):
        assert callable(getattr(twflow.Engine, m))
    assert twflow.OPT_SHIFT == 5
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr) and twflow.abi_version() == 4  # additive within ABI 4


def test_header_compiles_as_c99_and_tw_shift_is_40_bytes(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, tw_ticket t, const uint8_t* a, const uint8_t* b) {\n"
                   "  tw_shift s;\n"
                   "  uint32_t prof[32];\n"
                   "  int n = 0, plan[10];\n"
                   "  n += tw_set_option(e, TW_OPT_SHIFT, 64);\n"
                   "  n += tw_ticket_shift(e, t, &s);\n"
                   "  n += tw_debug_shift_plan(8, 8, 64, plan, 10);\n"
                   "  n += tw_stage_shift(e, a, b, 8, 8, 8, 64, 0, 0, &s);\n"
                   "  return n + tw_stage_shift(e, a, b, 8, 8, 8, 64, 1, prof, &s); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu", sizeof(tw_shift));\n' +
                   "".join('  printf(" %%zu", offsetof(tw_shift, %s));\n' % f for f in FIELDS) +
                   '  printf(" %d %d %d %d %d %d %d %d\\n", (int)TW_OPT_SHIFT, (int)TW_DF_PYR_LEVEL_LDS, (int)TW_DF_SHIFT_PROFILES,\n'
                   "         (int)TW_DF_SHIFT_SEARCH, (int)TW_DF_SHIFT_VERIFY, (int)TW_DF_FLOW_SHIFT_INIT, (int)TW_DF_WARP_RESIDUAL,\n"
                   "         (int)TW_DF_COUNT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:8] == [40] + OFFSETS
    opt, lds, prof, search, verify, init, warp, count = got[8:]
    assert opt == 5
    # the four families sit between TW_DF_PYR_LEVEL_LDS and TW_DF_WARP_RESIDUAL: every neighbourhood the earlier features'
    # tests pin (warp / change scan / iter grid, and the tail from TW_DF_HIT_REGIONS on) keeps its order
    assert [prof, search, verify, init, warp] == [lds + 1, lds + 2, lds + 3, lds + 4, lds + 5]
    assert C.sizeof(twflow.Shift) == 40
    assert [(f, getattr(twflow.Shift, f).offset) for f in FIELDS] == list(zip(FIELDS, OFFSETS))
    L = twflow.lib()
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert len(names) == count and names[prof:init + 1] == FAMILIES
    assert len(set(names)) == len(names)


def test_null_engine_and_bad_arguments_are_refused_without_a_device(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    rec = twflow.Shift()
    rec.dx = 7
    img = np.zeros((4, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert L.tw_set_option(None, twflow.OPT_SHIFT, 1) == bad
    assert L.tw_ticket_shift(None, 1, C.byref(rec)) == bad
    assert L.tw_stage_shift(None, img.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 4, 4, 4, 8, 0, None, C.byref(rec)) == bad
    assert rec.dx == 7


def test_shift_plan_is_a_pure_host_function(twflow):
    L = twflow.lib()
    v = (C.c_int * 10)()
    assert L.tw_debug_shift_plan(320, 240, 100, v, 10) == 10
    lds_x, lds_y, rx, ry, gx, block, budget = list(v)[:7]
    assert (lds_x, lds_y, rx, ry, gx) == (1, 1, 100, 100, 2) and block % 64 == 0 and budget <= 64 * 1024
    # an axis stays in LDS exactly while both of its profiles (2 * L words) fit the budget
    edge = budget // 8
    for w, want in ((edge, 1), (edge + 1, 0), (32768, 0)):
        assert L.tw_debug_shift_plan(w, 4, 1024, v, 10) == 10 and (v[0], v[1]) == (want, 1)
        assert L.tw_debug_shift_plan(4, w, 1024, v, 10) == 10 and (v[0], v[1]) == (1, want)
    assert edge < 32768  # (the longest admitted axis does not fit: the device-memory path exists for a reason)
    assert L.tw_debug_shift_plan(7, 3, 8, v, 10) == 10 and (v[2], v[3]) == (3, 1)  # r = min(R, L / 2)
    for args in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (4, 4, 1025)):
        assert L.tw_debug_shift_plan(*args, v, 10) == 0
    assert L.tw_debug_shift_plan(4, 4, 8, None, 10) == 0 and L.tw_debug_shift_plan(4, 4, 8, v, 3) == 3


def test_the_stub_keeps_the_options_argument_check_and_computes_the_definition(tmp_path):
    """TW_OPT_SHIFT takes 0 .. 1024; anything else answers TW_E_BAD_PARAMETER and leaves the option as it was (the stub backend
    keeps the library's rule: an engine of the library itself needs a device).  tw_ticket_shift does not consume the ticket, is
    refused for a pair submitted with the option off, for a null `out`, an unknown and a waited ticket, and answers the
    definition computed on the CPU: compared here with tests/shift_ref.py on a shifted page."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    h, w, sx, sy = 96, 128, -9, 21
    E, T = S.shifted_pair(np.random.default_rng(5), h, w, sx, sy, pad=40)
    stride = w + 5
    buf = np.full((2, h, stride), 0xEE, np.uint8)
    buf[0, :, :w] = E
    buf[1, :, :w] = T
    (tmp_path / "pair.bin").write_bytes(buf.tobytes())
    src = tmp_path / "opt.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include <vector>\n'
                   '#include "twflow.h"\n'
                   "int main(int argc, char** argv) {\n"
                   "  tw_params p; tw_default_params(&p);\n"
                   "  tw_engine* e = nullptr;\n"
                   "  if (tw_engine_create(0, &p, 2, &e) != TW_OK) return 2;\n"
                   "  const int vals[] = {0, 1, 1024, 1025, -1, 4096, 30};\n"
                   '  for (int v : vals) printf("%%d ", (int)tw_set_option(e, TW_OPT_SHIFT, v));\n'
                   "  const int w = %d, h = %d, stride = %d;\n"
                   "  std::vector<unsigned char> img(2 * (size_t)h * stride);\n"
                   '  FILE* f = fopen(argv[1], "rb");\n'
                   "  if (!f || fread(img.data(), 1, img.size(), f) != img.size()) return 3;\n"
                   "  fclose(f);\n"
                   "  tw_ticket t; tw_vector out[4]; int n = 0; tw_shift s, s2; float sec;\n"
                   "  tw_submit_u8(e, img.data(), img.data() + (size_t)h * stride, w, h, stride, 4, 0.0, &t);\n"
                   '  printf("%%d ", (int)tw_ticket_shift(e, t, &s));\n'
                   '  printf("%%d ", (int)tw_ticket_shift(e, t, &s2));\n'
                   '  printf("%%d ", (int)tw_ticket_shift(e, t, nullptr));\n'
                   '  printf("%%d ", (int)tw_ticket_shift(e, t + 1000, &s2));\n'
                   '  printf("%%d ", (int)tw_wait(e, t, out, 4, &n, &sec));\n'
                   '  printf("%%d\\n", (int)tw_ticket_shift(e, t, &s2));\n'
                   '  printf("%%d %%d %%d %%d %%d %%llu %%llu\\n", s.dx, s.dy, s.applied, s.n_shift, s.n_zero,\n'
                   "         (unsigned long long)s.sad_shift, (unsigned long long)s.sad_zero);\n"
                   "  tw_set_option(e, TW_OPT_SHIFT, 0);\n"
                   "  tw_submit_u8(e, img.data(), img.data() + (size_t)h * stride, w, h, stride, 4, 0.0, &t);\n"
                   '  printf("%%d ", (int)tw_ticket_shift(e, t, &s2));\n'
                   '  printf("%%d\\n", (int)tw_wait(e, t, out, 4, &n, &sec));\n'
                   "  tw_engine_destroy(e);\n"
                   "  return 0; }\n" % (w, h, stride))
    exe = str(tmp_path / "opt")
    srcs = [str(src)] + [os.path.join(HOST, f) for f in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe] + srcs +
                          ["-lpthread"])
    env = dict(os.environ, TW_STUB_DEVICES="1")
    env.pop("TW_STUB_TRACE", None)
    lines = subprocess.check_output([exe, str(tmp_path / "pair.bin")], text=True, env=env).splitlines()
    # the option's statuses (the refused 4096 leaves 1024, then 30 is set); two calls on one ticket, a null out, an unknown
    # ticket, the wait, a call on the waited ticket
    assert lines[0].split() == ["0", "0", "0", "1", "1", "1", "0", "0", "0", "1", "1", "0", "1"]
    want = S.estimate(E, T, 30)
    assert (want.dx, want.dy, want.applied) == (sx, sy, 1)
    assert [int(v) for v in lines[1].split()] == list(want)
    assert lines[2].split() == ["1", "0"]  # option off: refused, and the ticket is still waitable
