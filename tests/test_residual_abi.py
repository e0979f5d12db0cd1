"""The residual (tw_change, TW_OPT_RESIDUAL, tw_ticket_changes, tw_stage_warp_residual, TW_DF_WARP_RESIDUAL, TW_DF_CHANGE_SCAN):
the ABI side, no GPU.  The device side is tests/test_gpu_residual.py, the host layer tests/test_host_residual.py, the
reference tests/residual_ref.py."""
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
NEW_SYMBOLS = ("tw_ticket_changes", "tw_stage_warp_residual")
FIELDS = ["x", "y", "n_diff", "n_unexplained", "max_diff", "max_unexplained"]


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
    for m in ("set_residual", "changes", "stage_warp_residual"):
        assert callable(getattr(twflow.Engine, m))
    assert twflow.OPT_RESIDUAL == 4
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr) and twflow.abi_version() == 4  # additive within ABI 4


def test_header_compiles_as_c99_and_tw_change_is_24_bytes(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, tw_ticket t, const uint8_t* a, const uint8_t* b, const float* flow) {\n"
                   "  tw_change c[4];\n"
                   "  int n = 0, cells[16];\n"
                   "  n += tw_set_option(e, TW_OPT_RESIDUAL, 16);\n"
                   "  n += tw_ticket_changes(e, t, c, 4, &n);\n"
                   "  n += tw_ticket_changes(e, t, 0, 0, &n);\n"
                   "  return n + tw_stage_warp_residual(e, a, b, 8, 8, 8, flow, 4, 16, cells, &n, c); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu", sizeof(tw_change));\n' +
                   "".join('  printf(" %%zu", offsetof(tw_change, %s));\n' % f for f in FIELDS) +
                   '  printf(" %d %d %d %d %d\\n", (int)TW_OPT_RESIDUAL, (int)TW_DF_WARP_RESIDUAL, (int)TW_DF_CHANGE_SCAN,\n'
                   "         (int)TW_DF_FLOW_ITER_GRID, (int)TW_DF_COUNT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:7] == [24, 0, 4, 8, 12, 16, 20]
    opt, warp, scan, iter_grid, count = got[7:]
    assert opt == 4
    # the two families sit in front of TW_DF_FLOW_ITER_GRID: the enum's tail from there on is pinned by the tests of the
    # features that added it
    assert scan == warp + 1 and iter_grid == scan + 1
    assert C.sizeof(twflow.Change) == 24
    assert [(f, getattr(twflow.Change, f).offset) for f in FIELDS] == [(f, 4 * i) for i, f in enumerate(FIELDS)]
    L = twflow.lib()
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert len(names) == count and names[warp] == "tw_warp_residual" and names[scan] == "tw_change_scan"
    assert len(set(names)) == len(names)


def test_null_engine_is_refused_by_every_new_call(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    n = C.c_int(7)
    recs = (twflow.Change * 2)()
    cells = (C.c_int * 16)()
    img = np.zeros((4, 4), np.uint8)
    f = np.zeros((2, 4, 4), np.float32)
    u8p = C.POINTER(C.c_uint8)
    assert L.tw_set_option(None, twflow.OPT_RESIDUAL, 1) == bad
    assert L.tw_ticket_changes(None, 1, recs, 2, C.byref(n)) == bad
    assert L.tw_stage_warp_residual(None, img.ctypes.data_as(u8p), img.ctypes.data_as(u8p), 4, 4, 4,
                                    f.ctypes.data_as(C.POINTER(C.c_float)), 1, 16, cells, C.byref(n), recs) == bad
    assert n.value == 7


def test_the_stub_exports_the_call_and_keeps_the_options_argument_check(tmp_path):
    """TW_OPT_RESIDUAL takes 0 .. 254; anything else answers TW_E_BAD_PARAMETER and leaves the option as it was (the stub
    backend keeps the library's rule: an engine of the library itself needs a device).  tw_ticket_changes does not consume
    the ticket, and is refused for a pair submitted with the option off."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "opt.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   "int main() {\n"
                   "  tw_params p; tw_default_params(&p);\n"
                   "  tw_engine* e = nullptr;\n"
                   "  if (tw_engine_create(0, &p, 2, &e) != TW_OK) return 2;\n"
                   "  const int vals[] = {0, 1, 254, 255, -1, 256, 9};\n"
                   '  for (int v : vals) printf("%d ", (int)tw_set_option(e, TW_OPT_RESIDUAL, v));\n'
                   "  unsigned char a[64] = {10}, b[64] = {40};\n"
                   "  tw_ticket t; tw_vector out[4]; int n = 0, nc = 0; tw_change c[4]; float s;\n"
                   "  tw_submit_u8(e, a, b, 8, 8, 8, 4, 0.0, &t);\n"
                   '  printf("%d ", (int)tw_ticket_changes(e, t, c, 4, &nc));\n'
                   '  printf("%d ", (int)tw_ticket_changes(e, t, c, 4, &nc));\n'
                   '  printf("%d ", (int)tw_wait(e, t, out, 4, &n, &s));\n'
                   '  printf("%d ", (int)tw_ticket_changes(e, t, c, 4, &nc));\n'
                   '  printf("%d %d %d %d %d\\n", n, nc, c[0].n_diff, c[0].n_unexplained, c[0].max_diff);\n'
                   "  tw_set_option(e, TW_OPT_RESIDUAL, 0);\n"
                   "  tw_submit_u8(e, a, b, 8, 8, 8, 4, 0.0, &t);\n"
                   '  printf("%d ", (int)tw_ticket_changes(e, t, c, 4, &nc));\n'
                   '  printf("%d\\n", (int)tw_wait(e, t, out, 4, &n, &s));\n'
                   "  tw_engine_destroy(e);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "opt")
    srcs = [str(src)] + [os.path.join(HOST, f) for f in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe] + srcs +
                          ["-lpthread"])
    env = dict(os.environ, TW_STUB_DEVICES="1")
    env.pop("TW_STUB_TRACE", None)
    lines = subprocess.check_output([exe], text=True, env=env).splitlines()
    # the option's statuses; two calls on one ticket, the wait, a call on the waited ticket; then n, the count, the echo record
    assert lines[0].split() == ["0", "0", "0", "1", "1", "1", "0", "0", "0", "0", "1", "1", "1", "9", "9", "30"]
    assert lines[1].split() == ["1", "0"]  # option off: refused, and the ticket is still waitable
