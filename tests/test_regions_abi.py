"""Hit regions (tw_region, TW_OPT_REGIONS, tw_wait_regions, tw_stage_hit_regions, TW_DF_HIT_REGIONS): the ABI side, no GPU.
The device side is tests/test_gpu_regions.py, the host layer tests/test_host_regions.py, the reference tests/regions_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
NEW_SYMBOLS = ("tw_wait_regions", "tw_stage_hit_regions")
FIELDS = ["x", "y", "width", "height", "count", "peak_x", "peak_y", "peak_dx", "peak_dy"]


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
    for m in ("set_regions", "wait_regions", "stage_hit_regions"):
        assert callable(getattr(twflow.Engine, m))
    assert twflow.MAX_REGIONS == 256 and twflow.OPT_REGIONS == 3
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr) and twflow.abi_version() == 4  # additive within ABI 4


def test_header_compiles_as_c99_and_tw_region_is_36_bytes(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, tw_ticket t, const float* fields, tw_vector* out, float* sec) {\n"
                   "  tw_region r[TW_MAX_REGIONS];\n"
                   "  tw_rect ign[TW_MAX_IGNORE];\n"
                   "  int n, nr, of[4], ni = 0;\n"
                   "  ign[0].x = ign[0].y = 0; ign[0].width = ign[0].height = 1;\n"
                   "  n = tw_set_option(e, TW_OPT_REGIONS, 1);\n"
                   "  n += tw_wait_regions(e, t, out, 4, &n, of, r, TW_MAX_REGIONS, &nr, sec);\n"
                   "  n += tw_wait_regions(e, t, out, 4, &n, 0, 0, 0, &nr, sec);\n"
                   "  return n + tw_stage_hit_regions(e, fields, 1, 8, 8, 1, 1.0, 1, ign, &ni, &nr, r, of); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu", sizeof(tw_region));\n' +
                   "".join('  printf(" %%zu", offsetof(tw_region, %s));\n' % f for f in FIELDS) +
                   '  printf(" %d %d %d %d %d %d %d\\n", (int)TW_MAX_REGIONS, (int)TW_OPT_REGIONS, (int)TW_DF_FLOW_ITER_GRID,\n'
                   "         (int)TW_DF_HIT_REGIONS, (int)TW_DF_JPEG_IDCT, (int)TW_DF_FLOW_EXPORT, (int)TW_DF_COUNT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:10] == [36, 0, 4, 8, 12, 16, 20, 24, 28, 32]
    max_regions, opt, iter_grid, hit_regions, jpeg, export, count = got[10:]
    assert (max_regions, opt) == (256, 3)
    # TW_DF_HIT_REGIONS sits between TW_DF_FLOW_ITER_GRID and TW_DF_JPEG_IDCT: the six families from TW_DF_JPEG_IDCT on are
    # pinned next to one another by the tests of the features that added them, the last three at the enum's end
    assert hit_regions == iter_grid + 1 and jpeg == hit_regions + 1 and (export, count) == (jpeg + 5, jpeg + 6)
    assert C.sizeof(twflow.Region) == 36 and twflow.REGION_DTYPE.itemsize == 36
    assert [(f, getattr(twflow.Region, f).offset) for f in FIELDS] == [(f, 4 * i) for i, f in enumerate(FIELDS)]
    assert [(f, twflow.REGION_DTYPE.fields[f][1]) for f in FIELDS] == [(f, 4 * i) for i, f in enumerate(FIELDS)]
    # ... and the library's family table agrees with the header
    L = twflow.lib()
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert len(names) == count and names[hit_regions] == "tw_hit_regions" and names[jpeg] == "tw_jpeg_idct"
    assert len(set(names)) == len(names)
    assert names[-3:] == ["tw_resize_u8", "tw_flow_area_init", "tw_flow_export"]


def test_null_engine_is_refused_by_every_new_call(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    n, nr = C.c_int(7), C.c_int(7)
    regs = (twflow.Region * 2)()
    of = (C.c_int * 2)()
    f = np.zeros((1, 2, 4, 4), np.float32)
    assert L.tw_set_option(None, twflow.OPT_REGIONS, 1) == bad
    assert L.tw_wait_regions(None, 1, None, 0, C.byref(n), of, regs, 2, C.byref(nr), None) == bad
    assert L.tw_stage_hit_regions(None, f.ctypes.data_as(C.POINTER(C.c_float)), 1, 4, 4, 1, 1.0, 1, None, None, C.byref(nr),
                                  regs, of) == bad
    assert (n.value, nr.value) == (7, 7)


def test_the_options_argument_check_on_the_stub(tmp_path):
    """TW_OPT_REGIONS takes 0 .. 8; anything else answers TW_E_BAD_PARAMETER and leaves the option as it was (the stub
    backend keeps the library's rule: an engine of the library itself needs a device)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "opt.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   "int main() {\n"
                   "  tw_params p; tw_default_params(&p);\n"
                   "  tw_engine* e = nullptr;\n"
                   "  if (tw_engine_create(0, &p, 2, &e) != TW_OK) return 2;\n"
                   "  const int vals[] = {0, 1, 8, 9, -1, 256, 3};\n"
                   '  for (int v : vals) printf("%d ", (int)tw_set_option(e, TW_OPT_REGIONS, v));\n'
                   "  unsigned char a[64] = {1}, b[64] = {2};\n"
                   "  tw_ticket t; tw_vector out[4]; int n = 0, nr = 0, of[4]; tw_region r[4]; float s;\n"
                   "  tw_submit_u8(e, a, b, 8, 8, 8, 4, 0.0, &t);\n"
                   '  printf("%d ", (int)tw_wait_regions(e, t, out, 4, &n, of, r, 4, &nr, &s));\n'
                   '  printf("%d %d %d %d\\n", n, nr, of[0], r[0].count);\n'
                   "  tw_set_option(e, TW_OPT_REGIONS, 0);\n"
                   "  tw_submit_u8(e, a, b, 8, 8, 8, 4, 0.0, &t);\n"
                   '  printf("%d ", (int)tw_wait_regions(e, t, out, 4, &n, of, r, 4, &nr, &s));\n'
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
    assert lines[0].split() == ["0", "0", "0", "1", "1", "1", "0", "0", "1", "1", "0", "1"]  # statuses; then n, regions, of, count
    assert lines[1].split() == ["1", "0"]  # option off: refused, and the ticket is still waitable
