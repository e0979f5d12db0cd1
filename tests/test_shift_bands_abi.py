"""The shift bands (tw_shift_band, TW_OPT_SHIFT_BANDS, tw_ticket_shift_bands, tw_stage_shift_bands, tw_debug_band_plan,
TW_DF_BAND_* and TW_DF_FLOW_BAND_INIT): the ABI side, no GPU.  The device side is tests/test_gpu_shift_bands.py, the host layer
tests/test_host_shift_bands.py, the reference tests/band_ref.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import band_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
PKG = os.path.join(ROOT, "tidal-wave_amd")
NEW_SYMBOLS = ("tw_ticket_shift_bands", "tw_stage_shift_bands", "tw_debug_band_plan")
FIELDS = ["y", "rows", "dy", "applied", "n_shift", "n_zero", "sad_shift", "sad_zero"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32]
FAMILIES = ["tw_band_rows", "tw_band_search", "tw_band_verify", "tw_flow_band_init"]


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
    for m in ("set_shift_bands", "shift_bands", "stage_shift_bands", "band_plan"):
        assert callable(getattr(twflow.Engine, m))
    assert twflow.OPT_SHIFT_BANDS == 6
    hdr = open(os.path.join(ROOT, "include", "twflow.h")).read()
    assert re.search(r"#define TWFLOW_ABI_VERSION 4\b", hdr) and twflow.abi_version() == 4  # additive within ABI 4


def test_header_compiles_as_c99_and_tw_shift_band_is_40_bytes(tmp_path, twflow):
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int f(tw_engine* e, tw_ticket t, const uint8_t* a, const uint8_t* b) {\n"
                   "  tw_shift s;\n"
                   "  tw_shift_band bands[4];\n"
                   "  uint16_t sig[64];\n"
                   "  int n = 0, nb = 0, plan[9];\n"
                   "  n += tw_set_option(e, TW_OPT_SHIFT_BANDS, 64);\n"
                   "  n += tw_ticket_shift_bands(e, t, bands, 4, &nb);\n"
                   "  n += tw_debug_band_plan(8, 8, 64, 32, plan, 9);\n"
                   "  n += tw_stage_shift_bands(e, a, b, 8, 8, 8, 64, 32, 0, 0, &s, bands, &nb);\n"
                   "  return n + tw_stage_shift_bands(e, a, b, 8, 8, 8, 64, 32, 1, sig, &s, bands, &nb); }\n")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])
    lay = tmp_path / "layout.c"
    lay.write_text('#include <stddef.h>\n'
                   '#include <stdio.h>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu", sizeof(tw_shift_band));\n' +
                   "".join('  printf(" %%zu", offsetof(tw_shift_band, %s));\n' % f for f in FIELDS) +
                   '  printf(" %d %d %d %d %d %d %d %d\\n", (int)TW_OPT_SHIFT_BANDS, (int)TW_DF_SPAN_SCAN_SEG, (int)TW_DF_BAND_ROWS,\n'
                   "         (int)TW_DF_BAND_SEARCH, (int)TW_DF_BAND_VERIFY, (int)TW_DF_FLOW_BAND_INIT, (int)TW_DF_BLUR_SOLVE4Q,\n"
                   "         (int)TW_DF_COUNT);\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([_cc(), "-std=c99", "-Wall", "-Werror", str(lay), "-I", os.path.join(ROOT, "include"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:9] == [40] + OFFSETS
    opt, seg, rows, search, verify, init, solve4q, count = got[9:]
    assert opt == 6
    # the four families stand directly in front of TW_DF_BLUR_SOLVE4Q (behind TW_DF_SPAN_SCAN_SEG): the chain from there to
    # TW_DF_COUNT, which the earlier features' tests pin, keeps its order
    assert [rows, search, verify, init, solve4q] == [seg + 1, seg + 2, seg + 3, seg + 4, seg + 5]
    assert C.sizeof(twflow.ShiftBand) == 40
    assert [(f, getattr(twflow.ShiftBand, f).offset) for f in FIELDS] == list(zip(FIELDS, OFFSETS))
    L = twflow.lib()
    names = []
    while L.tw_debug_family_name(len(names)) is not None:
        names.append(L.tw_debug_family_name(len(names)).decode())
    assert len(names) == count and names[rows:init + 1] == FAMILIES and names[solve4q] == "tw_blur_solve4q"
    assert len(set(names)) == len(names)


def test_null_engine_and_bad_arguments_are_refused_without_a_device(twflow):
    L = twflow.lib()
    bad = twflow.TW_E_BAD_PARAMETER
    rec = twflow.Shift()
    rec.dx = 7
    bands = (twflow.ShiftBand * 2)()
    bands[0].dy = 9
    n = C.c_int(-3)
    img = np.zeros((4, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    a = img.ctypes.data_as(u8p)
    assert L.tw_set_option(None, twflow.OPT_SHIFT_BANDS, 64) == bad
    assert L.tw_ticket_shift_bands(None, 1, bands, 2, C.byref(n)) == bad
    assert L.tw_stage_shift_bands(None, a, a, 4, 4, 4, 8, 32, 0, None, C.byref(rec), bands, C.byref(n)) == bad
    assert (rec.dx, bands[0].dy, n.value) == (7, 9, -3)


def test_band_plan_is_a_pure_host_function(twflow):
    L = twflow.lib()
    v = (C.c_int * 9)()

    def plan(w, h, radius, band):
        assert L.tw_debug_band_plan(w, h, radius, band, v, 9) == 9
        return list(v)
    # 320 x 240, R = 100, B = 32: 8 bands (the last of 16 rows), 5 blocks, r = 100; LDS: 2 * 5 * (32 + min(240, 232)) bytes
    nb, nblk, lds, nbytes, budget, r, gx, block, vgx = plan(320, 240, 100, 32)
    assert (nb, nblk, lds, nbytes, r) == (8, 5, 1, 2 * 5 * (32 + 232), 100)
    assert budget == 96 * 1024 and block == 1024 and gx == (240 * 5 + 255) // 256 and vgx == 15
    assert plan(320, 240, 100, 48)[0] == 5 and plan(320, 241, 100, 48)[0] == 6 and plan(320, 20, 100, 32)[0] == 1
    assert plan(1, 33, 8, 32)[:2] == [2, 1] and plan(64, 33, 8, 32)[1] == 1 and plan(65, 33, 8, 32)[1] == 2
    assert plan(320, 7, 100, 32)[5] == 3  # r = min(R, h / 2)
    # 3840 x 2160 at B = 64: 60 blocks, 120 * (64 + 64 + 2 r) bytes.  R = 345 is the last radius that stays in LDS (98 160
    # bytes of 98 304), R = 346 the first that does not (98 400)
    assert plan(3840, 2160, 345, 64)[2:4] == [1, 98160] and plan(3840, 2160, 346, 64)[2:4] == [0, 98400]
    # ... at R = 345 the last band height is 64 (80: 120 * (80 + 80 + 690) = 102 000) and the last width 3840 (3841: 61 blocks)
    assert plan(3840, 2160, 345, 80)[2:4] == [0, 102000]
    assert plan(3841, 2160, 345, 64)[1:4] == [61, 0, 122 * 818]
    # the rows of T a band can reach are clipped to the image: R = 1024 at 1080 rows reads all of them, and still fits
    assert plan(1920, 1080, 1024, 64)[2:6] == [1, 60 * (64 + 1080), budget, 540]
    assert plan(3840, 2160, 1024, 64)[2:4] == [0, 120 * (64 + 64 + 2048)]
    assert plan(64, 1080, 1024, 1024)[2:4] == [1, 2 * (1024 + 1080)]
    for args in ((0, 4, 8, 32), (4, 0, 8, 32), (4, 4, 0, 32), (4, 4, 1025, 32), (4, 4, 8, 0), (4, 4, 8, 16), (4, 4, 8, 33),
                 (4, 4, 8, 1040)):
        assert L.tw_debug_band_plan(*args, v, 9) == 0
    assert L.tw_debug_band_plan(4, 4, 8, 32, None, 9) == 0 and L.tw_debug_band_plan(4, 4, 8, 32, v, 3) == 3


def test_the_stub_keeps_the_options_argument_check_and_computes_the_definition(tmp_path):
    """TW_OPT_SHIFT_BANDS takes 0 and the multiples of 16 in 32 .. 1024; anything else answers TW_E_BAD_PARAMETER and leaves the
    option as it was.  tw_ticket_shift_bands does not consume the ticket, reports nb whatever the cap, is refused for a pair
    submitted without both options on, for a null n, a null out with cap > 0, an unknown and a waited ticket, and answers the
    definition computed on the CPU: compared here with tests/band_ref.py on a page with an inserted block.  The program links
    every new symbol from the stub."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    h, w, at, ins, sx = 200, 192, 70, 30, -9
    E, T = BR.inserted_pair(np.random.default_rng(5), h, w, at, ins, sx, pad=40)
    stride = w + 5
    buf = np.full((2, h, stride), 0xEE, np.uint8)
    buf[0, :, :w] = E
    buf[1, :, :w] = T
    (tmp_path / "pair.bin").write_bytes(buf.tobytes())
    src = tmp_path / "opt.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include <vector>\n'
                   '#include "twflow.h"\n'
                   '#include "twflow_debug.h"\n'
                   "int main(int argc, char** argv) {\n"
                   "  tw_params p; tw_default_params(&p);\n"
                   "  tw_engine* e = nullptr;\n"
                   "  if (tw_engine_create(0, &p, 2, &e) != TW_OK) return 2;\n"
                   "  const int vals[] = {0, 32, 1024, 16, 33, 1040, -1, 48};\n"
                   '  for (int v : vals) printf("%%d ", (int)tw_set_option(e, TW_OPT_SHIFT_BANDS, v));\n'
                   "  const int w = %d, h = %d, stride = %d;\n"
                   "  std::vector<unsigned char> img(2 * (size_t)h * stride);\n"
                   '  FILE* f = fopen(argv[1], "rb");\n'
                   "  if (!f || fread(img.data(), 1, img.size(), f) != img.size()) return 3;\n"
                   "  fclose(f);\n"
                   "  const unsigned char *a = img.data(), *b = img.data() + (size_t)h * stride;\n"
                   "  tw_ticket t; tw_vector out[4]; int n = 0, nb = -1, nb2 = -1; tw_shift_band s[8], s2[8]; float sec;\n"
                   "  // the bands option without TW_OPT_SHIFT: ignored\n"
                   "  tw_submit_u8(e, a, b, w, h, stride, 4, 0.0, &t);\n"
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, s2, 8, &nb2));\n'
                   '  printf("%%d\\n", (int)tw_wait(e, t, out, 4, &n, &sec));\n'
                   "  tw_set_option(e, TW_OPT_SHIFT, 60);\n"
                   "  tw_submit_u8(e, a, b, w, h, stride, 4, 0.0, &t);\n"
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, s, 8, &nb));\n'
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, s2, 1, &nb2));\n'
                   '  printf("%%d ", nb2);\n'
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, s2, 8, nullptr));\n'
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, nullptr, 8, &nb2));\n'
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t, nullptr, 0, &nb2));\n'
                   '  printf("%%d ", (int)tw_ticket_shift_bands(e, t + 1000, s2, 8, &nb2));\n'
                   '  printf("%%d ", (int)tw_wait(e, t, out, 4, &n, &sec));\n'
                   '  printf("%%d\\n", (int)tw_ticket_shift_bands(e, t, s2, 8, &nb2));\n'
                   '  printf("%%d\\n", nb);\n'
                   "  for (int i = 0; i < nb; i++)\n"
                   '    printf("%%d %%d %%d %%d %%d %%d %%llu %%llu\\n", s[i].y, s[i].rows, s[i].dy, s[i].applied, s[i].n_shift, s[i].n_zero,\n'
                   "           (unsigned long long)s[i].sad_shift, (unsigned long long)s[i].sad_zero);\n"
                   "  int plan[9];\n"
                   '  printf("%%d\\n", tw_debug_band_plan(w, h, 60, 48, plan, 9));\n'
                   "  tw_shift g;\n"
                   '  printf("%%d\\n", (int)tw_stage_shift_bands(nullptr, a, b, stride, w, h, 60, 48, 0, nullptr, &g, s2, &nb2));\n'
                   "  tw_engine_destroy(e);\n"
                   "  return 0; }\n" % (w, h, stride))
    exe = str(tmp_path / "opt")
    srcs = [str(src)] + [os.path.join(HOST, f) for f in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe] + srcs +
                          ["-lpthread"])
    env = dict(os.environ, TW_STUB_DEVICES="1")
    env.pop("TW_STUB_TRACE", None)
    lines = subprocess.check_output([exe, str(tmp_path / "pair.bin")], text=True, env=env).splitlines()
    # the option's statuses (the refused values leave 1024, then 48 is set); without TW_OPT_SHIFT: refused, still waitable
    assert lines[0].split() == ["0", "0", "0", "1", "1", "1", "1", "0", "1", "0"]
    # two calls on one ticket (the second with cap 1: nb reported), a null n, a null out with cap 8, a null out with cap 0, an
    # unknown ticket, the wait, a call on the waited ticket
    assert lines[1].split() == ["0", "0", "5", "1", "1", "0", "1", "0", "1"]
    g, want = BR.estimate(E, T, 60, 48)
    assert g.dx == sx and int(lines[2]) == len(want) == 5
    assert [[int(v) for v in ln.split()] for ln in lines[3:8]] == [list(b) for b in want]
    assert (want[0].dy, want[0].applied) == (0, 1) and (want[2].dy, want[2].applied) == (ins, 1)
    assert lines[8:10] == ["9", "1"]
