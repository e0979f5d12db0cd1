"""Pairs of unequal size (tw_submit_*_sized, tw_stage_resize_u8): the ABI side and the host layer on the stub backend,
no GPU.  The device side is tests/test_gpu_resize_u8.py (the kernel alone) and tests/test_gpu_reconcile.py (the batch path).
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
SUBMITS = ("tw_submit_u8_sized", "tw_submit_png8_sized", "tw_submit_dev_sized")
NEW_SYMBOLS = SUBMITS + ("tw_stage_resize_u8",)


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
    assert set(twflow.SYMBOLS) == decl
    assert twflow.abi_version() == 4  # additive within ABI 4


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "t.c"
    src.write_text('#include "twflow.h"\n'
                   "int f(tw_engine* e, const unsigned char* a, const tw_flow_in* i, const tw_flow_out* o, tw_ticket* t) {\n"
                   "  int r = tw_submit_u8_sized(e, a, 8, 8, 8, a, 5, 11, 5, 10, 5.0, i, o, t);\n"
                   "  r += tw_submit_png8_sized(e, a, 3, 8, 8, a, 4, 5, 11, 10, 5.0, i, o, t);\n"
                   "  r += tw_submit_dev_sized(e, a, 8, 8, 16, a, 5, 11, 32, 10, 5.0, i, o, t);\n"
                   "  return r + tw_stage_resize_u8(e, a, 5, 11, (unsigned char*)0, 8, 8); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "t.o")])


def test_resize_family_unique_and_last_three_unchanged(twflow):
    dbg = open(os.path.join(ROOT, "include", "twflow_debug.h")).read()
    fams = re.findall(r"^\s+(TW_DF_[A-Z0-9_]+)", dbg.split("enum tw_debug_family")[1].split("};")[0], flags=re.M)
    assert fams[-3:] == ["TW_DF_FLOW_INIT", "TW_DF_FLOW_EXPORT", "TW_DF_COUNT"]
    assert fams.index("TW_DF_RESIZE_U8") == fams.index("TW_DF_PAIR_SAME") + 1 == fams.index("TW_DF_FLOW_INIT") - 1
    L = twflow.lib()
    names = [L.tw_debug_family_name(i) for i in range(len(fams) - 1)]
    assert names[fams.index("TW_DF_RESIZE_U8")] == b"tw_resize_u8"
    assert names.count(b"tw_resize_u8") == 1
    assert len(set(names)) == len(names)
    assert L.tw_debug_family_name(len(fams) - 1) is None


def test_null_engine_is_refused(twflow):
    L = twflow.lib()
    img = (C.c_uint8 * 256)()
    tk = C.c_int64()
    bad = twflow.TW_E_BAD_PARAMETER
    assert L.tw_submit_u8_sized(None, img, 8, 8, 8, img, 9, 7, 9, 0, 0.0, None, None, C.byref(tk)) == bad
    assert L.tw_submit_png8_sized(None, img, 0, 8, 8, img, 0, 9, 7, 0, 0.0, None, None, C.byref(tk)) == bad
    assert L.tw_submit_dev_sized(None, img, 8, 8, 8, img, 9, 7, 9, 0, 0.0, None, None, C.byref(tk)) == bad
    assert L.tw_stage_resize_u8(None, img, 9, 7, img, 8, 8) == bad


def test_python_submit_refuses_a_shape_mismatch_without_reconcile(twflow):
    """The default of Engine.submit is unchanged: any shape mismatch is DontMatchSize before the library is asked."""
    e = twflow.Engine.__new__(twflow.Engine)  # (no device: the check comes before any call into the library)
    e._h = C.c_void_p()
    with pytest.raises(twflow.TwError) as ei:
        e.submit(np.zeros((8, 8), np.uint8), np.zeros((8, 9), np.uint8))
    assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE


def _build_stub_library(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path / "libstub.so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HOST, "stub_twflow.cpp"),
                        "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return so


def test_stub_library_exports_the_submit_symbols_and_applies_the_size_rule(tmp_path):
    S = C.CDLL(_build_stub_library(tmp_path))
    for s in SUBMITS:
        assert hasattr(S, s), s
    u8p, vp = C.POINTER(C.c_uint8), C.c_void_p
    S.tw_submit_u8_sized.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_ssize_t, u8p, C.c_int, C.c_int, C.c_ssize_t, C.c_int,
                                     C.c_double, vp, vp, C.POINTER(C.c_int64)]
    S.tw_engine_create.argtypes = [C.c_int, vp, C.c_int, C.POINTER(vp)]
    S.tw_engine_destroy.argtypes = [vp]
    S.tw_engine_destroy.restype = None
    eng = vp()
    assert S.tw_engine_create(0, None, 4, C.byref(eng)) == 0
    img = (C.c_uint8 * 4096)()
    tk = C.c_int64()
    assert S.tw_submit_u8_sized(eng, img, 20, 20, 20, img, 25, 15, 25, 10, 5.0, None, None, C.byref(tk)) == 0
    assert tk.value == 1
    for tw_, th_ in ((26, 20), (20, 14), (25, 26)):
        assert S.tw_submit_u8_sized(eng, img, 20, 20, 20, img, tw_, th_, tw_, 10, 5.0, None, None, C.byref(tk)) == 3
    assert S.tw_submit_u8_sized(eng, img, 20, 20, 20, img, 22, 20, 21, 10, 5.0, None, None, C.byref(tk)) == 1  # stride < width
    assert S.tw_submit_u8_sized(eng, img, 20, 20, 20, img, 20, 20, 20, 10, 5.0, None, None, C.byref(tk)) == 0
    assert tk.value == 2  # the refusals consumed no ticket
    S.tw_engine_destroy(eng)


PROBE = r'''
#include <stdio.h>
#include <condition_variable>
#include <mutex>
#include <string>
#include "../twhost.h"
using namespace twhost;
// argv: pairs of (expect path, target path); one JSON line per response (an error comes without its pair's names)
int main(int argc, char** argv) {
    std::mutex m; std::condition_variable cv; int n = 0; bool fin = false;
    Observer o;
    o.onNext = [&](const Response& r) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"%s\", \"target\": \"%s\", \"width\": %d, \"height\": %d, \"vectors\": %d}\n",
               r.status.c_str(), r.target_image.c_str(), r.width, r.height, (int)r.vectors.size());
        n++; cv.notify_all(); };
    o.onError = [&](const std::string& e) {
        std::lock_guard<std::mutex> lk(m);
        printf("{\"status\": \"ERROR\", \"reason\": \"%s\"}\n", e.c_str());
        n++; cv.notify_all(); };
    o.onCompleted = [&](const Report&) { std::lock_guard<std::mutex> lk(m); fin = true; cv.notify_all(); };
    Parameter p; tw_default_params(&p.optParam); p.numThreads = 1; p.batch = 8;
    Manager* mg = new Manager(o); mg->start(p); mg->waitReady();
    for (int i = 0; i + 2 < argc; i += 2) mg->request(argv[1 + i], argv[2 + i]);
    { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return n >= (argc - 1) / 2; }); }
    mg->stop(); { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return fin; }); } delete mg;
    return 0;
}
'''


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


@pytest.fixture(scope="module")
def probe():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(os.path.join(HOST, "build"), exist_ok=True)
    src = os.path.join(HOST, "build", "reconcile_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    exe = os.path.join(HOST, "build", "reconcile_probe")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, src] +
                       [os.path.join(HOST, n) for n in ("stub_twflow.cpp", "twhost.cpp", "jpeg_gray.cpp", "tw_inflate.cpp")] +
                       ["-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("device_reconcile", ["1", "0"])
def test_host_layer_reconciles_or_refuses_file_pairs_on_the_stub_backend(probe, tmp_path, device_reconcile):
    """A file pair 3 px narrower gets a response under TW_DEVICE_RECONCILE=1 (tw_submit_*_sized) and =0 (the host's own
    resize); a pair 6 px apart answers "Don't match image size" under both, before anything is submitted."""
    from PIL import Image
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (90, 120), dtype=np.uint8)
    near, far = a[:, :117].copy(), a[:84, :].copy()
    near[0, 0] = a[0, 0] ^ 0x80  # (the stub flags a pair whose first pixels differ)
    paths = {}
    for name, img in (("a", a), ("near", near), ("far", far)):
        paths[name + ".pgm"] = str(tmp_path / (name + ".pgm"))
        _write_pgm(paths[name + ".pgm"], img)
        paths[name + ".png"] = str(tmp_path / (name + ".png"))
        Image.fromarray(np.dstack([img] * 3 + [np.full_like(img, 255)])).save(paths[name + ".png"])
    args = []
    for ext in (".pgm", ".png"):
        args += [paths["a" + ext], paths["near" + ext], paths["a" + ext], paths["far" + ext]]
    env = dict(os.environ, TW_DEVICE_RECONCILE=device_reconcile, TW_STUB_DEVICES="1", TW_NUMA="0")
    r = subprocess.run([probe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    res = [json.loads(line) for line in r.stdout.strip().splitlines()]
    assert len(res) == 4
    errors = [x for x in res if x["status"] == "ERROR"]
    assert [x["reason"] for x in errors] == ["Don't match image size"] * 2, res
    answered = {os.path.basename(x["target"]): x for x in res if x["status"] != "ERROR"}
    assert sorted(answered) == ["near.pgm", "near.png"], res
    for x in answered.values():
        assert (x["width"], x["height"]) == (120, 90)
        assert x["status"] == "SUSPICIOUS" and x["vectors"] == 1  # the stub saw the target's own first pixel
