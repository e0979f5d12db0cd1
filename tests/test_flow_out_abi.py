"""Dense flow fields from batched submissions (tw_submit_*_flow, tw_dev_download): the ABI side, no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tw_submit_u8_flow", "tw_submit_png8_flow", "tw_submit_dev_flow", "tw_dev_download")


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
    assert set(twflow.SYMBOLS) == decl


def test_flow_export_family_has_a_unique_name(twflow):
    dbg = open(os.path.join(ROOT, "include", "twflow_debug.h")).read()
    fams = re.findall(r"^\s+(TW_DF_[A-Z0-9_]+)", dbg.split("enum tw_debug_family")[1].split("};")[0], flags=re.M)
    assert fams[-2:] == ["TW_DF_FLOW_EXPORT", "TW_DF_COUNT"]
    L = twflow.lib()
    names = [L.tw_debug_family_name(i) for i in range(len(fams) - 1)]
    assert names[fams.index("TW_DF_FLOW_EXPORT")] == b"tw_flow_export"
    assert names.count(b"tw_flow_export") == 1


def test_null_engine_and_bad_arguments_are_refused(twflow):
    """A null engine answers TW_E_BAD_PARAMETER from every new entry point; nothing falls back to a host computation."""
    L = twflow.lib()
    img = (C.c_uint8 * 64)()
    buf = (C.c_float * 128)()
    fo = twflow.FlowOut(C.cast(buf, C.c_void_p), 32, twflow.FLOW_PLANAR)
    tk = C.c_int64()
    assert L.tw_submit_u8_flow(None, img, img, 8, 8, 8, 0, 0.0, C.byref(fo), C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
    assert L.tw_submit_png8_flow(None, img, 0, img, 0, 8, 8, 0, 0.0, C.byref(fo), C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
    assert L.tw_submit_dev_flow(None, img, img, 8, 8, 8, 0, 0.0, C.byref(fo), C.byref(tk)) == twflow.TW_E_BAD_PARAMETER
    assert L.tw_dev_download(None, buf, img, 16) == twflow.TW_E_BAD_PARAMETER


def test_no_device_means_error(twflow):
    """Without a device an engine cannot be made, so no flow destination is ever written by anything but the GPU; with one,
    the Python layer refuses a destination of the wrong shape before the library sees it."""
    import numpy as np
    if twflow.device_count() == 0:
        with pytest.raises(twflow.TwError) as ei:
            twflow.Engine(0)
        assert ei.value.code == twflow.TW_E_DEVICE
    with pytest.raises(twflow.TwError) as ei:
        twflow._flow_out(np.zeros((3, 8, 8), np.float32), 8, 8)
    assert ei.value.code == twflow.TW_E_BAD_PARAMETER
    fo = twflow._flow_out(np.zeros((2, 8, 8), np.float32)[:, :, :5], 5, 8)
    assert (fo.pitch, fo.layout) == (32, twflow.FLOW_PLANAR)
    fo = twflow._flow_out(np.zeros((8, 9, 2), np.float32)[:, :5], 5, 8)
    assert (fo.pitch, fo.layout) == (72, twflow.FLOW_INTERLEAVED)


def test_c99_consumer_of_tw_flow_out_compiles_and_links(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "consumer.c"
    src.write_text(r"""
#include <stdio.h>
#include "twflow.h"
int main(void)
{
    float field[2 * 8 * 8];
    unsigned char a[64] = {0};
    tw_flow_out o;
    tw_ticket t = 0;
    void* d = 0;
    o.data = field;
    o.pitch = 8 * sizeof(float);
    o.layout = TW_FLOW_PLANAR;
    printf("%d %d %d\n", (int)tw_submit_u8_flow(0, a, a, 8, 8, 8, 0, 0.0, &o, &t), TW_FLOW_INTERLEAVED,
           (int)tw_dev_download(0, field, d, 4));
    (void)tw_submit_png8_flow; (void)tw_submit_dev_flow;
    return 0;
}
""")
    exe = tmp_path / "consumer"
    libdir = os.path.join(ROOT, "tidal-wave_amd")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", libdir, "-ltwflow", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["1", "1", "1"]


def test_flow_export_uses_no_scratch(tmp_path):
    """The compiler's resource report of tw_flow_export for gfx950: no scratch (the 4-pixel tail loops stay in registers)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tidal-wave_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", str(tmp_path / "k.s"),
                        os.path.join(csrc, "twflow.hip"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900, cwd=csrc)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")
    mine = [b for b in blocks if b.startswith("_ZN3twk14tw_flow_export")]
    assert len(mine) == 1, "tw_flow_export not in the report"
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0][:600]
