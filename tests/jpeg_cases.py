"""What the JPEG tests share (test_jpeg_luma_host.py, test_gpu_jpeg.py): the host decoder behind a C API, compiled at test
time from host/jpeg_gray.cpp; a numpy int64 restatement of libjpeg's jidctint written from the algorithm; the block
generators; the committed fixtures.  Not a test module."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEG_DIR = os.path.join(GOLDEN, "jpeg")

# the three entry points of the split decoder behind plain C (plain g++, no sanitizer)
PROBE = r'''
#include <string.h>
#include "../twhost.h"
extern "C" {
// 1: decoded; info = {w, h, bw, bh}, quant[64]; *coef = a new[] block of bw * bh * 64 values (free_coef).  0: refused, and
// info holds whatever the decoder reported (nothing: zeros)
int decode_jpeg_luma(const uint8_t* d, size_t n, int* info, uint16_t* quant, int16_t** coef)
{
    twhost::JpegLuma l;
    const bool ok = twhost::decode_jpeg_luma(d, n, l);
    info[0] = l.w; info[1] = l.h; info[2] = l.bw; info[3] = l.bh;
    *coef = nullptr;
    if (!ok) return 0;
    memcpy(quant, l.quant, 128);
    *coef = new int16_t[l.coef.size() ? l.coef.size() : 1];
    memcpy(*coef, l.coef.data(), l.coef.size() * 2);
    return 1;
}
void free_coef(int16_t* p) { delete[] p; }
void jpeg_luma_to_gray(int w, int h, int bw, int bh, const uint16_t* quant, const int16_t* coef, uint8_t* out)
{
    twhost::JpegLuma l;
    l.w = w; l.h = h; l.bw = bw; l.bh = bh;
    memcpy(l.quant, quant, 128);
    l.coef.assign(coef, coef + (size_t)bw * bh * 64);
    std::vector<uint8_t> g;
    twhost::jpeg_luma_to_gray(l, g);
    memcpy(out, g.data(), g.size());
}
// 1: decoded, wh = {w, h} and, when cap is large enough, out = the gray image; 0: refused, wh as the decoder left it
int decode_jpeg_gray(const uint8_t* d, size_t n, uint8_t* out, size_t cap, int* wh)
{
    std::vector<uint8_t> g;
    wh[0] = wh[1] = 0;
    if (!twhost::decode_jpeg_gray(d, n, g, wh[0], wh[1])) return 0;
    if (g.size() <= cap) memcpy(out, g.data(), g.size());
    return 1;
}
}
'''

_lib = None


def host_lib():
    """The .so of PROBE + jpeg_gray.cpp under host/build/ (None without g++)."""
    global _lib
    if _lib is not None:
        return _lib
    if shutil.which("g++") is None:
        return None
    build = os.path.join(HOST, "build")
    os.makedirs(build, exist_ok=True)
    src = os.path.join(build, "jpeg_luma_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    so = os.path.join(build, "libjpeg_luma_probe.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src, os.path.join(HOST, "jpeg_gray.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _lib = bind(so)
    return _lib


def bind(so):
    L = C.CDLL(so)
    u8p, i16p, u16p, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(C.c_uint16), C.POINTER(C.c_int)
    L.decode_jpeg_gray.argtypes = [C.c_char_p, C.c_size_t, u8p, C.c_size_t, ip]
    if hasattr(L, "decode_jpeg_luma"):
        L.decode_jpeg_luma.argtypes = [C.c_char_p, C.c_size_t, ip, u16p, C.POINTER(i16p)]
        L.free_coef.argtypes = [i16p]
        L.jpeg_luma_to_gray.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u16p, i16p, u8p]
        L.jpeg_luma_to_gray.restype = None
    return L


class Luma:
    """decode_jpeg_luma's result: w, h, coef [bh, bw, 64] int16, quant [64] uint16."""

    def __init__(self, w, h, coef, quant):
        self.w, self.h, self.coef, self.quant = w, h, np.ascontiguousarray(coef, np.int16), np.ascontiguousarray(quant, np.uint16)


def decode_luma(data):
    """(Luma or None, (w, h) as the decoder reported them)"""
    L = host_lib()
    info = (C.c_int * 4)()
    quant = np.zeros(64, np.uint16)
    p = C.POINTER(C.c_int16)()
    ok = L.decode_jpeg_luma(data, len(data), info, quant.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(p))
    if not ok:
        return None, (info[0], info[1])
    w, h, bw, bh = info
    coef = np.ctypeslib.as_array(p, shape=(bh, bw, 64)).copy()
    L.free_coef(p)
    return Luma(w, h, coef, quant), (w, h)


def luma_to_gray(luma):
    L = host_lib()
    bh, bw = luma.coef.shape[:2]
    out = np.empty((luma.h, luma.w), np.uint8)
    L.jpeg_luma_to_gray(luma.w, luma.h, bw, bh, luma.quant.ctypes.data_as(C.POINTER(C.c_uint16)),
                        luma.coef.ctypes.data_as(C.POINTER(C.c_int16)), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def decode_gray(data, lib=None):
    """(gray image or None, (w, h) as the decoder reported them)"""
    L = lib or host_lib()
    wh = (C.c_int * 2)()
    cap = 1 << 22
    out = np.empty(cap, np.uint8)
    if not L.decode_jpeg_gray(data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, wh):
        return None, (wh[0], wh[1])
    assert wh[0] * wh[1] <= cap
    return out[:wh[0] * wh[1]].reshape(wh[1], wh[0]).copy(), (wh[0], wh[1])


def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = (int(v) for v in f.readline().split())
        assert f.readline().strip() == b"255"
        return np.frombuffer(f.read(), np.uint8).reshape(h, w)


def fixture_names():
    return sorted(n[:-4] for n in os.listdir(JPEG_DIR) if n.endswith(".jpg"))


def fixture(name):
    """(file bytes, the committed libjpeg gray decode)"""
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        data = f.read()
    return data, read_pgm(os.path.join(JPEG_DIR, name + ".pgm"))


def capture1(rev):
    """The reference's own JPEG fixture of a revision and its committed gray decode."""
    with open(os.path.join(GOLDEN, "tree", rev, "scenario1", "capture1.jpg"), "rb") as f:
        data = f.read()
    return data, read_pgm(os.path.join(GOLDEN, "%s_scenario1_capture1.pgm" % rev))


def damaged_variants():
    """name -> bytes: the cuts and flips of test_node_addon.py::test_jpeg_decode_survives_damaged_files."""
    src = capture1("expected")[0]
    rng = np.random.default_rng(11)
    out = {}
    for i, cut in enumerate((3, 20, 200, len(src) // 3, len(src) // 2, len(src) - 2)):
        out["cut%d" % i] = src[:cut]
    for i in range(12):
        b = bytearray(src)
        for pos in rng.integers(2, len(b), 8):
            b[int(pos)] = int(rng.integers(0, 256))
        out["flip%d" % i] = bytes(b)
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---- libjpeg's jidctint (the "slow integer" inverse DCT), restated from the algorithm -----------------------------------
# Loeffler-Ligtenberg-Moschytz with 13-bit constants: FIX(x) = round(x * 2^13)
def _fix(x):
    return int(round(x * 8192))


def _pass(v, shift):
    """One 8-point pass over the last axis: v [..., 8] int64 -> [..., 8] int64, descaled by `shift` with rounding."""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., k] for k in range(8))
    # even part: a rotation of (2, 6) and a butterfly of (0, 4)
    z1 = (v2 + v6) * _fix(0.541196100)
    t2 = z1 - v6 * _fix(1.847759065)
    t3 = z1 + v2 * _fix(0.765366865)
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    # odd part
    z1, z2, z3, z4 = v7 + v1, v5 + v3, v7 + v3, v5 + v1
    z5 = (z3 + z4) * _fix(1.175875602)
    o0 = v7 * _fix(0.298631336)
    o1 = v5 * _fix(2.053119869)
    o2 = v3 * _fix(3.072711026)
    o3 = v1 * _fix(1.501321110)
    z1 = -z1 * _fix(0.899976223)
    z2 = -z2 * _fix(2.562915447)
    z3 = -z3 * _fix(1.961570560) + z5
    z4 = -z4 * _fix(0.390180644) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    rnd = 1 << (shift - 1)
    out = [e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3]
    return np.stack([(x + rnd) >> shift for x in out], -1)


def idct_reference(coef, quant):
    """coef [N, 64] int16, quant [N, 64] or [64] uint16 -> [N, 8, 8] uint8: dequantise, columns (descale 13 - 2), rows
    (descale 13 + 2 + 3), then libjpeg's range_limit table indexed with (x & 1023)."""
    v = (coef.astype(np.int64) * np.asarray(quant).astype(np.int64)).reshape(-1, 8, 8)
    ws = _pass(v.transpose(0, 2, 1), 13 - 2).transpose(0, 2, 1)  # every column
    o = _pass(ws, 13 + 2 + 3) & 1023
    table = np.empty(1024, np.uint8)  # range_limit: 0..127 -> 128..255, then 255s, then 0s, 896..1023 -> 0..127
    table[:128] = np.arange(128, 256)
    table[128:512] = 255
    table[512:896] = 0
    table[896:] = np.arange(0, 128)
    return table[o]


def random_blocks(n, seed, full_range):
    """(coef [n, 64] int16, quant [64] uint16).  full_range: every int16 / uint16 value, with -32768, 32767 and 65535 forced
    in; otherwise what a valid file holds: a quality-style table and coefficients within the DCT's range for it."""
    rng = np.random.default_rng(seed)
    if full_range:
        coef = rng.integers(-32768, 32768, (n, 64)).astype(np.int16)
        quant = rng.integers(0, 65536, 64).astype(np.uint16)
        coef[0, :] = -32768
        coef[1 % n, :] = 32767
        coef[2 % n, ::2] = -32768
        coef[2 % n, 1::2] = 32767
        quant[[0, 7, 9, 63]] = 65535
        quant[5] = 0
        return coef, quant
    quant = rng.integers(1, 64, 64).astype(np.uint16)
    lim = (1024 // quant.astype(np.int64)).astype(np.int64)
    coef = (rng.integers(-1000, 1001, (n, 64)) % (2 * lim + 1) - lim).astype(np.int16)
    sparse = rng.random((n, 64)) < 0.6  # most AC coefficients of a real file are zero
    sparse[:, 0] = False
    coef[sparse] = 0
    return coef, quant


def blocks_to_image(px, bw, bh, w, h):
    """[bh * bw, 8, 8] block pixels -> the cropped [h, w] image"""
    img = px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
    return img[:h, :w]
