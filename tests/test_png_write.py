"""The diff image's PNG writer (tidal-wave_amd/host/tw_png_write.h): a stand-alone program with its own main() writes files
from raw pixels; PIL and the project's own decoder (host/inflate_test_api.cpp) read them back, and both equal the input.  The
sizes sit on the stored-block seams of the zlib stream (65 535 bytes per block).  The same program built with AddressSanitizer
and UBSan and run on its own ends clean.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")

# (width, height, pitch): 1 x 1, 7 x 5, 397 x 99 with a padded pitch, then raw streams of h * (1 + 3 w) = 65 535, 65 536 and
# 131 070 bytes: exactly one block, one block and one byte, exactly two blocks
CASES = [(1, 1, 3), (7, 5, 21), (397, 99, 1200), (28, 771, 84), (85, 256, 256), (28, 1542, 89)]
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "tw_png_write.h"
// pngw in.raw width height pitch out.png : pitch * height bytes in, a PNG out
int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    const long pitch = atol(argv[4]);
    // exactly the bytes the writer may read: the last row has no padding behind it
    std::vector<uint8_t> px((size_t)pitch * (h - 1) + 3 * (size_t)w);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) return 3;
    fclose(f);
    if (twhost::png_write_rgb8(argv[5], nullptr, w, h, pitch)) return 4;   // refused, nothing written
    if (twhost::png_write_rgb8(argv[5], px.data(), 0, h, pitch)) return 4;
    if (twhost::png_write_rgb8(argv[5], px.data(), w, h, 3 * w - 1)) return 4;
    return twhost::png_write_rgb8(argv[5], px.data(), w, h, pitch) ? 0 : 1;
}
"""


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp / "pngw.cpp"
    src.write_text(MAIN)
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", HOST] + flags + ["-o", exe, str(src)])
    return exe


@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pngw"), [], "pngw")


@pytest.fixture(scope="module")
def decoder():
    r = subprocess.run(["make", "-s", "-C", HOST, "inflate_test"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    L = C.CDLL(os.path.join(HOST, "build", "libinflate_test.so"))
    L.twt_load_rows.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_size_t)]
    L.twt_unfilter.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t]
    return L


def _pixels(w, h, pitch):
    rng = np.random.default_rng(w * 1000 + h)
    buf = np.full((h, pitch), 0xEE, np.uint8)
    buf[:, :3 * w] = rng.integers(0, 256, (h, 3 * w), dtype=np.uint8)
    return buf


def _write(exe, tmp, w, h, pitch):
    buf = _pixels(w, h, pitch)
    raw, png = tmp / ("in_%dx%d.raw" % (w, h)), tmp / ("out_%dx%d.png" % (w, h))
    raw.write_bytes(buf.tobytes()[:pitch * (h - 1) + 3 * w])
    subprocess.check_call([exe, str(raw), str(w), str(h), str(pitch), str(png)])
    return buf[:, :3 * w].reshape(h, w, 3), png


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    p, out = 8, []
    while p < len(data):
        n = int.from_bytes(data[p:p + 4], "big")
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        assert int.from_bytes(data[p + 8 + n:p + 12 + n], "big") == zlib.crc32(kind + body), kind  # a correct CRC-32
        out.append((kind, body))
        p += 12 + n
    assert p == len(data)
    return out


@pytest.mark.parametrize("w,h,pitch", CASES, ids=["%dx%d" % c[:2] for c in CASES])
def test_files_decode_to_the_input_in_pil_and_in_the_projects_decoder(writer, decoder, tmp_path, w, h, pitch):
    from PIL import Image
    want, png = _write(writer, tmp_path, w, h, pitch)
    data = png.read_bytes()
    ch = _chunks(data)
    assert [k for k, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])  # depth 8, colour type 2
    z = ch[1][1]
    raw = h * (1 + 3 * w)
    blocks = -(-raw // 65535)
    assert len(z) == 2 + 5 * blocks + raw + 4 and (z[0] << 8 | z[1]) % 31 == 0
    p = 2
    for b in range(blocks):  # stored blocks: BFINAL on the last only, LEN and its complement
        k = min(65535, raw - 65535 * b)
        assert z[p] == (1 if b == blocks - 1 else 0) and int.from_bytes(z[p + 1:p + 3], "little") == k
        assert int.from_bytes(z[p + 3:p + 5], "little") == k ^ 0xffff
        p += 5 + k
    stream = zlib.decompress(z)
    assert len(stream) == raw and int.from_bytes(z[-4:], "big") == zlib.adler32(stream)  # a correct Adler-32
    with Image.open(png) as im:
        assert im.mode == "RGB" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), want)
    out = C.create_string_buffer(raw + 64)
    ww, hh, cc, n = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    assert decoder.twt_load_rows(str(png).encode(), out, raw + 64, C.byref(ww), C.byref(hh), C.byref(cc), C.byref(n)) == 1
    assert (ww.value, hh.value, cc.value, n.value) == (w, h, 3, raw)
    rows = C.create_string_buffer(out.raw[:raw], raw)
    assert decoder.twt_unfilter(rows, 3 * w, h, 3) == 1
    got = np.frombuffer(rows.raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (got[:, 0] == 0).all() and np.array_equal(got[:, 1:].reshape(h, w, 3), want)


def test_the_seam_sizes_are_on_the_seams():
    sizes = [h * (1 + 3 * w) for w, h, _ in CASES]
    assert sizes[3:] == [65535, 65536, 131070] and sizes[2] > 65535 and sizes[1] < 65535
    assert CASES[2][2] > 3 * CASES[2][0] and CASES[5][2] % 4 == 1  # a padded pitch, an odd one


def test_the_writer_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """host code on the CPU: the program carries the sanitizers' runtimes itself (linked statically) and is run on its own, in
    the environment as it is — the test preloads nothing and takes nothing away"""
    exe = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                            "-static-libubsan"], "pngw_san")
    from PIL import Image
    for w, h, pitch in CASES:
        buf = _pixels(w, h, pitch)
        raw, png = tmp_path / "in.raw", tmp_path / "out.png"
        raw.write_bytes(buf.tobytes()[:pitch * (h - 1) + 3 * w])
        r = subprocess.run([exe, str(raw), str(w), str(h), str(pitch), str(png)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (w, h, r.stderr[-2000:])
        with Image.open(png) as im:
            assert np.array_equal(np.asarray(im), buf[:, :3 * w].reshape(h, w, 3))
