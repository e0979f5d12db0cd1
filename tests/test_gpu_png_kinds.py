"""tw_submit_png / tw_stage_png_decode: palette, 1- / 2- / 4-bit gray, 16-bit gray and 16-bit gray + alpha PNG rows on the
device (kernel tw_png_unfilter; DESIGN.md §7 "PNG kinds on the device").

Parity bar: BYTE-EXACT, the way tests/test_gpu_png.py sets it.  Images are FILTERED here in numpy at byte level (ISO/IEC
15948 §9.2 with the kind's byte distance max(1, bits per pixel / 8)) and the kernel has to give back the converted image.
The expected gray is computed in numpy from the packed samples: the bits unpacked most significant first, v * 255 // max
for gray, libpng 1.5's truncating 15-bit formula on PLTE[v] for palette, the high byte for 16 bits.  Through the whole
call the reference's golden pair gives the reference's 24 golden vectors in every form it can be handed over in.
"""
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
ADDON = os.path.join(HOST, "build", "Release", "tidalwave.node")

# name -> (IHDR colour type, bit depth, samples per pixel)
KINDS = {"gray1": (0, 1, 1), "gray2": (0, 2, 1), "gray4": (0, 4, 1), "gray16": (0, 16, 1),
         "pal1": (3, 1, 1), "pal2": (3, 2, 1), "pal4": (3, 4, 1), "pal8": (3, 8, 1), "ga16": (4, 16, 2)}


def gray15(rgb):
    """libpng 1.5.12 rgb_to_gray as OpenCV 2.4.9 configures it: truncated 15-bit coefficients, truncated sum."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (9797 * r + 19234 * g + 3737 * b) >> 15
    return np.where((r == g) & (g == b), r, y).astype(np.uint8)


def filter_bytes(raw, bpp, types):
    """raw [h, nb] uint8 (a row's bytes) -> filtered rows [h, 1 + nb]: filter type types[y] per row, the left neighbour
    bpp bytes back (§9.2)."""
    h, nb = raw.shape
    x = raw.astype(np.int32)
    left = np.zeros_like(x)
    left[:, bpp:] = x[:, :-bpp] if nb > bpp else 0
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    ul = np.zeros_like(x)
    ul[1:] = left[:-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    pred = np.stack([np.zeros_like(x), left, up, (left + up) >> 1, paeth])
    t = np.asarray(types)
    out = np.empty((h, 1 + nb), np.uint8)
    out[:, 0] = t
    out[:, 1:] = (x - pred[t, np.arange(h)]) & 255
    return out


def make_image(kind, w, h, rng, smooth=True):
    """(row bytes [h, nb], byte distance, palette or None, expected gray [h, w]) of a random image of this kind; the pad
    bits of a packed row's last byte are random."""
    ct, depth, spp = KINDS[kind]
    plte = None
    if depth == 16:
        v = rng.integers(0, 65536, (h, w, spp))
        if smooth:
            v[h // 3: h // 2] = (np.cumsum(rng.integers(-300, 301, (max(h // 2 - h // 3, 0), w, spp)), axis=1) + 32768) & 65535
        raw = np.stack([v >> 8, v & 255], -1).reshape(h, w * spp * 2).astype(np.uint8)
        return raw, 2 * spp, None, (v[..., 0] >> 8).astype(np.uint8)
    v = rng.integers(0, 1 << depth, (h, w))
    if smooth and depth == 8:
        v[h // 3: h // 2] = (np.cumsum(rng.integers(-2, 3, (max(h // 2 - h // 3, 0), w)), axis=1) + 128) & 255
    if ct == 3:
        plte = rng.integers(0, 256, (1 << depth, 3)).astype(np.uint8)
        plte[::3] = plte[::3, :1]  # every third entry is a gray triplet: the r == g == b shortcut
        want = gray15(plte)[v]
    else:
        want = (v * 255 // ((1 << depth) - 1)).astype(np.uint8)
    if depth == 8:
        return v.astype(np.uint8), 1, plte, want
    nb = (w * depth + 7) // 8
    bits = np.zeros((h, nb * 8), np.uint8)
    bits[:, :w * depth] = ((v[..., None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, w * depth)
    bits[:, w * depth:] = rng.integers(0, 2, (h, nb * 8 - w * depth))
    return np.packbits(bits, axis=1), 1, plte, want


SHAPES = [  # w, h, waves (0 = the engine's choice)
    (1, 1, 0), (3, 2, 0), (8, 5, 0), (9, 5, 0), (33, 3, 0), (64, 40, 0), (67, 70, 0),
    (37, 130, 1),    # three bands of 64 rows
    (333, 257, 4),   # 257 rows cross a band of 256
    (2500, 70, 0),   # wider than 2048: four waves per image
]
STAGE_CASES = [(k, w, h, wv) for k in KINDS for (w, h, wv) in SHAPES] + [("pal8", 1920, 1080, 0), ("gray1", 1920, 1080, 0)]


@pytest.mark.parametrize("kind,w,h,waves", STAGE_CASES)
def test_stage_png_decode_every_kind_and_filter_type(engine, twflow, kind, w, h, waves):
    ct, depth, _ = KINDS[kind]
    rng = np.random.default_rng(w * 7 + h * 3 + ct * 31 + depth)
    raw, bpp, plte, want = make_image(kind, w, h, rng)
    engine.launch_counts(reset=True)
    for types in (rng.integers(0, 5, h), np.full(h, 4), np.full(h, 3), np.arange(h) % 5):
        rows = filter_bytes(raw, bpp, types)
        got = engine.stage_png_decode(twflow.PngRows(rows, w, h, ct, depth, plte), waves)
        assert np.array_equal(got, want), "types %s..." % list(types[:6])
    cnt = engine.launch_counts()
    assert cnt["tw_png_unfilter"] == 4 and cnt.last_z["tw_png_unfilter"] == 1, cnt


@pytest.mark.parametrize("ch,ct", [(1, 0), (2, 4), (3, 2), (4, 6)])
def test_stage_png_decode_equals_stage_png_unfilter_on_the_8_bit_kinds(engine, twflow, ch, ct):
    w, h = 67, 70
    rng = np.random.default_rng(ch)
    raw = rng.integers(0, 256, (h, w * ch), dtype=np.uint8)
    rows = filter_bytes(raw, ch, rng.integers(0, 5, h))
    assert np.array_equal(engine.stage_png_decode(twflow.PngRows(rows, w, h, ct, 8)), engine.stage_png_unfilter(rows, ch, w, h))


IDENT = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)


def test_png_kernel_time_is_the_same_kernel_timed(engine, twflow):
    """tw_debug_png_kernel_time: one untimed launch and `iters` timed ones of tw_png_unfilter, a positive time for one; the
    refusals of tw_stage_png_decode."""
    rng = np.random.default_rng(9)
    raw, bpp, plte, _ = make_image("pal4", 67, 70, rng)
    img = twflow.PngRows(filter_bytes(raw, bpp, np.arange(70) % 5), 67, 70, 3, 4, plte)
    engine.launch_counts(reset=True)
    us = engine.png_kernel_time(img, iters=3)
    assert 0.0 < us < 1e5
    assert engine.launch_counts()["tw_png_unfilter"] == 4
    with pytest.raises(twflow.TwError) as ei:
        engine.png_kernel_time(twflow.PngRows(raw, 67, 70, 2, 16), iters=3)
    assert ei.value.code == twflow.TW_E_UNSUPPORTED


def as_gray16(g, rng):
    """A gray image as 16-bit gray rows' bytes: value << 8 | a random low byte."""
    return np.stack([g, rng.integers(0, 256, g.shape, dtype=np.uint8)], -1).reshape(g.shape[0], -1)


def test_golden_pair_in_every_form_gives_the_golden_vectors(twflow, golden):
    case = golden["revision2_capture2"]
    want = [(d["x"], d["y"], d["dx"], d["dy"]) for d in case["vector"]]
    a, b = case["expect_img"], case["target_img"]
    h, w = a.shape
    assert (w, h) == (180, 117)
    rng = np.random.default_rng(5)
    types = np.arange(h) % 5
    span, thr = case["span"], float(case["threshold"])
    P = twflow.PngRows
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        # (the 16-bit pair first: the batch's slots are sized by its first filtered image, and all four pairs fit them)
        ga, gb = filter_bytes(as_gray16(a, rng), 2, types), filter_bytes(as_gray16(b, rng), 2, types)
        t2 = e.submit_png(P(ga, w, h, 0, 16), P(gb, w, h, 0, 16), span, thr)
        pa, pb = filter_bytes(a, 1, types), filter_bytes(b, 1, rng.integers(0, 5, h))
        t1 = e.submit_png(P(pa, w, h, 3, 8, IDENT), P(pb, w, h, 3, 8, IDENT), span, thr)
        t3 = e.submit_png(P(pa, w, h, 3, 8, IDENT), P(b, w, h), span, thr)  # mixed pair: plain gray target
        la, lb = e.host_array(pa.shape), e.host_array(gb.shape)             # page-locked: DMA in place
        la[:] = pa
        lb[:] = gb
        t4 = e.submit_png(P(la, w, h, 3, 8, IDENT), P(lb, w, h, 0, 16), span, thr)
        for t in (t1, t2, t3, t4):
            res = e.wait(t)
            assert res["status"] == "SUSPICIOUS" and res["vector"] == want


def pack(v, depth):
    h, w = v.shape
    nb = (w * depth + 7) // 8
    bits = np.zeros((h, nb * 8), np.uint8)
    bits[:, :w * depth] = ((v[..., None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, w * depth)
    return np.packbits(bits, axis=1)


@pytest.fixture(scope="module")
def lossy_pair():
    import synth
    return synth.make_pair(2, 135, 243)  # one painted rectangle; 243 pixels: 4- and 1-bit rows end inside a byte


def test_lossy_kinds_answer_the_oracle_on_the_decoded_grays(twflow, oracle, lossy_pair):
    """A pair quantised to 16 and to 2 levels, as palette-4, gray-4 and gray-1: the vectors of the oracle on the grays that
    numpy decodes from the same samples."""
    a, b = lossy_pair
    h, w = a.shape
    types = np.arange(h) % 5
    plte16 = np.repeat((np.arange(16) * 16 + 3).astype(np.uint8)[:, None], 3, 1)
    plte16[5] = (90, 70, 120)  # two entries that are no gray triplets
    plte16[11] = (160, 190, 150)
    forms = []  # (colour type, depth, palette, samples a, samples b, gray a, gray b)
    qa, qb = a >> 4, b >> 4
    forms.append((3, 4, plte16, qa, qb, gray15(plte16)[qa], gray15(plte16)[qb]))
    forms.append((0, 4, None, qa, qb, (qa * 17).astype(np.uint8), (qb * 17).astype(np.uint8)))
    ba, bb = a >> 7, b >> 7
    forms.append((0, 1, None, ba, bb, (ba * 255).astype(np.uint8), (bb * 255).astype(np.uint8)))
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        tickets = []
        for ct, depth, plte, sa, sb, ga, gb in forms:
            ra, rb = filter_bytes(pack(sa, depth), 1, types), filter_bytes(pack(sb, depth), 1, types)
            img = twflow.PngRows(ra, w, h, ct, depth, plte)
            assert np.array_equal(e.stage_png_decode(img), ga)
            tickets.append(e.submit_png(img, twflow.PngRows(rb, w, h, ct, depth, plte), 10, 2.0))
        for t, (_, _, _, _, _, ga, gb) in zip(tickets, forms):
            fx, fy = oracle.farneback(ga, gb)
            assert e.wait(t)["vector"] == oracle.span_scan(fx, fy, 10, 2.0)


def test_sized_palette_target_equals_submit_u8_on_the_resized_decode(twflow, lossy_pair):
    a, b = lossy_pair
    h, w = a.shape
    tw_, th_ = w - 3, h + 2
    bt = np.ascontiguousarray(np.vstack([b, b[-2:]])[:, :tw_])
    types = np.arange(th_) % 5
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        resized = e.stage_resize_u8(bt, w, h)
        want = e.wait(e.submit(a, resized, 10, 2.0))["vector"]
        ea = twflow.PngRows(filter_bytes(a, 1, np.arange(h) % 5), w, h, 3, 8, IDENT)
        tb = twflow.PngRows(filter_bytes(bt, 1, types), tw_, th_, 3, 8, IDENT)
        assert e.wait(e.submit_png(ea, tb, 10, 2.0))["vector"] == want
        far = np.ascontiguousarray(b[:, :w - 6])
        t_before = e.submit(a, b, 10, 2.0)
        with pytest.raises(twflow.TwError) as ei:
            e.submit_png(ea, twflow.PngRows(filter_bytes(far, 1, np.zeros(h, int)), w - 6, h, 3, 8, IDENT), 10, 2.0)
        assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
        t_after = e.submit(a, b, 10, 2.0)
        assert t_after[0] == t_before[0] + 1  # the refusal consumed no ticket
        e.wait(t_before)
        e.wait(t_after)


def test_rgba_pair_is_launch_for_launch_the_png8_call(twflow, lossy_pair):
    a, b = lossy_pair
    h, w = a.shape
    rgba = lambda g: np.dstack([g, np.roll(g, 3, 1), 255 - g, g]).reshape(h, w * 4)
    ra, rb = filter_bytes(rgba(a), 4, np.arange(h) % 5), filter_bytes(rgba(b), 4, np.arange(h) % 5)
    counts, results = [], []
    for new in (False, True):
        with twflow.Engine(0, twflow.default_params(), slots=4) as e:
            e.launch_counts(reset=True)
            if new:
                t = e.submit_png(twflow.PngRows(ra, w, h, 6, 8), twflow.PngRows(rb, w, h, 6, 8), 10, 2.0)
            else:
                t = e.submit_png8(ra, 4, rb, 4, w, h, 10, 2.0)
            results.append(e.wait(t)["vector"])
            counts.append(dict(e.launch_counts()))
    assert counts[0] == counts[1]
    assert results[0] == results[1]


def test_bad_palette_index_fails_its_own_ticket_only(twflow, oracle, lossy_pair):
    a, b = lossy_pair
    h, w = a.shape
    plte = np.repeat((np.arange(10) * 25).astype(np.uint8)[:, None], 3, 1)
    ia, ib = (a.astype(np.int64) * 10 // 256).astype(np.uint8), (b.astype(np.int64) * 10 // 256).astype(np.uint8)
    bad = ia.copy()
    bad[h // 2, w // 2] = 10
    types = np.arange(h) % 5
    P = lambda idx: twflow.PngRows(filter_bytes(idx, 1, types), w, h, 3, 8, plte)
    fx, fy = oracle.farneback(plte[ia][..., 0], plte[ib][..., 0])
    want = oracle.span_scan(fx, fy, 10, 2.0)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        t0 = e.submit_png(P(ia), P(ib), 10, 2.0)
        t1 = e.submit_png(P(bad), P(ib), 10, 2.0)
        t2 = e.submit_png(P(ia), P(ib), 10, 2.0)
        assert e.wait(t0)["vector"] == want
        with pytest.raises(twflow.TwError) as ei:
            e.wait(t1)
        assert ei.value.code == twflow.TW_E_BAD_IMAGE_FORMAT and "expected" in str(ei.value)
        assert e.wait(t2)["vector"] == want
        with pytest.raises(twflow.TwError) as ei:
            e.stage_png_decode(P(bad))
        assert ei.value.code == twflow.TW_E_BAD_IMAGE_FORMAT
        assert np.array_equal(e.stage_png_decode(P(ia)), plte[ia][..., 0])  # every index below 10: accepted


def test_refusals_queue_nothing(twflow):
    w, h = 64, 48
    rng = np.random.default_rng(3)
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    P = twflow.PngRows
    plain = P(gray, w, h)
    rows = lambda nb: filter_bytes(rng.integers(0, 256, (h, nb), dtype=np.uint8), 1, np.zeros(h, int))
    plte = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    bad_filter = filter_bytes(rng.integers(0, 256, (h, w // 8), dtype=np.uint8), 1, np.zeros(h, int))
    bad_filter[2, 0] = 5
    fmt, uns = twflow.TW_E_BAD_IMAGE_FORMAT, twflow.TW_E_UNSUPPORTED
    cases = [
        (P(rows(w * 3 // 2), w, h, 2, 4), fmt),                          # colour type 2 at depth 4
        (P(rows(w), w, h, 3, 8), fmt),                                   # palette without PLTE
        (P(rows(w), w, h, 3, 8, plte, palette_entries=0), fmt),
        (P(rows(w), w, h, 3, 8, np.vstack([plte, plte[:1]]), palette_entries=257), fmt),
        (P(rows(w * 6), w, h, 2, 16), uns),                              # RGB16: a valid kind the device does not take
        (P(bad_filter, w, h, 0, 1), fmt),                                # filter byte 5 in row 2, at the gray-1 row length
    ]
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        first = e.submit(gray, gray, 10, 5.0)
        e.launch_counts(reset=True)
        for img, code in cases:
            for pair in ((img, plain), (plain, img)):
                with pytest.raises(twflow.TwError) as ei:
                    e.submit_png(pair[0], pair[1], 10, 5.0)
                assert ei.value.code == code, (img.color_type, img.bit_depth, img.palette_entries)
        assert sum(e.launch_counts().values()) == 0
        last = e.submit(gray, gray, 10, 5.0)
        assert last[0] == first[0] + 1  # no refusal consumed a ticket
        e.wait(first)
        e.wait(last)


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def write_palette_png(path, g):
    """g as a palette-8 file with the identity gray palette, adaptive-looking filters (y % 5)."""
    h, w = g.shape
    raw = filter_bytes(g, 1, np.arange(h) % 5).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)) +
                _chunk(b"PLTE", IDENT.tobytes()) + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the built addon is not available")
def test_cli_on_the_golden_pair_as_palette_files(tmp_path, golden):
    case = golden["revision2_capture2"]
    pa, pb = str(tmp_path / "expect.png"), str(tmp_path / "target.png")
    write_palette_png(pa, case["expect_img"])
    write_palette_png(pb, case["target_img"])
    outs = []
    for kinds in ("1", "0"):
        r = subprocess.run(["node", "commandline.js", "-threshold", "5", "-span", "10", "-pyrLevels", "3", pa, pb],
                           cwd=HOST, capture_output=True, text=True, timeout=120, env=dict(os.environ, TW_DEVICE_PNG_KINDS=kinds))
        assert r.returncode == 0, r.stderr
        docs = json.loads("[" + r.stdout.replace("}\n{", "},{") + "]")
        assert docs[0]["status"] == "SUSPICIOUS" and docs[0]["vector"] == case["vector"]
        assert docs[-1] == {"request": 1, "data": 1, "error": 0}
        for d in docs:
            d.pop("time", None)
        outs.append(docs)
    assert outs[0] == outs[1]
