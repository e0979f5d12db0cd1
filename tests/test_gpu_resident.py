"""Resident images on the device: tw_image_keep / tw_image_create_u8 / tw_image_release and tw_submit_image_png / _jpeg
(DESIGN.md §7 "Resident images").

Every comparison is bit for bit on the hit vectors at span 4 and threshold 0 — every fourth pixel of the field whose flow is
not exactly zero, (dx, dy) as the device holds them — and, for the pairs with a flow destination, on the dense field.  The
reference of a resident pair is the plain submit of the same bytes on the same engine; one case also goes against the oracle.

Shapes: 97 x 61 — odd, so the unaligned and partial-tile paths, and the update / window kernels at every level; 333 x 41
under TW_MFREE=2 on a fresh engine, where level 0 runs tw_flow_iter (asserted from the launch counts) and the batch schedule
launches tw_pair_same.  Rows of 97 and 333 bytes put every row of an image at another offset from a 4-byte boundary.
"""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J

pytestmark = pytest.mark.gpu
SPAN, THR = 4, 0.0
SHAPES = {"97x61": (97, 61, False), "333x41_mfree": (333, 41, True)}  # w, h, TW_MFREE=2


@pytest.fixture(params=list(SHAPES))
def shape(request, monkeypatch):
    w, h, mfree = SHAPES[request.param]
    monkeypatch.delenv("TW_SAME_IMAGE", raising=False)
    monkeypatch.delenv("TW_LANES", raising=False)
    if mfree:
        monkeypatch.setenv("TW_MFREE", "2")
        monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    else:
        monkeypatch.delenv("TW_MFREE", raising=False)
    return w, h, mfree


@pytest.fixture
def small(monkeypatch):
    monkeypatch.delenv("TW_MFREE", raising=False)
    return 97, 61


# ---- images in every form ----------------------------------------------------------------------------------------------
_frames = {}


def frames(w, h):
    """f0, f1, f2, f3: four frames of one size (a synthetic screenshot, two warps of it, another screenshot)"""
    import synth
    if (w, h) not in _frames:
        a, b = synth.make_pair(0, h, w)
        c = synth.make_pair(1, h, w)[1]
        d = synth.make_pair(4, h, w)[1]
        assert len({a.tobytes(), b.tobytes(), c.tobytes(), d.tobytes()}) == 4
        _frames[(w, h)] = tuple(np.ascontiguousarray(x) for x in (a, b, c, d))
    return _frames[(w, h)]


def gray15(rgb):
    """libpng 1.5's rgb_to_gray as the device computes it"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return np.where((r == g) & (g == b), r, (9797 * r + 19234 * g + 3737 * b) >> 15).astype(np.uint8)


def filter_rows(raw, bpp):
    """raw [h, nb] -> filtered rows [h, 1 + nb], filter types 0 (none), 1 (sub), 2 (up) in turn (ISO/IEC 15948 §9.2)"""
    h, nb = raw.shape
    x = raw.astype(np.int32)
    left = np.zeros_like(x)
    left[:, bpp:] = x[:, :-bpp]
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    t = np.arange(h) % 3
    pred = np.stack([np.zeros_like(x), left, up])[t, np.arange(h)]
    out = np.empty((h, 1 + nb), np.uint8)
    out[:, 0] = t
    out[:, 1:] = (x - pred) & 255
    return out


def as_rgba(twflow, g):
    """(PngRows of an RGBA image, the gray image the device makes of it, the arrays to overwrite)"""
    h, w = g.shape
    rgba = np.stack([g, np.roll(g, 3, 1), 255 - g, np.full_like(g, 200)], -1)
    rows = filter_rows(rgba.reshape(h, w * 4), 4)
    img = twflow.PngRows(rows, w, h, 6, 8)
    return img, gray15(rgba), [img._rows]


def as_pal4(twflow, g):
    h, w = g.shape
    v = (g >> 4).astype(np.uint8)
    plte = np.stack([np.arange(16) * 17, (np.arange(16) * 29) % 256, 255 - np.arange(16) * 13], -1).astype(np.uint8)
    nb = (w * 4 + 7) // 8
    bits = np.zeros((h, nb * 8), np.uint8)
    bits[:, :w * 4] = ((v[..., None] >> np.arange(3, -1, -1)) & 1).reshape(h, w * 4)
    rows = filter_rows(np.packbits(bits, axis=1), 1)
    img = twflow.PngRows(rows, w, h, 3, 4, plte)
    return img, gray15(plte)[v], [img._rows]


def as_jpeg(twflow, g, q=3):
    """(JpegLuma whose coefficients are the image's forward DCT, the gray image jidctint makes of them, ...)"""
    h, w = g.shape
    bh, bw = -(-h // 8), -(-w // 8)
    pad = np.pad(g.astype(np.float64) - 128, ((0, bh * 8 - h), (0, bw * 8 - w)), mode="edge")
    k = np.arange(8)
    D = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5)
    blocks = pad.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    coef = np.rint(D @ blocks @ D.T / q).astype(np.int16).reshape(bh, bw, 64)  # (the orthonormal 8 x 8 DCT is libjpeg's scale)
    quant = np.full(64, q, np.uint16)
    gray = np.ascontiguousarray(J.blocks_to_image(J.idct_reference(coef.reshape(-1, 64), quant), bw, bh, w, h))
    assert np.abs(gray.astype(int) - g).max() <= 8  # (the picture, up to the quantisation)
    luma = twflow.JpegLuma(coef, quant, w, h)
    return luma, gray, [luma._coef]


def vectors(e, ticket):
    r = e.wait(ticket)
    return r["status"], r["vector"]


def plain(e, a, b, **kw):
    return vectors(e, e.submit(a, b, SPAN, THR, **kw))


# ---- keep, then resubmit -----------------------------------------------------------------------------------------------
KINDS = ["pageable_gray", "page_locked_gray", "rgba_rows", "pal4_rows", "jpeg_coef"]


def submit_kind(twflow, e, kind, g, target):
    """The plain submit of (g in this form, gray target): (ticket, the gray image the batch sees, the host sources)"""
    if kind == "pageable_gray":
        a = g.copy()
        return e.submit(a, target, SPAN, THR), g, [a]
    if kind == "page_locked_gray":
        a, b = e.host_array(g.shape), e.host_array(g.shape)
        a[...] = g
        b[...] = target
        return e.submit(a, b, SPAN, THR), g, [a, b]
    if kind == "jpeg_coef":
        luma, gray, src = as_jpeg(twflow, g)
        return e.submit_jpeg(luma, target, SPAN, THR), gray, src
    img, gray, src = (as_rgba if kind == "rgba_rows" else as_pal4)(twflow, g)
    return e.submit_png(img, twflow.PngRows(target, target.shape[1], target.shape[0]), SPAN, THR), gray, src


@pytest.mark.parametrize("kind", KINDS)
def test_keep_then_resubmit(twflow, oracle, shape, kind):
    w, h, mfree = shape
    f0, f1, f2, f3 = frames(w, h)
    rgba_t, rgba_gray, _ = as_rgba(twflow, f2)
    jpeg_t, jpeg_gray, _ = as_jpeg(twflow, f3)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        tk, gray, sources = submit_kind(twflow, e, kind, f0, f1)
        img = e.keep(tk, "expect")
        assert img.size == (w, h)
        first = vectors(e, tk)
        for s in sources:
            s[...] = 0  # the host source is gone: what follows reads the device's copy
        want = {"gray": plain(e, gray, f1), "rgba": plain(e, gray, rgba_gray), "jpeg": plain(e, gray, jpeg_gray)}
        assert first == want["gray"] and len(first[1]) > 0
        if kind == "pageable_gray" and not mfree:
            fx, fy = oracle.farneback(gray, f1)
            assert first[1] == oracle.span_scan(fx, fy, SPAN, THR)
        made = e.image(gray)
        for im in (img, made):
            assert vectors(e, e.submit_image(im, f1, SPAN, THR)) == want["gray"]
            assert vectors(e, e.submit_image(im, rgba_t, SPAN, THR)) == want["rgba"]
            assert vectors(e, e.submit_image(im, jpeg_t, SPAN, THR)) == want["jpeg"]
        assert want["gray"] != want["rgba"] != want["jpeg"]
        if mfree:
            assert e.launch_counts().flow_iter() > 0
        img.release()
        made.release()
        assert e.resident()["images"] == 0 and e.resident()["bytes_in_use"] == 0


# ---- sequences: the target of one pair is the expected image of the next -------------------------------------------------
@pytest.mark.parametrize("form", ["gray", "rgba_rows", "jpeg_coef"])
def test_kept_target_is_the_next_pairs_expected_image(twflow, shape, form):
    w, h, _ = shape
    f0, f1, f2, _ = frames(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        if form == "gray":
            g1, t0 = f1, e.submit(f0, f1, SPAN, THR)
        elif form == "rgba_rows":
            img1, g1, _ = as_rgba(twflow, f1)
            t0 = e.submit_png(twflow.PngRows(f0, w, h), img1, SPAN, THR)
        else:
            luma1, g1, _ = as_jpeg(twflow, f1)
            t0 = e.submit_jpeg(f0, luma1, SPAN, THR)
        e.launch_counts(reset=True)
        kept = e.keep(t0, "target")  # (rows / coefficients: the slot is written when the batch launches — the copy waits)
        t1 = e.submit_image(kept, f2, SPAN, THR)  # ... and this pair sits in that very batch
        got0, got1 = vectors(e, t0), vectors(e, t1)
        cnt = e.launch_counts()
        assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1  # one batch of two pairs
        kept.release()
        assert got0 == plain(e, f0, g1)
        assert got1 == plain(e, g1, f2)
        assert e.resident()["bytes_in_use"] == 0


# ---- mixed batches -------------------------------------------------------------------------------------------------------
def test_resident_and_ordinary_pairs_share_a_batch(twflow, shape):
    w, h, mfree = shape
    f0, f1, f2, f3 = frames(w, h)
    pairs = [(f0, f1), (f1, f2), (f2, f2), (f3, f0)]  # (the third pair is identical)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        e.launch_counts(reset=True)
        want = [e.submit(a, b, SPAN, THR) for a, b in pairs]
        want = [vectors(e, t) for t in want]
        flags_plain, cnt_plain = e.same_flags(), e.launch_counts(reset=True)
        assert all(len(v[1]) > 0 for i, v in enumerate(want) if i != 2) and len({str(v) for v in want}) == 4
        res = {i: e.image(pairs[i][0]) for i in (1, 2)}
        e.launch_counts(reset=True)
        tks = [e.submit_image(res[i], b, SPAN, THR) if i in res else e.submit(a, b, SPAN, THR) for i, (a, b) in enumerate(pairs)]
        got = [vectors(e, t) for t in tks]
        flags, cnt = e.same_flags(), e.launch_counts(reset=True)
        assert got == want
        assert cnt == cnt_plain  # the launches of ONE batch of four ordinary pairs, family by family
        assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1
        assert flags == flags_plain
        if mfree:
            assert cnt.flow_iter() > 0 and cnt["tw_pair_same"] >= 1
            assert flags == [0, 0, 1, 0]


# ---- reconcile ------------------------------------------------------------------------------------------------------------
def test_resident_expected_image_reconciles_or_refuses_the_target(twflow):
    import synth
    a = np.ascontiguousarray(synth.make_pair(0, 80, 100)[0])
    b = np.ascontiguousarray(synth.make_pair(0, 78, 103)[1])
    far = np.ascontiguousarray(synth.make_pair(0, 80, 106)[1])
    tgt, _, _ = as_rgba(twflow, b)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        want = vectors(e, e.submit_png(twflow.PngRows(a, 100, 80), tgt, SPAN, THR))
        img = e.image(a)
        e.launch_counts(reset=True)
        assert vectors(e, e.submit_image(img, tgt, SPAN, THR)) == want
        assert e.launch_counts()["tw_resize_u8"] == 1
        assert vectors(e, e.submit_image(img, b, SPAN, THR)) == vectors(e, e.submit(a, b, SPAN, THR, reconcile=True))
        before = e.submit(a, a, SPAN, THR)
        with pytest.raises(twflow.TwError) as ei:
            e.submit_image(img, far, SPAN, THR)
        assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
        with pytest.raises(twflow.TwError) as ei:
            e.submit_image(img, as_rgba(twflow, far)[0], SPAN, THR)
        assert ei.value.code == twflow.TW_E_DONT_MATCH_SIZE
        after = e.submit(a, a, SPAN, THR)
        assert after[0] == before[0] + 1  # no ticket consumed
        e.wait(before), e.wait(after)


# ---- fields -----------------------------------------------------------------------------------------------------------------
def test_init_and_flow_work_for_a_resident_pair(twflow, shape):
    w, h, _ = shape
    f0, f1, _, _ = frames(w, h)
    rng = np.random.default_rng(3)
    init = (rng.random((2, h, w), np.float32) * 4 - 2).astype(np.float32)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out = e.host_array((4, 2, h, w), np.float32)
        out[...] = np.nan
        img = e.image(f0)
        want_f = vectors(e, e.submit(f0, f1, SPAN, THR, flow=out[0]))
        got_f = vectors(e, e.submit_image(img, f1, SPAN, THR, flow=out[1]))
        want_i = vectors(e, e.submit(f0, f1, SPAN, THR, init=init, flow=out[2]))
        got_i = vectors(e, e.submit_image(img, f1, SPAN, THR, init=init, flow=out[3]))
        assert got_f == want_f and got_i == want_i and want_i != want_f
        assert not np.isnan(out).any()
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
        assert np.array_equal(out[2].view(np.uint32), out[3].view(np.uint32))
        gx, gy, _ = e.calculate_internal(f0, f1)
        assert np.array_equal(out[1].view(np.uint32), np.stack([gx, gy]).view(np.uint32))


# ---- lifetime ---------------------------------------------------------------------------------------------------------------
def test_release_before_flush_and_steady_state_storage(twflow, small):
    w, h = small
    f0, f1, _, _ = frames(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        want, want_same = plain(e, f0, f1), plain(e, f1, f1)
        img = e.image(f0)
        tk = e.submit_image(img, f1, SPAN, THR)
        img.release()  # the open batch still reads it
        with pytest.raises(twflow.TwError) as ei:
            e.submit_image(img, f1, SPAN, THR)  # ... but the handle is gone
        assert ei.value.code == twflow.TW_E_BAD_PARAMETER
        r = e.resident()
        assert r["images"] == 1 and r["bytes_in_use"] == (w * h + 255) // 256 * 256
        e.flush()
        assert vectors(e, tk) == want
        r = e.resident()
        assert r["images"] == 0 and r["bytes_in_use"] == 0 and r["chunk_allocs"] == 1 and r["bytes_reserved"] >= 64 << 20
        mem1 = None
        for i in range(200):
            tk = e.submit(f0, f1, SPAN, THR)
            kept = e.keep(tk, "expect" if i % 2 else "target")
            e.wait_count(tk)
            if i % 50 == 0:
                assert vectors(e, e.submit_image(kept, f1, SPAN, THR)) == (want if i % 2 else want_same)  # (f0, f1) / (f1, f1)
            kept.release()
            if mem1 is None:
                mem1 = (e.memory(), e.resident())
        assert (e.memory(), e.resident()) == mem1
        assert e.resident()["chunk_allocs"] == 1 and e.memory()["device_bytes"] >= e.resident()["bytes_reserved"]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_handles_and_tickets_are_refused_and_nothing_is_consumed(twflow, small):
    w, h = small
    f0, f1, _, _ = frames(w, h)
    bad = twflow.TW_E_BAD_PARAMETER
    with twflow.Engine(0, twflow.default_params(), slots=2) as e, twflow.Engine(0, twflow.default_params(), slots=2) as other:
        L = e._L
        want = plain(e, f0, f1)
        waited = e.submit(f0, f1, SPAN, THR)
        e.wait(waited)
        foreign = other.image(f0)
        released = e.image(f0)
        released.release()
        live = e.image(f0)
        opened = e.submit(f0, f1, SPAN, THR)  # an open batch of one pair
        rows = twflow.PngRows(f1, w, h)
        luma = twflow.JpegLuma.from_gray(f1)
        out, tk = C.c_void_p(), C.c_int64(-5)
        garbage = C.c_void_p(0x10)  # (never dereferenced: looked up)
        for handle in (released._h, foreign._h, None, garbage):
            assert L.tw_submit_image_png(e._h, handle, C.byref(rows), SPAN, THR, None, None, C.byref(tk)) == bad
            assert L.tw_submit_image_jpeg(e._h, handle, C.byref(luma), SPAN, THR, None, None, C.byref(tk)) == bad
            assert L.tw_image_release(e._h, handle) == bad
            assert L.tw_image_size(e._h, handle, None, None) == bad
        for ticket, which in ((waited[0], 0), (opened[0] + 1, 0), (0, 0), (-1, 1), (opened[0], 2), (opened[0], -1)):
            assert L.tw_image_keep(e._h, ticket, which, C.byref(out)) == bad
            assert not out.value
        assert L.tw_image_keep(e._h, opened[0], 0, None) == bad
        assert tk.value == -5
        assert e.resident()["images"] == 1
        nxt = e.submit_image(live, f1, SPAN, THR)
        assert nxt[0] == opened[0] + 1  # the next ticket number is unchanged, the open batch took the pair
        assert vectors(e, opened) == want and vectors(e, nxt) == want
        assert foreign.size == (w, h)  # (the other engine's image is untouched)
