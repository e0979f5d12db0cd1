"""Ignore regions on the device: tw_mask_rects and the tw_submit_*_ignore calls (DESIGN.md §7 "Ignore regions").

The kernel alone goes through tw_stage_mask_rects, byte for byte against numpy — t[y0:y1, x0:x1] = e[y0:y1, x0:x1] after
clipping — on the whole edited image and on the 512 guard bytes around the target's slot (the entry point itself refuses a
written byte of the slot's padding).  Sizes: 67 x 41 (w % 4 == 3: rows at every offset from a 4-byte boundary), 64 x 8,
5 x 3, 1 x 1, and 333 x 9 for a rectangle wider than one 256-byte tile.

The pipeline is compared bit for bit at span 4 and threshold 0 with the plain submit of the host-edited target on the same
engine, minus the vectors whose grid point lies inside a rectangle; the shapes and image builders are those of
tests/test_gpu_resident.py (97 x 61, and 333 x 41 under TW_MFREE=2 where the batch schedule launches tw_pair_same).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_resident import SPAN, THR, as_jpeg, as_pal4, as_rgba, frames, plain, shape, small, vectors  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- the numpy reference ---------------------------------------------------------------------------------------------------
def clip(rects, w, h):
    out = []
    for x, y, rw, rh in rects:
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + rw, w), min(y + rh, h)
        if x0 < x1 and y0 < y1:
            out.append((x0, y0, x1, y1))
    return out


def edit(expect, target, rects):
    """the host-edited target: inside every clipped rectangle the expected image's pixels"""
    t = np.array(target, np.uint8, copy=True)
    h, w = t.shape
    for x0, y0, x1, y1 in clip(rects, w, h):
        t[y0:y1, x0:x1] = expect[y0:y1, x0:x1]
    return t


def outside(vecs, rects, w, h):
    cl = clip(rects, w, h)
    return [v for v in vecs if not any(x0 <= v[0] < x1 and y0 <= v[1] < y1 for x0, y0, x1, y1 in cl)]


def reference(e, expect, target, rects, **kw):
    """(status, vectors) of the plain submit of the edited target, minus the vectors inside the rectangles; and how many
    of its vectors the rectangles suppress"""
    h, w = expect.shape
    _, vecs = plain(e, expect, edit(expect, target, rects), **kw)
    left = outside(vecs, rects, w, h)
    return ("OK" if not left else "SUSPICIOUS", left), len(vecs) - len(left)


def main_rects(w, h):
    """one rectangle in the middle of the image (the warp around it reaches in: vectors to suppress) and one at the edge,
    clipped, at odd offsets"""
    return [(w // 3 + 1, h // 4 + 1, w // 3, h // 2), (w - 9, -3, 20, 11)]


# ---- the kernel alone ------------------------------------------------------------------------------------------------------
def stage_images(w, h, seed=0):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, 256, (h, w), dtype=np.uint8)
    t = e ^ rng.integers(1, 256, (h, w), dtype=np.uint8)  # differs from e in every byte
    return e, t


def check_stage(eng, w, h, rects, nonempty):
    e, t = stage_images(w, h)
    eng.launch_counts(reset=True)
    out, guard = eng.stage_mask_rects(e, t, rects, guard=True)
    want = edit(e, t, rects)
    assert np.array_equal(out, want)
    assert (guard == 0xA5).all()
    cnt = eng.launch_counts()
    assert cnt["tw_mask_rects"] == (1 if nonempty else 0)
    if nonempty:
        assert cnt.last_z["tw_mask_rects"] == nonempty
    return out


SIZES = [(67, 41), (64, 8), (5, 3), (1, 1)]


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_single_rectangles(engine, w, h):
    for x in range(8):  # 1 x 1 at every byte lane
        for y in (0, h // 2, h - 1):
            check_stage(engine, w, h, [(x, y, 1, 1)], 1 if x < w else 0)
    assert np.array_equal(check_stage(engine, w, h, [(0, 0, w, h)], 1), stage_images(w, h)[0])  # the whole image
    check_stage(engine, w, h, [(w // 2, 0, 1, h)], 1)  # one column
    check_stage(engine, w, h, [(0, h // 2, w, 1)], 1)  # one row
    check_stage(engine, w, h, [(w - 1, 0, 1, h)], 1)  # the last column
    # clipped at each edge, and a negative origin
    check_stage(engine, w, h, [(-5, h // 3, 7, 2)], 1)
    check_stage(engine, w, h, [(w - 2, h // 3, 40, 2)], 1)
    check_stage(engine, w, h, [(w // 3, -4, 3, 6)], 1)
    check_stage(engine, w, h, [(w // 3, h - 1, 3, 50)], 1)
    check_stage(engine, w, h, [(-3, -2, 5, 4)], 1)
    check_stage(engine, w, h, [(-3, -2, 2 ** 31 - 1, 2 ** 31 - 1)], 1)  # x + width beyond 32 bits: the whole image
    # wholly outside, zero area: nothing changes, nothing is launched
    for r in [(w, 0, 3, 3), (0, h, 3, 3), (-4, 0, 4, 3), (0, -4, 3, 4), (1, 1, 0, 5), (1, 1, 5, 0), (0, 0, 0, 0),
              (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31, 5, 5)]:
        assert np.array_equal(check_stage(engine, w, h, [r], 0), stage_images(w, h)[1])
    assert np.array_equal(check_stage(engine, w, h, [], 0), stage_images(w, h)[1])


@pytest.mark.parametrize("w,h", [(67, 41), (64, 8)])
def test_kernel_several_rectangles(engine, w, h):
    # two rectangles that meet inside one dword, on the same rows, in each order: byte stores, no read-modify-write
    a, b = (0, 1, 5, h - 2), (5, 1, 4, h - 2)
    check_stage(engine, w, h, [a, b], 2)
    check_stage(engine, w, h, [b, a], 2)
    check_stage(engine, w, h, [(1, 0, 2, h), (3, 0, 1, h), (4, 0, 3, h)], 3)  # three inside dwords 0 and 1
    # overlapping
    check_stage(engine, w, h, [(2, 1, 30, 5), (17, 3, 40, 4)], 2)
    # 32 rectangles, one of them empty after clipping
    rects = [((7 * i) % (w - 2), (5 * i) % (h - 1), 1 + i % 9, 1 + i % 4) for i in range(31)] + [(w, 0, 1, 1)]
    check_stage(engine, w, h, rects, 31)
    check_stage(engine, w, h, rects[:31] + [(0, h - 1, 3, 1)], 32)


def test_kernel_rectangle_wider_than_a_tile(engine):
    check_stage(engine, 333, 9, [(3, 1, 325, 7)], 1)
    check_stage(engine, 333, 9, [(0, 0, 333, 9), (1, 8, 300, 1), (50, 2, 4, 4)], 3)  # (the grid tiles the largest one)


def test_refusals_leave_the_engine_usable_and_consume_no_ticket(twflow, small):
    w, h = small
    f0, f1, _, _ = frames(w, h)
    bad = twflow.TW_E_BAD_PARAMETER
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        L = e._L
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
        want, _ = reference(e, f0, f1, [(10, 10, 20, 20)])
        opened = e.submit(f0, f1, SPAN, THR)  # an open batch of one pair
        img = e.image(f0)
        rows, luma = twflow.PngRows(f1, w, h), twflow.JpegLuma.from_gray(f1)
        rows0, luma0 = twflow.PngRows(f0, w, h), twflow.JpegLuma.from_gray(f0)
        r33 = (twflow.Rect * 33)(*[twflow.Rect(1, 1, 2, 2)] * 33)
        neg_w = (twflow.Rect * 2)(twflow.Rect(1, 1, 2, 2), twflow.Rect(5, 5, -1, 3))
        neg_h = (twflow.Rect * 1)(twflow.Rect(5, 5, 3, -1))
        tk = C.c_int64(-5)
        out = np.empty((h, w), np.uint8)
        for rs, n in ((r33, 33), (r33, -1), (neg_w, 2), (neg_h, 1), (None, 1)):
            assert L.tw_submit_u8_ignore(e._h, u8(f0), w, h, w, u8(f1), w, h, w, SPAN, THR, None, None, rs, n, C.byref(tk)) == bad
            assert L.tw_submit_png_ignore(e._h, C.byref(rows0), C.byref(rows), SPAN, THR, None, None, rs, n, C.byref(tk)) == bad
            assert L.tw_submit_jpeg_ignore(e._h, C.byref(luma0), C.byref(luma), SPAN, THR, None, None, rs, n, C.byref(tk)) == bad
            assert L.tw_submit_image_png_ignore(e._h, img._h, C.byref(rows), SPAN, THR, None, None, rs, n, C.byref(tk)) == bad
            assert L.tw_submit_image_jpeg_ignore(e._h, img._h, C.byref(luma), SPAN, THR, None, None, rs, n, C.byref(tk)) == bad
            assert L.tw_stage_mask_rects(e._h, u8(f0), u8(f1), w, h, rs, n, u8(out), None) == bad
        assert tk.value == -5
        nxt = e.submit(f0, f1, SPAN, THR, ignore=[(10, 10, 20, 20)])
        assert nxt[0] == opened[0] + 1  # the next ticket number is unchanged, the open batch took the pair
        assert vectors(e, opened) == plain(e, f0, f1) and vectors(e, nxt) == want


# ---- the pipeline ----------------------------------------------------------------------------------------------------------
FORMS = ["gray", "rgba_rows", "pal4_rows", "jpeg_coef"]


def target_form(twflow, form, g):
    """(what the submit calls take, the gray image the device makes of it)"""
    if form == "gray":
        return g, g
    t, gray, _ = {"rgba_rows": as_rgba, "pal4_rows": as_pal4, "jpeg_coef": as_jpeg}[form](twflow, g)
    return t, gray


def submit_form(twflow, e, form, expect, t, **kw):
    h, w = expect.shape
    if form == "gray":
        return e.submit(expect, t, SPAN, THR, **kw)
    if form == "jpeg_coef":
        return e.submit_jpeg(expect, t, SPAN, THR, **kw)
    return e.submit_png(twflow.PngRows(expect, w, h), t, SPAN, THR, **kw)


@pytest.mark.parametrize("resident", [False, True], ids=["host_expect", "resident_expect"])
@pytest.mark.parametrize("form", FORMS)
def test_masked_pair_equals_the_host_edited_target(twflow, shape, form, resident):
    w, h, mfree = shape
    f0, f1, _, _ = frames(w, h)
    rects = main_rects(w, h)
    t, gray_t = target_form(twflow, form, f1)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        want, suppressed = reference(e, f0, gray_t, rects)
        assert suppressed > 0 and len(want[1]) > 0  # the filter is exercised: the warp reaches into the rectangle
        unmasked = plain(e, f0, gray_t)
        e.launch_counts(reset=True)
        if resident:
            img = e.image(f0)
            tk = e.submit_image(img, t, SPAN, THR, ignore=rects)
        else:
            tk = submit_form(twflow, e, form, f0, t, ignore=rects)
        got = vectors(e, tk)
        cnt = e.launch_counts()
        assert got == want and got != unmasked
        assert cnt["tw_mask_rects"] == 1 and cnt.last_z["tw_mask_rects"] == 2
        if resident:
            # the expected image was not written: the plain pair against it is the plain pair
            assert vectors(e, e.submit_image(img, t, SPAN, THR)) == unmasked
            img.release()
        if mfree:
            assert cnt.flow_iter() > 0


@pytest.mark.parametrize("form", ["gray", "rgba_rows", "jpeg_coef"])
def test_mask_is_applied_after_the_resize(twflow, oracle, form):
    import synth
    w, h = 100, 80
    a = np.ascontiguousarray(synth.make_pair(0, h, w)[0])
    b = np.ascontiguousarray(synth.make_pair(0, h - 2, w + 3)[1])  # 3 px wider, 2 px shorter
    rects = main_rects(w, h)
    t, gray_t = target_form(twflow, form, b)
    resized = oracle.reconcile_target(gray_t, w, h)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        want, suppressed = reference(e, a, resized, rects)
        assert suppressed > 0 and len(want[1]) > 0
        e.launch_counts(reset=True)
        got = vectors(e, submit_form(twflow, e, form, a, t, ignore=rects, **({"reconcile": True} if form == "gray" else {})))
        cnt = e.launch_counts()
        assert got == want
        assert cnt["tw_resize_u8"] == 1 and cnt["tw_mask_rects"] == 1
        img = e.image(a)
        assert vectors(e, e.submit_image(img, t, SPAN, THR, ignore=rects)) == want


def test_mixed_batch_of_masked_and_ordinary_pairs(twflow, shape):
    w, h, mfree = shape
    f0, f1, f2, f3 = frames(w, h)
    pairs = [(f0, f1), (f1, f2), (f2, f3), (f3, f0), (f0, f2), (f1, f3)]
    r32 = [((11 * i) % (w - 5), (7 * i) % (h - 3), 2 + i % 11, 1 + i % 5) for i in range(30)] + [(w, 0, 5, 5), (3, 3, 0, 9)]
    ign = [[], [(w // 2, h // 3, 20, 12)], [], r32, main_rects(w, h), []]
    nonempty = sum(len(clip(r, w, h)) for r in ign)
    assert nonempty == 1 + 30 + 2
    with twflow.Engine(0, twflow.default_params(), slots=6) as e:
        want = [reference(e, a, b, r)[0] for (a, b), r in zip(pairs, ign)]
        e.launch_counts(reset=True)
        tks = [e.submit(a, b, SPAN, THR) for a, b in pairs]
        unmasked = [vectors(e, t) for t in tks]
        cnt_plain = e.launch_counts(reset=True)
        tks = [e.submit(a, b, SPAN, THR, ignore=r) if r else e.submit(a, b, SPAN, THR) for (a, b), r in zip(pairs, ign)]
        got = [vectors(e, t) for t in tks]
        cnt = e.launch_counts(reset=True)
        assert got == want
        for i in (0, 2, 5):
            assert got[i] == unmasked[i]  # the pairs without rectangles are unaffected
        for i in (1, 3, 4):
            assert got[i] != unmasked[i]
        assert cnt["tw_mask_rects"] == 1 and cnt.last_z["tw_mask_rects"] == nonempty
        assert cnt_plain["tw_mask_rects"] == 0
        for fam in cnt:
            if fam != "tw_mask_rects":
                assert cnt[fam] == cnt_plain[fam], fam
        assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1  # one batch


def test_no_rectangles_is_the_plain_call(twflow, shape):
    w, h, _ = shape
    f0, f1, f2, _ = frames(w, h)
    rgba, _ = target_form(twflow, "rgba_rows", f2)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        img = e.image(f0)
        counts, results = [], []
        for kw in ({}, {"ignore": []}, {"ignore": [(w, 0, 4, 4), (2, 2, 0, 0)]}):  # (all empty after clipping: the same)
            e.launch_counts(reset=True)
            tks = [e.submit(f0, f1, SPAN, THR, **kw), e.submit_png(twflow.PngRows(f0, w, h), rgba, SPAN, THR, **kw),
                   e.submit_image(img, f1, SPAN, THR, **kw)]
            results.append([vectors(e, t) for t in tks])
            counts.append(e.launch_counts(reset=True))
        assert results[1] == results[0] and results[2] == results[0]
        assert counts[1] == counts[0] and counts[2] == counts[0]
        assert counts[1]["tw_mask_rects"] == 0 and counts[1].last_z == counts[0].last_z


def test_pair_identical_after_masking_takes_the_identical_pair_path(twflow, shape):
    w, h, mfree = shape
    f0, f1, _, _ = frames(w, h)
    rect = (w // 3, h // 4, 25, 13)
    t = f0.copy()
    x, y, rw, rh = rect
    t[y:y + rh, x:x + rw] = f1[y:y + rh, x:x + rw]  # differs only inside the rectangle
    t[y + 2, x + 3] ^= 0x55
    assert not np.array_equal(t, f0)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        tks = [e.submit(f0, t, SPAN, THR, ignore=[rect]), e.submit(f0, t, SPAN, THR), e.submit(f0, f1, SPAN, THR),
               e.submit(f0, f0, SPAN, THR)]
        e.flush()
        flags = e.same_flags()
        got = [vectors(e, tk) for tk in tks]
        cnt = e.launch_counts()
        # (at threshold 0 an identical pair itself reports flow of rounding size: the masked pair answers what the identical
        # pair answers, minus the rectangle; at the reference's default threshold of 5 px it answers nothing)
        left = outside(got[3][1], [rect], w, h)
        assert got[0] == ("OK" if not left else "SUSPICIOUS", left)
        assert got[1] != got[3] and outside(got[1][1], [rect], w, h) != left
        assert vectors(e, e.submit(f0, t, SPAN, 5.0, ignore=[rect])) == ("OK", [])
        assert vectors(e, e.submit(f0, f0, SPAN, 5.0)) == ("OK", [])
        if mfree:
            assert cnt["tw_pair_same"] >= 1
            assert flags == [1, 0, 0, 1]  # tw_pair_same reads the masked target


def test_dense_field_of_a_masked_pair_is_not_filtered(twflow, shape):
    w, h, _ = shape
    f0, f1, _, _ = frames(w, h)
    rects = main_rects(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out = e.host_array((2, 2, h, w), np.float32)
        out[...] = np.nan
        (want, suppressed) = reference(e, f0, f1, rects, flow=out[0])
        got = vectors(e, e.submit(f0, f1, SPAN, THR, flow=out[1], ignore=rects))
        assert got == want and suppressed > 0
        assert not np.isnan(out).any()
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
        x0, y0, x1, y1 = clip(rects, w, h)[0]
        assert np.any(out[1][:, y0:y1, x0:x1] != 0)  # the flow inside the rectangle is there, and not zero


def test_kept_target_of_a_masked_pair_is_the_masked_target(twflow, shape):
    w, h, _ = shape
    f0, f1, f2, _ = frames(w, h)
    rects = main_rects(w, h)
    edited = edit(f0, f1, rects)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        want0, _ = reference(e, f0, f1, rects)
        want1 = plain(e, edited, f2)
        assert want1 != plain(e, f1, f2)
        t0 = e.submit(f0, f1, SPAN, THR, ignore=rects)
        kept = e.keep(t0, "target")  # before the batch launches: the copy waits for tw_mask_rects
        t1 = e.submit_image(kept, f2, SPAN, THR)
        assert vectors(e, t0) == want0 and vectors(e, t1) == want1
        t2 = e.submit(f0, f1, SPAN, THR, ignore=rects)
        e.flush()
        kept2 = e.keep(t2, "target")  # after the launch: behind the mask on the copy stream
        assert vectors(e, t2) == want0
        assert vectors(e, e.submit_image(kept2, f2, SPAN, THR)) == want1
        kept.release()
        kept2.release()
        assert e.resident()["bytes_in_use"] == 0


@pytest.mark.parametrize("form", ["gray", "rgba_rows"])
def test_masked_frame_sequence_inside_one_batch(twflow, shape, form):
    """the kept (masked) target of one pair is the expected image of the next masked pair of the same batch: that pair's
    rectangles read the earlier pair's slot, behind that pair's own rectangles"""
    w, h, _ = shape
    f0, f1, f2, f3 = frames(w, h)
    ra, rb = main_rects(w, h), [(w // 4, h // 3, w // 2, h // 3)]
    t1, g1 = target_form(twflow, form, f1)
    t2, g2 = target_form(twflow, form, f2)
    t3, g3 = target_form(twflow, form, f3)
    e1 = edit(f0, g1, ra)
    e2 = edit(e1, g2, rb)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        want = [reference(e, f0, g1, ra)[0], reference(e, e1, g2, rb)[0], reference(e, e2, g3, ra)[0], plain(e, e2, g3)]
        e.launch_counts(reset=True)
        tk0 = submit_form(twflow, e, form, f0, t1, ignore=ra)
        k1 = e.keep(tk0, "target")
        tk1 = e.submit_image(k1, t2, SPAN, THR, ignore=rb)
        k2 = e.keep(tk1, "target")
        tk2 = e.submit_image(k2, t3, SPAN, THR, ignore=ra)
        tk3 = e.submit_image(k2, t3, SPAN, THR)
        got = [vectors(e, t) for t in (tk0, tk1, tk2, tk3)]
        cnt = e.launch_counts()
        assert got == want
        assert cnt["tw_span_scan"] + cnt["tw_span_scan_seg"] == 1  # one batch
        assert cnt["tw_mask_rects"] == 3  # three rounds: each pair's rectangles behind the pair it reads
        k1.release()
        k2.release()
        assert e.resident()["bytes_in_use"] == 0


def test_count_only_wait_and_a_small_cap(twflow, shape):
    w, h, _ = shape
    f0, f1, _, _ = frames(w, h)
    rects = main_rects(w, h)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        want, suppressed = reference(e, f0, f1, rects)
        n_all = len(want[1])
        assert suppressed > 0 and n_all > 7
        n, _ = e.wait_count(e.submit(f0, f1, SPAN, THR, ignore=rects))
        assert n == n_all
        r = e.wait(e.submit(f0, f1, SPAN, THR, ignore=rects), cap=7)
        assert r["count"] == n_all and r["vector"] == want[1][:7] and r["status"] == "SUSPICIOUS"
        r = e.wait(e.submit(f0, f1, SPAN, THR, ignore=rects), cap=0)
        assert r["count"] == n_all and r["vector"] == []


def test_more_hits_than_the_eager_copy_holds(twflow, oracle):
    """a pair with more than 1024 hits: the filter reads the records from the batch's own region"""
    import synth
    w, h = 180, 117
    a, b = (np.ascontiguousarray(x) for x in synth.make_pair(0, h, w))
    rects = [(40, 30, 60, 40)]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        _, vecs = vectors(e, e.submit(a, edit(a, b, rects), 2, THR))
        left = outside(vecs, rects, w, h)
        assert len(vecs) > 1024 and len(left) > 1024 and len(left) < len(vecs)
        tk = e.submit(a, b, 2, THR, ignore=rects)
        assert e.wait(tk)["vector"] == left
        assert e.wait_count(e.submit(a, b, 2, THR, ignore=rects))[0] == len(left)


def test_golden_pair_against_the_oracle(twflow, oracle, golden):
    case = next(c for c in golden.values() if c["expect_img"].shape == (117, 180) and c["vector"])
    a, b = np.ascontiguousarray(case["expect_img"]), np.ascontiguousarray(case["target_img"])
    ys, xs = np.nonzero(a != b)
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
    assert x1 - x0 > 4 and y1 - y0 > 4
    whole = [(x0, y0, x1 - x0, y1 - y0)]
    half = [(x0, y0, (x1 - x0) // 2, y1 - y0)]  # the painted area's left half: the right half still differs
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        assert vectors(e, e.submit(a, b, case["span"], float(case["threshold"]), ignore=whole)) == ("OK", [])
        fx, fy = oracle.farneback(a, a)  # (identical after the mask: at threshold 0 what is left is rounding-size flow)
        left = outside(oracle.span_scan(fx, fy, SPAN, THR), whole, 180, 117)
        assert vectors(e, e.submit(a, b, SPAN, THR, ignore=whole)) == ("OK" if not left else "SUSPICIOUS", left)
        fx, fy = oracle.farneback(a, edit(a, b, half))
        ref = oracle.span_scan(fx, fy, SPAN, THR)
        left = outside(ref, half, 180, 117)
        assert 0 < len(left) < len(ref)  # vectors inside the rectangle exist and are suppressed
        assert vectors(e, e.submit(a, b, SPAN, THR, ignore=half)) == ("SUSPICIOUS", left)
