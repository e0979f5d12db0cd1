"""What the calls on a ticket answer alike: tw_wait, tw_wait_regions, tw_ticket_changes, tw_ticket_shift, tw_ticket_shift_bands,
tw_ticket_hits, tw_ticket_overlay and tw_image_keep.  A pair's own error (a palette index beyond PLTE) is answered by every one
of them, by the non-consuming ones any number of times; a collected ticket is unknown to all of them; a batch opened without
an option refuses that option's call and stays waitable.  The values themselves are the other test files' business."""
import numpy as np
import pytest

from test_gpu_png_kinds import filter_bytes

pytestmark = pytest.mark.gpu

W, H, SPAN, THR, TOL = 48, 64, 10, 2.0, 8
BAD_TARGET = "bad palette index in the target image"
UNKNOWN = "unknown ticket"
# the library's own texts, word for word
OFF = {
    "wait_regions": "tw_wait_regions: the ticket's batch was opened with TW_OPT_REGIONS off",
    "changes": "tw_ticket_changes: the ticket's batch was opened with TW_OPT_RESIDUAL off",
    "shift": "tw_ticket_shift: the ticket's batch was opened with TW_OPT_SHIFT off",
    "shift_bands": "tw_ticket_shift_bands: the ticket's batch was opened without TW_OPT_SHIFT_BANDS and TW_OPT_SHIFT on",
}


def refused(twflow, e, call, code, text):
    with pytest.raises(twflow.TwError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert e._L.tw_last_error(e._h).decode() == text
    assert str(ei.value) == "twflow status %d: %s" % (code, text)


def calls(e, tk):
    """every call on a ticket, by name; the first five do not consume it"""
    return {
        "changes": lambda: e.changes(tk),
        "shift": lambda: e.shift(tk),
        "shift_bands": lambda: e.shift_bands(tk),
        "hits": lambda: e.hits(tk),
        "overlay": lambda: e.overlay(tk, TOL, np.zeros(3 * W * H, np.uint8)).copy(),
        "wait_regions": lambda: e.wait_regions(tk),
        "wait": lambda: e.wait(tk),
        "keep": lambda: e.keep(tk),
    }


NON_CONSUMING = ("changes", "shift", "shift_bands", "hits", "overlay")


def test_the_calls_on_a_ticket_answer_alike(twflow):
    rng = np.random.default_rng(5)
    plte = np.repeat((np.arange(8) * 32).astype(np.uint8)[:, None], 3, 1)
    yy, xx = np.mgrid[0:H, 0:W]
    ia = (((xx // 6 + yy // 5) + rng.integers(0, 2, (H, W))) % 8).astype(np.uint8)
    ib = np.roll(ia, (2, 1), (0, 1))
    bad = ib.copy()
    bad[H // 2, W // 2] = 8  # (PLTE has entries 0 .. 7)
    types = np.arange(H) % 5
    P = lambda idx: twflow.PngRows(filter_bytes(idx, 1, types), W, H, 3, 8, plte)  # noqa: E731
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        e.set_regions(2)
        e.set_residual(TOL)
        e.set_shift(8)
        e.set_shift_bands(32)
        t_bad, t_ok = e.submit_png(P(ia), P(bad), SPAN, THR), e.submit_png(P(ia), P(ib), SPAN, THR)
        fmt, par = twflow.TW_E_BAD_IMAGE_FORMAT, twflow.TW_E_BAD_PARAMETER

        # the pair's own error: every non-consuming call, twice over, then the wait that collects the ticket
        on_bad = calls(e, t_bad)
        for name in NON_CONSUMING + NON_CONSUMING:
            refused(twflow, e, on_bad[name], fmt, BAD_TARGET)
        refused(twflow, e, on_bad["wait_regions"], fmt, BAD_TARGET)
        # collected: unknown to every call
        for name, call in on_bad.items():
            refused(twflow, e, call, par, UNKNOWN)

        # the sound pair of the same batch: the same answer twice, and still waitable
        on_ok = calls(e, t_ok)
        for name in NON_CONSUMING:
            first, second = on_ok[name](), on_ok[name]()
            assert np.array_equal(first, second) if name == "overlay" else first == second, name
        assert len(on_ok["shift_bands"]()) == H // 32
        on_ok["wait_regions"]()
        refused(twflow, e, on_ok["hits"], par, UNKNOWN)

        # a batch opened with the options off refuses their calls, and a plain wait still collects the ticket
        e.set_regions(0)
        e.set_residual(0)
        e.set_shift(0)
        e.set_shift_bands(0)
        t_off = e.submit_png(P(ia), P(ib), SPAN, THR)
        on_off = calls(e, t_off)
        for name, text in OFF.items():
            refused(twflow, e, on_off[name], par, text)
        assert on_off["wait"]()["width"] == W
        refused(twflow, e, on_off["wait"], par, UNKNOWN)
