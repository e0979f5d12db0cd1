"""The submit path (twflow.hip: Submit) where the rest of the suite does not reach and a reordering of its steps would
break silently: a refused submission next to an OPEN batch, and tw_submit_png8_flow_init, which no other test calls.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_init_abi import farneback_with_init  # noqa: E402
from test_gpu_png import GOLDEN, png_filter, read_png_rows  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPAN, THR = 120, 90, 5, 0.5


def _good_pairs():
    rng = np.random.default_rng(8)
    out = []
    for shift in (1, 2):
        a = rng.integers(0, 256, (H, W), dtype=np.uint8)
        out.append((a, np.roll(a, shift, axis=0)))
    return out


def _refusals(twflow, e, a, b):
    """(what, call, status) of one refused submission of each kind; every argument but the bad one is a good one."""
    pa, pb = twflow._u8(a), twflow._u8(b)
    rows = png_filter(a[:, :, None], np.zeros(H, int))
    rows[5, 0] = 5
    pageable = np.empty((2, H, W), np.float32)
    field = np.zeros((H, W + 1, 2), np.float32)
    return [
        ("span -1", lambda: e.submit(a, b, -1, THR), twflow.TW_E_BAD_PARAMETER),
        ("stride below the width", lambda: e.submit_ptr(pa, pb, W, H, W - 1, SPAN, THR), twflow.TW_E_BAD_PARAMETER),
        ("PNG filter byte 5", lambda: e.submit_png8(rows, 1, b, 0, W, H, SPAN, THR), twflow.TW_E_BAD_IMAGE_FORMAT),
        ("pageable flow destination", lambda: e.submit(a, b, SPAN, THR, flow=pageable), twflow.TW_E_BAD_PARAMETER),
        ("initial field's pitch no multiple of 4",
         lambda: e.submit(a, b, SPAN, THR, init=(field.ctypes.data, W * 8 + 2, twflow.FLOW_INTERLEAVED)),
         twflow.TW_E_BAD_PARAMETER),
        ("0-wide image", lambda: e.submit_ptr(pa, pb, 0, H, W, SPAN, THR), twflow.TW_E_BAD_PARAMETER),
    ]


def test_refused_submissions_leave_the_open_batch_as_it_was(twflow, oracle):
    """One good pair opens a batch of a 4-slot engine; one refusal of each kind follows; a second good pair then joins the
    SAME batch: consecutive tickets, both answers the oracle's, and the launches — counts and the last grid z per family —
    those of a control engine that saw the two good pairs only (one batch of two, nothing flushed early)."""
    pairs = _good_pairs()
    want = [oracle.span_scan(*oracle.farneback(a, b), SPAN, THR) for a, b in pairs]
    with twflow.Engine(0, twflow.default_params(), slots=4) as ctl:
        tk = [ctl.submit(a, b, SPAN, THR) for a, b in pairs]
        assert [ctl.wait(t)["vector"] for t in tk] == want
        ctl_counts = ctl.launch_counts()
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        t1 = e.submit(*pairs[0], SPAN, THR)
        for what, call, status in _refusals(twflow, e, *pairs[1]):
            with pytest.raises(twflow.TwError) as ei:
                call()
            assert ei.value.code == status, what
        t2 = e.submit(*pairs[1], SPAN, THR)
        assert t2[0] == t1[0] + 1  # a refusal consumes no ticket
        assert [e.wait(t1)["vector"], e.wait(t2)["vector"]] == want
        counts = e.launch_counts()
        assert dict(counts) == dict(ctl_counts) and counts.last_z == ctl_counts.last_z


def test_png8_flow_init_on_golden_fixture(twflow, oracle, golden):
    """tw_submit_png8_flow_init on the 180x117 fixture, a plain gray image beside filtered RGBA rows, a non-zero initial
    field, a page-locked destination: field and vectors are those of submit(init=, flow=) on the decoded gray images,
    and the oracle's with that initial field."""
    case = golden["revision2_capture2"]
    span, thr = case["span"], float(case["threshold"])
    a, b = case["expect_img"], case["target_img"]
    rb, w, h, chb = read_png_rows(os.path.join(GOLDEN, "tree", "revision2", "scenario2", "capture2.png"))
    assert (h, w) == a.shape == b.shape
    f = (np.random.default_rng(1003).standard_normal((h, w, 2)) * 3.0).astype(np.float32)
    fx, fy = farneback_with_init(oracle, a, b, f)
    want_vec = oracle.span_scan(fx, fy, span, thr)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        out = e.host_array((2, 2, h, w), np.float32)
        out[...] = np.nan
        got_png = e.wait(e.submit_png8(a, 0, rb, chb, w, h, span, thr, flow=out[0], init=f))
        got_u8 = e.wait(e.submit(a, b, span, thr, flow=out[1], init=f))
        assert e.launch_counts()["tw_png_unfilter"] == 1
        assert got_png["vector"] == got_u8["vector"] == want_vec
        # (out is the engine's page-locked memory: compared before the engine closes)
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], np.stack([fx, fy]))
