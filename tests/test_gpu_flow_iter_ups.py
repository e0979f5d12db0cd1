"""tw_flow_iter's upsampling first iteration (MODE 1) at the edges of its resize tables, bit for bit against the oracle.

The kernel computes resize(prevFlow, INTER_LINEAR) * (1 / pyrScale) in place of the flow load: two horizontal taps per
pixel, coarse columns sx and min(sx + 1, pw - 1), a single-tap tail for the columns >= xmax, and a row entry (yofs, beta)
fetched one chunk ahead of the taps.  What can go wrong is the clamped tap at the right edge, odd coarse widths, fractional
weights, rows clamped at the top (yofs = -1) and bottom (yofs + 1 = ph), and the row entry across a row-segment start.
Every case compares `Engine.stage_flow_iter(R0, R1, prev=...)` bit for bit with oracle.flow_upsample ->
oracle.update_matrices -> oracle.update_flow(..., 30, 0) and asserts from the launch counters that the tw_flow_iter_ups
family ran.

The stage entry point refuses levels lower than 20 rows (tests/test_gpu_parity.py pins that), so the two shapes of the
case list that are lower — 333 x 7 from 167 x 4 and 481 x 11 from 289 x 7 — are asserted to be REFUSED as they stand, and
run at the smallest admissible odd height instead, 21 rows, with the same widths, coarse widths and scale: 21 rows are
still fewer than one chunk ring (35 rows) and no multiple of the chunk (5 rows).  At scales 0.6 and 0.75 the weights are
fractional but the single-tap tail is ONE column, as at 0.5; a case at scale 0.3 adds a tail of two columns.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_oracle_stages_f64 as S  # noqa: E402
from conftest import planar  # noqa: E402
from test_gpu_stages_f64 import _oracle_iter, ran, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
OUT = 160  # output columns per strip

# id: (fine w, h, coarse pw, ph, pyrScale, strips, (TW_FI_MAXSEG, TW_FI_MINSTEPS) or None, segments)
CASES = {
    "right_edge": (320, 20, 160, 10, 0.5, 2, None, 1),
    "odd_coarse_width": (321, 23, 161, 12, 0.5, 3, None, 1),
    "ragged_third_strip": (333, 21, 167, 11, 0.5, 3, None, 1),
    "scale_075": (320, 20, 240, 15, 0.75, 2, None, 1),
    "scale_06": (481, 21, 289, 13, 0.6, 4, None, 1),
    "ragged_two_segments": (700, 64, 350, 32, 0.5, 5, (2, 5), 2),
    # beyond the case list: an upsample by more than 3 is what it takes for SEVERAL single-tap tail columns (the tail
    # starts at w - 0.5 / scale - 0.5: one column at 0.5, 0.6 and 0.75, two at 0.3)
    "two_tail_columns": (320, 20, 96, 6, 0.3, 2, None, 1),
}
TOO_LOW = {"ragged_third_strip": (333, 7, 167, 4, 0.5), "scale_06": (481, 11, 289, 7, 0.6)}


def resize_tab(src, dst):
    """(ofs, clamped ofs, dmax) of cv::resize(INTER_LINEAR) along one axis, as imgwarp.cpp computes them: the float32
    coordinate from a double product; `ofs` before any clamp (rows are clamped at use), the column form clamped."""
    scale = 1.0 / (float(dst) / src)
    f = ((np.arange(dst) + 0.5) * scale - 0.5).astype(F32)
    ofs = np.floor(f).astype(np.int64)
    dmax = int(np.argmax(ofs + 1 >= src)) if (ofs + 1 >= src).any() else dst
    return ofs, np.clip(ofs, 0, src - 1), dmax


def make_case(w, h, pw, ph):
    rng = np.random.default_rng(w * 1000 + h)
    R0, R1 = S.fields(rng, h, w)
    R0[h // 2:, w // 2:] = 0  # flat quadrant: the regulariser decides there
    R1[h // 2:, w // 2:] = 0
    prev = (rng.standard_normal((ph, pw, 2)) * 2).astype(F32)
    prev[0, 0, 0] = -0.0
    prev[ph - 1, pw - 1, 1] = -0.0
    # displacements far larger than the image, either sign: in the interior, in the last coarse column (the clamped
    # tap) and in the first and last coarse rows (the clamped rows)
    big = F32(2 * (w + h))
    prev[ph // 3, pw // 4: pw // 4 + 5, 0] = big
    prev[ph // 2, pw // 2: pw // 2 + 3, 1] = -big
    prev[1::4, pw - 1, 0] = -big
    prev[2::4, pw - 2, 1] = big
    prev[0, 3::17, 1] = big
    prev[ph - 1, 5::19, 0] = -big
    return R0, R1, prev


@pytest.mark.parametrize("name", list(CASES))
def test_upsampling_iteration_bit_exact(twflow, oracle, monkeypatch, name):
    w, h, pw, ph, scale, strips, knobs, segments = CASES[name]
    for var, v in zip(("TW_FI_MAXSEG", "TW_FI_MINSTEPS"), knobs or (None, None)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))
    # the geometry the case is there for, from the resize rule itself
    yofs, _, _ = resize_tab(ph, h)
    _, xofs, xmax = resize_tab(pw, w)
    assert yofs[0] == -1 and yofs[h - 1] + 1 == ph, (yofs[0], yofs[h - 1], ph)
    assert xmax < w and xofs[w - 1] == pw - 1, (xmax, xofs[w - 1])  # tail columns: both taps are the last coarse column
    if name == "right_edge":
        assert xmax == w - 1
    if name == "two_tail_columns":
        assert w - xmax == 2, xmax
    if name == "odd_coarse_width":
        assert pw % 2 == 1 and w % 2 == 1 and h % 5 != 0
    R0, R1, prev = make_case(w, h, pw, ph)
    up = oracle.flow_upsample(prev, w, h, scale)
    assert (np.abs(up) > w + h).any() and (np.abs(up[:, xmax:]) > w + h).any()  # samples pushed out of the image
    want = planar(_oracle_iter(oracle, R0, R1, up))
    with twflow.Engine(0, twflow.default_params(pyrScale=scale), slots=1) as e:
        plan = e.flow_iter_plan(w, h, 1)
        assert plan.strips == strips == (w + OUT - 1) // OUT and plan.segments == segments, plan
        e.launch_counts(reset=True)
        got = e.stage_flow_iter(planar(R0), planar(R1), prev=planar(prev))
        cnt = ran(e, "tw_flow_iter_ups", 1)
        assert cnt.flow_iter() == 1 and cnt.last_z["tw_flow_iter_ups"] == 1, cnt
        same_bits(got, want, "tw_stage_flow_iter upsampled %s %dx%d from %dx%d" % (name, w, h, pw, ph))


@pytest.mark.parametrize("name", list(TOO_LOW))
def test_levels_lower_than_20_rows_are_refused(twflow, name):
    """The two shapes of the case list below the entry point's 20-row floor: no launch, TW_E_UNSUPPORTED."""
    w, h, pw, ph, scale = TOO_LOW[name]
    R0, R1, prev = make_case(w, h, pw, ph)
    with twflow.Engine(0, twflow.default_params(pyrScale=scale), slots=1) as e:
        e.launch_counts(reset=True)
        with pytest.raises(twflow.TwError) as ei:
            e.stage_flow_iter(planar(R0), planar(R1), prev=planar(prev))
        assert ei.value.code == twflow.TW_E_UNSUPPORTED
        assert e.launch_counts().flow_iter() == 0


def test_batch_of_three_pairs_two_levels(twflow, oracle, monkeypatch):
    """Three pairs through the batch path with both levels of a two-level plan on tw_flow_iter: level 1 from zero flow,
    level 0 upsampling it.  640 x 48 has ONE level (a level exists only while both sides stay >= 32 pixels), so the size
    is the smallest for which the schedule's predicate says yes twice: 639 x 64 (level 1: 320 x 32; 319.5 columns round
    half to even).  TW_MFREE=2 lifts the workgroup-count gate a batch of three does not pass."""
    import synth
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.setenv("TW_RAMP", "0")
    h, w, n = 64, 639, 3
    pairs = [synth.make_pair(i, h, w) for i in range(n)]
    want = [np.stack(oracle.farneback(a, b, oracle.default_params())) for a, b in pairs]
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.num_levels(w, h) == 1
        assert [e.level_runs_flow_iter(w, h, k, n) for k in range(2)] == [True, True]
        # smallest: the predicate is monotone in both sides (a level needs >= 32 rows and, for tw_flow_iter, >= 320
        # columns), so one column or one row less is all there is to try
        smaller = [(64, 638), (63, 639)]
        assert not any(e.num_levels(ww, hh) == 1 and all(e.level_runs_flow_iter(ww, hh, k, n) for k in range(2))
                       for hh, ww in smaller), "a smaller size runs both levels through tw_flow_iter"
        e.launch_counts(reset=True)
        out, _ = e.flow_batch([p[0] for p in pairs], [p[1] for p in pairs], layout="planar")
        cnt = e.launch_counts(reset=True)
        assert cnt["tw_flow_iter_ups"] == 1 and cnt["tw_flow_iter_zero"] == 1 and cnt["tw_update_matrices"] == 0, cnt
        assert cnt.last_z["tw_flow_iter_ups"] == 3, cnt.last_z
        for i in range(n):
            same_bits(out[i], want[i], "639x64 batch, pair %d" % i)
