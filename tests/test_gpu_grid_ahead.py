"""The grid-only last level-0 iteration (tw_flow_iter<15, 3>) with its loads a step ahead of their use.

The step of the grid-only iteration combines chunk st + 7 from R0 registers that were loaded during the step before (two
register sets that swap roles with the loop's unroll by two; the prologue loads the first chunk's), as its taps always were.
What can go wrong with that, and nowhere else: a register set in the wrong role at a segment's start (the prologue's extra
load feeds step 0's combine) or end (the loop's remainder step after an even or an odd number of steps), in segments of one
step and of two (no pass through the unrolled loop, exactly one), in segments shorter than the 7-chunk ring (every chunk a
step loads ahead lies outside the segment and is clamped into the image), and a last step of fewer than five rows.

Every comparison is on float bits.
Part 1: tw_stage_flow_iter_grid against the oracle's one iteration sampled at [::span, ::span] — the inputs, references and
        helpers of tests/test_gpu_grid_final.py, heights and TW_FI_MAXSEG / TW_FI_MINSTEPS chosen for the segment shapes above.
Part 2: one batch on a gate-lifted engine: hit vectors == oracle == the same batch under TW_GRID_FINAL=0.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_grid_final as GF  # noqa: E402
from test_gpu_stages_f64 import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
TH = GF.TH
NCH = 7  # chunks of the LDS ring's window (2 * 15 + 5 rows)

# 320: two full strips; 321: a third strip whose only grid column is the image's last column (spans 5, 10)
WIDTHS = [320, 321]
SPANS = [5, 7, 10]
# steps of 5 rows (the iteration takes levels of 20 rows and more): 20 -> 4; 23 -> 5 (the last of 3 rows); 41 -> 9 (the last of
# 1 row: the image's last row, a grid row of spans 5 and 10); 47 -> 10 (the last of 2 rows)
HEIGHTS = [20, 23, 41, 47]
# (TW_FI_MAXSEG, TW_FI_MINSTEPS); a segment has at least two steps, so only a strip's last segment can have one.
# Default: one segment at these heights — 4 and 5 steps (even and odd, shorter than the ring), 9 and 10 (longer).
# (64, 2): 20 rows -> segments of 2, 2 steps; 23 -> 2, 2, 1; 41 -> 2, 2, 2, 2, 1; 47 -> five of 2.
# (64, 3): 20 -> 4; 23 -> 3, 2; 41 -> 3, 3, 3; 47 -> 3, 3, 3, 1 (the one step of the last segment has 2 rows)
KNOBS = [(None, None), (64, 2), (64, 3)]
KNOB_IDS = ["default", "maxseg64_minsteps2", "maxseg64_minsteps3"]


def set_knobs(monkeypatch, knobs):
    for name, v in zip(("TW_FI_MAXSEG", "TW_FI_MINSTEPS"), knobs):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def segment_steps(plan):
    """Steps of every segment of a strip, first to last."""
    return [plan.nt] * (plan.segments - 1) + [plan.nt_last]


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_stage_grid_against_the_sampled_iteration(twflow, oracle, monkeypatch, knobs, h):
    set_knobs(monkeypatch, knobs)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        for w in WIDTHS:
            plan = e.flow_iter_plan(w, h, 1)
            refs = GF.stage_refs(oracle, h, w)
            for span in SPANS:
                ng, no, rstar, empty = GF.grid_steps(plan, h, span)
                print("gridahead h=%d w=%d span=%d knobs=%s strips=%d segment_steps=%s grid_steps=%d other_steps=%d rstar=%s" % (
                    h, w, span, knobs, plan.strips, segment_steps(plan), ng, no, sorted(rstar)))
                assert ng == -(-h // span)  # (every grid row lies in exactly one step)
                for name, R0, R1, flow, want in refs:
                    e.launch_counts(reset=True)
                    got = e.stage_flow_iter_grid(R0, R1, flow, span)
                    cnt = e.launch_counts(reset=True)
                    assert cnt["tw_flow_iter_grid"] == 1 and cnt["tw_flow_iter"] == 1 and cnt.flow_iter() == 1, cnt
                    same_bits(got, want[::span, ::span], "tw_stage_flow_iter_grid %dx%d span %d %s, %s" % (w, h, span, knobs, name))


def test_the_cases_reach_what_they_are_there_for(twflow, monkeypatch):
    """The segment shapes the heights and knobs above are there for, from the launch's own plan."""
    segs = {}
    for knobs in KNOBS:
        set_knobs(monkeypatch, knobs)
        with twflow.Engine(0, twflow.default_params(), slots=1) as e:
            for h in HEIGHTS:
                for w in WIDTHS:
                    plan = e.flow_iter_plan(w, h, 1)
                    assert sum(segment_steps(plan)) == -(-h // TH) and min(segment_steps(plan)) >= 1, plan
                    segs[(knobs, h, w)] = segment_steps(plan)
    every = [n for s in segs.values() for n in s]
    assert 1 in every, "no segment of one step"
    assert 2 in every, "no segment of two steps"
    assert any(n > 2 and n % 2 for n in every), "no odd step count above two"
    assert any(n > 2 and n % 2 == 0 for n in every), "no even step count above two"
    assert any(len(s) > 1 and s[-1] == 1 for s in segs.values()), "no last segment of one step"
    assert segs[((64, 2), 23, 320)] == [2, 2, 1] and segs[((64, 3), 47, 320)] == [3, 3, 3, 1]
    assert any(h % TH for (_, h, _) in segs), "no last step of fewer than five rows"
    assert any(len(s) > 1 and s[-1] == 1 and h % TH for (_, h, _), s in segs.items()), "no one-step last segment of fewer than five rows"
    assert any(2 < n < NCH for n in every), "no segment of more than two steps that is shorter than the ring"
    assert any(n > NCH for n in every), "no segment longer than the ring"


@pytest.fixture
def gate_lifted(monkeypatch):
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.setenv("TW_RAMP", "0")
    for name in ("TW_LANES", "TW_GRID_FINAL", "TW_FI_MAXSEG", "TW_FI_MINSTEPS"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_batch_vectors(twflow, oracle, gate_lifted):
    """Four pairs of 397 x 99 (three strips, 20 steps with a last one of 4 rows): vectors == oracle == TW_GRID_FINAL=0."""
    pairs = GF.batch_pairs(GF.BH, GF.BW, 4)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        got, cnt = GF.submit_all(e, pairs, 10)
        gate_lifted.setenv("TW_GRID_FINAL", "0")
        full, cnt_full = GF.submit_all(e, pairs, 10)
        assert cnt["tw_flow_iter_grid"] == 1 and cnt["tw_span_gather"] == 0, cnt
        assert cnt_full["tw_flow_iter_grid"] == 0 and cnt_full["tw_span_gather"] == 1, cnt_full
        for i in range(4):
            f = GF.oracle_field(oracle, GF.BH, GF.BW, i, 3)
            want = oracle.span_scan(f[0], f[1], 10, 0.0)
            assert len(want) > 0 or i == 3
            assert got[i] == want, "pair %d: grid-only vectors differ from the oracle's" % i
            assert full[i] == want, "pair %d: TW_GRID_FINAL=0 vectors differ from the oracle's" % i
