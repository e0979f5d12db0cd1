"""The grid-only last level-0 iteration: tw_flow_iter's MODE 3, its place in the batch schedule, its switch.

A batch that returns hit records alone reads the last level-0 field only at the span-grid points (gx * span, gy * span), so
its last iteration runs phase C (FarnebackUpdateMatrices into the LDS ring) at every pixel and the window sums and the solve
only where a grid point is, writes the samples and stores no field (tw_flow_iter<15, 3>; TW_GRID_FINAL=0 restores the full
iteration + tw_span_gather).  What can go wrong: the grid-step predicate at segment starts that are no multiple of the span
and in segments without any grid row, r* (the grid row's offset in its 5-row step), the last grid row / column being the
image's last, strips whose only grid column is their last, the ring row a step's V reads, and — a hang, not a wrong bit —
wave 15 counting other barriers than the other waves.

Every comparison is on float bits.
Part 1: the stage entry point against the oracle's one iteration (the helper tests/test_gpu_flow_iter_geometry.py uses for
        tw_stage_flow_iter) sampled at [::span, ::span].
Part 2: batches on a gate-lifted engine (TW_MFREE=2): hit vectors == oracle == the same batch under TW_GRID_FINAL=0, the launch
        counters of every way into and out of the new path.
Part 3: one batch that passes the default gate.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_oracle_stages_f64 as S  # noqa: E402
from conftest import planar  # noqa: E402
from test_gpu_stages_f64 import _oracle_iter, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TH = 5  # rows per step (FI_TH)

# 320: two full strips; 321: a third strip whose only grid column is the image's last column (spans 5, 10, 16); 330; 481
WIDTHS = [320, 321, 330, 481]
# 20: fewer steps than the ring primes; 41: the last grid row is the last image row (spans 5, 10); 47: a last step of 2
# rows; 104
HEIGHTS = [20, 41, 47, 104]
# 5: a grid row in every step; 7: r* takes all of 0 .. 4; 10; 16; 33
SPANS = [5, 7, 10, 16, 33]
# default knobs; (TW_FI_MAXSEG, TW_FI_MINSTEPS) = (64, 3): segments that start on rows that are no multiple of the span, and
# (span 16, 33) segments with no grid row at all
DEFAULT, SHORT = (None, None), (64, 3)

_REF = {}


def stage_inputs(h, w):
    """Three input sets of one size: (name, R0, R1, flow)."""
    rng = np.random.default_rng(h * 11 + w)
    R0, R1 = S.fields(rng, h, w)
    R0[h // 2:, w // 2:] = 0  # flat quadrant: the regulariser decides there
    R1[h // 2:, w // 2:] = 0
    cases = S.flow_cases(rng, h, w)
    small = cases[0][1].copy()  # sigma 2
    small[0, 0, 0] = -0.0       # (a grid point of every span)
    small[h - 1, w - 1, 1] = -0.0
    return [("flat quadrant, -0.0", R0, R1, small),
            ("flow leaves the image", R0, R1, cases[1][1]),  # sigma 40
            ("R1 = R0", R0, R0, cases[0][1])]


def stage_refs(oracle, h, w):
    """[(name, planar R0, planar R1, planar flow, the oracle's iteration (h, w, 2))], computed once per size."""
    if (h, w) not in _REF:
        _REF[(h, w)] = [(name, planar(R0), planar(R1), planar(flow), _oracle_iter(oracle, R0, R1, flow))
                        for name, R0, R1, flow in stage_inputs(h, w)]
    return _REF[(h, w)]


def grid_steps(plan, h, span):
    """(grid steps, other steps, set of r*, segments without a grid row) of a launch — for the log only."""
    n_grid, n_other, rstar, empty = 0, 0, set(), 0
    for seg in range(plan.segments):
        ys = seg * plan.nt * TH
        steps = min(plan.nt, (h - ys + TH - 1) // TH)
        had = 0
        for st in range(steps):
            y0 = ys + TH * st
            gy = -(-y0 // span)
            if gy * span < min(y0 + TH, h):
                had += 1
                rstar.add(gy * span - y0)
        n_grid += had
        n_other += steps - had
        empty += had == 0
    return n_grid, n_other, rstar, empty


@pytest.mark.parametrize("knobs", [DEFAULT, SHORT], ids=["default", "maxseg64_minsteps3"])
@pytest.mark.parametrize("h", HEIGHTS)
def test_stage_grid_against_the_sampled_iteration(twflow, oracle, monkeypatch, knobs, h):
    for name, v in zip(("TW_FI_MAXSEG", "TW_FI_MINSTEPS"), knobs):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        for w in WIDTHS:
            plan = e.flow_iter_plan(w, h, 1)
            refs = stage_refs(oracle, h, w)
            for span in SPANS:
                ng, no, rstar, empty = grid_steps(plan, h, span)
                print("gridfinal h=%d w=%d span=%d knobs=%s strips=%d segments=%d nt=%d grid_steps=%d other_steps=%d rstar=%s "
                      "segments_without_grid_row=%d" % (h, w, span, knobs, plan.strips, plan.segments, plan.nt, ng, no,
                                                        sorted(rstar), empty))
                assert ng == -(-h // span)  # (every grid row lies in exactly one step)
                for name, R0, R1, flow, want in refs:
                    e.launch_counts(reset=True)
                    got = e.stage_flow_iter_grid(R0, R1, flow, span)
                    cnt = e.launch_counts(reset=True)
                    assert cnt["tw_flow_iter_grid"] == 1 and cnt["tw_flow_iter"] == 1 and cnt.flow_iter() == 1, cnt
                    same_bits(got, want[::span, ::span], "tw_stage_flow_iter_grid %dx%d span %d %s, %s" % (w, h, span, knobs, name))


def test_the_cases_reach_what_they_are_there_for(twflow, monkeypatch):
    """The geometry the lists above are there for, computed from the launch's own plan."""
    monkeypatch.setenv("TW_FI_MAXSEG", "64")
    monkeypatch.setenv("TW_FI_MINSTEPS", "3")
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        short = {(h, span): grid_steps(e.flow_iter_plan(320, h, 1), h, span) for h in HEIGHTS for span in SPANS}
        plans = {h: e.flow_iter_plan(320, h, 1) for h in HEIGHTS}
    assert short[(104, 7)][2] == {0, 1, 2, 3, 4}
    assert all(short[(h, 5)][1] == 0 for h in HEIGHTS)  # span 5: a grid row in every step
    assert any(short[(h, span)][3] > 0 for h in HEIGHTS for span in (16, 33)), "no segment without a grid row"
    assert any(p.segments > 1 and (p.nt * TH) % 10 for p in plans.values()), "no segment starts off the span-10 grid"
    assert (41 - 1) % 5 == 0 and (41 - 1) % 10 == 0 and (321 - 1) % 16 == 0 and 321 - 1 == 2 * 160


# ---- part 2: batches on a gate-lifted engine ------------------------------------------------------------------------------
BH, BW = 99, 397  # three strips (160 + 160 + 77 columns), 20 steps with a last one of 4 rows; level 1 (198 x 49) on the tile kernels


@pytest.fixture
def gate_lifted(monkeypatch):
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.setenv("TW_RAMP", "0")
    monkeypatch.delenv("TW_LANES", raising=False)
    monkeypatch.delenv("TW_GRID_FINAL", raising=False)
    return monkeypatch


_PAIRS = {}
_FIELDS = {}


def batch_pairs(h, w, n):
    """n synth pairs; pair 3 of every four is identical (tw_pair_same flags it)."""
    import synth
    if (h, w) not in _PAIRS:
        _PAIRS[(h, w)] = [synth.make_pair(i, h, w, kind=(0, 1, 2, 3)[i]) for i in range(4)]
        assert np.array_equal(*_PAIRS[(h, w)][3])
    return [_PAIRS[(h, w)][i % 4] for i in range(n)]


def oracle_field(oracle, h, w, i, it):
    key = (h, w, i % 4, it)
    if key not in _FIELDS:
        a, b = batch_pairs(h, w, 4)[i % 4]
        _FIELDS[key] = np.stack(oracle.farneback(a, b, oracle.default_params(pyrIterations=it)))
    return _FIELDS[key]


def submit_all(e, pairs, span, thr=0.0):
    e.launch_counts(reset=True)
    tk = [e.submit(a, b, span, thr) for a, b in pairs]
    got = [e.wait(t)["vector"] for t in tk]
    return got, e.launch_counts(reset=True)


@pytest.mark.parametrize("it", [1, 2, 3, 4])
def test_batch_vectors_and_counters(twflow, oracle, gate_lifted, it):
    """Spans 5, 10, 16 (and 4, which keeps the full path): vectors == oracle == the same batch under TW_GRID_FINAL=0."""
    pairs = batch_pairs(BH, BW, 4)
    with twflow.Engine(0, twflow.default_params(pyrIterations=it), slots=4) as e:
        levels = e.num_levels(BW, BH)
        runs = [e.level_runs_flow_iter(BW, BH, k, 4) for k in range(levels + 1)]
        assert runs[0], runs
        fi_levels = sum(runs)
        for span in (4, 5, 10, 16):
            gate_lifted.delenv("TW_GRID_FINAL", raising=False)
            got, cnt = submit_all(e, pairs, span)
            assert e.same_flags() == [0, 0, 0, 1]
            gate_lifted.setenv("TW_GRID_FINAL", "0")
            full, cnt_full = submit_all(e, pairs, span)
            print("gridfinal batch it=%d span=%d grid=%d gather=%d flow_iter=%d" % (
                it, span, cnt["tw_flow_iter_grid"], cnt["tw_span_gather"], cnt["tw_flow_iter"]))
            for i in range(4):
                f = oracle_field(oracle, BH, BW, i, it)
                want = oracle.span_scan(f[0], f[1], span, 0.0)
                assert len(want) > 0 or i == 3
                assert got[i] == want, "it %d span %d pair %d: grid-only vectors differ from the oracle's" % (it, span, i)
                assert full[i] == want, "it %d span %d pair %d: TW_GRID_FINAL=0 vectors differ from the oracle's" % (it, span, i)
            new_path = it >= 2 and span >= TH
            assert cnt["tw_flow_iter_grid"] == (1 if new_path else 0), cnt       # (one level-0 chunk)
            assert cnt["tw_span_gather"] == (0 if new_path else 1), cnt
            assert cnt_full["tw_flow_iter_grid"] == 0 and cnt_full["tw_span_gather"] == 1, cnt_full
            # the tw_flow_iter family counts what it counted: the grid launch IS the level's last MODE 0 iteration
            for c in (cnt, cnt_full):
                assert c["tw_flow_iter"] == (it - 1) * fi_levels and c.flow_iter() == it * fi_levels, c
                assert c["tw_blur_grid"] == 0, c
            assert {k: v for k, v in cnt.items() if k not in ("tw_flow_iter_grid", "tw_span_gather")} == \
                   {k: v for k, v in cnt_full.items() if k not in ("tw_flow_iter_grid", "tw_span_gather")}


def test_a_flow_destination_keeps_the_full_path(twflow, oracle, gate_lifted):
    """One pair of the batch wants its field: the whole batch takes the full last iteration, and the field is the oracle's."""
    pairs = batch_pairs(BH, BW, 4)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        out = e.host_array((2, BH, BW), np.float32)
        e.launch_counts(reset=True)
        tk = [e.submit(a, b, 10, 0.0, flow=(out if i == 1 else None)) for i, (a, b) in enumerate(pairs)]
        got = [e.wait(t)["vector"] for t in tk]
        cnt = e.launch_counts(reset=True)
        assert cnt["tw_flow_iter_grid"] == 0 and cnt["tw_span_gather"] == 1 and cnt["tw_flow_export"] >= 1, cnt
        same_bits(np.array(out), oracle_field(oracle, BH, BW, 1, 3), "field of the pair with a destination")
        for i in range(4):
            f = oracle_field(oracle, BH, BW, i, 3)
            assert got[i] == oracle.span_scan(f[0], f[1], 10, 0.0), i


def test_scan_fused_option_keeps_its_launches(twflow, oracle, gate_lifted):
    """TW_OPT_SCAN_FUSED_FINAL: tw_update_matrices + tw_blur_grid as before, never the grid-only iteration."""
    pairs = batch_pairs(BH, BW, 4)
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        e.set_option(twflow.OPT_SCAN_FUSED_FINAL, 1)
        got, cnt = submit_all(e, pairs, 10)
        assert cnt["tw_blur_grid"] == 1 and cnt["tw_flow_iter_grid"] == 0 and cnt["tw_span_gather"] == 0, cnt
        assert cnt["tw_flow_iter"] == 1 and cnt["tw_flow_iter_ups"] + cnt["tw_flow_iter_zero"] == 1, cnt
        for i in range(4):
            f = oracle_field(oracle, BH, BW, i, 3)
            assert got[i] == oracle.span_scan(f[0], f[1], 10, 0.0), i


@pytest.mark.parametrize("lanes", [1, 2])
def test_parts_of_a_batch(twflow, oracle, gate_lifted, lanes):
    """Eight pairs with the default TW_RAMP, as one part or one per TW_LANES=2 lane: every level-0 chunk ends in the grid-only
    iteration and writes its own pairs' grids."""
    if lanes == 2:
        gate_lifted.setenv("TW_LANES", "2")
    gate_lifted.delenv("TW_RAMP", raising=False)
    pairs = batch_pairs(BH, BW, 8)
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        got, cnt = submit_all(e, pairs, 10)
        assert cnt["tw_flow_iter_grid"] == lanes and cnt.last_z["tw_flow_iter_grid"] == 8 // lanes, (cnt, cnt.last_z)
        assert cnt["tw_span_gather"] == 0, cnt
        for i in range(8):
            f = oracle_field(oracle, BH, BW, i, 3)
            assert got[i] == oracle.span_scan(f[0], f[1], 10, 0.0), i


# ---- part 3: the default gate ----------------------------------------------------------------------------------------------
def test_default_gate(twflow, oracle, monkeypatch):
    """24 pairs of 640 x 480 pass level_runs_flow_iter without TW_MFREE: one level-0 chunk, one grid-only launch."""
    for name in ("TW_MFREE", "TW_LATENCY_STREAMS", "TW_RAMP", "TW_LANES", "TW_GRID_FINAL"):
        monkeypatch.delenv(name, raising=False)
    h, w, n = 480, 640, 24
    pairs = batch_pairs(h, w, n)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        assert e.level_runs_flow_iter(w, h, 0, n)
        got, cnt = submit_all(e, pairs, 10, 1.0)
        assert cnt["tw_flow_iter_grid"] == 1 and cnt.last_z["tw_flow_iter_grid"] == n and cnt["tw_span_gather"] == 0, (cnt, cnt.last_z)
        for i in range(n):
            f = oracle_field(oracle, h, w, i, 3)
            assert got[i] == oracle.span_scan(f[0], f[1], 10, 1.0), i
