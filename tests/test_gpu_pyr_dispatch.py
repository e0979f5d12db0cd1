"""The choice of a pyramid level's kernel (choose_pyr in twflow.hip), edge by edge.

Every case of tests/pyr_cases.py is a single tw_stage_pyr_level call.  Which side of an edge a size is on is read off
`Engine.pyr_plan` (tw_debug_pyr_plan: the function launch_pyr itself takes its kernel, grid and LDS size from) and asserted as
reached; the launch counters prove that the planned family — tw_pyr_level_lds apart from tw_pyr_level since this file — is the
one that ran; tail columns and clipped rows are asserted from the plan where a case has them; the output equals the oracle's level bit for bit and lies inside the float64 reference's bound
(tests/test_pyr_cases.py pins the oracle's level to that reference on the CPU).  The launches that write two levels
(tw_pyr_k3f, tw_pyr_23) run through their own entry points at every size of the table the plan calls eligible, and are refused
at the others.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyr_cases as PC  # noqa: E402
import test_oracle_stages_f64 as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _ceil_div(a, b):
    return -(-a // b)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ in bits, first at %r: got %r want %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v[0]) for v in np.nonzero(bad)), got[bad][:1], want[bad][:1])


@pytest.fixture(scope="module")
def engines(twflow):
    """One engine per (pyrScale, pyrLevels) of the table, made on first use (no environment switch set)."""
    made = {}

    def get(scale, levels):
        if (scale, levels) not in made:
            made[(scale, levels)] = twflow.Engine(0, twflow.default_params(pyrScale=scale, pyrLevels=levels), slots=1)
        return made[(scale, levels)]
    yield get
    for e in made.values():
        e.close()


def run_case(e, oracle, case):
    img = PC.image(case)
    assert e.num_levels(case.w0, case.h0) == len(PC.F.level_plan(case.w0, case.h0, case.scale, case.levels)) - 1
    e.launch_counts(reset=True)
    got = e.stage_pyr_level(img, case.level)
    ran = {k: v for k, v in e.launch_counts(reset=True).items() if v}
    plan = e.pyr_plan(case.w0, case.h0, case.level)
    print("pyrplan %s: %s" % (case.name, plan))
    # the plan says what the case claims
    assert {k: getattr(plan, k) for k in case.want} == case.want, (case.name, plan)
    assert (plan.w, plan.h, plan.ksize) == PC.level(case)[:3] and plan.mode == PC.resize_mode(case), (case.name, plan)
    # single-tap tail columns and clipped last rows are where the reference's coordinate rule puts them, and the cases made
    # for them have them (tests/test_pyr_cases.py: which levels do)
    assert (plan.xmax, plan.yclip) == PC.tail_and_clip(case), (case.name, plan)
    assert (plan.xmax < plan.w) == ("tail_columns" in case.rows) and (plan.yclip > 0) == ("clipped_rows" in case.rows), (case.name, plan)
    # the planned family is the one that ran, once
    staged = plan.kernel == "tw_pyr_level_lds"
    assert plan.family == ("tw_pyr_level_lds" if staged else plan.kernel), plan
    assert ran == ({"tw_pyr_level": 1, "tw_pyr_level_lds": 1} if staged else {plan.family: 1}), (case.name, plan, ran)
    # the grid covers the level with the planned tiles, and the staged kernels stay inside plan_geometry's LDS budget
    assert (plan.grid_x, plan.grid_y) == (_ceil_div(plan.w, plan.tile_cols), _ceil_div(plan.h, plan.rows)), plan
    assert plan.block == 256 and plan.aligned4 == (case.w0 % 4 == 0 and plan.kernel != "tw_pyr_level"), plan
    assert (plan.pitch > 0) == (plan.kernel in ("tw_pyr_taps", "tw_pyr_level_lds")) and plan.pitch % 4 == 0, plan
    assert (plan.lds == 0) == (plan.kernel == "tw_pyr_k3") and plan.lds <= (64 if plan.pitch else 160) * 1024, plan
    # the values
    assert got.shape == (plan.h, plan.w)
    same_bits(got, PC.oracle_level(oracle, case), "%s %r" % (case.name, plan))
    S.check("gpu", "pyr_case", case.name, got, *PC.reference(case.name))
    return plan, got


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if not c.env])
def test_each_case_takes_the_planned_kernel_and_equals_the_oracle(engines, oracle, name):
    case = PC.BY_NAME[name]
    run_case(engines(case.scale, case.levels), oracle, case)


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if c.env])
def test_cases_only_a_switch_reaches(twflow, oracle, monkeypatch, name):
    """The generic kernels' exact-halving (mode == 2) branch — no admitted parameters reach it, TW_PYR_GENERIC=1 / 2 do — and
    the unstaged kernel's single-tap tail column and clipped last row, which admitted parameters reach in the staged kernel only."""
    case = PC.BY_NAME[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    with twflow.Engine(0, twflow.default_params(pyrScale=case.scale, pyrLevels=case.levels), slots=1) as e:
        run_case(e, oracle, case)


def _sizes(pred):
    seen = []
    for c in PC.CASES:
        key = (c.w0, c.h0, c.scale, c.levels)
        if not c.env and key not in seen and pred(c):
            seen.append(key)
    return seen


@pytest.mark.parametrize("w0,h0,scale,levels", _sizes(lambda c: "fused23" in c.want))
def test_fused23_entry_follows_the_plan(twflow, engines, w0, h0, scale, levels):
    """tw_pyr_23 where the plan says eligible — bit for bit the two per-level launches — and a refusal everywhere else."""
    e = engines(scale, levels)
    case = next(c for c in PC.CASES if (c.w0, c.h0, c.scale, c.levels) == (w0, h0, scale, levels) and "fused23" in c.want)
    plan = e.pyr_plan(w0, h0, 0)
    assert plan.fused23 == case.want["fused23"], plan
    img = PC.image(case)
    e.launch_counts(reset=True)
    if not plan.fused23:
        with pytest.raises(twflow.TwError) as ei:
            e.stage_pyr_fused23(img)
        assert ei.value.code == twflow.TW_E_UNSUPPORTED
        assert not any(e.launch_counts().values())
        return
    I3, I2 = e.stage_pyr_fused23(img)
    cnt = e.launch_counts(reset=True)
    assert {k: v for k, v in cnt.items() if v} == {"tw_pyr_23": 1} and plan.threads23_pair == 1024, (cnt, plan)
    same_bits(I3, e.stage_pyr_level(img, 3), "tw_pyr_23 level 3 of %dx%d" % (w0, h0))
    same_bits(I2, e.stage_pyr_level(img, 2), "tw_pyr_23 level 2 of %dx%d" % (w0, h0))


@pytest.mark.parametrize("w0,h0,scale,levels", _sizes(lambda c: "fused01" in c.want))
def test_fused01_entry_follows_the_plan(twflow, engines, w0, h0, scale, levels):
    """tw_pyr_k3f where the plan says eligible (even sizes of the 0.5 pyramid) — bit for bit tw_pyr_k3<0> and <2> — and a
    refusal for the odd size and for pyrScale 0.6."""
    e = engines(scale, levels)
    case = next(c for c in PC.CASES if (c.w0, c.h0, c.scale, c.levels) == (w0, h0, scale, levels) and "fused01" in c.want)
    plan = e.pyr_plan(w0, h0, 1)
    assert plan.fused01 == case.want["fused01"], plan
    img = PC.image(case)
    e.launch_counts(reset=True)
    if not plan.fused01:
        with pytest.raises(twflow.TwError) as ei:
            e.stage_pyr_fused01(img)
        assert ei.value.code == twflow.TW_E_UNSUPPORTED
        assert not any(e.launch_counts().values())
        return
    I0, I1 = e.stage_pyr_fused01(img)
    cnt = e.launch_counts(reset=True)
    assert {k: v for k, v in cnt.items() if v} == {"tw_pyr_k3f": 1}, cnt
    same_bits(I0, e.stage_pyr_level(img, 0), "tw_pyr_k3f level 0 of %dx%d" % (w0, h0))
    same_bits(I1, e.stage_pyr_level(img, 1), "tw_pyr_k3f level 1 of %dx%d" % (w0, h0))
    assert e.pyr_plan(w0, h0, 0).kernel == e.pyr_plan(w0, h0, 1).kernel == "tw_pyr_k3"


def test_pyr23_workgroup_size_one_pair_a_batch_and_the_switch(twflow, oracle, monkeypatch):
    """tw_pyr_23<1024> for one pair's images (the stage entry, above), <512> for a batch's — two pairs of the smallest eligible
    size, their fields against the oracle — and <256> only under TW_PYR23_THREADS=256, run once here, bit for bit the others."""
    import synth
    w0 = h0 = 256
    case = PC.BY_NAME["f23_256_l3"]
    img = PC.image(case)
    pairs = [synth.make_pair(i, h0, w0) for i in range(2)]
    monkeypatch.setenv("TW_RAMP", "0")  # (a cold-start ramp would launch the batch in pieces no plan knows in advance)
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        plan = e.pyr_plan(w0, h0, 3)
        assert (plan.fused23, plan.threads23_pair, plan.threads23_batch) == (True, 1024, 512), plan
        view = e.level_plan(w0, h0, 0, 2, any_fout=True)
        rows = view.parts[0]
        assert view.kind == "batch" and len(view.parts) == 1 and (rows[3].per, rows[3].launches) == (2, 1), view
        out = e.host_array((2, 2, h0, w0), np.float32)
        e.launch_counts(reset=True)
        tk = [e.submit(a, b, 0, 5.0, flow=out[i]) for i, (a, b) in enumerate(pairs)]
        for t in tk:
            e.wait(t)
        cnt = e.launch_counts(reset=True)
        assert rows[3].images == 2 and rows[2].images == 1, rows  # (level 3's launch writes level 2's images too)
        assert cnt["tw_pyr_23"] == 1 and cnt.last_z["tw_pyr_23"] == 4, cnt  # four images: the 512-thread instantiation
        for i, (a, b) in enumerate(pairs):
            same_bits(out[i], np.stack(oracle.farneback(a, b)), "pair %d of the batch" % i)
        want3, want2 = e.stage_pyr_fused23(img)
    monkeypatch.setenv("TW_PYR23_THREADS", "256")
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        plan = e.pyr_plan(w0, h0, 3)
        assert (plan.threads23_pair, plan.threads23_batch) == (256, 256), plan
        I3, I2 = e.stage_pyr_fused23(img)
        assert e.launch_counts()["tw_pyr_23"] == 1
    same_bits(I3, want3, "tw_pyr_23<256> level 3")
    same_bits(I2, want2, "tw_pyr_23<256> level 2")
    same_bits(I3, PC.oracle_level(oracle, case), "tw_pyr_23<256> level 3 against the oracle")


def test_the_plan_refuses_what_it_cannot_answer(twflow, engines):
    e = engines(0.5, 3)
    L = twflow.lib()
    import ctypes as C
    v = (C.c_int * 23)()
    assert L.tw_debug_pyr_plan(None, 64, 64, 0, 64, v, 23) == -1
    assert L.tw_debug_pyr_plan(e._h, 64, 64, 0, 64, None, 23) == 0
    assert L.tw_debug_pyr_plan(e._h, 64, 64, 2, 64, v, 23) == 0  # (64 x 64 has levels 0 and 1)
    assert L.tw_debug_pyr_plan(e._h, 64, 64, -1, 64, v, 23) == 0 and L.tw_debug_pyr_plan(e._h, 0, 64, 0, 64, v, 23) == 0
    assert L.tw_debug_pyr_plan(e._h, 64, 64, 1, 64, v, 5) == 5
    # an odd row stride forbids whole-dword loads whatever the image's address
    assert e.pyr_plan(64, 64, 1).aligned4 and not e.pyr_plan(64, 64, 1, stride=65).aligned4


def test_the_plan_does_not_depend_on_what_ran_before(twflow, oracle):
    """tw_debug_pyr_plan answers for 4-byte-aligned image addresses, before any launch and after a batch at odd addresses (whose
    launches take the byte path); and that batch leaves nothing behind for the launches after it: a stage call and an aligned
    pair equal the oracle, the pair launch for launch what a fresh engine does.  64 x 64: levels 0 and 1, both tw_pyr_k3."""
    import ctypes as C
    w = h = 64
    base = np.random.default_rng(64).integers(0, 256, (h, w + 8), dtype=np.uint8)
    a, b = np.ascontiguousarray(base[:, 8:]), np.ascontiguousarray(base[:, :w])  # noise and a copy shifted by 8 pixels
    want = oracle.span_scan(*oracle.farneback(a, b), 10, 5.0)
    assert len(want) > 0

    def plans(e):
        return [e.pyr_plan(w, h, k) for k in (0, 1)]

    with twflow.Engine(0, twflow.default_params(), slots=1) as e, twflow.Engine(0, twflow.default_params(), slots=1) as fresh:
        before = plans(e)
        assert all(p.kernel == "tw_pyr_k3" and p.aligned4 for p in before), before
        assert not any(e.pyr_plan(w, h, k, stride=65).aligned4 for k in (0, 1))
        # a device pair at odd addresses
        da, db = (e.upload(np.concatenate([np.zeros(1, np.uint8), g.ravel()])) for g in (a, b))
        res = e.wait(e.submit_dev(C.c_void_p(da.value + 1), C.c_void_p(db.value + 1), w, h, w, 10, 5.0))
        assert res["vector"] == want
        assert plans(e) == before
        same_bits(e.stage_pyr_level(a, 1), oracle.pyr_level(a, oracle.level_plan(w, h)[1]), "level 1 after a batch at odd addresses")
        e.launch_counts(reset=True)
        assert e.diff(a, b, 10, 5.0)["vector"] == want
        assert fresh.diff(a, b, 10, 5.0)["vector"] == want
        got, ref = e.launch_counts(), fresh.launch_counts()
        assert got == ref and got.last_z == ref.last_z, (got, ref)
