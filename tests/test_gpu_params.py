"""The parameter axis on the GPU: polyN 1..7 and every non-default parameter on every schedule.

Part 1 — tw_stage_polyexp for polyN 1..7 x polySigma {0 (= 0.3 polyN), 1.1, 1.5, 3.0}, one engine per pair, on shapes
that cross the 240-column x 8-row polyexp tile in both directions, tiny shapes and 1080p (once for an even, once for
an odd polyN).  Each result is compared twice: with the CPU oracle bit for bit (uint32 view), and with the float64
reference of tests/farneback_f64.py inside its own bound on every pixel.  A negative control per polyN shows that the
device output differs from the oracle's for polyN +- 1, and the scalar and 240 x 16-tile kernels of the variants
library run every polyN too.

Part 2 — parameter sets (expansion, window, box window, pyramid / iterations) x schedules (single pair at 640 x 480 and
1080p, a 24-pair batch, the same batch in chunks and on two lanes, a batch with initial fields): dense flow and vectors
against the oracle, bit for bit over whole fields, and the kernel families that ran asserted from launch_counts().
Each (set, schedule) prints one `param_lattice | set | schedule | family=launches ...` line (run with -s);
profiles/param_lattice.md is that table from an MI355X run.
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import farneback_f64 as F  # noqa: E402
import test_oracle_stages_f64 as S  # noqa: E402
from conftest import interleaved  # noqa: E402
from test_flow_init_abi import farneback_with_init  # noqa: E402
from test_gpu_stages_f64 import EDGES, ran  # noqa: E402
from test_oracle_params import POLY_N, image  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def same_bits(got, want, what):
    """Equal as uint32: -0.0 is not 0.0 (none of these inputs produces a NaN)."""
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ in bits, first at %r: got %r want %r" % (
            what, int(bad.sum()), got.size, at, float(got[at]), float(want[at])))


# ---- tw_engine_create refuses the switches of kernels the default library does not carry -------------------------------------------
VARIANT_SWITCHES = [("TW_POLY_VARIANT", "0"), ("TW_BLUR_VARIANT", "8"), ("TW_BLUR_PIPE", "3"), ("TW_BLUR_SMALL", "2"),
                    ("TW_BLUR_SMALL_LEVELS", "-1,3"), ("TW_UPD_NY", "1")]


@pytest.mark.parametrize("name,value", VARIANT_SWITCHES)
def test_the_default_library_refuses_a_variants_switch(twflow, monkeypatch, name, value):
    import ctypes as C
    L = twflow.lib()
    assert L.tw_has_variants() == 0
    monkeypatch.setenv(name, value)
    h = C.c_void_p(1)
    assert L.tw_engine_create(0, None, 1, C.byref(h)) == twflow.TW_E_UNSUPPORTED
    assert not h.value


def test_the_default_library_admits_the_default_values_of_those_switches(twflow, monkeypatch):
    import ctypes as C
    L = twflow.lib()
    assert L.tw_has_variants() == 0
    monkeypatch.setenv("TW_UPD_NY", "2")
    monkeypatch.setenv("TW_BLUR_SMALL", "1")
    h = C.c_void_p()
    assert L.tw_engine_create(0, None, 1, C.byref(h)) == twflow.TW_OK and h.value
    L.tw_engine_destroy(h)


# ---- part 1: tw_stage_polyexp over polyN x polySigma -----------------------------------------------------------------------
STAGE_SIGMAS = (0.0, 1.1, 1.5, 3.0)
TILE_ROWS = [(7, 239), (8, 240), (9, 241), (15, 479), (16, 480), (17, 481)]  # (h, w) around 8 rows x 240 columns
TINY = [(1, 1), (1, 5), (5, 1), (3, 5)]
BIG = {(4, 0.0): [(1080, 1920)], (5, 1.1): [(1080, 1920)]}  # once for an even polyN, once for an odd one


@pytest.mark.parametrize("sg", STAGE_SIGMAS)
@pytest.mark.parametrize("n", POLY_N)
def test_stage_polyexp_every_polyn_and_sigma(twflow, oracle, n, sg):
    with twflow.Engine(0, twflow.default_params(polyN=n, polySigma=sg), slots=1) as e:
        e.launch_counts(reset=True)
        for h, w in EDGES + TILE_ROWS + TINY + BIG.get((n, sg), []):
            I = image(h, w)
            got = interleaved(e.stage_polyexp(I))
            ran(e, "tw_polyexp", 1)
            case = "%dx%d/n%d/s%g" % (w, h, n, sg)
            same_bits(got, oracle.polyexp(I, n, sg), "polyexp " + case)
            ref, bound = F.polyexp(I, 0.0, n, sg)
            assert np.isfinite(bound).all(), case
            S.check("gpu", "polyexp", case, got, ref, bound)
        if sg == 3.0:
            # negative control: at sigma 3.0 the outer taps carry weight, so the oracle's result for polyN +- 1 is another
            # one (tests/test_oracle_params.py shows it leaves the reference's bound on > 90 % of the values)
            I = image(37, 241)
            got = interleaved(e.stage_polyexp(I))
            for m in (n - 1, n + 1):
                if 1 <= m <= 7:
                    other = oracle.polyexp(I, m, sg)
                    differ = float((got.view(np.uint32) != other.view(np.uint32)).mean())
                    print("negative control polyN %d against the oracle's polyN %d: %.1f %% of the values differ" % (
                        n, m, 100 * differ))
                    assert differ > 0.9, (n, m, differ)


@pytest.mark.parametrize("variant", ["0", "2"])
def test_polyexp_variants_every_polyn(twflow, oracle, variant, monkeypatch):
    """The scalar kernel (TW_POLY_VARIANT=0) and the 240 x 16-tile kernel (=2) of the variants library, every polyN, at a
    shape past two tile columns and one past one tile in both directions (17 rows: a second 16-row tile of one row)."""
    monkeypatch.setenv("TW_POLY_VARIANT", variant)
    for n in POLY_N:
        sg = (0.0, 1.1, 3.0)[n % 3]
        with twflow.use_variants_library() as L, twflow.Engine(0, twflow.default_params(polyN=n, polySigma=sg), slots=1) as e:
            assert L.tw_has_variants() == 1
            e.launch_counts(reset=True)
            for h, w in ((17, 481), (37, 241)):
                I = image(h, w)
                got = interleaved(e.stage_polyexp(I))
                ran(e, "tw_polyexp", 1)
                case = "%dx%d/n%d/s%g/variant%s" % (w, h, n, sg, variant)
                same_bits(got, oracle.polyexp(I, n, sg), "polyexp " + case)
                S.check("gpu", "polyexp", case, got, *F.polyexp(I, 0.0, n, sg))


# ---- part 2: parameter sets x schedules ------------------------------------------------------------------------------------
EXPANSION = [dict(polyN=1), dict(polyN=2), dict(polyN=3, polySigma=0.0), dict(polyN=4), dict(polyN=5, polySigma=1.1),
             dict(polyN=6, polySigma=3.0)]
WINDOW = [dict(winSize=s) for s in (29, 32, 33, 49, 50, 52)]
BOX = [dict(flags=0), dict(flags=0, winSize=50)]
PYRAMID = [dict(pyrScale=0.6), dict(pyrScale=0.8, pyrLevels=4), dict(pyrIterations=0), dict(pyrLevels=0)]
SETS = EXPANSION + WINDOW + BOX + PYRAMID
SETS_1080P = [dict(polyN=5, polySigma=1.1), dict(polyN=2), dict(winSize=50), dict(flags=0)]
ONE_PER_AXIS = [dict(polyN=4), dict(winSize=33), dict(flags=0), dict(pyrScale=0.6)]
H, W, NB = 480, 640, 24

WIN15 = ("tw_blur_solve4", "tw_blur_solve4q", "tw_blur_solve_pp")  # the 31-tap window's kernels of the product library
WIN25 = ("tw_blur_solve4y", "tw_blur_solve8")                      # the 51-tap window's
GENERIC = ("tw_blur_solve_generic",)
BOXFAM = ("tw_box",)
FLOW_ITER = ("tw_flow_iter", "tw_flow_iter_ups", "tw_flow_iter_zero")
ITERATION = WIN15 + WIN25 + GENERIC + BOXFAM + FLOW_ITER + ("tw_blur_variant", "tw_blur_grid", "tw_twin")


def name(kw):
    return ",".join("%s=%g" % (k, v) for k, v in kw.items())


def window_family(kw):
    """The families a set's window launches belong to outside tw_flow_iter (launch_blur dispatches on winSize / 2)."""
    if kw.get("pyrIterations", 3) == 0:
        return ()
    if not kw.get("flags", 256) & 256:
        return BOXFAM
    m = kw.get("winSize", 30) // 2
    return WIN15 if m == 15 else WIN25 if m == 25 else GENERIC


def record(kw, schedule, cnt):
    print("param_lattice | %s | %s | %s" % (name(kw), schedule, " ".join("%s=%d" % (k, v) for k, v in cnt.items() if v)))


def assert_families(kw, cnt, flow_iter_allowed=False):
    """The set's own window family ran, and no other family that averages a window."""
    own = window_family(kw) + (FLOW_ITER if flow_iter_allowed else ())
    assert sum(cnt[f] for f in own) >= (1 if own else 0), (kw, dict(cnt))
    for f in ITERATION:
        if f not in own:
            assert cnt[f] == 0, (kw, f, dict(cnt))


class Wants:
    """The oracle's fields for (parameter set, size, pair), computed once on a small thread pool (the oracle is plain C
    behind ctypes: no shared state, the interpreter lock released) and kept for every schedule that needs them."""

    def __init__(self, oracle):
        import synth
        self.oracle = oracle
        self.pairs = {(H, W, i): synth.make_pair(i, H, W) for i in range(4)}
        self.pairs[(1080, 1920, 0)] = synth.make_pair(0, 1080, 1920)
        jobs = [(name(kw), kw, 1080, 1920, 0) for kw in SETS_1080P] + [(name(kw), kw, H, W, i) for kw in SETS for i in range(4)]
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda j: np.stack(oracle.farneback(*self.pairs[j[2:]], oracle.default_params(**j[1]))), jobs))
        self.fields = {(j[0],) + j[2:]: r for j, r in zip(jobs, res)}

    def field(self, kw, h, w, i):
        return self.fields[(name(kw), h, w, i)]  # planar (2, h, w)

    def vectors(self, kw, h, w, i, span, thr):
        f = self.field(kw, h, w, i)
        return self.oracle.span_scan(f[0], f[1], span, thr)


@pytest.fixture(scope="module")
def wants(oracle):
    return Wants(oracle)


def single_pair(twflow, wants, kw, h, w, i):
    a, b = wants.pairs[(h, w, i)]
    with twflow.Engine(0, twflow.default_params(**kw), slots=1) as e:
        e.launch_counts(reset=True)
        gx, gy, _ = e.calculate_internal(a, b)
        v = e.diff(a, b, 10, 0.0)["vector"]
        cnt = e.launch_counts()
    record(kw, "single pair %dx%d" % (w, h), cnt)
    want = wants.field(kw, h, w, i)
    same_bits(gx, want[0], "flowx %s %dx%d" % (name(kw), w, h))
    same_bits(gy, want[1], "flowy %s %dx%d" % (name(kw), w, h))
    assert v == wants.vectors(kw, h, w, i, 10, 0.0), kw
    assert len(v) > 1000 or kw.get("pyrIterations") == 0, (kw, len(v))  # (threshold 0: every grid point with a non-zero flow)
    # every set fails a clause of the twin schedule (polyN == 7, winSize / 2 == 15, Gaussian, three exact halvings, >= 1
    # iteration): the expansion is a launch of its own, twice (calculate_internal, diff) per level
    assert cnt["tw_twin"] == 0 and cnt["tw_polyexp"] >= 2, (kw, dict(cnt))
    assert cnt.flow_iter() == 0, (kw, dict(cnt))  # a single pair keeps the tile kernels
    assert_families(kw, cnt)
    return cnt


@pytest.mark.parametrize("kw", SETS, ids=name)
def test_single_pair_480x640(twflow, wants, kw):
    single_pair(twflow, wants, kw, H, W, SETS.index(kw) % 2)  # (pairs 0 and 1 are warped all over)


@pytest.mark.parametrize("kw", SETS_1080P, ids=name)
def test_single_pair_1080p(twflow, wants, kw):
    single_pair(twflow, wants, kw, 1080, 1920, 0)


def batch(twflow, wants, kw, schedule, check_counts):
    ex = [wants.pairs[(H, W, i % 4)][0] for i in range(NB)]
    tg = [wants.pairs[(H, W, i % 4)][1] for i in range(NB)]
    with twflow.Engine(0, twflow.default_params(**kw), slots=NB) as e:
        e.launch_counts(reset=True)
        out, res = e.flow_batch(ex, tg, layout="planar", span=10, threshold=0.0)
        cnt = e.launch_counts()
        record(kw, schedule, cnt)
        for i in range(NB):
            same_bits(out[i], wants.field(kw, H, W, i % 4), "%s, %s, pair %d" % (name(kw), schedule, i))
        vec = [wants.vectors(kw, H, W, i, 10, 0.0) for i in range(4)]
        assert all(res[i]["vector"] == vec[i % 4] for i in range(NB)), (kw, schedule)
        assert len(vec[0]) > 1000 or kw.get("pyrIterations") == 0  # (no iteration: the flow stays zero)
        check_counts(e, cnt)


@pytest.mark.parametrize("kw", SETS, ids=name)
def test_batch_of_24(twflow, wants, kw):
    assert not {"TW_MFREE", "TW_CHUNK_TILES", "TW_LANES"} & set(os.environ)

    def check(e, cnt):
        levels = e.num_levels(W, H)
        runs = [e.level_runs_flow_iter(W, H, k, NB) for k in range(levels + 1)]
        if kw in EXPANSION:
            # the tw_flow_iter schedule exactly as the default parameters take it (test_pipeline_with_m_free_iterations)
            assert runs == [True, False, False, False], runs
            assert cnt["tw_flow_iter_ups"] == 1 and cnt["tw_flow_iter"] == 2 and cnt["tw_flow_iter_zero"] == 0, dict(cnt)
            assert cnt.last_z["tw_flow_iter"] == NB and cnt.last_z["tw_flow_iter_ups"] == NB, cnt.last_z
            assert cnt["tw_update_matrices"] == 3, dict(cnt)
            assert cnt["tw_polyexp"] == levels + 1 and cnt.last_z["tw_polyexp"] == 2 * NB, (dict(cnt), cnt.last_z)
            assert_families(kw, cnt, flow_iter_allowed=True)
        elif kw in WINDOW or kw in BOX:
            assert not any(runs) and cnt.flow_iter() == 0, (runs, dict(cnt))
            assert_families(kw, cnt)
            assert max(cnt.last_z[f] for f in window_family(kw)) >= 2, cnt.last_z  # batched launches, not pair by pair
        elif kw.get("pyrIterations") == 0:
            assert not any(runs), runs
            assert_families(kw, cnt)  # no iteration kernel at all
        else:
            # another pyramid, the default window: every level the schedule's own predicate names runs tw_flow_iter for its
            # three iterations, the others the tile kernels
            assert cnt.flow_iter() == 3 * sum(runs) and sum(runs) >= 1, (runs, dict(cnt))
            assert (sum(cnt[f] for f in WIN15) > 0) == (not all(runs)), (runs, dict(cnt))
            assert_families(kw, cnt, flow_iter_allowed=True)
    batch(twflow, wants, kw, "batch of 24", check)


@pytest.mark.parametrize("env", [dict(TW_CHUNK_TILES="100"), dict(TW_CHUNK_TILES="100", TW_LANES="2")],
                         ids=lambda env: "+".join(sorted(env)))
@pytest.mark.parametrize("kw", ONE_PER_AXIS, ids=name)
def test_batch_of_24_in_chunks_and_on_two_lanes(twflow, wants, kw, env, monkeypatch):
    """Level 0 in several launches (TW_CHUNK_TILES=100), and those on two streams (TW_LANES=2)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)

    def check(e, cnt):
        chunk = e.level_chunk(W, H, 0)
        assert chunk * 3 <= NB, chunk
        assert cnt["tw_flow_export"] >= 3, dict(cnt)  # one per level-0 chunk, before the next chunk reuses the buffer
        assert_families(kw, cnt, flow_iter_allowed=window_family(kw) == WIN15)
    batch(twflow, wants, kw, "batch of 24, " + " ".join("%s=%s" % kv for kv in sorted(env.items())), check)


@pytest.mark.parametrize("kw", [dict(polyN=4), dict(flags=0)], ids=name)
def test_batch_with_initial_fields_and_destinations(twflow, oracle, wants, kw):
    """tw_submit_u8_flow_init with flow destinations: four pairs in one batch, three with a field (sigma 3 px noise), one
    starting from zero, against farneback_with_init — the oracle's stages in orc_farneback's loop."""
    pairs = [wants.pairs[(H, W, i)] for i in range(4)]
    init = [None if i == 2 else (np.random.default_rng(50 + i).standard_normal((H, W, 2)) * 3).astype(F32) for i in range(4)]
    p = oracle.default_params(**kw)
    with ThreadPoolExecutor(4) as ex:
        want = list(ex.map(lambda i: np.stack(farneback_with_init(oracle, pairs[i][0], pairs[i][1], init[i], p)), range(4)))
    same_bits(want[2], wants.field(kw, H, W, 2), "farneback_with_init without a field is orc_farneback")
    with twflow.Engine(0, twflow.default_params(**kw), slots=4) as e:
        e.launch_counts(reset=True)
        out, res = e.flow_batch([a for a, _ in pairs], [b for _, b in pairs], layout="planar", span=10, threshold=0.0, init=init)
        out = np.array(out)  # (page-locked memory of the engine: copied before it closes)
        cnt = e.launch_counts()
    record(kw, "batch of 4, initial fields", cnt)
    for i in range(4):
        same_bits(out[i], want[i], "%s, initial field, pair %d" % (name(kw), i))
        assert res[i]["vector"] == oracle.span_scan(want[i][0], want[i][1], 10, 0.0), (kw, i)
    assert cnt["tw_flow_area_init"] >= 1 and cnt["tw_flow_export"] >= 1 and cnt["tw_polyexp"] >= 1, dict(cnt)
    assert_families(kw, cnt, flow_iter_allowed=window_family(kw) == WIN15)
