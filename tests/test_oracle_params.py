"""The parameter axis on the CPU: polyN 1..7 x polySigma of the oracle's expansion against the float64 reference, whether
that comparison can tell neighbouring parameters apart, and both sides of every edge of tw_engine_create's predicate.

tests/test_oracle_stages_f64.py::test_polyexp_every_pixel pins (7, 1.5), (5, 1.1) and (7, 0) on one shape each; this
module runs every admitted polyN with five sigmas (0 = the 0.3 * polyN default) on shapes from 1 x 1 to one past two
polyexp tiles (240 columns x 8 rows on the device), every pixel, the bound the reference returns being the only
tolerance.  tests/test_gpu_params.py points the same checks at the kernels.  Each comparison prints `f64ref ...` and the
discrimination test prints the fraction of values beyond the bound (run with -s); profiles/param_lattice.md records them.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import farneback_f64 as F
import test_oracle_stages_f64 as S

F32 = np.float32
POLY_N = (1, 2, 3, 4, 5, 6, 7)
SIGMAS = (0.0, 0.4, 1.1, 1.5, 3.0)
SHAPES = [(1, 1), (3, 5), (9, 241), (37, 240), (17, 481)]  # (h, w); 3 x 5 is smaller than every window


def image(h, w):
    """The input of test_gpu_stages_f64.test_stage_polyexp: a smoothed random image with a constant rectangle."""
    rng = np.random.default_rng(h * 7 + w)
    I = (ndimage.gaussian_filter(rng.random((h, w)), 1.0) * 255).astype(F32)
    I[h // 4: h // 2, w // 3: w // 2] = 17.25
    return I


# ---- (a) oracle == reference, every pixel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", POLY_N)
def test_polyexp_every_polyn_and_sigma(oracle, n):
    for sg in SIGMAS:
        for h, w in SHAPES:
            I = image(h, w)
            ref, bound = F.polyexp(I, 0.0, n, sg)
            assert np.isfinite(bound).all(), (n, sg, h, w)
            S.check("oracle", "polyexp", "%dx%d/n%d/s%g" % (w, h, n, sg), oracle.polyexp(I, n, sg), ref, bound)


def test_sigma_zero_is_three_tenths_of_polyn(oracle):
    """polySigma < FLT_EPSILON means 0.3 * polyN: the same bits as that sigma given outright, for every polyN."""
    I = image(37, 241)
    for n in POLY_N:
        assert np.array_equal(oracle.polyexp(I, n, 0.0).view(np.uint32), oracle.polyexp(I, n, n * 0.3).view(np.uint32)), n
        assert not np.array_equal(oracle.polyexp(I, n, 0.0), oracle.polyexp(I, n, n * 0.3 + 0.1)), n


# ---- (b) the comparison discriminates ---------------------------------------------------------------------------------------
def outside(got, ref, bound):
    return S.ratio(got, ref, bound)[2] / ref.size


@pytest.mark.parametrize("n", POLY_N)
def test_neighbouring_parameters_leave_the_bound(oracle, n):
    """At sigma 3.0 the outer taps carry weight for every polyN (at sigma 1.1 those of polyN 6 and 7 are below float32
    resolution, and n +- 1 would pass): the oracle's result for polyN n - 1 and n + 1, judged against the reference for
    n, must be outside the bound on more than 90 % of the values, and the result for 1.01 * sigma on more than half —
    else the inputs have degenerated into something every kernel passes."""
    h, w, sg = 37, 241, 3.0
    I = image(h, w)
    ref, bound = F.polyexp(I, 0.0, n, sg)
    assert S.ratio(oracle.polyexp(I, n, sg), ref, bound)[2] == 0
    for m in (n - 1, n + 1):
        if 1 <= m <= 7:
            frac = outside(oracle.polyexp(I, m, sg), ref, bound)
            print("f64ref discriminate polyN %d judged as %d at sigma %g: %.1f %% of %d values beyond the bound" % (
                m, n, sg, 100 * frac, ref.size))
            assert frac > 0.9, (n, m, frac)
    frac = outside(oracle.polyexp(I, n, 1.01 * sg), ref, bound)
    print("f64ref discriminate polyN %d sigma %g judged as %g: %.1f %% of %d values beyond the bound" % (
        n, 1.01 * sg, sg, 100 * frac, ref.size))
    assert frac > 0.5, (n, frac)


# ---- (c) tw_engine_create's predicate ----------------------------------------------------------------------------------------
def create(twflow, device=-1, **kw):
    """tw_engine_create's status for the default parameters with `kw` changed.  The parameter predicate returns before
    the device is looked at, so a refused set gives its own status on any machine; an admitted set goes on to the device
    check, which answers TW_E_DEVICE for device -1 with or without a GPU (and for device 0 on a machine without one)."""
    h = C.c_void_p()
    p = twflow.default_params(**kw)
    rc = twflow.lib().tw_engine_create(device, C.byref(p), 1, C.byref(h))
    assert not h.value, kw
    return rc


ADMITTED = [dict(polyN=1), dict(polyN=7), dict(winSize=2), dict(winSize=65), dict(pyrScale=0.999), dict(pyrScale=1e-9),
            dict(pyrIterations=0), dict(pyrLevels=0), dict(polyN=1, winSize=2, pyrIterations=0, pyrLevels=0)]
REFUSED = [(dict(polyN=0), "TW_E_UNSUPPORTED"), (dict(polyN=8), "TW_E_UNSUPPORTED"), (dict(polyN=-1), "TW_E_UNSUPPORTED"),
           (dict(winSize=1), "TW_E_UNSUPPORTED"), (dict(winSize=66), "TW_E_UNSUPPORTED"), (dict(winSize=0), "TW_E_UNSUPPORTED"),
           (dict(pyrScale=0.0), "TW_E_UNSUPPORTED"), (dict(pyrScale=-0.5), "TW_E_UNSUPPORTED"),
           (dict(pyrScale=1.0), "TW_E_UNSUPPORTED"), (dict(pyrScale=float("nan")), "TW_E_UNSUPPORTED"),
           (dict(pyrIterations=-1), "TW_E_BAD_PARAMETER"), (dict(pyrLevels=-1), "TW_E_BAD_PARAMETER")]


@pytest.mark.parametrize("kw", ADMITTED, ids=repr)
def test_predicate_admits(twflow, kw):
    assert create(twflow, **kw) == twflow.TW_E_DEVICE, kw
    if twflow.device_count() == 0:
        assert create(twflow, device=0, **kw) == twflow.TW_E_DEVICE, kw


@pytest.mark.parametrize("kw,status", REFUSED, ids=lambda v: repr(v) if isinstance(v, dict) else v)
def test_predicate_refuses(twflow, kw, status):
    assert create(twflow, **kw) == getattr(twflow, status), kw
    assert create(twflow, device=0, **kw) == getattr(twflow, status), kw
