"""Initial flow fields (tw_submit_*_flow_init, OPTFLOW_USE_INITIAL_FLOW) on the GPU.

Every field is compared bit for bit (np.array_equal on float32) with farneback_with_init of tests/test_flow_init_abi.py —
the numpy INTER_AREA restatement composed with the oracle's stages — and every vector list with oracle.span_scan of that
field.  Pairs without a field are compared with the plain submission of the same pair.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_init_abi import farneback_with_init  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _pairs(n, h, w):
    import synth
    return [synth.make_pair(i, h, w) for i in range(n)]


def _field(seed, h, w, layout="interleaved", pad=0, amp=3.0):
    """A smooth-ish random full-resolution field; rows padded by `pad` floats (the view has the real width)."""
    rng = np.random.default_rng(1000 + seed)
    f = (rng.standard_normal((h, w, 2)) * amp).astype(F32)
    if layout == "interleaved":
        a = np.full((h, w + pad, 2), np.nan, F32)
        a[:, :w] = f
        return a[:, :w], f
    a = np.full((2, h, w + pad), np.nan, F32)
    a[:, :, :w] = np.moveaxis(f, 2, 0)
    return a[:, :, :w], f


def _want(oracle, pair, f, params=None):
    fx, fy = farneback_with_init(oracle, pair[0], pair[1], f, params)
    return np.stack([fx, fy])


def _planar_out(e, n, h, w):
    arr = e.host_array((n, 2, h, w), np.float32)
    arr[...] = np.nan
    return arr


def _fam(e, name):
    return e.launch_counts()[name]


def _last_z(e, name):
    import twflow
    L = twflow.lib()
    n = 64
    counts = (C.c_ulonglong * n)()
    lz = (C.c_ulonglong * n)()
    nf = L.tw_debug_launch_counts(e._h, counts, lz, n, 0)
    for i in range(nf):
        if L.tw_debug_family_name(i) == name.encode():
            return lz[i]
    raise KeyError(name)


@pytest.mark.parametrize("hw", [(117, 180), (480, 640), (1079, 1917)])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_host_batches_both_layouts(twflow, oracle, hw, layout):
    """Generic (180x117, 1917x1079) and fast (640x480) paths; page-locked and pageable fields with padded rows."""
    h, w = hw
    n = 4 if w < 1000 else 2
    pairs = _pairs(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        out = _planar_out(e, n, h, w)
        fields, tk = [], []
        for i in range(n):
            view, f = _field(i, h, w, layout, pad=5)
            if i % 2 == 0:  # page-locked (DMA-ed in place): a host_array copy of the padded view
                pin = e.host_array(view.base.shape, np.float32)
                pin[...] = view.base
                view = pin[:, :w] if layout == "interleaved" else pin[:, :, :w]
            fields.append((view, f))
            tk.append(e.submit(*pairs[i], 10, 0.0, flow=out[i], init=view))
        e.launch_counts(reset=False)
        res = [e.wait(t) for t in tk]
        assert _fam(e, "tw_flow_area_init") >= 1
        for i in range(n):
            want = _want(oracle, pairs[i], fields[i][1])
            assert np.array_equal(out[i], want), "pair %d" % i
            assert res[i]["vector"] == oracle.span_scan(want[0], want[1], 10, 0.0)


def test_1080p_pair_in_a_16_pair_batch(twflow, oracle):
    """Span 4, threshold 0, a 16-pair 1080p host batch (fast path, ratio 8, LDS staging): one coarsest-level launch of the
    init kernel for all 16 pairs; the pair with a field matches the restatement, the others the plain submission."""
    h, w, n = 1080, 1920, 16
    pairs = _pairs(2, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain_out = _planar_out(e, n, h, w)
        plain = [e.wait(t) for t in [e.submit(*pairs[i % 2], 4, 0.0, flow=plain_out[i]) for i in range(n)]]
        out = _planar_out(e, n, h, w)
        _, f = _field(3, h, w)
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[i % 2], 4, 0.0, flow=out[i], init=f if i == 5 else None) for i in range(n)]
        res = [e.wait(t) for t in tk]
        assert _fam(e, "tw_flow_area_init") == 1 and _last_z(e, "tw_flow_area_init") == n
        want = _want(oracle, pairs[1], f)
        assert np.array_equal(out[5], want)
        assert res[5]["vector"] == oracle.span_scan(want[0], want[1], 4, 0.0)
        for i in range(n):
            if i != 5:
                assert np.array_equal(out[i], plain_out[i]) and res[i]["vector"] == plain[i]["vector"], "pair %d" % i


def test_unusual_parameters(twflow, oracle):
    """pyrLevels 0 (a copy at scale 1), pyrScale 0.6 (a scale that is not a power of two), one iteration, box window."""
    h, w = 240, 320
    pairs = _pairs(2, h, w)
    for kw in (dict(pyrLevels=0), dict(pyrScale=0.6, pyrLevels=3), dict(pyrIterations=1), dict(flags=0),
               dict(pyrScale=0.6, flags=0, pyrIterations=1)):
        p = twflow.default_params(**kw)
        op = oracle.default_params(**kw)
        with twflow.Engine(0, p, slots=2) as e:
            out = _planar_out(e, 2, h, w)
            fs = [_field(i, h, w)[1] for i in range(2)]
            tk = [e.submit(*pairs[i], 0, 5.0, flow=out[i], init=fs[i]) for i in range(2)]
            for t in tk:
                e.wait(t)
            for i in range(2):
                assert np.array_equal(out[i], _want(oracle, pairs[i], fs[i], op)), (kw, i)


@pytest.mark.parametrize("env", [dict(), dict(TW_CHUNK_TILES="100"), dict(TW_CHUNK_TILES="100", TW_LANES="2")])
def test_mixed_batches_one_launch_per_chunk(twflow, oracle, env, monkeypatch):
    """Pairs without a field equal the plain submission bit for bit; the init kernel runs once per coarsest-level chunk
    (TW_CHUNK_TILES=100: one pair per launch; TW_LANES=2: the two halves on two streams)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w, n = 480, 640, 6
    pairs = _pairs(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain_out = _planar_out(e, n, h, w)
        plain = [e.wait(t) for t in [e.submit(*pairs[i], 10, 2.0, flow=plain_out[i]) for i in range(n)]]
        chunk = e.level_chunk(w, h, e.num_levels(w, h))
        out = _planar_out(e, n, h, w)
        fs = {1: _field(1, h, w)[1], 4: _field(4, h, w, "planar")[0]}
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[i], 10, 2.0, flow=out[i], init=fs.get(i)) for i in range(n)]
        res = [e.wait(t) for t in tk]
        lanes = 2 if env.get("TW_LANES") == "2" else 1
        per_lane = -(-n // lanes)
        want_launches = lanes * -(-per_lane // min(chunk, per_lane))
        assert _fam(e, "tw_flow_area_init") == want_launches
        for i in range(n):
            if i in fs:
                f = fs[i] if fs[i].shape == (h, w, 2) else np.moveaxis(fs[i], 0, 2)
                want = _want(oracle, pairs[i], f)
                assert np.array_equal(out[i], want), "pair %d" % i
                assert res[i]["vector"] == oracle.span_scan(want[0], want[1], 10, 2.0)
            else:
                assert np.array_equal(out[i], plain_out[i]) and res[i]["vector"] == plain[i]["vector"], "pair %d" % i


_TORCH_CHILD = r"""
import sys
import numpy as np
import torch  # before the library: torch's HIP runtime must be the one the process loads first (as in bench.py)
torch.cuda.init()
sys.path[:0] = sys.argv[1:]
import oracle, synth, twflow
from test_flow_init_abi import farneback_with_init
F32 = np.float32
def want_of(pair, f):
    return np.stack(farneback_with_init(oracle, pair[0], pair[1], f))
h, w, n = 480, 640, 3
pairs = [synth.make_pair(i, h, w) for i in range(n)]
fs = [(np.random.default_rng(1000 + i).standard_normal((h, w, 2)) * 3.0).astype(F32) for i in range(n)]
dev = torch.device("cuda", 0)
ex = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
tg = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
init = torch.from_numpy(np.stack(fs)).to(dev)
with twflow.Engine(0, twflow.default_params(), slots=n) as e:
    # flow_batch: torch images, a stacked torch init tensor, fields out on the device
    out, _ = e.flow_batch(ex, tg, layout="interleaved", span=0, init=init)
    got = out.cpu().numpy()
    want = [want_of(pairs[i], fs[i]) for i in range(n)]
    for i in range(n):
        assert np.array_equal(np.moveaxis(got[i], 2, 0), want[i]), ("flow_batch", i)
    # tw_submit_dev_flow_init: a planar device field with padded rows (a raw tuple), a device destination
    pf = torch.full((2, h, w + 8), float("nan"), dtype=torch.float32, device=dev)
    pf[:, :, :w] = torch.from_numpy(np.ascontiguousarray(np.moveaxis(fs[0], 2, 0))).to(dev)
    d1 = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.wait(e.submit_dev(ex[0].data_ptr(), tg[0].data_ptr(), w, h, w, 0, 5.0, flow=d1,
                        init=(pf.data_ptr(), (w + 8) * 4, twflow.FLOW_PLANAR)))
    assert np.array_equal(np.moveaxis(d1.cpu().numpy(), 2, 0), want[0]), "submit_dev"
    # chaining: pair 0's destination, waited, is pair 1's initial field (it never leaves HBM)
    d2 = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    e.wait(e.submit_dev(ex[1].data_ptr(), tg[1].data_ptr(), w, h, w, 0, 5.0, flow=d2, init=d1))
    w2 = want_of(pairs[1], np.ascontiguousarray(np.moveaxis(want[0], 0, 2)))
    assert np.array_equal(np.moveaxis(d2.cpu().numpy(), 2, 0), w2), "chained"
print("torch ok")
"""


def test_device_inits_and_chaining():
    """Device fields through flow_batch (torch tensors) and tw_submit_dev_flow_init; pair 0's device destination, once
    waited, is pair 1's initial field.  In a child process, so that torch is imported before the library."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, os.path.join(root, "tidal-wave_amd"), os.path.join(root, "oracle"),
                        os.path.join(root, "tests")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "torch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("hw", [(480, 640), (1080, 1920)])
def test_single_pair_schedule(twflow, oracle, hw):
    """A slots=1 engine: the single-pair schedule (twin launches at 1080p) with the coarsest update reading the field."""
    h, w = hw
    pairs = _pairs(1, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=1) as e:
        out = _planar_out(e, 1, h, w)
        _, f = _field(7, h, w)
        e.launch_counts(reset=True)
        t = e.submit(*pairs[0], 10, 1.0, flow=out[0], init=f)
        r = e.wait(t)
        assert _fam(e, "tw_flow_area_init") == 1
        want = _want(oracle, pairs[0], f)
        assert np.array_equal(out[0], want)
        assert r["vector"] == oracle.span_scan(want[0], want[1], 10, 1.0)


def test_ramp_pieces(twflow, oracle):
    """A 64-slot engine fed host pairs from idle: the cold-start ramp's pieces each start behind their own uploads —
    host fields are uploaded behind the same marks, and each piece's coarsest level runs the init kernel."""
    h, w, n = 240, 320, 64
    pairs = _pairs(4, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        plain_out = _planar_out(e, n, h, w)
        for t in [e.submit(*pairs[i % 4], 0, 5.0, flow=plain_out[i]) for i in range(n)]:
            e.wait(t)
        out = _planar_out(e, n, h, w)
        fs = {i: _field(i, h, w)[1] for i in (0, 17, 40, 63)}
        e.launch_counts(reset=True)
        tk = [e.submit(*pairs[i % 4], 0, 5.0, flow=out[i], init=fs.get(i)) for i in range(n)]
        for t in tk:
            e.wait(t)
        assert _fam(e, "tw_flow_area_init") >= 3  # (three ramp pieces, one coarsest-level launch each)
        for i in range(n):
            if i in fs:
                assert np.array_equal(out[i], _want(oracle, pairs[i % 4], fs[i])), "pair %d" % i
            else:
                assert np.array_equal(out[i], plain_out[i]), "pair %d" % i


def test_zero_field_equals_no_field_through_the_nonzero_kernels(twflow, monkeypatch):
    """init = 0 gives the field of no init, but through the kernels that read a flow: tw_update_matrices with zero_flow
    off, and tw_flow_iter<15,0> instead of <15,2> where the coarsest level is M-free (TW_MFREE=2, TW_MFREE_MIN_W=64)."""
    h, w, n = 720, 1280, 2
    pairs = _pairs(n, h, w)
    for env in (dict(), dict(TW_MFREE="2", TW_MFREE_MIN_W="64")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with twflow.Engine(0, twflow.default_params(), slots=n) as e:
            lv = e.num_levels(w, h)
            mfree = e.level_runs_flow_iter(w, h, lv, n)
            assert mfree == bool(env)
            a = _planar_out(e, n, h, w)
            e.launch_counts(reset=True)
            for t in [e.submit(*pairs[i], 0, 5.0, flow=a[i]) for i in range(n)]:
                e.wait(t)
            c0 = e.launch_counts(reset=True)
            b = _planar_out(e, n, h, w)
            z = np.zeros((h, w, 2), F32)
            for t in [e.submit(*pairs[i], 0, 5.0, flow=b[i], init=z) for i in range(n)]:
                e.wait(t)
            c1 = e.launch_counts()
            assert np.array_equal(a, b)
            assert c1["tw_flow_area_init"] == 1 and c0["tw_flow_area_init"] == 0
            if mfree:
                assert c1["tw_flow_iter_zero"] == c0["tw_flow_iter_zero"] - 1
                assert c1["tw_flow_iter"] == c0["tw_flow_iter"] + 1


def test_refusals(twflow):
    """Refused with TW_E_BAD_PARAMETER before anything is queued: null data, pitch below the row / not a multiple of 4,
    unknown layout, memory of another device, a device field that overruns its allocation."""
    h, w = 64, 96
    a, b = _pairs(1, h, w)[0]
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        d = e.upload(np.zeros(h * w * 8, np.uint8)).value
        bad = [(0, w * 8, twflow.FLOW_INTERLEAVED), (d, w * 8 - 4, twflow.FLOW_INTERLEAVED),
               (d, w * 8 + 2, twflow.FLOW_INTERLEAVED), (d, w * 4, 7), (d, w * 8 + 4, twflow.FLOW_INTERLEAVED),
               (d + 8, w * 8, twflow.FLOW_INTERLEAVED)]
        if twflow.device_count() > 1:
            with twflow.Engine(1, twflow.default_params(), slots=1) as e1:
                bad.append((e1.upload(np.zeros(h * w * 8, np.uint8)).value, w * 8, twflow.FLOW_INTERLEAVED))
                for fi in bad[-1:]:
                    with pytest.raises(twflow.TwError) as ei:
                        e.submit(a, b, 0, 5.0, init=fi)
                    assert ei.value.code == twflow.TW_E_BAD_PARAMETER
                bad.pop()
        e.launch_counts(reset=True)
        for fi in bad:
            with pytest.raises(twflow.TwError) as ei:
                e.submit(a, b, 0, 5.0, init=fi)
            assert ei.value.code == twflow.TW_E_BAD_PARAMETER, fi
        e.flush()
        assert sum(e.launch_counts().values()) == 0  # nothing was queued
        # non-finite values are passed through, not refused
        f = np.full((h, w, 2), np.inf, F32)
        e.wait(e.submit(a, b, 0, 5.0, init=f))


def test_batches_without_init_launch_what_they_did(twflow):
    """The same init-free batch launches the same families and counts before any field was seen and after."""
    h, w, n = 480, 640, 8
    pairs = _pairs(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        def run(init_pair=None):
            e.launch_counts(reset=True)
            tk = [e.submit(*pairs[i], 10, 5.0, init=None if i != init_pair else _field(i, h, w)[1]) for i in range(n)]
            res = [e.wait(t) for t in tk]
            return e.launch_counts(reset=True), res
        c0, r0 = run()
        c1, _ = run(init_pair=3)
        c2, r2 = run()
        assert c1["tw_flow_area_init"] == 1 and c0["tw_flow_area_init"] == 0
        assert c0 == c2
        assert [r["vector"] for r in r0] == [r["vector"] for r in r2]


def test_memory_staging_once(twflow):
    """tw_debug_memory grows by the host-field staging region (slots fields) and the source tables once; a second batch
    with host fields adds nothing."""
    h, w, n = 240, 320, 4
    pairs = _pairs(n, h, w)
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        for t in [e.submit(*pairs[i], 10, 5.0) for i in range(n)]:
            e.wait(t)
        m0 = e.memory()
        f = _field(0, h, w)[1]
        for t in [e.submit(*pairs[i], 10, 5.0, init=f) for i in range(n)]:
            e.wait(t)
        m1 = e.memory()
        slot = (w * h * 8 + 255) // 256 * 256
        table = 24 * n + 256  # (FlowDst: pointer, pitch, layout, pad)
        assert m1["device_bytes"] - m0["device_bytes"] == n * slot + 256 + table
        for t in [e.submit(*pairs[i], 10, 5.0, init=f) for i in range(n)]:
            e.wait(t)
        assert e.memory()["device_bytes"] == m1["device_bytes"]
