"""Identical pairs in the batch schedule: tw_pair_same's flags, the skipped second expansions, tw_flow_iter's redirect.

A pair whose second image is byte for byte its first gets flag 1 from tw_pair_same; at the levels tw_flow_iter runs the
pair's second pyramid image and polynomial expansion are then not computed, and the kernel reads the first expansion in
their place.  What can go wrong: a reader that still takes the skipped (stale) expansion, a level whose readers do not
honour the flag losing its second expansion, the compare kernel's row heads and tails, the per-part flag ranges.  Every
flow is compared bit for bit with oracle.farneback.  The stale data is made real by running a batch of three warped
pairs through the engine first: the workspace of every slot then holds another image's coefficients.

Shapes: 639 x 64 is the smallest size at which both levels of a plan run tw_flow_iter (tests/test_gpu_flow_iter_ups.py);
640 x 128 adds a third level (160 x 32) that runs the update and window kernels.  Dense rows of 639 bytes put every row
at another offset from a 16-byte boundary: the compare kernel's vector path has a head and a tail in every row.
TW_MFREE=2 lifts the workgroup-count gate a batch of three pairs does not pass.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_stages_f64 import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 64, 639


@pytest.fixture(autouse=True)
def _schedule(monkeypatch):
    monkeypatch.setenv("TW_MFREE", "2")
    monkeypatch.setenv("TW_LATENCY_STREAMS", "0")
    monkeypatch.delenv("TW_SAME_IMAGE", raising=False)
    monkeypatch.delenv("TW_LANES", raising=False)


_cache = {}


def pair(kind, h=H, w=W, index=None):
    """synth pair of one kind (0 / 1 warped, 2 painted rectangle, 3 identical), computed once per session."""
    import synth
    key = (kind, h, w, index)
    if key not in _cache:
        _cache[key] = synth.make_pair(kind if index is None else index, h, w, kind=kind)
    return _cache[key]


def want_of(oracle, a, b):
    key = ("want", a.shape, a.tobytes(), b.tobytes())
    if key not in _cache:
        _cache[key] = np.stack(oracle.farneback(a, b, oracle.default_params()))
    return _cache[key]


def check_flows(oracle, out, pairs, what):
    for i, (a, b) in enumerate(pairs):
        same_bits(out[i], want_of(oracle, a, b), "%s, pair %d" % (what, i))


def batch(e, pairs):
    """One batch through the engine: (flows, flags, launch counts of the batch)."""
    e.launch_counts(reset=True)
    out, _ = e.flow_batch([p[0] for p in pairs], [p[1] for p in pairs], layout="planar")
    return out, e.same_flags(), e.launch_counts(reset=True)


def stale_then_mixed(twflow, oracle, h, w, levels_on_flow_iter):
    """Batch 1 of three warped pairs, then [identical, warped, painted] on the same engine."""
    first = [pair(0, h, w), pair(1, h, w), pair(0, h, w, index=4)]
    second = [pair(3, h, w), pair(1, h, w), pair(2, h, w)]
    assert all(not np.array_equal(a, b) for a, b in first) and np.array_equal(*second[0])
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        assert e.num_levels(w, h) == len(levels_on_flow_iter) - 1
        assert [e.level_runs_flow_iter(w, h, k, 3) for k in range(len(levels_on_flow_iter))] == levels_on_flow_iter
        out1, flags1, cnt1 = batch(e, first)
        check_flows(oracle, out1, first, "%dx%d first batch" % (w, h))
        out2, flags2, cnt2 = batch(e, second)
        check_flows(oracle, out2, second, "%dx%d second batch" % (w, h))
    return flags1, cnt1, flags2, cnt2


def test_stale_second_expansion_is_never_read(twflow, oracle, monkeypatch):
    """Case 1: slot 0's second expansion still holds batch 1's warped image when batch 2's identical pair runs."""
    monkeypatch.setenv("TW_RAMP", "0")
    flags1, cnt1, flags2, cnt2 = stale_then_mixed(twflow, oracle, H, W, [True, True])
    assert flags1 == [0, 0, 0] and flags2 == [1, 0, 0], (flags1, flags2)
    assert cnt2["tw_pair_same"] == 1 and cnt2.last_z["tw_pair_same"] == 3, cnt2
    assert cnt2["tw_update_matrices"] == 0 and cnt2.flow_iter() > 0, cnt2
    monkeypatch.setenv("TW_SAME_IMAGE", "0")
    _, off1, _, off2 = stale_then_mixed(twflow, oracle, H, W, [True, True])
    for on, off in ((cnt1, off1), (cnt2, off2)):
        assert off["tw_pair_same"] == 0
        assert {k: v for k, v in on.items() if k != "tw_pair_same"} == {k: v for k, v in off.items() if k != "tw_pair_same"}
        assert on["tw_pair_same"] == 1


def test_level_on_the_window_kernels_keeps_both_expansions(twflow, oracle, monkeypatch):
    """Case 2: 640 x 128 — levels 0 and 1 on tw_flow_iter, level 2 (160 x 32) on the update and window kernels, which read
    the second expansion itself: it must have been computed, over batch 1's."""
    monkeypatch.setenv("TW_RAMP", "0")
    _, _, flags2, cnt2 = stale_then_mixed(twflow, oracle, 128, 640, [True, True, False])
    assert flags2 == [1, 0, 0], flags2
    assert cnt2["tw_update_matrices"] >= 1 and cnt2.flow_iter() > 0 and cnt2["tw_pair_same"] == 1, cnt2


def one_byte(a, y, x):
    b = a.copy()
    b[y, x] ^= 0x40
    return a, b


def test_compare_kernel_edges_one_byte(twflow, oracle, monkeypatch):
    """Case 3: pairs that differ in exactly one byte — the first pixel, the last pixel, the last byte of a middle row."""
    monkeypatch.setenv("TW_RAMP", "0")
    a = pair(3)[0]
    pairs = [one_byte(a, 0, 0), one_byte(a, H - 1, W - 1), one_byte(a, H // 2 - 1, W - 1)]
    assert all(int((p != q).sum()) == 1 for p, q in pairs)
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        out, flags, cnt = batch(e, pairs)
        assert flags == [0, 0, 0] and cnt["tw_pair_same"] == 1, (flags, cnt)
        check_flows(oracle, out, pairs, "one byte differs")


def test_compare_kernel_strided_device_pairs(twflow, oracle, monkeypatch):
    """Case 3, device-resident images with rows of 656 bytes for 639 pixels: the padding differs and the visible pixels do
    not (flag 1); the last visible byte of a row differs and the padding does not (flag 0); identical pixels in a second
    image that starts one byte off the first's alignment (the byte path; flag 1)."""
    monkeypatch.setenv("TW_RAMP", "0")
    stride = 656
    a = pair(3)[0]
    rng = np.random.default_rng(7)

    def padded(img, fill, lead=0):
        buf = np.full(lead + H * stride, fill, np.uint8)
        rows = buf[lead:].reshape(H, stride)
        rows[:, :W] = img
        return buf, rows

    pa0, _ = padded(a, 0)
    pb0, rows_b0 = padded(a, 0)
    rows_b0[:, W:] = rng.integers(1, 256, (H, stride - W), dtype=np.uint8)
    pa1, _ = padded(a, 0)
    b1 = one_byte(a, H // 2, W - 1)[1]
    pb1, _ = padded(b1, 0)
    pa2, _ = padded(a, 0)
    pb2, _ = padded(a, 0, lead=1)
    pairs = [(a, a), (a, b1), (a, a)]
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        out = e.host_array((3, 2, H, W), np.float32)
        dev = [(e.upload(p), e.upload(q)) for p, q in ((pa0, pb0), (pa1, pb1), (pa2, pb2))]
        e.launch_counts(reset=True)
        tickets = []
        for i, (da, db) in enumerate(dev):
            db = C.c_void_p(db.value + 1) if i == 2 else db
            tickets.append(e.submit_dev(da, db, W, H, stride, 0, 5.0, flow=out[i]))
        for t in tickets:
            e.wait(t)
        flags, cnt = e.same_flags(), e.launch_counts(reset=True)
        assert flags == [1, 0, 1] and cnt["tw_pair_same"] == 1 and cnt.flow_iter() > 0, (flags, cnt)
        check_flows(oracle, out, pairs, "strided device pairs")


def eight(identical_at):
    kinds = (0, 1, 2)
    return [pair(3) if i in identical_at else pair(kinds[i % 3]) for i in range(8)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_parts_of_eight_slots(twflow, oracle, monkeypatch, lanes):
    """Case 4: eight host pairs, the default TW_RAMP; one part, or with TW_LANES=2 one part per lane ([0, 4) and [4, 8)):
    identical pairs at the first and the last slot of each part."""
    if lanes == 2:
        monkeypatch.setenv("TW_LANES", "2")
    monkeypatch.delenv("TW_RAMP", raising=False)
    at = (0, 7) if lanes == 1 else (0, 3, 4, 7)
    pairs = eight(at)
    with twflow.Engine(0, twflow.default_params(), slots=8) as e:
        batch(e, eight(()))  # (every slot's workspace holds a differing pair's data)
        out, flags, cnt = batch(e, pairs)
        assert flags == [1 if i in at else 0 for i in range(8)], flags
        assert cnt["tw_pair_same"] == lanes and cnt.last_z["tw_pair_same"] == 8 // lanes, cnt
        check_flows(oracle, out, pairs, "eight slots, %d lane(s)" % lanes)


def test_parts_of_the_cold_start_ramp(twflow, oracle, monkeypatch):
    """Beyond the case list: the ramp needs 64 slots (pieces [0, 16), [16, 32), [32, 64) of a full first batch on an idle
    engine), so eight slots never take it.  Identical pairs at the first and the last slot of each piece."""
    monkeypatch.delenv("TW_RAMP", raising=False)
    at = (0, 15, 16, 31, 32, 63)
    kinds = (0, 1, 2)
    pairs = [pair(3) if i in at else pair(kinds[i % 3]) for i in range(64)]
    with twflow.Engine(0, twflow.default_params(), slots=64) as e:
        out, flags, cnt = batch(e, pairs)
        # a fresh engine is idle, so its first full batch of host pairs always goes out in the three pieces
        # (tests/test_gpu_parity.py::test_cold_start_ramp asserts the same of the expansion launches)
        assert cnt["tw_pair_same"] == 3 and cnt.last_z["tw_pair_same"] == 32, (cnt, cnt.last_z)
        assert cnt["tw_polyexp"] == 3 * 2 and cnt.last_z["tw_polyexp"] == 2 * 32, (cnt, cnt.last_z)
        assert flags == [1 if i in at else 0 for i in range(64)], flags
        check_flows(oracle, out, pairs, "64 slots")


def test_scan_fused_final_level0_keeps_both_expansions(twflow, oracle, monkeypatch):
    """Beyond the case list: with TW_OPT_SCAN_FUSED_FINAL level 0's last iteration is tw_update_matrices + tw_blur_grid, which
    read the second expansion itself — level 0 gets a null table (both expansions, over batch 1's), level 1 still skips.
    No flow destination (a batch with one never takes the fused last iteration): the hit vectors are compared."""
    monkeypatch.setenv("TW_RAMP", "0")
    first = [pair(0), pair(1), pair(0, index=4)]
    second = [pair(3), pair(1), pair(2)]
    with twflow.Engine(0, twflow.default_params(), slots=3) as e:
        e.set_option(twflow.OPT_SCAN_FUSED_FINAL, 1)
        for pairs, flags in ((first, [0, 0, 0]), (second, [1, 0, 0])):
            e.launch_counts(reset=True)
            tk = [e.submit(a, b, 10, 0.0) for a, b in pairs]
            got = [e.wait(t)["vector"] for t in tk]
            assert e.same_flags() == flags
            cnt = e.launch_counts()
            assert cnt["tw_blur_grid"] == 1 and cnt["tw_update_matrices"] == 1 and cnt.flow_iter() > 0, cnt
            assert cnt["tw_pair_same"] == 1, cnt
            for i, (a, b) in enumerate(pairs):
                w_ = want_of(oracle, a, b)
                assert got[i] == oracle.span_scan(w_[0], w_[1], 10, 0.0), "pair %d" % i


def test_switch_off(twflow, oracle, monkeypatch):
    """Case 5: TW_SAME_IMAGE=0 launches no tw_pair_same, reports every flag 0, and computes case 1's flows."""
    monkeypatch.setenv("TW_RAMP", "0")
    monkeypatch.setenv("TW_SAME_IMAGE", "0")
    flags1, cnt1, flags2, cnt2 = stale_then_mixed(twflow, oracle, H, W, [True, True])
    assert flags1 == [0, 0, 0] and flags2 == [0, 0, 0], (flags1, flags2)
    assert cnt1["tw_pair_same"] == 0 and cnt2["tw_pair_same"] == 0, (cnt1, cnt2)
