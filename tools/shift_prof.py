#!/usr/bin/env python3
"""The figures of profiles/shift.md: what the shift estimation (TW_OPT_SHIFT) costs.  Needs a GPU.

    shift_prof.py [BATCHES]      (default 6; prints one JSON line)

Batches of 256 pairs of 1080p at span 10, threshold 5, on one engine: text-like pages moved by (0, 40), (25, 60), (-30, 7) and
one identical pair (tests/shift_ref.py's generator), in three arms: the option off, radius 64, radius 1024.
  kernels   the engine's own events around the scan-class launches (tw_prof_select(TW_K_SCAN)): on minus off is the feature's
            launches of a batch — two memsets, tw_shift_profiles, tw_shift_search, tw_shift_verify<0> and <1> once per part,
            tw_flow_shift_init once per coarsest-level chunk.  Per kernel: run this script under a kernel trace with statistics
            and read the tw_shift_* / tw_flow_shift_init rows (every launch of them comes from the timed batches).
  rates     wall-clock pairs/s of the same batches without a profiling class, through the Python submit loop; "on" also calls
            tw_ticket_shift before every wait.
`value` with the option off against the parent commit is bench.py's own figure, run on both trees in one lease.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shift_ref  # noqa: E402
import twflow  # noqa: E402

W, H, SPAN, THR, PAIRS = 1920, 1080, 10, 5.0, 256
ARMS = (("off", 0), ("r64", 64), ("r1024", 1024))
FAMILIES = ("tw_shift_profiles", "tw_shift_search", "tw_shift_verify", "tw_flow_shift_init")


def run_batches(e, pairs, batches, radius):
    """(pairs/s, scan-class ms per batch, hits, applied pairs, launch counts) of `batches` batches of PAIRS pairs"""
    e.prof_read(twflow.K_SCAN)
    e.launch_counts(reset=True)
    hits = applied = 0
    t0 = time.perf_counter()
    for _ in range(batches):
        tks = [e.submit(*pairs[j % len(pairs)], SPAN, THR) for j in range(PAIRS)]
        for t in tks:
            if radius:
                applied += e.shift(t)[2]
            hits += e.wait_count(t)[0]
    dt = time.perf_counter() - t0
    ms, _ = e.prof_read(twflow.K_SCAN)
    return batches * PAIRS / dt, ms / batches, hits, applied, e.launch_counts()


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    rng = np.random.default_rng(1)
    pairs = [shift_ref.shifted_pair(rng, H, W, sx, sy) for sx, sy in ((0, 40), (25, 60), (-30, 7))]
    pairs.append((pairs[0][0], pairs[0][0].copy()))
    res = {"batches": batches, "pairs_per_batch": PAIRS}
    with twflow.Engine(0, twflow.default_params(), slots=PAIRS) as e:
        run_batches(e, pairs, 2, 0)  # warm: plans, buffers, clocks
        rounds = []
        # pairs/s with no profiling class selected (a selected class changes the batch's schedule), then the events
        for prof in (False, True):
            if prof:
                e.prof_select(twflow.K_SCAN, 0)
            for name, radius in ARMS * 2:
                e.set_shift(radius)
                run_batches(e, pairs, 1, radius)  # (the option's buffers are made by its first batch)
                pps, ms, hits, applied, cnt = run_batches(e, pairs, batches, radius)
                row = {"arm": name, "hits_per_batch": hits // batches, "applied_per_batch": applied // batches,
                       "launches_per_batch": {k: cnt[k] // batches for k in FAMILIES}}
                row.update({"scan_class_ms_per_batch": round(ms, 4)} if prof else {"pairs_per_s": round(pps, 1)})
                rounds.append(row)
        e.set_shift(0)
        res["rounds"] = rounds

        def mean(arm, key):
            v = [r[key] for r in rounds if r["arm"] == arm and key in r]
            return sum(v) / len(v)
        res["kernels_ms_per_batch"] = {a: round(mean(a, "scan_class_ms_per_batch") - mean("off", "scan_class_ms_per_batch"), 4)
                                       for a, r in ARMS if r}
        res["pairs_per_s"] = {a: round(mean(a, "pairs_per_s"), 1) for a, _ in ARMS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
