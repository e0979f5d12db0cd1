#!/usr/bin/env python3
"""The figures of profiles/residual.md: what the residual (TW_OPT_RESIDUAL) costs.  Needs a GPU.

    residual_prof.py [BATCHES]      (default 6; prints one JSON line)

Batches of 256 pairs of 1080p at span 10, threshold 5, bench.py's synthetic pairs (synth.make_pair(i), 4 distinct), on one
engine, in three arms: the option off; the option off with TW_GRID_FINAL=0 (the schedule a residual batch takes: the full last
iteration + tw_span_gather); the option on (tolerance 16).
  kernels   the engine's own events around the scan-class launches (tw_prof_select(TW_K_SCAN)): on minus TW_GRID_FINAL=0 is
            tw_warp_residual (one launch per level-0 chunk) + tw_change_scan (one per batch).
  rates     wall-clock pairs/s of the same batches without a profiling class: off against TW_GRID_FINAL=0 is what giving up
            the grid-only last iteration costs, TW_GRID_FINAL=0 against on what the two kernels and the copies cost.
`value` with the option off against the parent commit is bench.py's own figure, run on both trees in one lease.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))
import synth  # noqa: E402
import twflow  # noqa: E402

W, H, SPAN, THR, PAIRS, TOL = 1920, 1080, 10, 5.0, 256, 16
ARMS = (("off", 0, None), ("off_full_last_iteration", 0, "0"), ("on", TOL, None))


def run_batches(e, pairs, batches, tol):
    """(pairs/s, scan-class ms per batch, hits, change records, launch counts) of `batches` batches of PAIRS pairs"""
    e.prof_read(twflow.K_SCAN)
    e.launch_counts(reset=True)
    hits = cells = 0
    t0 = time.perf_counter()
    for _ in range(batches):
        tks = [e.submit(*pairs[j % len(pairs)], SPAN, THR) for j in range(PAIRS)]
        for t in tks:
            if tol:
                cells += e.changes(t, cap=0)[1]
            hits += e.wait_count(t)[0]
    dt = time.perf_counter() - t0
    ms, _ = e.prof_read(twflow.K_SCAN)
    return batches * PAIRS / dt, ms / batches, hits, cells, e.launch_counts()


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    pairs = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, H, W)) for i in range(4)]
    res = {"batches": batches, "pairs_per_batch": PAIRS, "tol": TOL}
    with twflow.Engine(0, twflow.default_params(), slots=PAIRS) as e:
        run_batches(e, pairs, 2, 0)  # warm: plans, buffers, clocks
        rounds = []
        # pairs/s with no profiling class selected (a selected class changes the batch's schedule), then the events
        for prof in (False, True):
            if prof:
                e.prof_select(twflow.K_SCAN, 0)
            for name, tol, grid_final in ARMS * 2:
                if grid_final is None:
                    os.environ.pop("TW_GRID_FINAL", None)
                else:
                    os.environ["TW_GRID_FINAL"] = grid_final
                e.set_residual(tol)
                run_batches(e, pairs, 1, tol)  # (the option's buffers are made by its first batch)
                pps, ms, hits, cells, cnt = run_batches(e, pairs, batches, tol)
                row = {"arm": name, "hits_per_batch": hits // batches, "changes_per_batch": cells // batches,
                       "launches_per_batch": {k: cnt[k] // batches for k in ("tw_warp_residual", "tw_change_scan", "tw_span_gather",
                                                                             "tw_flow_iter_grid")}}
                row.update({"scan_class_ms_per_batch": round(ms, 4)} if prof else {"pairs_per_s": round(pps, 1)})
                rounds.append(row)
        os.environ.pop("TW_GRID_FINAL", None)
        res["rounds"] = rounds

        def mean(arm, key):
            v = [r[key] for r in rounds if r["arm"] == arm and key in r]
            return sum(v) / len(v)
        res["kernels_ms_per_batch"] = round(mean("on", "scan_class_ms_per_batch") -
                                            mean("off_full_last_iteration", "scan_class_ms_per_batch"), 4)
        res["pairs_per_s"] = {a: round(mean(a, "pairs_per_s"), 1) for a, _, _ in ARMS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
