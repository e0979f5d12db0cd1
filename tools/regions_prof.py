#!/usr/bin/env python3
"""The figures of profiles/regions.md: what tw_hit_regions (TW_OPT_REGIONS) costs.  Needs a GPU.

    regions_prof.py [BATCHES]      (default 6; prints one JSON line)

  mix         batches of 256 pairs of 1080p at span 10, threshold 5, bench.py's synthetic pairs (synth.make_pair(i), 4 distinct),
              with the option off and on (gap 1) on one engine: the engine's own events around the scan launches
              (tw_prof_select(TW_K_SCAN): tw_span_gather + tw_span_scan, and with the option on tw_hit_regions behind them) —
              the difference per batch is tw_hit_regions; and the wall-clock pairs/s of the same batches, off against on.
  worst_case  tw_hit_regions alone (tw_stage_hit_regions, the event pair around that one launch) on the 192 x 108 grid of a
              1080p pair at span 10 whose hits are a boustrophedon path — one component about 10 000 points long — and on
              a grid where every point is a hit: 256 pairs per launch, the batch's shape (a workgroup with 136 KB of LDS per
              pair, one per CU), and 16 pairs per launch beside it.  (The 256 fields are 4.2 GB of host memory.)
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

W, H, SPAN, THR, PAIRS = 1920, 1080, 10, 5.0, 256


def run_batches(e, pairs, batches):
    """(pairs/s, scan-class ms per batch, hits, regions launches) of `batches` batches of PAIRS pairs"""
    e.prof_read(twflow.K_SCAN)
    e.launch_counts(reset=True)
    hits = 0
    t0 = time.perf_counter()
    for _ in range(batches):
        tks = [e.submit(*pairs[j % len(pairs)], SPAN, THR) for j in range(PAIRS)]
        hits += sum(e.wait_count(t)[0] for t in tks)
    dt = time.perf_counter() - t0
    ms, _ = e.prof_read(twflow.K_SCAN)
    return batches * PAIRS / dt, ms / batches, hits, e.launch_counts()["tw_hit_regions"]


def boustrophedon(gh, gw):
    m = np.zeros((gh, gw), bool)
    m[::2] = True
    for i, y in enumerate(range(1, gh - 1, 2)):
        m[y, gw - 1 if i % 2 == 0 else 0] = True
    return m


def stage_ms(e, mask, npairs, reps=3):
    f = np.zeros((npairs, 2, H, W), np.float32)
    f[:, 0, ::SPAN, ::SPAN] = np.where(mask, np.float32(9.0), np.float32(0.5))
    e.stage_hit_regions(f, SPAN, THR, 1)  # warm
    e.prof_read(twflow.K_SCAN)
    out = []
    for _ in range(reps):
        nreg, _, _ = e.stage_hit_regions(f, SPAN, THR, 1)
        out.append(e.prof_read(twflow.K_SCAN)[0])
    return {"ms_per_launch": [round(v, 4) for v in out], "pairs_per_launch": npairs, "hits_per_pair": int(mask.sum()),
            "regions_per_pair": int(nreg[0])}


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    pairs = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, H, W)) for i in range(4)]
    res = {"batches": batches, "pairs_per_batch": PAIRS}
    with twflow.Engine(0, twflow.default_params(), slots=PAIRS) as e:
        run_batches(e, pairs, 2)  # warm: plans, buffers, clocks
        rounds = []
        # pairs/s with no profiling class selected (a selected class changes the batch's schedule), then the events
        for prof in (False, True):
            if prof:
                e.prof_select(twflow.K_SCAN, 0)
            for gap in (0, 1, 0, 1):
                e.set_regions(gap)
                run_batches(e, pairs, 1)  # (the option's buffers are made by its first batch)
                pps, ms, hits, launches = run_batches(e, pairs, batches)
                row = {"gap": gap, "hits_per_batch": hits // batches, "tw_hit_regions_launches": launches}
                row.update({"scan_class_ms_per_batch": round(ms, 4)} if prof else {"pairs_per_s": round(pps, 1)})
                rounds.append(row)
        res["mix"] = rounds
        off = [r["scan_class_ms_per_batch"] for r in rounds if not r["gap"] and "scan_class_ms_per_batch" in r]
        on = [r["scan_class_ms_per_batch"] for r in rounds if r["gap"] and "scan_class_ms_per_batch" in r]
        res["tw_hit_regions_ms_per_batch"] = round(sum(on) / len(on) - sum(off) / len(off), 4)
        e.set_regions(0)
        gh, gw = -(-H // SPAN), -(-W // SPAN)
        res["worst_case"] = {"boustrophedon": stage_ms(e, boustrophedon(gh, gw), PAIRS),
                             "every_point": stage_ms(e, np.ones((gh, gw), bool), PAIRS),
                             "boustrophedon_16": stage_ms(e, boustrophedon(gh, gw), 16),
                             "every_point_16": stage_ms(e, np.ones((gh, gw), bool), 16)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
