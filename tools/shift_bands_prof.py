#!/usr/bin/env python3
"""The figures of profiles/shift_bands.md: what the shift bands (TW_OPT_SHIFT_BANDS) cost on top of the shift.  Needs a GPU.

    shift_bands_prof.py [BATCHES]      (default 4; prints one JSON line)

Batches of 256 pairs of 1080p at span 10, threshold 5, on one engine: text-like pages with 40, 70 and 24 foreign rows inserted
at rows 400, 250 and 700 and one identical pair (tests/band_ref.py's generator), in five arms: both options off; the shift alone
at radius 64 and 1024; the shift with bands of 64 rows at radius 64 and 1024.
  kernels   the engine's own events around the scan-class launches (tw_prof_select(TW_K_SCAN)): bands minus shift alone is the
            feature's launches of a batch — one memset, tw_band_rows, tw_band_search, tw_band_verify<0> and <1> once per part,
            and tw_flow_band_init in tw_flow_shift_init's place once per coarsest-level chunk.  Per kernel: run this script
            under a kernel trace with statistics and read the tw_band_* / tw_flow_band_init rows next to tw_shift_profiles'.
  rates     wall-clock pairs/s of the same batches without a profiling class, through the Python submit loop; the band arms
            also call tw_ticket_shift_bands before every wait.
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
import band_ref  # noqa: E402
import twflow  # noqa: E402

W, H, SPAN, THR, PAIRS, BAND = 1920, 1080, 10, 5.0, 256, 64
ARMS = (("off", 0, 0), ("shift_r64", 64, 0), ("bands_r64", 64, BAND), ("shift_r1024", 1024, 0), ("bands_r1024", 1024, BAND))
FAMILIES = ("tw_shift_profiles", "tw_shift_search", "tw_shift_verify", "tw_flow_shift_init",
            "tw_band_rows", "tw_band_search", "tw_band_verify", "tw_flow_band_init")


def run_batches(e, pairs, batches, radius, band):
    """(pairs/s, scan-class ms per batch, hits, applied bands, launch counts) of `batches` batches of PAIRS pairs"""
    e.prof_read(twflow.K_SCAN)
    e.launch_counts(reset=True)
    hits = applied = 0
    t0 = time.perf_counter()
    for _ in range(batches):
        tks = [e.submit(*pairs[j % len(pairs)], SPAN, THR) for j in range(PAIRS)]
        for t in tks:
            if radius and band:
                applied += sum(b[3] for b in e.shift_bands(t))
            elif radius:
                e.shift(t)
            hits += e.wait_count(t)[0]
    dt = time.perf_counter() - t0
    ms, _ = e.prof_read(twflow.K_SCAN)
    return batches * PAIRS / dt, ms / batches, hits, applied, e.launch_counts()


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(1)
    pairs = [band_ref.inserted_pair(rng, H, W, at, ins) for at, ins in ((400, 40), (250, 70), (700, 24))]
    pairs.append((pairs[0][0], pairs[0][0].copy()))
    res = {"batches": batches, "pairs_per_batch": PAIRS, "band": BAND}
    with twflow.Engine(0, twflow.default_params(), slots=PAIRS) as e:
        run_batches(e, pairs, 2, 0, 0)  # warm: plans, buffers, clocks
        rounds = []
        # pairs/s with no profiling class selected (a selected class changes the batch's schedule), then the events
        for prof in (False, True):
            if prof:
                e.prof_select(twflow.K_SCAN, 0)
            for name, radius, band in ARMS * 2:
                e.set_shift(radius)
                e.set_shift_bands(band)
                run_batches(e, pairs, 1, radius, band)  # (the options' buffers are made by their first batch)
                pps, ms, hits, applied, cnt = run_batches(e, pairs, batches, radius, band)
                row = {"arm": name, "hits_per_batch": hits // batches, "applied_bands_per_batch": applied // batches,
                       "launches_per_batch": {k: cnt[k] // batches for k in FAMILIES}}
                row.update({"scan_class_ms_per_batch": round(ms, 4)} if prof else {"pairs_per_s": round(pps, 1)})
                rounds.append(row)
        e.set_shift(0)
        e.set_shift_bands(0)
        res["rounds"] = rounds

        def mean(arm, key):
            v = [r[key] for r in rounds if r["arm"] == arm and key in r]
            return sum(v) / len(v)
        res["scan_class_ms_per_batch"] = {a: round(mean(a, "scan_class_ms_per_batch"), 4) for a, _, _ in ARMS}
        res["bands_minus_shift_ms_per_batch"] = {
            r: round(mean("bands_" + r, "scan_class_ms_per_batch") - mean("shift_" + r, "scan_class_ms_per_batch"), 4)
            for r in ("r64", "r1024")}
        res["pairs_per_s"] = {a: round(mean(a, "pairs_per_s"), 1) for a, _, _ in ARMS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
