#!/usr/bin/env python3
"""HBM traffic per launch of the level-0 kernels from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE).

usage: pmc_traffic.py <dir-FETCH_SIZE> <dir-WRITE_SIZE> <out.json> [out.md]
Units and gfx950 corrections as MI355X_MICROARCH.md §HBM prescribes: both counters are in KiB; FETCH_SIZE counts
128-B requests at 64 B, i.e. reads exactly half of a coalesced stream -> doubled; WRITE_SIZE is exact.
Only the largest grid of each kernel (the level-0 launches of the 1080p bench) goes into the JSON."""
import collections
import csv
import glob
import json
import os
import sys
import time

NAMES = {"tw_blur_solve": "tw_blur_solve", "tw_polyexp": "tw_polyexp", "tw_update_matrices": "tw_update_matrices",
         "tw_pyr_k3<0>": "tw_pyr_level", "tw_span_scan": "tw_span_scan"}


def load(d, cname):
    agg = collections.defaultdict(list)
    for f in glob.glob(d + "/**/*_counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == cname:
                k = (r["Kernel_Name"].replace("void ", "").replace("twk::", ""), int(r["Grid_Size"]))
                agg[k].append(float(r["Counter_Value"]))
    return {k: sum(v) / len(v) for k, v in agg.items()}, {k: len(v) for k, v in agg.items()}


def main():
    fetch, nf = load(sys.argv[1], "FETCH_SIZE")
    write, _ = load(sys.argv[2], "WRITE_SIZE")
    rows = []
    for k in fetch:
        rd = fetch[k] * 1024 * 2
        wr = write.get(k, 0.0) * 1024
        rows.append((k[0], k[1], nf[k], rd, wr))
    rows.sort(key=lambda r: -(r[3] + r[4]) * r[2])
    # threads per PAIR of one level-0 launch at 1920x1080 (to turn a grid size into pairs per launch)
    per_pair = {"tw_blur_solve": 9 * 135 * 256, "tw_polyexp": 2 * 8 * 135 * 256, "tw_update_matrices": 30 * 135 * 256,
                "tw_pyr_level": 2 * 8 * 135 * 256, "tw_span_scan": 1024}
    out = {}
    for prefix, name in NAMES.items():
        cand = [r for r in rows if r[0].startswith(prefix) and r[1] % per_pair[name] == 0]
        if cand:
            big = max(cand, key=lambda r: (r[1], r[2]))  # the largest level-0 launch (a whole engine batch)
            out[name] = {"bytes_per_launch": round(big[3] + big[4]), "pairs_per_launch": big[1] // per_pair[name],
                         "read_bytes": round(big[3]), "write_bytes": round(big[4])}
    # where the figures come from (bench.py reads this file as a static input, so it says when and on what
    # code it was measured).  TW_GIT_COMMIT: the GPU box has no .git; the job script passes the commit it was cut from.
    out["_provenance"] = {"measured_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                          "commit": os.environ.get("TW_GIT_COMMIT", "unknown"),
                          "command": "rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE (separate passes) -- python3 "
                                     "bench.py --steps 1 --warmup 1 --batch 128 --full --no-cpu-baseline --no-prof --no-extras "
                                     "(tools/final_profile.sh)"}
    # round 5: the level's iterations are tw_flow_iter launches (no M in HBM) unless TW_MFREE=0; the plain iteration
    # (<15, 0>: 2 of the 3 launches of a level) is then the dominant kernel and takes the "tw_blur_solve" slot bench.py reads
    # (a 1080p pair is 12 strips x 1, 2, 3 or 4 row segments of 1 024 threads: the launch covers the same batch as the
    # polynomial expansion's level-0 launch, whose pairs the grid arithmetic above has already told)
    fi = [r for r in rows if r[0].startswith("tw_flow_iter<15, 0") and r[1] % (12 * 1024) == 0]
    if fi and out.get("tw_polyexp"):
        big = max(fi, key=lambda r: (r[1], r[2]))
        out["tw_blur_solve"] = {"bytes_per_launch": round(big[3] + big[4]), "pairs_per_launch": out["tw_polyexp"]["pairs_per_launch"],
                                "read_bytes": round(big[3]), "write_bytes": round(big[4]), "kernel": "tw_flow_iter<15, 0>",
                                "grid_threads": big[1]}
    json.dump(out, open(sys.argv[3], "w"), indent=1)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write("# HBM traffic per launch (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)\n\n")
            f.write("FETCH_SIZE x 1024 x 2 (gfx950 half-count correction), WRITE_SIZE x 1024.\n\n")
            f.write("| kernel | grid (threads) | launches | read MB | write MB | total MB |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| `%s` | %d | %d | %.1f | %.1f | %.1f |\n" % (r[0][:70], r[1], r[2], r[3] / 1e6, r[4] / 1e6,
                                                                   (r[3] + r[4]) / 1e6))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
