#!/usr/bin/env python3
"""The figures of profiles/overlay.md: what a diff image (tw_ticket_overlay) costs.  Needs a GPU.

    overlay_prof.py [typical|worst|all] [CALLS]      (default all, 50 calls; prints one JSON line)

1080p, span 10, threshold 5, the bench's synthetic pairs (synth.make_pair).
  typical   one batch of the bench's 4 distinct pairs; tw_ticket_overlay on the pair with the most hits, CALLS times each to a
            device destination, to a page-locked host block and to pageable memory: wall time per call.
  worst     tw_stage_overlay with every grid point a hit of maximal length (dx = dy = 1024): the same kernels, launched CALLS / 10
            times (the call's wall time includes its uploads and is not reported).
  copy      the project's copy yardstick (tw_debug_copy_rate) at the base kernel's byte count, 5 B per pixel.
  png       the host time of the PNG writer (host/tw_png_write.h) on a 1080p picture: a stand-alone program built here.
The kernels' own times are device timestamps from a kernel trace of a run of ONE phase (typical or worst), so that every
tw_overlay_* launch of the run belongs to it; the library brackets none of these launches with events of its own (they are
outside a batch's timed region).  The trace is taken around this script and read back by it:

    rocprofv3 --kernel-trace --stats -d prof_typical -o typical -- python tools/overlay_prof.py typical 50
    python tools/overlay_prof.py stats prof_typical/typical_results.db        (one JSON line: a row per kernel and grid)
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))
import synth  # noqa: E402
import twflow  # noqa: E402

W, H, SPAN, THR, TOL = 1920, 1080, 10, 5.0, 16
PNG_MAIN = r"""
#include <chrono>
#include <stdio.h>
#include <vector>
#include "tw_png_write.h"
int main(int argc, char** argv)
{
    const int w = 1920, h = 1080, reps = 10;
    std::vector<uint8_t> px((size_t)w * h * 3);
    for (size_t i = 0; i < px.size(); i++) px[i] = (uint8_t)(i * 2654435761u >> 24);
    std::vector<uint8_t> out;
    double enc = 0, file = 0;
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        twhost::png_encode_rgb8(px.data(), w, h, 3 * w, out);
        auto t1 = std::chrono::steady_clock::now();
        twhost::png_write_rgb8(argv[1], px.data(), w, h, 3 * w);
        auto t2 = std::chrono::steady_clock::now();
        enc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        file += std::chrono::duration<double, std::milli>(t2 - t1).count();
    }
    printf("%.3f %.3f %zu\n", enc / reps, file / reps, out.size());
    return 0;
}
"""


def wall_ms(fn, calls):
    fn()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def typical(e, calls):
    pairs = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, H, W)) for i in range(4)]
    tks = [e.submit(a, b, SPAN, THR) for a, b in pairs]
    hits = [e.hits(t) for t in tks]
    tk = tks[int(np.argmax(hits))]
    n = 3 * W * H
    d = e.upload(np.zeros(n, np.uint8))
    pinned = e.host_array((n,))
    pageable = np.empty(n, np.uint8)
    res = {"hits_per_pair": hits, "hits_of_the_rendered_pair": max(hits),
           "device_ms": wall_ms(lambda: e.overlay(tk, TOL, out=d), calls),
           "page_locked_ms": wall_ms(lambda: e.overlay(tk, TOL, out=pinned), calls),
           "pageable_ms": wall_ms(lambda: e.overlay(tk, TOL, out=pageable), calls)}
    for t in tks:
        e.wait(t)
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def worst(e, calls):
    a, b = (np.ascontiguousarray(x) for x in synth.make_pair(0, H, W))
    hits = [(x, y, 1024.0, 1024.0) for y in range(0, H, SPAN) for x in range(0, W, SPAN)]
    for _ in range(max(1, calls // 10)):
        e.stage_overlay(a, b, [], hits, [], TOL)
    return {"hits": len(hits), "launches": max(1, calls // 10)}


def png_writer():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(PNG_MAIN)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tidal-wave_amd", "host"), "-o", exe, src])
        enc, file, size = subprocess.check_output([exe, os.path.join(d, "o.png")], text=True).split()
    return {"encode_ms": float(enc), "encode_and_write_ms": float(file), "file_bytes": int(size)}


def trace_stats(db_path):
    """the tw_overlay_* launches of a kernel trace's result database (table `kernels`: name, duration in ns, grid in threads),
    grouped by kernel and grid: launches, min / median / mean / max in microseconds — the rows of profiles/overlay.md section 1"""
    import sqlite3
    import statistics
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, duration, grid_x, grid_y, workgroup_x, vgpr_count from kernels where name like '%tw_overlay%' "
                      "order by start").fetchall()
    by = {}
    for name, dur, gx, gy, wx, vgpr in rows:
        by.setdefault((name.split("(")[0].replace("void twk::", ""), gx // max(wx, 1), gy, wx, vgpr), []).append(dur / 1e3)
    return [{"kernel": k[0], "workgroups": [k[1], k[2]], "threads": k[3], "vgprs": k[4], "launches": len(v), "min_us": round(min(v), 2),
             "median_us": round(statistics.median(v), 2), "mean_us": round(sum(v) / len(v), 2), "max_us": round(max(v), 2)}
            for k, v in by.items()]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "stats":
        print(json.dumps(trace_stats(sys.argv[2])))
        return
    phase = sys.argv[1] if len(sys.argv) > 1 else "all"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    res = {"phase": phase, "calls": calls, "size": [W, H]}
    with twflow.Engine(0, twflow.default_params(), slots=4) as e:
        if phase in ("typical", "all"):
            res["typical"] = typical(e, calls)
        if phase in ("worst", "all"):
            res["worst"] = worst(e, calls)
        if phase == "all":
            # the yardstick counts what it reads and what it writes: a copy of 2.5 B per pixel moves the base kernel's 5
            nbytes = 5 * W * H // 2 // 16 * 16
            gbps = e.copy_rate_gbps(nbytes=nbytes, reps=50)
            res["copy"] = {"bytes_moved": 2 * nbytes, "gbps": round(gbps, 1), "us_for_5_bytes_per_pixel": round(2 * nbytes / gbps * 1e-3, 2)}
    if phase == "all":
        res["png"] = png_writer()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
