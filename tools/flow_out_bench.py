"""Cost of dense flow output from batched submissions (tw_submit_dev_flow / tw_submit_u8 + host destinations).

Workload: 1080p pairs resident in HBM, 128-pair batches, two batches in flight (submit batch k, then collect batch k-1),
modes alternated in the same process after a warm-up:
  none          tw_submit_dev, no destination (bench.py's path)
  dev_planar    device destinations, planar
  dev_inter     device destinations, (dx, dy) interleaved
  host          page-locked host destinations, interleaved (export -> HBM staging -> device-to-host stream)
Prints one JSON line (pairs/s per mode: median over rounds, plus every round) and writes it to --out.

  python tools/flow_out_bench.py [--batches 8] [--rounds 3] [--modes none,dev_planar,dev_inter,host] [--out FILE]
  python tools/flow_out_bench.py --stats KERNEL_STATS_CSV [--pairs 128]   # rocprofv3 --kernel-trace --stats output:
      tw_flow_export us per launch and bytes/us (16 B/px) against tw_copy_f4 (the copy yardstick) of the same trace
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))

W, H = 1920, 1080


def stats(path, pairs):
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}

    def avg_ns(prefix):
        m = [r for n, r in rows.items() if prefix in n]
        if not m:
            return None, 0
        calls = sum(int(r["Calls"]) for r in m)
        return sum(float(r["TotalDurationNs"]) for r in m) / calls, calls

    exp_ns, exp_calls = avg_ns("tw_flow_export")
    cp_ns, cp_calls = avg_ns("tw_copy_f4")
    out = {"tw_flow_export_calls": exp_calls, "tw_copy_f4_calls": cp_calls}
    if exp_ns:
        eb = 16.0 * W * H * pairs
        out.update(tw_flow_export_us=exp_ns / 1e3, tw_flow_export_bytes=eb, tw_flow_export_GBps=eb / exp_ns)
    if cp_ns:
        cb = 2.0 * (1 << 30)  # Engine.copy_rate_gbps default: 1 GiB read + 1 GiB written per launch
        out.update(tw_copy_f4_us=cp_ns / 1e3, tw_copy_f4_GBps=cb / cp_ns)
    if exp_ns and cp_ns:
        out["frac_of_copy"] = out["tw_flow_export_GBps"] / out["tw_copy_f4_GBps"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="timed batches per mode and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--modes", default="none,dev_planar,dev_inter,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--pairs", type=int, default=128)
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats, a.pairs)))
        return
    import numpy as np
    import torch
    import synth
    import twflow

    if twflow.device_count() < 1:
        raise SystemExit("no HIP device")
    modes = a.modes.split(",")
    n = a.slots
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        dev = [(e.upload(x), e.upload(y)) for x, y in (synth.make_pair(i, H, W) for i in range(8))]
        # two destination sets per mode: batch k writes set k % 2 while batch k - 1 (the other set) is collected
        d = torch.device("cuda", 0)
        dsets = {"dev_planar": [torch.empty((n, 2, H, W), dtype=torch.float32, device=d) for _ in range(2)],
                 "dev_inter": [torch.empty((n, H, W, 2), dtype=torch.float32, device=d) for _ in range(2)]}
        if "host" in modes:
            dsets["host"] = [e.host_array((n, H, W, 2), np.float32) for _ in range(2)]
        torch.cuda.synchronize()

        def run(mode, batches):
            pend = []
            t0 = time.perf_counter()
            for b in range(batches + 1):
                if b < batches:
                    outs = dsets.get(mode)
                    tk = []
                    for i in range(n):
                        pa, pb = dev[(b * n + i) % len(dev)]
                        fl = None if outs is None else outs[b % 2][i]
                        tk.append(e.submit_dev(pa, pb, W, H, W, 10, 5.0, flow=fl))
                else:
                    tk = []
                for t in pend:
                    e.wait_count(t)
                pend = tk
            return batches * n / (time.perf_counter() - t0)

        for m in modes:  # warm-up: plans, workspace, staging, the device-to-host stream
            run(m, 2)
        per = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                per[m].append(run(m, a.batches))
        copy_gbps = e.copy_rate_gbps()
    res = {"workload": "%dx%d, %d-pair batches, HBM-resident inputs, span 10" % (W, H, n), "batches": a.batches,
           "rounds": a.rounds, "pairs_per_s": {m: statistics.median(v) for m, v in per.items()}, "rounds_pairs_per_s": per,
           "copy_yardstick_GBps": copy_gbps}
    ps = res["pairs_per_s"]
    if "none" in ps:
        res["ratio_to_none"] = {m: v / ps["none"] for m, v in ps.items()}
    if "host" in ps:
        res["host_d2h_GBps"] = ps["host"] * W * H * 8 / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
