"""Cost of initial flow fields in batched submissions (tw_submit_dev_flow_init / tw_submit_u8_flow_init).

Workload: 1080p pairs, 128-pair batches, two batches in flight (submit batch k, then collect batch k-1), modes alternated
in the same process after a warm-up:
  none        tw_submit_dev, HBM-resident images, no field (bench.py's path)
  dev_init    the same with a device field per pair (interleaved, read in place by tw_flow_area_init)
  host_none   tw_submit_u8 of page-locked host images, no field
  host_init   the same with a page-locked host field per pair (uploaded to the context's HBM staging on the copy stream)
Prints one JSON line (pairs/s per mode: median over rounds, plus every round) and writes it to --out.

  python tools/flow_init_bench.py [--batches 8] [--rounds 3] [--modes none,dev_init,host_none,host_init] [--out FILE]
  python tools/flow_init_bench.py --stats KERNEL_STATS_CSV [--pairs 128]   # rocprofv3 --kernel-trace --stats output:
      tw_flow_area_init us per launch and its read rate (8 B/px of the full-resolution field) against tw_copy_f4
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

    ini_ns, ini_calls = avg_ns("tw_flow_area_init")
    cp_ns, cp_calls = avg_ns("tw_copy_f4")
    out = {"tw_flow_area_init_calls": ini_calls, "tw_copy_f4_calls": cp_calls}
    if ini_ns:
        rb = 8.0 * W * H * pairs  # the full-resolution fields read (the 0.26 MB per pair written is left out)
        out.update(tw_flow_area_init_us=ini_ns / 1e3, tw_flow_area_init_read_bytes=rb, tw_flow_area_init_GBps=rb / ini_ns)
    if cp_ns:
        cb = 2.0 * (1 << 30)  # Engine.copy_rate_gbps default: 1 GiB read + 1 GiB written per launch
        out.update(tw_copy_f4_us=cp_ns / 1e3, tw_copy_f4_GBps=cb / cp_ns)
    if ini_ns and cp_ns:
        out["frac_of_copy"] = out["tw_flow_area_init_GBps"] / out["tw_copy_f4_GBps"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="timed batches per mode and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--modes", default="none,dev_init,host_none,host_init")
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
        imgs = [synth.make_pair(i, H, W) for i in range(8)]
        dev = [(e.upload(x), e.upload(y)) for x, y in imgs]
        host = []
        for x, y in imgs:
            hx, hy = e.host_array((H, W)), e.host_array((H, W))
            hx[...], hy[...] = x, y
            host.append((hx, hy))
        rng = np.random.default_rng(0)
        fields = [(rng.standard_normal((H, W, 2)) * 3).astype(np.float32) for _ in range(4)]
        d = torch.device("cuda", 0)
        dfields = [torch.from_numpy(f).to(d) for f in fields]
        hfields = []
        for f in fields:
            p = e.host_array((H, W, 2), np.float32)
            p[...] = f
            hfields.append(p)
        torch.cuda.synchronize()

        def run(mode, batches):
            pend = []
            t0 = time.perf_counter()
            for b in range(batches + 1):
                tk = []
                for i in range(n if b < batches else 0):
                    k = (b * n + i) % len(imgs)
                    if mode in ("none", "dev_init"):
                        ini = dfields[k % 4] if mode == "dev_init" else None
                        tk.append(e.submit_dev(dev[k][0], dev[k][1], W, H, W, 10, 5.0, init=ini))
                    else:
                        ini = hfields[k % 4] if mode == "host_init" else None
                        tk.append(e.submit(host[k][0], host[k][1], 10, 5.0, init=ini))
                for t in pend:
                    e.wait_count(t)
                pend = tk
            return batches * n / (time.perf_counter() - t0)

        for m in modes:  # warm-up: plans, workspace, staging
            run(m, 2)
        per = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                per[m].append(run(m, a.batches))
        copy_gbps = e.copy_rate_gbps()
    res = {"workload": "%dx%d, %d-pair batches, span 10" % (W, H, n), "batches": a.batches, "rounds": a.rounds,
           "pairs_per_s": {m: statistics.median(v) for m, v in per.items()}, "rounds_pairs_per_s": per,
           "copy_yardstick_GBps": copy_gbps}
    ps = res["pairs_per_s"]
    if "none" in ps and "dev_init" in ps:
        res["dev_init_ratio"] = ps["dev_init"] / ps["none"]
    if "host_none" in ps and "host_init" in ps:
        res["host_init_ratio"] = ps["host_init"] / ps["host_none"]
    if "host_init" in ps:
        res["host_init_h2d_GBps"] = ps["host_init"] * (W * H * 8 + 2 * W * H) / 1e9  # field + both images
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
