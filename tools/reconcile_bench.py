"""Cost of the size reconcile on the device (tw_submit_u8_sized -> tw_resize_u8) in batched submissions.

Workload: 1080p pairs from page-locked host memory, 128-pair batches, two batches in flight (submit batch k, then collect
batch k-1), modes alternated in the same process after a warm-up:
  none   every target 1920 x 1080 (the plain tw_submit_u8: no resize launch)
  one8   every eighth target 1923 x 1077, resized to the pair's size on the device
  all    every target 1923 x 1077
Prints one JSON line (pairs/s per mode: median over rounds, plus every round) and writes it to --out.

  python tools/reconcile_bench.py [--batches 8] [--rounds 3] [--modes none,one8,all] [--out FILE]
  python tools/reconcile_bench.py --stats KERNEL_STATS_CSV   # rocprofv3 --kernel-trace --stats output (a run of its own):
      tw_resize_u8 us per launch and its rate (source read + destination written) against tw_copy_f4
  python tools/reconcile_bench.py --e2e 1024 [--threads 16]   # tools/e2e_files.py's input (PNG files through
      host/index.js create(), numThreads 8) with every target 3 px narrower: pairs/s with TW_DEVICE_RECONCILE=1 against =0
      at --threads decode threads (needs node); the files are written to a temporary directory and removed afterwards
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))

W, H = 1920, 1080
TW, TH = 1923, 1077


def stats(path):
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}

    def avg_ns(prefix):
        m = [r for n, r in rows.items() if prefix in n]
        if not m:
            return None, 0
        calls = sum(int(r["Calls"]) for r in m)
        return sum(float(r["TotalDurationNs"]) for r in m) / calls, calls

    rs_ns, rs_calls = avg_ns("tw_resize_u8")
    cp_ns, cp_calls = avg_ns("tw_copy_f4")
    out = {"tw_resize_u8_calls": rs_calls, "tw_copy_f4_calls": cp_calls}
    if rs_ns:
        nb = float(TW * TH + W * H)  # one launch per pair at submit time: the source read, the destination written
        out.update(tw_resize_u8_us=rs_ns / 1e3, tw_resize_u8_bytes=nb, tw_resize_u8_GBps=nb / rs_ns)
    if cp_ns:
        cb = 2.0 * (1 << 30)  # Engine.copy_rate_gbps default: 1 GiB read + 1 GiB written per launch
        out.update(tw_copy_f4_us=cp_ns / 1e3, tw_copy_f4_GBps=cb / cp_ns)
    return out


def e2e(pairs, threads):
    from PIL import Image
    import synth
    d = tempfile.mkdtemp(prefix="twrec_")
    try:
        return e2e_in(d, pairs, threads)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def e2e_in(d, pairs, threads):
    from PIL import Image
    import synth
    os.makedirs(os.path.join(d, "expected", "s"))
    os.makedirs(os.path.join(d, "target", "s"))
    for i in range(pairs):
        pe, pt = os.path.join(d, "expected", "s", "p%04d.png" % i), os.path.join(d, "target", "s", "p%04d.png" % i)
        if i < 4:
            x, y = synth.make_pair(i, H, W)
            Image.fromarray(x).save(pe, compress_level=3)
            Image.fromarray(y[:, :W - 3].copy()).save(pt, compress_level=3)
        else:  # the four distinct pairs again (hard links: the decoder reads and inflates every file all the same)
            os.link(os.path.join(d, "expected", "s", "p%04d.png" % (i % 4)), pe)
            os.link(os.path.join(d, "target", "s", "p%04d.png" % (i % 4)), pt)
    js = ("var T=require('./index'); var t0=Date.now(); var n=0;"
          "var t=T.create(process.argv[1],{expectDir:process.argv[2], numThreads:8});"
          "t.on('data',function(){n++}); t.on('error',function(e){console.error(JSON.stringify(e))});"
          "t.on('finish',function(r){console.log(JSON.stringify({report:r, data:n, ms:Date.now()-t0}))});")
    res = {"workload": "%d PNG pairs from files, %dx%d against %dx%d, numThreads 8, %s decode threads" % (pairs, W, H, W - 3, H, threads),
           "pairs_per_s": {}, "runs": {}}
    for sw in ("1", "0", "1", "0"):  # alternated: two runs each
        env = dict(os.environ, TW_DEVICE_RECONCILE=sw, TW_DECODE_THREADS=str(threads))
        r = subprocess.run(["node", "-e", js, os.path.join(d, "target"), os.path.join(d, "expected")],
                           cwd=os.path.join(ROOT, "tidal-wave_amd", "host"), capture_output=True, text=True, env=env)
        if r.returncode != 0:
            raise SystemExit("node failed: " + r.stderr[-2000:])
        out = json.loads(r.stdout.strip().splitlines()[-1])
        if out["data"] != pairs:
            raise SystemExit("TW_DEVICE_RECONCILE=%s: %d of %d pairs answered: %s" % (sw, out["data"], pairs, r.stderr[-500:]))
        res["runs"].setdefault("device_reconcile_" + sw, []).append(pairs / (out["ms"] / 1e3))
    for k, v in res["runs"].items():
        res["pairs_per_s"][k] = max(v)
    res["ratio"] = res["pairs_per_s"]["device_reconcile_1"] / res["pairs_per_s"]["device_reconcile_0"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="timed batches per mode and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--modes", default="none,one8,all")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--e2e", type=int, default=0, help="pairs of the file-path comparison (0: the batch comparison)")
    ap.add_argument("--threads", type=int, default=16, help="decode threads of the file-path comparison")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats)))
        return
    if a.e2e:
        line = json.dumps(e2e(a.e2e, a.threads))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import numpy as np
    import synth
    import twflow

    if twflow.device_count() < 1:
        raise SystemExit("no HIP device")
    modes = a.modes.split(",")
    n = a.slots
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        host = []
        rng = np.random.default_rng(0)
        for i in range(8):
            x, y = synth.make_pair(i, H, W)
            hx, hy, ht = e.host_array((H, W)), e.host_array((H, W)), e.host_array((TH, TW))
            hx[...], hy[...] = x, y
            # (the content of the other-size target does not matter for the cost: the pair's own target, cropped and padded)
            ht[...] = rng.integers(0, 256, (TH, TW), dtype=np.uint8)
            ht[:, :W] = y[:TH]
            host.append((hx, hy, ht))

        def run(mode, batches):
            pend = []
            t0 = time.perf_counter()
            for b in range(batches + 1):
                tk = []
                for i in range(n if b < batches else 0):
                    k = (b * n + i) % len(host)
                    other = mode == "all" or (mode == "one8" and i % 8 == 7)
                    tk.append(e.submit(host[k][0], host[k][2 if other else 1], 10, 5.0, reconcile=True))
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
        counts = e.launch_counts()
        copy_gbps = e.copy_rate_gbps()
    res = {"workload": "%dx%d, %d-pair batches from page-locked memory, span 10, other-size targets %dx%d" % (W, H, n, TW, TH),
           "batches": a.batches, "rounds": a.rounds, "pairs_per_s": {m: statistics.median(v) for m, v in per.items()},
           "rounds_pairs_per_s": per, "tw_resize_u8_launches": counts["tw_resize_u8"], "copy_yardstick_GBps": copy_gbps}
    ps = res["pairs_per_s"]
    for m in ("one8", "all"):
        if "none" in ps and m in ps:
            res[m + "_ratio"] = ps[m] / ps["none"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
