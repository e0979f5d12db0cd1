"""What tw_pair_same costs where nothing is identical: TW_SAME_IMAGE=0 against =1 on all-warped pairs.

Workload: bench.py's step shape — 1080p pairs resident in HBM (tw_submit_dev), 128-pair engine batches, up to three
batches outstanding — over warped pairs only (synth kinds 0 and 1): every flag is 0, nothing is skipped, the difference
between the two settings is the compare launch.  TW_SAME_IMAGE is read when the engine is created, so every run is a
child process of its own; the two settings alternate, `--rounds` runs each.  `--kinds 0,1,2,3` runs the bench's own mix
(one pair in four identical) the same way.  TWFLOW_LIB selects the library as for every tool.

  python tools/same_image_ab.py [--rounds 3] [--batches 16] [--slots 128] [--kinds 0,1] [--out FILE]

Prints one JSON line: pairs/s of every run, the means, on/off - 1, and the spread (max / min - 1) of each setting.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))

W, H = 1920, 1080


def child(a):
    import synth
    import twflow

    if twflow.device_count() < 1:
        raise SystemExit("no HIP device")
    kinds = [int(k) for k in a.kinds.split(",")]
    n = a.slots
    with twflow.Engine(0, twflow.default_params(), slots=n) as e:
        pairs = [synth.make_pair(i, H, W, kind=kinds[i % len(kinds)]) for i in range(max(4, len(kinds)))]
        dev = [(e.upload(x), e.upload(y)) for x, y in pairs]
        cursor = [0]

        def run(batches):
            inflight = []
            t0 = time.perf_counter()
            for _ in range(batches):
                tk = []
                for j in range(n):
                    da, db = dev[(cursor[0] + j) % len(dev)]
                    tk.append(e.submit_dev(da, db, W, H, W, 10, 5.0))
                cursor[0] += n
                inflight.append(tk)
                if len(inflight) > 2:
                    for t in inflight.pop(0):
                        e.wait_count(t)
            for tk in inflight:
                for t in tk:
                    e.wait_count(t)
            return batches * n / (time.perf_counter() - t0)

        run(4)  # warm-up: plans, workspace, clocks
        rate = run(a.batches)
        flags = sum(e.same_flags())
        cnt = e.launch_counts()
    print(json.dumps({"pairs_per_s": rate, "flags_set_last_batch": flags, "tw_pair_same_launches": cnt["tw_pair_same"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16, help="timed 128-pair batches per run")
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--kinds", default="0,1", help="synth pair kinds cycled through (0, 1 warped; 2 painted; 3 identical)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    runs = {"0": [], "1": []}
    detail = {"0": [], "1": []}
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--batches", str(a.batches), "--slots", str(a.slots),
            "--kinds", a.kinds]
    for _ in range(a.rounds):
        for sw in ("0", "1"):
            env = dict(os.environ, TW_SAME_IMAGE=sw)
            out = subprocess.run(argv, env=env, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
            r = json.loads(out.strip().splitlines()[-1])
            runs[sw].append(r["pairs_per_s"])
            detail[sw].append(r)
    mean = {k: sum(v) / len(v) for k, v in runs.items()}
    res = {"workload": "%dx%d from HBM, %d-pair batches, kinds %s, %d timed batches per run" % (W, H, a.slots, a.kinds, a.batches),
           "pairs_per_s": {"TW_SAME_IMAGE=0": runs["0"], "TW_SAME_IMAGE=1": runs["1"]},
           "mean": {"TW_SAME_IMAGE=0": mean["0"], "TW_SAME_IMAGE=1": mean["1"]},
           "on_over_off_minus_1": mean["1"] / mean["0"] - 1,
           "spread": {k: max(v) / min(v) - 1 for k, v in (("TW_SAME_IMAGE=0", runs["0"]), ("TW_SAME_IMAGE=1", runs["1"]))},
           "flags_set_last_batch": {"TW_SAME_IMAGE=1": [r["flags_set_last_batch"] for r in detail["1"]]},
           "tw_pair_same_launches": {"TW_SAME_IMAGE=0": [r["tw_pair_same_launches"] for r in detail["0"]],
                                     "TW_SAME_IMAGE=1": [r["tw_pair_same_launches"] for r in detail["1"]]}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
