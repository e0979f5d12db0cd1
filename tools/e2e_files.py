#!/usr/bin/env python3
"""End-to-end service throughput from FILES (decode included): writes N synthetic 1080p pairs as PNG (or JPEG), runs them
through host/index.js create() (addon -> decode pool -> libtwflow.so) and prints pairs/s.  Needs a GPU + node.

    e2e_files.py [N [DECODE_THREADS]] [--corpus gray|rgba|palette|mixed|jpeg] [--host DIR] [--json]
                 [--copies] [--passes K] [--resident MB] [--ignore N]
    e2e_files.py --kernel-time

  --corpus   the kind of file: 8-bit gray (the default, what this tool has always written), RGBA, palette-8 with the
             identity gray palette, mixed = one pair in 32 palette-8 and the rest RGBA, or jpeg = baseline quality-90
             4:2:0 JPEGs of the same images as r = g = b colour files (what a screenshot tool writes)
  --host     the host/ directory whose index.js and addon run (default: this tree's): A/B against another build
  --json     one JSON line instead of the text
  --copies   the expected files beyond the four distinct ones are COPIES, each a file of its own, not hard links (the
             targets stay hard links): what a cache keyed by a file's identity needs to see N baselines instead of four
  --passes   K passes over the same pairs through ONE long-lived TidalWave instance (calc() per pair, dispose() after the
             last pass) instead of one create() run; pairs/s per pass, and with TW_DEBUG_BATCHTIME=1 in the environment the
             mean of the batches' "decode", "prepare + arena" and "submit + flush" columns per pass
  --resident MB   the instance's residentMB option (resident expected images; implies --passes 2 unless given): pass 1 is
             all misses, pass 2 all hits when the budget holds the corpus (1080p: 2 MB per expected file)
  --ignore N  every pair gets N ignore rectangles of 300 x 200 pixels (index.js's `ignore` option, calcIgnoring per pair with
             --passes): the cost of the masked path from files; 0 (the default) makes the calls this tool has always made
  --kernel-time   no files: tw_png_unfilter per 1080p image for RGBA, palette-8 and 1-bit gray rows, event-timed
             (tw_debug_png_kernel_time, 20 launches between two events, the median of 7 such figures)
The environment goes through unchanged (TW_DEVICE_PNG_KINDS=0 keeps palette files on the host, TW_DEVICE_JPEG=0 / 1 a
JPEG's inverse DCT on the host / on the device; TW_DEBUG_BATCHTIME=1 prints where each batch's host time goes)."""
import argparse
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
import synth  # noqa: E402


def save(img, path, kind):
    import numpy as np
    from PIL import Image
    if kind == "palette":
        im = Image.fromarray(img, mode="P")
        im.putpalette([v for i in range(256) for v in (i, i, i)])
    elif kind == "rgba":
        im = Image.fromarray(np.dstack([img, img, img, np.full_like(img, 255)]))
    elif kind == "jpeg":
        Image.fromarray(np.dstack([img, img, img])).save(path, "JPEG", quality=90, subsampling=2, progressive=False)
        return
    else:
        im = Image.fromarray(img)
    im.save(path, compress_level=3)


def kernel_time():
    import numpy as np
    import twflow
    w, h = 1920, 1080
    rng = np.random.default_rng(1)
    rows = lambda nb: np.concatenate([(np.arange(h) % 5).astype(np.uint8)[:, None],
                                      rng.integers(0, 256, (h, nb), dtype=np.uint8)], 1)  # filter types 0-4 in turn
    ident = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    kinds = (("rgba", twflow.PngRows(rows(w * 4), w, h, 6, 8)), ("palette8", twflow.PngRows(rows(w), w, h, 3, 8, ident)),
             ("gray1", twflow.PngRows(rows(w // 8), w, h, 0, 1)))
    out = {}
    with twflow.Engine(0, twflow.default_params(), slots=2) as e:
        for rep in range(7):  # the kinds in turn, so that a drift of the clock touches all of them alike
            for name, img in kinds:
                out.setdefault(name, []).append(e.png_kernel_time(img, 20))
    print(json.dumps({"tw_png_unfilter_us_per_1080p_image": {k: {"median": round(statistics.median(v), 1),
                                                                 "min": round(min(v), 1), "max": round(max(v), 1)}
                                                             for k, v in out.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=32)
    ap.add_argument("threads", nargs="?", default="")
    ap.add_argument("--corpus", default="gray", choices=("gray", "rgba", "palette", "mixed", "jpeg"))
    ap.add_argument("--host", default=os.path.join(ROOT, "tidal-wave_amd", "host"))
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--kernel-time", action="store_true")
    ap.add_argument("--copies", action="store_true")
    ap.add_argument("--passes", type=int, default=0)
    ap.add_argument("--resident", type=int, default=0)
    ap.add_argument("--ignore", type=int, default=0)
    a = ap.parse_args()
    passes = a.passes or (2 if a.resident else 0)  # 0: the one create() run this tool has always made
    if a.kernel_time:
        return kernel_time()
    n, threads = a.n, a.threads
    d = tempfile.mkdtemp(prefix="twe2e_")
    try:
        os.makedirs(os.path.join(d, "expected", "s"))
        os.makedirs(os.path.join(d, "target", "s"))
        made = {}  # (pair % 4, kind) -> its two files
        for i in range(n):
            kind = {"gray": "gray", "rgba": "rgba", "palette": "palette", "jpeg": "jpeg"}.get(a.corpus) or ("palette" if i % 32 == 5 else "rgba")
            ext = "jpg" if kind == "jpeg" else "png"
            pe, pt = os.path.join(d, "expected", "s", "p%04d.%s" % (i, ext)), os.path.join(d, "target", "s", "p%04d.%s" % (i, ext))
            if (i % 4, kind) not in made:
                img_a, img_b = synth.make_pair(i % 4, 1080, 1920)
                save(img_a, pe, kind)
                save(img_b, pt, kind)
                made[(i % 4, kind)] = (pe, pt)
            else:  # the four distinct pairs again (hard links: the decoder reads and inflates every file all the same)
                if a.copies:
                    shutil.copyfile(made[(i % 4, kind)][0], pe)
                else:
                    os.link(made[(i % 4, kind)][0], pe)
                os.link(made[(i % 4, kind)][1], pt)
        js = ("var T=require('./index'); var t0=Date.now(); var n=0, err=0;"
              "var opts={expectDir:process.argv[2], numThreads:8}; var ig=JSON.parse(process.argv[5]); if(ig.length) opts.ignore=ig;"
              "var t=T.create(process.argv[1],opts);"
              "t.on('data',function(){n++}); t.on('error',function(e){err++; console.error(JSON.stringify(e))});"
              "var rss0=process.memoryUsage().rss, rssMid=0; setTimeout(function(){rssMid=process.memoryUsage().rss}, 3000);"
              "t.on('finish',function(r){console.log(JSON.stringify({report:r, ms:Date.now()-t0, errors:err, rss_start_MB:rss0>>20, "
              "rss_at_3s_MB:rssMid>>20, rss_end_MB:process.memoryUsage().rss>>20}))});")
        if passes:
            js = ("var T=require('./index'), FS=require('fs'), Path=require('path');"
                  "var tdir=Path.join(process.argv[1],'s'), edir=Path.join(process.argv[2],'s'), passes=+process.argv[3], mb=+process.argv[4];"
                  "var names=FS.readdirSync(tdir).sort(); var opts={numThreads:8}; if(mb>0) opts.residentMB=mb;"
                  "var ig=JSON.parse(process.argv[5]);"
                  "var t=new T.TidalWave(opts); var ms=[], pass=0, left=0, t0=0, err=0;"
                  "function start(){pass++; console.error('TWE2E PASS '+pass); left=names.length; t0=Date.now();"
                  " names.forEach(function(n){if(ig.length) t.calcIgnoring(Path.join(edir,n), Path.join(tdir,n), ig);"
                  " else t.calc(Path.join(edir,n), Path.join(tdir,n))})}"
                  "function one(){if(--left===0){ms.push(Date.now()-t0); if(pass<passes) setTimeout(start,50); else t.dispose()}}"
                  "t.on('data',one); t.on('error',function(e){err++; console.error(JSON.stringify(e)); one()});"
                  "t.on('finish',function(r){console.log(JSON.stringify({report:r, ms:ms.reduce(function(x,y){return x+y},0), pass_ms:ms, errors:err}))});"
                  "start();")
        # N rectangles of 300 x 200 spread over the 1080p image (they may overlap from the seventh on)
        ignore = [{"x": 100 + 450 * (k % 4), "y": 80 + 330 * (k // 4 % 3), "width": 300, "height": 200} for k in range(a.ignore)]
        env = dict(os.environ)
        if threads:
            env["TW_DECODE_THREADS"] = threads
        t0 = time.time()
        r = subprocess.run(["node", "-e", js, os.path.join(d, "target"), os.path.join(d, "expected"), str(passes), str(a.resident),
                            json.dumps(ignore)],
                           cwd=a.host, capture_output=True, text=True, env=env)
        wall = time.time() - t0
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if r.returncode != 0 or not r.stdout.strip():
        sys.exit("node failed (%d): %s" % (r.returncode, r.stderr.strip()[-3000:]))
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if passes:
        # per pass: pairs/s and, from TW_DEBUG_BATCHTIME's lines, the mean "decode" milliseconds of a batch
        decode, prep, submit, cur = {}, {}, {}, 0
        for line in r.stderr.splitlines():
            if line.startswith("TWE2E PASS "):
                cur = int(line.split()[-1])
            elif ": decode " in line and cur:
                decode.setdefault(cur, []).append(float(line.split(": decode ")[1].split(" ms")[0]))
                prep.setdefault(cur, []).append(float(line.split("prepare + arena ")[1].split(",")[0]))
                submit.setdefault(cur, []).append(float(line.split("submit + flush ")[1].split(",")[0]))
        res = {"corpus": a.corpus, "pairs": n, "copies": a.copies, "resident_mb": a.resident, "host": os.path.relpath(a.host, ROOT),
               "pairs_per_s": [round(n / (ms / 1e3), 1) for ms in out["pass_ms"]], "pass_ms": out["pass_ms"],
               "decode_ms_per_batch": [round(statistics.mean(decode[k]), 2) if k in decode else None for k in range(1, passes + 1)],
               "prepare_arena_ms_per_batch": [round(statistics.mean(prep[k]), 2) if k in prep else None for k in range(1, passes + 1)],
               "submit_flush_ms_per_batch": [round(statistics.mean(submit[k]), 2) if k in submit else None for k in range(1, passes + 1)],
               "batches": [len(decode.get(k, [])) for k in range(1, passes + 1)], "report": out["report"], "errors": out["errors"],
               "ignore": a.ignore}
        print(json.dumps(res) if a.json else "\n".join("%s: %s" % kv for kv in res.items()))
        return
    rate = n / (out["ms"] / 1e3)
    if a.json:
        print(json.dumps({"corpus": a.corpus, "pairs": n, "decode_threads": threads or "auto", "host": os.path.relpath(a.host, ROOT),
                          "png_kinds": os.environ.get("TW_DEVICE_PNG_KINDS", "1"),
                          "device_jpeg": os.environ.get("TW_DEVICE_JPEG", "default"), "pairs_per_s": round(rate, 1), "ms": out["ms"],
                          "report": out["report"], "errors": out["errors"], "ignore": a.ignore}))
        return
    print(r.stdout.strip(), r.stderr.strip()[-3000:])
    print("pairs %d  decode_threads %s  corpus %s  service %.1f pairs/s (node wall %.2fs)" %
          (n, threads or "auto", a.corpus, rate, wall))


if __name__ == "__main__":
    main()
