#!/usr/bin/env python3
"""The workload of profiles/ignore_regions.md's kernel figures: batches of 32 pairs of 1080p RGBA rows (tw_submit_png_ignore),
four 300 x 200 ignore rectangles per pair, to be run under `rocprofv3 --kernel-trace --stats` (kernel trace only): one
tw_mask_rects launch per batch beside the batch's tw_png_unfilter launch.  Needs a GPU.

    ignore_regions_prof.py [BATCHES]      (default 4; prints what it launched as one JSON line)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tidal-wave_amd"))
import synth  # noqa: E402
import twflow  # noqa: E402

W, H, PAIRS = 1920, 1080, 32
RECTS = [(100, 80, 300, 200), (551, 413, 300, 200), (1002, 80, 300, 200), (1453, 743, 300, 200)]  # (odd offsets among them)


def rgba_rows(g):
    """an RGBA image with r = g = b = the gray image, as filter type 0 rows"""
    rgba = np.dstack([g, g, g, np.full_like(g, 255)]).reshape(H, W * 4)
    return np.concatenate([np.zeros((H, 1), np.uint8), rgba], 1)


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    imgs = []
    for i in range(4):
        a, b = synth.make_pair(i, H, W)
        imgs.append((twflow.PngRows(rgba_rows(a), W, H, 6, 8), twflow.PngRows(rgba_rows(b), W, H, 6, 8)))
    with twflow.Engine(0, twflow.default_params(), slots=PAIRS) as e:
        hits = 0
        for _ in range(batches):
            tks = [e.submit_png(*imgs[j % 4], 10, 5.0, ignore=RECTS) for j in range(PAIRS)]
            hits += sum(e.wait_count(t)[0] for t in tks)
        cnt = e.launch_counts()
    print(json.dumps({"batches": batches, "pairs_per_batch": PAIRS, "rects_per_pair": len(RECTS), "hits": hits,
                      "tw_mask_rects": cnt["tw_mask_rects"], "last_z": cnt.last_z["tw_mask_rects"],
                      "tw_png_unfilter": cnt["tw_png_unfilter"]}))


if __name__ == "__main__":
    main()
