#!/usr/bin/env python3
"""What one twhost::Consumer does, call for call, on the stub backend — to compare two versions of host/twhost.cpp.

    python tools/consumer_trace.py [--twhost PATH/TO/twhost.cpp] [--include DIR] [--out DIR]

builds tools/consumer_probe.cpp against the given twhost.cpp (default: the tree's; `git show REV:tidal-wave_amd/host/twhost.cpp`
into a scratch directory gives any other commit's — headers it includes beyond the tree's go into --include; the probe is
built against the tree's twhost.h, so the other commit's must lay out ConsumerShared as the tree's does) and THIS
tree's stub, runs every case below with 1 and with 4 decode threads, and prints one table row per case: the SHA-256 of the
responses in arrival order, the SHA-256 of the stub's call trace (TW_STUB_TRACE) and the trace's line count.  Two versions
behave alike when their tables are equal; within one table the 1-thread and 4-thread columns must be equal too.  A second
table runs EXTRAS_CASES with the per-pair extras on (extras_configs: each alone, all together, every refusal), with the hash of
the diff images where there are some; --extras-json writes it as tests/golden/consumer_extras_parent.json holds it.

The files of the cases are written here (at most 40 x 30 pixels); the JPEGs are the committed fixtures of tests/golden/jpeg.
tests/test_host_consumer_steps.py imports the cases and asserts on their traces.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tidal-wave_amd", "host")
JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_host_png_kinds import write_png  # noqa: E402

W, H = 40, 30
MB = 1 << 20
SWITCHES = ("TW_DEVICE_PNG", "TW_DEVICE_PNG_KINDS", "TW_DEVICE_RECONCILE", "TW_DEVICE_JPEG", "TW_RESIDENT_MB", "TW_SCAN_FUSED_FINAL",
            "TW_FAIR_SLACK", "TW_DEBUG_TAKES", "TW_DEBUG_BATCHTIME", "TW_STUB_BUSY_AT", "TW_STUB_BATCH_MS", "TW_STUB_TRACE", "TW_LOG")


def build(exe, twhost_cpp=None, include=None):
    """the probe against `twhost_cpp` (default: the tree's) and the tree's stub"""
    src = [os.path.join(ROOT, "tools", "consumer_probe.cpp"), os.path.join(HOST, "stub_twflow.cpp"),
           twhost_cpp or os.path.join(HOST, "twhost.cpp"), os.path.join(HOST, "jpeg_gray.cpp"), os.path.join(HOST, "tw_inflate.cpp")]
    inc = ["-I", include] if include else []
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST] + inc + ["-o", exe] + src + ["-lpthread"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_files(d):
    """name -> path of every file the cases use"""
    f = {}

    def rgb(name, first, w=W, h=H, seed=1, ctype=2):
        ch = {0: 1, 2: 3, 6: 4}[ctype]
        s = np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)
        s[0, 0, :] = first
        f[name] = os.path.join(d, name + ".png")
        write_png(f[name], s, ctype, 8)

    def pgm(name, first, w=W, h=H, seed=1):
        g = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
        g[0, 0] = first
        f[name] = os.path.join(d, name + ".pgm")
        with open(f[name], "wb") as o:
            o.write(b"P5\n%d %d\n255\n" % (w, h) + g.tobytes())

    for i in range(10):
        rgb("e%d" % i, 10 + i, seed=100 + i)
        rgb("t%d" % i, 10 + i if i % 3 else 200, seed=200 + i)  # every third pair differs
    pgm("t_pgm", 99, seed=3)
    pgm("e_pgm", 10, seed=4)
    pgm("t_pgm_narrow", 10, w=W - 3, seed=5)
    rgb("t_narrow", 10, w=W - 3, seed=6)
    rgb("t_narrow6", 10, w=W - 6, seed=7)
    rgb("e_small", 10, w=32, h=24, seed=8)
    rgb("t_small", 11, w=32, h=24, seed=9)
    rgb("e_tiny", 10, w=24, h=20, seed=10, ctype=6)
    rgb("t_tiny", 10, w=24, h=20, seed=11, ctype=0)
    # palette and 2-bit gray
    plte = [[10, 10, 10], [20, 40, 60], [30, 30, 30], [200, 100, 0]]
    idx = np.random.default_rng(12).integers(0, 4, (H, W, 1), dtype=np.uint8)
    f["pal"] = os.path.join(d, "pal.png")
    write_png(f["pal"], idx, 3, 8, plte=plte)
    f["gray2"] = os.path.join(d, "gray2.png")
    write_png(f["gray2"], np.random.default_rng(13).integers(0, 4, (H, W, 1), dtype=np.uint8), 0, 2)
    bad_idx = idx.copy()
    bad_idx[5, 7, 0] = 200  # an index beyond the four entries
    f["pal_bad"] = os.path.join(d, "pal_bad.png")
    write_png(f["pal_bad"], bad_idx, 3, 8, plte=plte)
    # damaged PNGs: e0's bytes with the middle of the compressed stream overwritten — as it stands (the chunk's CRC is
    # wrong) and with the CRC made right again (the header parses, the inflate fails: the fast path's own refusal)
    data = bytearray(open(f["e0"], "rb").read())
    at = data.index(b"IDAT")
    n = struct.unpack(">I", data[at - 4:at])[0]
    for k in range(at + 4 + n // 2, at + 4 + n // 2 + 24):
        data[k] ^= 0x5A
    f["bad_crc"] = os.path.join(d, "bad_crc.png")
    with open(f["bad_crc"], "wb") as o:
        o.write(bytes(data))
    data[at + 4 + n:at + 8 + n] = struct.pack(">I", zlib.crc32(bytes(data[at:at + 4 + n])) & 0xFFFFFFFF)
    for name in ("bad_e", "bad_t"):
        f[name] = os.path.join(d, name + ".png")
        with open(f[name], "wb") as o:
            o.write(bytes(data))
    f["missing"] = os.path.join(d, "missing.png")
    # the JPEG fixtures: 33 x 31 (two files), and 30 x 35 — 3 px narrower, 4 px taller
    f["jpg"] = os.path.join(JPEG_DIR, "baseline_gray_33x31.jpg")
    f["jpg_b"] = os.path.join(JPEG_DIR, "progressive_444_33x31.jpg")
    f["jpg_narrow"] = os.path.join(JPEG_DIR, "restart_gray_30x35.jpg")
    f["pgm_33"] = os.path.join(JPEG_DIR, "baseline_gray_33x31.pgm")
    rgb("e_33", 10, w=33, h=31, seed=14)
    rgb("t_33", 77, w=33, h=31, seed=15)
    return f


def pairs(f, *names):
    return [t for e, tg in names for t in ("R", f[e] if e else "", f[tg] if tg else "")]


def cases(f):
    """name -> (environment, resident budget in bytes, script)"""
    c = {}
    ten = [("e%d" % i, "t%d" % i) for i in range(10)]
    c["fast_ten_rgb"] = ({}, 0, pairs(f, *ten))
    c["pgm_target_among_pngs"] = ({}, 0, pairs(f, *[(e, "t_pgm" if i == 5 else t) for i, (e, t) in enumerate(ten)]))
    raw = ["M", W, H, 10, 10]
    c["raw_mixed_with_files"] = ({}, 0, raw + pairs(f, ten[0]) + ["M", W, H, 10, 99] + pairs(f, ten[1], ten[2]) + raw + ["M", 32, 24, 1, 2])
    for rec in (1, 0):
        env = {"TW_DEVICE_RECONCILE": str(rec)}
        c["narrower3_pgm_reconcile%d" % rec] = (env, 0, pairs(f, ("e_pgm", "t_pgm_narrow"), ("e_pgm", "t_pgm"), ("e0", "t_pgm_narrow")))
        c["narrower3_png_reconcile%d" % rec] = (env, 0, pairs(f, ("e0", "t_narrow"), ("e1", "t1"), ("e2", "t_narrow")))
        c["narrower3_jpeg_reconcile%d" % rec] = (env, 0, pairs(f, ("jpg", "jpg_narrow"), ("jpg", "jpg_b"), ("jpg_b", "jpg_narrow")))
    c["narrower6"] = ({}, 0, pairs(f, ("e0", "t_narrow6"), ("e1", "t1"), ("e_pgm", "t_narrow6")))
    c["jpeg_expected_png_target"] = ({}, 0, pairs(f, ("jpg", "t_33"), ("jpg", "e_33"), ("e_33", "jpg")))
    for k in (1, 0):
        c["palette_gray2_kinds%d" % k] = ({"TW_DEVICE_PNG_KINDS": str(k)}, 0,
                                          pairs(f, ("pal", "pal"), ("gray2", "pal"), ("e0", "gray2"), ("pal", "t0"), ("gray2", "gray2")))
    c["device_png0"] = ({"TW_DEVICE_PNG": "0"}, 0, pairs(f, *ten[:6]))
    for k in (0, 1):
        c["device_jpeg%d" % k] = ({"TW_DEVICE_JPEG": str(k)}, 0, pairs(f, ("jpg", "jpg_b"), ("jpg_b", "jpg"), ("jpg", "jpg"), ("jpg", "t_33"), ("jpg_b", "jpg")))
    c["damaged_both"] = ({}, 0, pairs(f, ("bad_e", "bad_t"), ("e0", "bad_t"), ("bad_e", "t0"), ("e1", "t1"), ("e2", "t2"), ("bad_crc", "bad_t"),
                                      ("e3", "bad_crc"), ("e4", "t4"), ("e5", "t5")))
    c["empty_and_missing"] = ({}, 0, pairs(f, ("", "t0"), ("e0", ""), ("missing", "t0"), ("e0", "missing"), ("e1", "t1")))
    sizes = [("e0", "t0"), ("e_small", "t_small"), ("e_tiny", "t_tiny")]
    c["three_sizes_interleaved"] = ({}, 0, pairs(f, *[sizes[i % 3] for i in range(10)]))
    shared = [("e0", "t%d" % (i % 10)) for i in range(12)]
    c["resident_twelve_share_expected"] = ({}, MB, pairs(f, *shared))
    c["resident_jpeg_targets"] = ({}, MB, pairs(f, *[("e_33", "jpg" if i % 2 else "jpg_b") for i in range(12)]))
    c["resident_leader_target_missing"] = ({}, MB, pairs(f, ("e0", "missing"), ("e0", "t1"), ("e0", "t2"), ("e0", "t3"), ("e0", "t4"), ("e0", "t5")))
    c["resident_bad_palette_expected"] = ({}, MB, pairs(f, ("pal_bad", "t0"), ("pal_bad", "t1"), ("e0", "t0"), ("pal_bad", "t2"),
                                                        ("pal_bad", "t3"), ("pal_bad", "pal"), ("e0", "t3"), ("pal_bad", "t0"), ("pal_bad", "t0")))
    c["resident_budget_below_one_image"] = ({}, 1000, pairs(f, *shared))
    c["resident_two_expected_budget_for_one"] = ({}, 1536, pairs(f, *[("e%d" % (i // 3 % 2), "t%d" % (i % 10)) for i in range(14)]))
    c["busy_at_third_submit"] = ({"TW_STUB_BUSY_AT": "3"}, 0, pairs(f, *ten[:7]))
    c["resident_busy_at_third_submit"] = ({"TW_STUB_BUSY_AT": "3"}, MB, pairs(f, *shared[:7]))
    return c


def with_regions(case, gap):
    """the case with hit regions on for the whole run (the probe's G: PairExtras::regions)"""
    env, budget, script = case
    return env, budget, ["G", gap] + list(script)


def with_residual(case, tol, minimum=0):
    """the case with the residual on for the whole run (the probe's D: PairExtras::residual, ::residualMin)"""
    env, budget, script = case
    return env, budget, ["D", tol, minimum] + list(script)


def with_shift(case, radius):
    """the case with the shift on for the whole run (the probe's S: PairExtras::shift)"""
    env, budget, script = case
    return env, budget, ["S", radius] + list(script)


def with_overlay(case, directory, tol=16):
    """the case with diff images on for the whole run (the probe's O: PairExtras::overlayDir, ::overlayTol)"""
    env, budget, script = case
    return env, budget, ["O", directory, tol] + list(script)


def with_shift_bands(case, radius, rows):
    """the case with the shift and its bands on for the whole run (the probe's S and B: PairExtras::shift, ::shiftBands)"""
    env, budget, script = case
    return env, budget, ["S", radius, "B", rows] + list(script)


# The second table: the per-pair extras ON.  EXTRAS_CASES under every configuration of extras_configs, 1 and 4 decode threads.
EXTRAS_CASES = ("fast_ten_rgb", "raw_mixed_with_files", "damaged_both", "empty_and_missing", "three_sizes_interleaved",
                "resident_twelve_share_expected", "resident_bad_palette_expected", "busy_at_third_submit", "narrower3_png_reconcile1")
# configuration -> the label of "engine: <label>: ..." that every pair of it answers
REFUSED = {"refused_gap9": "regions", "refused_tolerance255": "residual", "refused_radius1025": "shift", "refused_bands33": "shiftBands",
           "refused_overlay_tol256": "overlay", "refused_overlay_dir_missing": "overlay"}
ALL_ON_CALLS = ("tw_ticket_changes", "tw_ticket_shift", "tw_ticket_shift_bands", "tw_ticket_hits", "tw_ticket_overlay", "tw_wait_regions")


def extras_configs(odir):
    """name -> (the function that turns a case into the one with these extras on, whether it writes diff images into `odir`)"""
    def all_on(c):
        return with_overlay(with_shift_bands(with_residual(with_regions(c, 2), 12, 0), 64, 48), odir, 16)

    missing = os.path.join(odir, "missing")
    return {
        "regions2": (lambda c: with_regions(c, 2), False),
        "residual12_min0": (lambda c: with_residual(c, 12, 0), False),
        "residual12_min1": (lambda c: with_residual(c, 12, 1), False),
        "shift64": (lambda c: with_shift(c, 64), False),
        "shift64_bands48": (lambda c: with_shift_bands(c, 64, 48), False),
        "overlay16": (lambda c: with_overlay(c, odir, 16), True),
        "all_on": (all_on, True),
        "refused_gap9": (lambda c: with_regions(c, 9), False),
        "refused_tolerance255": (lambda c: with_residual(c, 255), False),
        "refused_radius1025": (lambda c: with_shift(c, 1025), False),
        "refused_bands33": (lambda c: with_shift_bands(c, 64, 33), False),
        "refused_overlay_tol256": (lambda c: with_overlay(c, odir, 256), True),
        "refused_overlay_dir_missing": (lambda c: with_overlay(c, missing, 16), False),
        "bands48_without_shift": (lambda c: (c[0], c[1], ["B", 48] + list(c[2])), False),
    }


def run_extras_row(exe, config, case, threads, workdir):
    """(responses, trace, SHA-256 of the diff images or None) of one case under one configuration.  A diff image's name starts
    with a hash of its target's full path, which differs from one work directory to the next: the responses read <fnv> there,
    and the pictures are hashed in the order of the rest of their names (then of their bytes), those rests included."""
    odir = os.path.join(workdir, "overlays")
    shutil.rmtree(odir, ignore_errors=True)
    os.makedirs(odir)
    turn_on, pictures = extras_configs(odir)[config]
    out, text = run_case(exe, turn_on(case), threads, workdir)
    out = re.sub(r"/[0-9a-f]{16}-", "/<fnv>-", out)
    png = None
    if pictures:
        h = hashlib.sha256()
        for rest, data in sorted((n[17:], open(os.path.join(odir, n), "rb").read()) for n in os.listdir(odir)):
            h.update(rest.encode() + b"\0" + data)
        png = h.hexdigest()[:16]
    if config in REFUSED:
        lines = out.strip().splitlines()[:-1]
        label = "ERROR|engine: %s: " % REFUSED[config]  # (a pair whose files cannot be read says so, engine or no engine)
        unread = ("ERROR|Can't open ", "ERROR|ExpectImagePath is empty.", "ERROR|TargetImagePath is empty.")
        assert any(ln.startswith(label) for ln in lines) and all(ln.startswith((label,) + unread) for ln in lines), (config, lines[:2])
        assert " tw_submit_" not in text and " tw_wait" not in text and not (pictures and os.listdir(odir)), config
    return out, text, png


def extras_rows(exe, f, workdir, out_dir=None):
    """"<configuration>/<case>" -> {"responses", "trace", "lines"[, "png"]} at 1 decode thread, and the rows whose 4-thread
    run differs from it"""
    rows, differ = {}, []
    all_cases = cases(f)
    for config in extras_configs(""):
        seen = set()
        for name in EXTRAS_CASES:
            got = []
            for threads in (1, 4):
                out, text, png = run_extras_row(exe, config, all_cases[name], threads, workdir)
                row = {"responses": sha(out), "trace": sha(text), "lines": text.count("\n")}
                if png is not None:
                    row["png"] = png
                got.append(row)
                seen.update(t.split(" ", 2)[1] for t in text.strip().splitlines())
                if out_dir:
                    os.makedirs(out_dir, exist_ok=True)
                    with open(os.path.join(out_dir, "%s.%s.%d.txt" % (config, name, threads)), "w") as o:
                        o.write(out + "---\n" + text)
            rows[config + "/" + name] = got[0]
            if got[0] != got[1]:
                differ.append(config + "/" + name)
        # the golden must not pin an accident: with everything on, every call of the extras is really made
        assert config != "all_on" or all(c in seen for c in ALL_ON_CALLS), sorted(seen)
    return rows, differ


def run_case(exe, case, threads, workdir, batch=4):
    """(responses as printed, the trace's text) of one case; every path under `workdir` or the tree reads <dir> / <root>"""
    env_more, budget, script = case
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(TW_STUB_DEVICES="1", TW_NUMA="0")
    env.update(env_more)
    trace = tempfile.NamedTemporaryFile(prefix="consumer_trace_", suffix=".txt", dir=workdir, delete=False)
    trace.close()
    env["TW_STUB_TRACE"] = trace.name
    r = subprocess.run([exe, str(threads), str(budget), str(batch)] + [str(t) for t in script], capture_output=True, text=True,
                       timeout=120, env=env)
    text = open(trace.name).read()
    os.unlink(trace.name)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.replace(workdir, "<dir>").replace(ROOT, "<root>")
    return out, text


def sha(s):
    return hashlib.sha256(s.encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--twhost", help="the twhost.cpp to build against (default: the tree's)")
    ap.add_argument("--include", help="a directory of headers that twhost.cpp includes, searched after host/")
    ap.add_argument("--out", help="keep every case's responses and trace in this directory")
    ap.add_argument("--extras-json", help="write the rows of the second table (the extras on) to this file, as tests/golden/consumer_extras_parent.json")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="consumer_trace_") as d:
        exe = build(os.path.join(d, "consumer_probe"), args.twhost, args.include)
        f = write_files(d)
        print("| case | responses, 1 thread | trace, 1 thread | lines | responses, 4 threads | trace, 4 threads | lines |")
        print("|---|---|---|---|---|---|---|")
        same = True
        for name, case in cases(f).items():
            row = []
            for threads in (1, 4):
                out, text = run_case(exe, case, threads, d)
                row += [sha(out), sha(text), str(text.count("\n"))]
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "%s.%d.txt" % (name, threads)), "w") as o:
                        o.write(out + "---\n" + text)
            same = same and row[:3] == row[3:]
            print("| %s | %s |" % (name, " | ".join(row)))
        print("\n1 and 4 decode threads: %s" % ("the same in every row" if same else "DIFFERENT"))
        rows, differ = extras_rows(exe, f, d, args.out)
        print("\n| configuration / case | responses | trace | lines | diff images |")
        print("|---|---|---|---|---|")
        for name, row in rows.items():
            print("| %s | %s | %s | %d | %s |" % (name, row["responses"], row["trace"], row["lines"], row.get("png", "")))
        print("\nthe extras on, 1 and 4 decode threads: %s" % ("the same in every row" if not differ else "DIFFERENT in " + ", ".join(differ)))
        if args.extras_json:
            with open(args.extras_json, "w") as o:
                json.dump({k: v for k, v in rows.items() if k not in differ}, o, indent=1, sort_keys=True)
                o.write("\n")
        return 0 if same and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
