#!/usr/bin/env python3
"""The engine's books, step by step: a fixed tour through every call that makes the engine allocate, with Engine.memory()
(tw_debug_memory) after every step.  Needs a GPU.

    TWFLOW_LIB=<a build of libtwflow.so> memory_books.py [OUT.json]     (prints the steps as one JSON document)

The books are sums of allocation sizes, so two builds of the library that allocate alike print the same document, byte for
byte: tests/golden/memory_books_parent.json is this tool's output for the library before the engine's buffers got owning
types (profiles/engine_buffers.md), and tests/test_gpu_memory_books.py holds the tree's library to it.

Every step waits for what it submitted, so the engine stays in its first context and a buffer that is created on first use
appears in exactly one step; every step runs twice (the second is named "... again") and the repeat must add nothing.  The
process-wide pagelock_* entries (tw_host_alloc / tw_host_register of anybody in the process) are left out.

Sizes: 384x96 — level 0 is wide enough for tw_flow_iter; 64x48 — too narrow for it; 640x480 — the workspace must grow.
Batch steps run on a four-slot engine, single-pair steps on a one-slot engine.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tidal-wave_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import synth  # noqa: E402

SPAN, THR = 10, 1.0
SIZES = ((384, 96), (64, 48), (640, 480))  # (width, height)


def books(e):
    return {k: v for k, v in e.memory().items() if not k.startswith("pagelock_")}


def _rows(img):
    """A gray image as PNG rows of filter type 0 (one channel, 8 bits)."""
    h, w = img.shape
    out = np.zeros((h, 1 + w), np.uint8)
    out[:, 1:] = img
    return out


def batch_steps(T, e, w, h):
    """(name, action) of every batch step at one size; an action submits, waits for everything and returns nothing."""
    pairs = [synth.make_pair(i, h, w) for i in range(4)]
    a, b = pairs[0]
    ident = np.repeat(np.arange(256, dtype=np.uint8), 3)  # the identity gray palette
    small = np.ascontiguousarray(b[:h - 3, :w - 2])

    def wait_all(tickets):
        for t in tickets:
            e.wait(t)

    def with_option(setter, value, collect):
        """The batch with the option on; collect(ticket) reads the first pair's extra result and leaves the ticket unwaited."""
        def run():
            setter(value)
            try:
                tickets = [e.submit(x, y, SPAN, THR) for x, y in pairs]
                e.flush()
                collect(tickets[0])
                wait_all(tickets)
            finally:
                setter(0)
        return run

    def jpeg():
        import jpeg_cases as J
        la, lb = (J.decode_luma(J.fixture(n)[0])[0] for n in ("golden_expected", "golden_revision2"))
        e.wait(e.submit_jpeg(T.JpegLuma(la.coef, la.quant, la.w, la.h), T.JpegLuma(lb.coef, lb.quant, lb.w, lb.h), SPAN, THR))

    def flow_out():
        out = e.host_array((4, 2, h, w), np.float32)
        wait_all([e.submit(x, y, SPAN, THR, flow=out[i]) for i, (x, y) in enumerate(pairs)])

    def flow_init():
        field = np.zeros((2, h, w), np.float32)
        wait_all([e.submit(x, y, SPAN, THR, init=field) for x, y in pairs])

    def overlay():
        dst = e.host_array((h, w, 3), np.uint8)
        t = e.submit(a, b, SPAN, THR)
        e.flush()
        e.overlay(t, 16, dst.ctypes.data)
        e.wait(t)

    def keep_and_submit_image():
        t = e.submit(a, b, SPAN, THR)
        img = e.keep(t, "expect")
        e.wait(t)
        e.wait(e.submit_image(img, T.PngRows(_rows(b), w, h, 0, 8), SPAN, THR))
        img.release()

    return [
        ("host u8 batch", lambda: wait_all([e.submit(x, y, SPAN, THR) for x, y in pairs])),
        ("png8 rows", lambda: wait_all([e.submit_png8(_rows(x), 1, _rows(y), 1, w, h, SPAN, THR) for x, y in pairs])),
        ("palette png", lambda: e.wait(e.submit_png(T.PngRows(_rows(a), w, h, 3, 8, ident), T.PngRows(_rows(b), w, h, 3, 8, ident),
                                                    SPAN, THR))),
        ("jpeg fixture", jpeg),
        ("sized pair", lambda: e.wait(e.submit(a, small, SPAN, THR, reconcile=True))),
        ("ignore pair", lambda: e.wait(e.submit(a, b, SPAN, THR, ignore=[(5, 7, 20, 10)]))),
        ("flow out to host", flow_out),
        ("flow init from host", flow_init),
        ("regions", with_option(e.set_regions, 2, e.hits)),
        ("residual", with_option(e.set_residual, 16, e.changes)),
        ("shift", with_option(e.set_shift, 8, e.shift)),
        ("overlay to host", overlay),
        ("keep and submit_image", keep_and_submit_image),
        ("calculate_internal", lambda: e.calculate_internal(a, b)),
    ]


def tour(T):
    """[[step name, books]] of the whole tour, in order."""
    steps = []

    def run(e, prefix, name, action):
        for again in ("", " again"):
            action()
            steps.append(["%s: %s%s" % (prefix, name, again), books(e)])

    with T.Engine(0, T.default_params(), slots=4) as e:
        steps.append(["slots=4: new engine", books(e)])
        for w, h in SIZES:
            for name, action in batch_steps(T, e, w, h):
                run(e, "slots=4 %dx%d" % (w, h), name, action)
    for what, params in (("slots=1", T.default_params()), ("slots=1 flags=0", T.default_params(flags=0))):
        with T.Engine(0, params, slots=1) as e:
            steps.append(["%s: new engine" % what, books(e)])
            for w, h in SIZES:
                a, b = synth.make_pair(0, h, w)
                run(e, "%s %dx%d" % (what, w, h), "diff", lambda: e.diff(a, b, SPAN, THR))
                run(e, "%s %dx%d" % (what, w, h), "calculate_internal", lambda: e.calculate_internal(a, b))
    return steps


def main():
    import twflow as T
    doc = json.dumps(tour(T), indent=1)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
