"""Feature combinations as data: one pair of a batch as a PairSpec, one batch as a Recipe (DESIGN.md §3 "Composition").

Plain module, no device.  A Pair is a PairSpec bound to two gray frames.  `reference(pair)` is what the batch must see — the
two gray images, the clipped rectangles and the initial field — computed on the CPU alone: the decode is numpy (gray15 over
the RGBA / palette samples) or jpeg_cases.idct_reference, the resize is oracle.reconcile_target, the mask is numpy slicing
after the resize, a kept target is the prepared (masked) target of the pair that kept it.  `submit(e, pair, span, thr)` makes
the one Engine.submit* call of the spec.  The expected answer of a pair is then the oracle's alone:

    field   = farneback_with_init(oracle, a, b_prepared, init)          (oracle.farneback without a field)
    vectors = oracle.span_scan(fx, fy, span, thr) minus the points inside a clipped rectangle
    regions = regions_ref.regions(vectors, gap, span, w, h)

Combinations the ABI does not have are refused with a ValueError (why_refused), never skipped.

The recipes: A - H are written out; M ("mixed") and the filler pairs of D are chosen by a deterministic greedy cover over
every legal PairSpec, so that every legal pair of factor values occurs in a batch that takes the grid-only path
(tests/test_compose_reference.py asserts it and prints the table).
"""
import dataclasses
import hashlib
import itertools

import numpy as np

import regions_ref as R
import twflow as T
from test_flow_init_abi import farneback_with_init
from test_gpu_ignore import clip, edit, outside
from test_gpu_resident import as_jpeg, as_pal4, as_rgba

GRAY = ("pageable_gray", "page_locked_gray")
DECODED = ("rgba_rows", "pal4_rows", "jpeg_coef")
RESIDENT = ("resident_created", "resident_kept_target")
EXPECTED_FORMS = GRAY + DECODED + ("device",) + RESIDENT
TARGET_FORMS = EXPECTED_FORMS[:6]
SIZES = ((3, -2), (-4, -5))  # (dw, dh) of a sized target: both shrink its rows, so that a batch's first RGBA image is its largest


@dataclasses.dataclass(frozen=True)
class PairSpec:
    expected: str = "pageable_gray"
    target: str = "pageable_gray"
    sized: bool = False      # the target comes (dw, dh) off the pair's size: the *_sized paths
    ignore: bool = False     # the shape's rectangles (rects_for)
    init: bool = False       # a host initial field
    keep: bool = False       # the pair's target is kept (Engine.keep(ticket, "target")) for a later pair of the batch
    identical: bool = False  # the target is the expected image
    patch: bool = False      # the target differs from the expected image inside the rectangles only (needs ignore)
    png8: bool = False       # tw_submit_png8 instead of tw_submit_png
    flow: bool = False       # the pair wants its dense field


def why_refused(s):
    """The reason the ABI has no call for this spec, or None."""
    if s.expected not in EXPECTED_FORMS or s.target not in EXPECTED_FORMS:
        return "unknown form"
    if s.target in RESIDENT:
        return "a resident target: tw_submit_image_* take a resident EXPECTED image only"
    if (s.expected == "device") != (s.target == "device"):
        return "tw_submit_dev* take both images from device memory, no other call takes one"
    if s.expected == "device" and (s.ignore or s.patch):
        return "tw_submit_dev* have no _ignore call: only host pairs are masked"
    if s.png8 and (s.ignore or s.patch):
        return "tw_submit_png8 has no _ignore call: use submit_png"
    if s.png8 and not ({s.expected, s.target} <= set(GRAY) | {"rgba_rows"}):
        return "tw_submit_png8 takes 8-bit rows of 1 - 4 channels or gray images"
    if "jpeg_coef" in (s.expected, s.target) and {s.expected, s.target} & {"rgba_rows", "pal4_rows"}:
        return "no call takes coefficients for one image and PNG rows for the other"
    if s.identical and s.sized:
        return "a target of another size is resampled: it is not the expected image"
    if s.identical and s.target in DECODED and s.target != s.expected:
        return "a lossy target form does not decode to the expected image"
    if s.identical and s.patch:
        return "identical and patch are two different targets"
    if s.patch and not s.ignore:
        return "patch needs the rectangles"
    if s.keep and s.target == "device" and s.sized:
        return "tw_image_keep of a reconciled device target launches the open batch: no frame sequence inside one batch"
    return None


def check(s):
    why = why_refused(s)
    if why:
        raise ValueError("%s: %s" % (s, why))


# ---- frames and rectangles ---------------------------------------------------------------------------------------------
FRAME_KINDS = (0, 1, 0, 1, 0, 1, 2, 1)  # at most 8 distinct pairs per shape: warps, and one painted rectangle
_FRAMES = {}


def frames(w, h):
    import synth
    if (w, h) not in _FRAMES:
        _FRAMES[(w, h)] = [tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, h, w, kind=k))
                           for i, k in enumerate(FRAME_KINDS)]
    return _FRAMES[(w, h)]


def rects_for(w, h):
    """The rectangles of a masked pair: one in the middle (the warp reaches in: vectors to suppress), one clipped by the
    bottom edge, one 1 x 1 exactly on a grid point of spans 5, 7 and 10, one covering the last grid column of those spans."""
    gy = 70 if h > 70 else 0
    out = [(w // 3 + 1, h // 4 + 1, w // 3, h // 2), (w // 3 + 1, h - 7, w // 4, 30), (70, gy, 1, 1), (w - 12, h // 4, 12, h // 3)]
    for span in (5, 7, 10):
        assert 70 % span == 0 and gy % span == 0 and w - 12 <= (w - 1) // span * span
    return out


def init_field(w, h, seed):
    return (np.random.default_rng(1000 + seed).random((2, h, w), np.float32) * 4 - 2).astype(np.float32)


def encode(form, g):
    """(what the submit call takes, the gray image the device makes of it)"""
    if form == "rgba_rows":
        return as_rgba(T, g)[:2]
    if form == "pal4_rows":
        return as_pal4(T, g)[:2]
    if form == "jpeg_coef":
        return as_jpeg(T, g)[:2]
    g = np.ascontiguousarray(g)
    return g, g


class Pair:
    """A PairSpec bound to two gray frames of one shape (and, for resident_kept_target, to the pair that kept its target)."""

    def __init__(self, oracle, spec, a_src, b_src, prev=None, seed=0):
        check(spec)
        self.spec = spec
        self.h, self.w = h, w = a_src.shape
        if spec.expected == "resident_kept_target":
            if prev is None or not prev.spec.keep:
                raise ValueError("resident_kept_target needs an earlier pair of the batch that keeps its target")
            self.a_obj, self.a = None, prev.b
        else:
            self.a_obj, self.a = encode(spec.expected, a_src)
        self.prev = prev
        self.rects = rects_for(w, h) if spec.ignore else []
        if spec.identical:
            t = a_src if spec.target == spec.expected else self.a
        elif spec.patch:
            t = self.a.copy()
            for x0, y0, x1, y1 in clip(self.rects, w, h):
                t[y0:y1, x0:x1] = b_src[y0:y1, x0:x1]
        else:
            t = b_src
        self.size = (w, h)
        if spec.sized:
            dw, dh = SIZES[seed % 2]
            self.size = (w + dw, h + dh)
            t = oracle.resize_u8_linear(t, w + dw, h + dh)
        self.t_obj, self.t_gray = encode(spec.target, t)
        resized = oracle.reconcile_target(self.t_gray, w, h) if spec.sized else self.t_gray
        self.b = edit(self.a, resized, self.rects)
        self.init = init_field(w, h, seed) if spec.init else None
        if spec.identical and not np.array_equal(self.a, self.b):
            raise ValueError("%s: the forms do not decode alike" % (spec,))
        self.same = int(np.array_equal(self.a, self.b))
        self._key = hashlib.sha1(self.a.tobytes() + self.b.tobytes() + (b"" if self.init is None else self.init.tobytes())).digest()

    # ---- the expected answer ----
    def field(self, oracle):
        k = (self._key, self.w, self.h)
        if k not in _FIELDS:
            fx, fy = (oracle.farneback(self.a, self.b) if self.init is None else
                      farneback_with_init(oracle, self.a, self.b, self.init))
            _FIELDS[k] = np.stack([fx, fy])
        return _FIELDS[k]

    def vectors(self, oracle, span, thr):
        f = self.field(oracle)
        return outside(oracle.span_scan(f[0], f[1], span, thr), self.rects, self.w, self.h)

    def regions(self, oracle, span, thr, gap):
        """(records, region_of) of regions_ref over the expected vectors"""
        return R.regions(self.vectors(oracle, span, thr), gap, span, self.w, self.h)

    # ---- the one submit call ----
    def submit(self, e, span, thr, resident=None, flow=None, live=None):
        """resident: the Image of a resident expected form (Engine.image(pair.a), or the kept target); live: a list that
        takes what must stay alive until the ticket is waited."""
        s, w, h = self.spec, self.w, self.h
        live = [] if live is None else live
        ign = list(self.rects) if s.ignore else None
        tw_, th_ = self.size

        def host(form, obj):
            if form == "page_locked_gray":
                p = e.host_array(obj.shape)
                p[...] = obj
                obj = p
            live.append(obj)
            return obj

        if s.expected == "device":
            da, db = e.upload(self.a), e.upload(self.t_gray)
            return e.submit_dev(da, db, w, h, w, span, thr, flow=flow, init=self.init,
                                target_size=(tw_, th_) if s.sized else None, target_stride=tw_ if s.sized else None)
        t = host(s.target, self.t_obj)
        if s.expected in RESIDENT:
            return e.submit_image(resident, t, span, thr, flow=flow, init=self.init, ignore=ign)
        a = host(s.expected, self.a_obj)
        if "jpeg_coef" in (s.expected, s.target):
            return e.submit_jpeg(a, t, span, thr, init=self.init, out=flow, ignore=ign)
        if s.png8:
            rows = [(x._rows, 4) if isinstance(x, T.PngRows) else (x, 0) for x in (a, t)]
            return e.submit_png8(rows[0][0], rows[0][1], rows[1][0], rows[1][1], w, h, span, thr, flow=flow, init=self.init,
                                 target_size=(tw_, th_) if s.sized else None)
        if {s.expected, s.target} & set(DECODED):
            pa, pt = (x if isinstance(x, T.PngRows) else T.PngRows(x, x.shape[1], x.shape[0]) for x in (a, t))
            live += [pa, pt]
            return e.submit_png(pa, pt, span, thr, flow=flow, init=self.init, ignore=ign)
        return e.submit(a, t, span, thr, flow=flow, init=self.init, reconcile=s.sized, ignore=ign)


_FIELDS = {}  # the oracle's fields, computed once per session


def reference(pair):
    """(a, b_prepared, rects, init): what the batch must see of this pair"""
    return pair.a, pair.b, clip(pair.rects, pair.w, pair.h), pair.init


def submit(e, pair, span, thr, **kw):
    return pair.submit(e, span, thr, **kw)


# ---- what a batch launches for its pairs' forms (flush_ctx, csrc/twflow.hip) -------------------------------------------
def decoded(s):
    """the pair goes through the batch's decode launches (its images wait in the filtered-rows slots)"""
    return bool({s.expected, s.target} & set(DECODED))


def mask_rounds(pairs):
    """tw_mask_rects launches: one, and one more for every masked pair whose expected image is the kept target of a masked pair"""
    if not any(p.rects for p in pairs):
        return 0
    rnd = {}
    for p in pairs:
        if p.rects:
            up = p.prev if p.spec.expected == "resident_kept_target" else None
            rnd[id(p)] = rnd[id(up)] + 1 if up is not None and up.rects else 0
    return max(rnd.values()) + 1


def decode_launches(pairs):
    """{family: launches} of the decode and resize kernels of one batch of these pairs"""
    specs = [p.spec for p in pairs]
    png = [s for s in specs if {s.expected, s.target} & {"rgba_rows", "pal4_rows"}]
    own = {p.size for p in pairs if p.spec.sized and p.spec.target in ("rgba_rows", "pal4_rows")}
    return {
        "tw_jpeg_idct": int(any("jpeg_coef" in (s.expected, s.target) for s in specs)),
        # the batch-wide launch, and one per distinct size of the filtered targets of another size
        "tw_png_unfilter": int(bool(png)) + len(own),
        # a gray host target: its own launch at submit time; decoded pairs: one launch per batch; device targets: one more
        "tw_resize_u8": (sum(1 for s in specs if s.sized and not decoded(s) and s.expected != "device") +
                         int(any(s.sized and decoded(s) for s in specs)) +
                         int(any(s.sized and s.expected == "device" for s in specs))),
        "tw_mask_rects": mask_rounds(pairs),
    }


# ---- recipes -------------------------------------------------------------------------------------------------------------
LIFTED = {"TW_MFREE": "2", "TW_LATENCY_STREAMS": "0", "TW_RAMP": "0"}  # the gate-lifted fixture of test_gpu_grid_final.py
RAMP = {"TW_MFREE": "2", "TW_LATENCY_STREAMS": "0"}                    # ... with the default TW_RAMP


@dataclasses.dataclass(frozen=True)
class Recipe:
    name: str
    w: int
    h: int
    slots: int
    env: tuple          # ((name, value), ...)
    span: int
    gap: int            # TW_OPT_REGIONS: 0 off
    specs: tuple
    lanes: int = 1
    ramp: bool = False  # the batch goes out in the cold-start ramp's three pieces
    scan_fused: bool = False
    frame_of: tuple = ()  # the frame pair of each spec (default: i % 6)

    @property
    def grid_only(self):
        """the batch ends in tw_flow_iter<15, 3> (LevelSchedule::grid_final)"""
        return not self.scan_fused and not any(s.flow for s in self.specs) and self.slots > 1 and self.span >= 5

    def pairs(self, oracle):
        key = (self.w, self.h, self.specs, self.frame_of)
        if key not in _PAIRS:
            fr, out, kept, kept_k = frames(self.w, self.h), [], None, -1
            for i, s in enumerate(self.specs):
                k = self.frame_of[i] if self.frame_of else i % 6
                if s.expected == "resident_kept_target" and k == kept_k:
                    k = (k + 1) % 6  # (the next frame of a sequence is another frame than the kept one)
                out.append(Pair(oracle, s, fr[k][0], fr[k][1], prev=kept, seed=k))
                if s.keep:
                    kept, kept_k = out[-1], k
            _PAIRS[key] = out
        return _PAIRS[key]

    def pieces(self):
        """the pairs of each part of the batch: the ramp's three pieces, one per lane, or the whole batch"""
        n = len(self.specs)
        if self.ramp:
            return [self.slots // 4, self.slots // 4, n - self.slots // 2]
        return [n - n // 2, n // 2] if self.lanes == 2 else [n]


_PAIRS = {}
P = PairSpec

A_SPECS = (
    P("rgba_rows", "pal4_rows", sized=True, ignore=True),
    P("jpeg_coef", "pageable_gray", ignore=True),
    P("pageable_gray", "jpeg_coef", sized=True),
    P("page_locked_gray", "page_locked_gray", init=True),
    P("pageable_gray", "pageable_gray", identical=True),
    P("resident_created", "rgba_rows", keep=True),
    P("resident_kept_target", "jpeg_coef", ignore=True),
)
# ... with device images, equal and sized, in place of the gray host pairs
A_DEV_SPECS = A_SPECS[:3] + (P("device", "device", sized=True, init=True), P("device", "device", identical=True)) + A_SPECS[5:]
# two masked, one sized in each half; the second half's masked pair reads the kept MASKED target of the pair before it (a
# second tw_mask_rects round), and one pair is identical only after masking
C_SPECS = (
    P("rgba_rows", "rgba_rows", sized=True, png8=True),
    P("pageable_gray", "pal4_rows", ignore=True),
    P("page_locked_gray", "pageable_gray", ignore=True, patch=True),
    P("jpeg_coef", "jpeg_coef", identical=True),
    P("pageable_gray", "page_locked_gray", sized=True, init=True),
    P("resident_created", "pageable_gray", ignore=True, keep=True),
    P("resident_kept_target", "rgba_rows", ignore=True),
    P("pal4_rows", "pageable_gray"),
)
E_SPECS = (
    P("rgba_rows", "pal4_rows"),
    P("pageable_gray", "jpeg_coef"),
    P("page_locked_gray", "pageable_gray", sized=True),
    P("pageable_gray", "pageable_gray", ignore=True),
    P("resident_created", "page_locked_gray"),
    P("pageable_gray", "pageable_gray", identical=True),
)
G_SPECS = A_SPECS[:3] + (dataclasses.replace(A_SPECS[3], flow=True),) + A_SPECS[4:]

# ---- factors and the greedy cover ----------------------------------------------------------------------------------------
PAIR_FACTORS = ("expected", "target", "sized", "ignore", "init", "keep", "identical")
BATCH_FACTORS = ("regions", "span", "lanes", "ramp")
VALUES = {"expected": EXPECTED_FORMS, "target": TARGET_FORMS, "sized": (False, True), "ignore": (False, True),
          "init": (False, True), "keep": (False, True), "identical": (False, True), "regions": (0, 1, 3), "span": (5, 7, 10),
          "lanes": (1, 2), "ramp": (False, True)}
NOT_DEVICE = tuple(f for f in EXPECTED_FORMS if f != "device")


def _each(fa, va, fb, vb, why):
    return [(((fa, a), (fb, b)), why) for a in va for b in vb]


# the pairs of values that cannot occur together, each with its reason
ILLEGAL = dict(
    _each("expected", ("device",), "target", TARGET_FORMS[:5], "tw_submit_dev* take both images from device memory") +
    _each("expected", NOT_DEVICE, "target", ("device",), "no other call takes a device image") +
    _each("expected", ("jpeg_coef",), "target", ("rgba_rows", "pal4_rows"), "no call takes coefficients and PNG rows") +
    _each("expected", ("rgba_rows", "pal4_rows"), "target", ("jpeg_coef",), "no call takes PNG rows and coefficients") +
    _each("expected", ("device",), "ignore", (True,), "tw_submit_dev* have no _ignore call") +
    _each("target", ("device",), "ignore", (True,), "tw_submit_dev* have no _ignore call") +
    _each("sized", (True,), "identical", (True,), "a resampled target is not the expected image") +
    _each("expected", DECODED, "ramp", (True,), "a batch with PNG rows or coefficients goes out whole (any_png, any_jpeg)") +
    _each("target", DECODED, "ramp", (True,), "a batch with PNG rows or coefficients goes out whole (any_png, any_jpeg)") +
    _each("ignore", (True,), "ramp", (True,), "a batch with a masked pair goes out whole (any_mask)") +
    _each("lanes", (2,), "ramp", (True,), "the ramp is the one-lane schedule's (e->lanes == 1)"))


def value_pairs(names):
    """every pair of values of two different factors among `names`, as ((factor, value), (factor, value)) in factor order"""
    return [((fa, a), (fb, b)) for fa, fb in itertools.combinations(names, 2) for a in VALUES[fa] for b in VALUES[fb]]


def spec_values(s):
    return [(f, getattr(s, f)) for f in PAIR_FACTORS]


def greedy_cover(forms):
    """Legal PairSpecs over `forms`, chosen one by one — always the first that covers the most still uncovered pairs of
    pair-level factor values — until every legal pair is covered.  Deterministic: the candidates are enumerated in order."""
    cands = [P(ex, tg, sized=sz, ignore=ig, init=it_, keep=kp, identical=idn)
             for ex in EXPECTED_FORMS for tg in TARGET_FORMS if ex in forms and tg in forms
             for sz in (False, True) for ig in (False, True) for it_ in (False, True) for kp in (False, True) for idn in (False, True)
             if not (ig and "ignore" not in forms)]
    cands = [s for s in cands if why_refused(s) is None]
    cover = lambda s: set(itertools.combinations(spec_values(s), 2))  # noqa: E731
    left = set().union(*(cover(s) for s in cands))
    chosen = []
    while left:
        best = max(cands, key=lambda s: len(cover(s) & left))
        chosen.append(best)
        left -= cover(best)
    # a batch's first filtered image must be its largest (an RGBA expected image); a kept target must precede its reader
    chosen.sort(key=lambda s: (s.expected != "rgba_rows", not (s.keep and s.expected != "resident_kept_target")))
    first_keep = next(i for i, s in enumerate(chosen) if s.keep and s.expected != "resident_kept_target")
    first_read = next((i for i, s in enumerate(chosen) if s.expected == "resident_kept_target"), len(chosen))
    assert first_keep < first_read
    return tuple(chosen)


M_SPECS = greedy_cover(set(EXPECTED_FORMS) | {"ignore"})
RAMP_FORMS = set(GRAY) | {"device"} | set(RESIDENT)
D_FILL = greedy_cover(RAMP_FORMS)


def d_specs(masked):
    """64 page-locked pairs: sized at 15, 16, 31, 32, 63, a created resident expected image at 0, 16, 32 (the first pair of
    each piece of the ramp), a field at 17, an identical pair at 3; the filler (D_FILL: every legal combination of the ramp's
    forms) from pair 4 on — host pairs at 15 and 31, where the ramp marks the copy stream; D': pair 40 masked."""
    lock = P("page_locked_gray", "page_locked_gray")
    specs = [lock] * 64
    for i in (15, 31, 63):
        specs[i] = dataclasses.replace(lock, sized=True)
    specs[0] = P("resident_created", "page_locked_gray")
    for i in (16, 32):
        specs[i] = P("resident_created", "page_locked_gray", sized=True)
    specs[17] = dataclasses.replace(lock, init=True)
    specs[3] = dataclasses.replace(lock, identical=True)
    free = [i for i in range(4, 63) if i not in (15, 16, 17, 31, 32, 40)]
    assert len(D_FILL) <= len(free)
    for i, s in zip(free, D_FILL):
        specs[i] = s
    if masked:
        specs[40] = dataclasses.replace(lock, ignore=True)
    return tuple(specs)


def _r(name, w, h, slots, env, span, gap, specs, **kw):
    return Recipe(name, w, h, slots, tuple(sorted(env.items())), span, gap, tuple(specs), **kw)


RECIPES = {r.name: r for r in [
    _r("A", 397, 99, 8, LIFTED, 10, 0, A_SPECS),
    _r("A_device", 397, 99, 8, LIFTED, 10, 0, A_DEV_SPECS),
    _r("B_span5_gap1", 397, 99, 8, LIFTED, 5, 1, A_SPECS),
    _r("B_span7_gap3", 397, 99, 8, LIFTED, 7, 3, A_SPECS),
    _r("C_lanes2", 397, 99, 8, dict(LIFTED, TW_LANES="2"), 10, 1, C_SPECS, lanes=2),
    _r("D_ramp", 333, 41, 64, RAMP, 10, 2, d_specs(False), ramp=True, frame_of=tuple(i % 6 for i in range(64))),
    _r("D_ramp_span5_gap0", 333, 41, 64, RAMP, 5, 0, d_specs(False), ramp=True, frame_of=tuple(i % 6 for i in range(64))),
    _r("D_ramp_span7_gap1", 333, 41, 64, RAMP, 7, 1, d_specs(False), ramp=True, frame_of=tuple(i % 6 for i in range(64))),
    _r("D_ramp_span10_gap3", 333, 41, 64, RAMP, 10, 3, d_specs(False), ramp=True, frame_of=tuple(i % 6 for i in range(64))),
    _r("D_masked", 333, 41, 64, RAMP, 10, 2, d_specs(True), frame_of=tuple(i % 6 for i in range(64))),
    _r("E_default_gate", 640, 480, 24, {}, 10, 1, E_SPECS * 4, frame_of=tuple(i % 6 for i in range(24))),
    _r("G_flow", 397, 99, 8, LIFTED, 10, 0, G_SPECS),
    _r("H_scan_fused", 397, 99, 8, LIFTED, 10, 0, A_SPECS, scan_fused=True),
] + [
    # the mixed batch under every (span, regions) and with both lane counts against each of them
    _r("M_span%d_gap%d_lanes%d" % (span, gap, lanes), 333, 41, len(M_SPECS), dict(LIFTED, **({"TW_LANES": "2"} if lanes == 2 else {})),
       span, gap, M_SPECS, lanes=lanes)
    for span, gap, lanes in ((5, 0, 1), (5, 1, 2), (5, 3, 1), (7, 0, 2), (7, 1, 1), (7, 3, 2), (10, 0, 1), (10, 1, 1), (10, 3, 2))
]}


def recipe_values(r):
    return [("regions", r.gap), ("span", r.span), ("lanes", r.lanes), ("ramp", r.ramp)]


def coverage():
    """{pair of values: [recipes]} over the recipes that take the grid-only path"""
    seen = {}
    for r in RECIPES.values():
        if not r.grid_only:
            continue
        rv = recipe_values(r)
        got = set(itertools.combinations(rv, 2))
        for s in r.specs:
            sv = spec_values(s)
            got |= set(itertools.combinations(sv, 2)) | {(a, b) for a in sv for b in rv}
        for p in got:
            seen.setdefault(p, []).append(r.name)
    return seen
