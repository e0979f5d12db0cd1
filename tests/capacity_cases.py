"""Full-capacity batches as data: the byte table of a batch, its distinct pairs, and the proof that a wrap cannot hide.

Plain module, no test in it (tests/test_gpu_capacity.py runs the cases, profiles/capacity.md shows the tables).

Every kernel of a batch finds its pair through blockIdx -> z and its planes at base + z * (bytes per pair); the host does
the same for the staging arrays.  `byte_table` lists, for one batch, every device array that is indexed by a pair: bytes per
pair, the largest index a kernel or copy applies to it, the largest byte offset, and the launches (which batch slot sits at
which index).  The sizes come from the engine's own plan where it exports them (Engine.level_plan, Engine.level_chunk,
Engine.num_levels, tw_grid_capacity); what it does not export is restated here with the line of csrc/twflow.hip it restates.

A batch of N slots holds K distinct pairs, slot s holding pair s % K.  `assert_wrap_cannot_hide` is integer arithmetic on
the table: an offset that lost 2^31, 2^32, 2^33 or any multiple of 2^32 must not be the offset of a slot that holds the same
pair, and a chunk buffer that a later launch reuses must not have held the same pair at the same index.  A kernel that
truncated z * (bytes per pair) would therefore read or write another pair's bytes (or the middle of a slot), and the
comparison of every slot with the oracle sees it.
"""
import collections
import ctypes as C
import dataclasses

import numpy as np

import twflow as T

P31, P32, P33 = 2 ** 31, 2 ** 32, 2 ** 33
POWERS = (P31, P32, P33)
CAP_MAX = 256  # tw_engine_create clamps slots (twflow.hip: `if (slots > 256) slots = 256`)
SCANREC_BYTES, FLOAT2_BYTES = 16, 8  # struct ScanRec {int x, y; float dx, dy;}; d_grid holds float2
RGN_LDS_POINTS = 32768  # twflow_kernels.hip.h: grids above it keep tw_hit_regions' label plane in d_lab

VEC = np.dtype([("x", "<i4"), ("y", "<i4"), ("dx", "<f8"), ("dy", "<f8")])  # tw_vector
assert VEC.itemsize == C.sizeof(T.Vector)


def round_up(v, m):
    return (v + m - 1) // m * m


# ---- the staging sizes, as csrc/twflow.hip computes them ----------------------------------------------------------------
def staged_image_bytes(w, h):
    """twflow.hip staged_image_bytes: a gray image's slot in d_img (256-byte aligned)"""
    return round_up(w * h, 256)


def flow_stage_slot(w, h):
    """twflow.hip flow_stage_slot: a pair's slot in d_fstage / d_istage"""
    return round_up(w * h * 8, 256)


def filtered_rows_slot(w, h, ch):
    """twflow.hip Submit::filt_need (png_rows_bytes): the slot of h filtered rows of 1 + w * ch bytes in d_filt — on a fresh
    engine (stage_png_rows takes max(filt_need, what the region already allows))"""
    return round_up(h * (1 + w * ch), 256)


def jpeg_coef_slot(w, h):
    """twflow.hip Submit::jpeg_coef_bytes: 128 bytes per stored 8 x 8 block"""
    return round_up(-(-w // 8) * -(-h // 8) * 128, 256)


def sized_target_slot(w, h):
    """twflow.hip stage of a sized host target: staged_image_bytes(w + 5, h + 5) per pair in d_tsrc"""
    return staged_image_bytes(w + 5, h + 5)


# ---- what a batch is made of ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Form:
    """What the pairs of a batch bring, as far as it decides which arrays exist."""
    images: str = "host"     # "host": gray host images (d_img); "device": the caller's device memory (no staging)
    rows_ch: int = 0         # > 0: filtered PNG rows of that many channels for both images (d_filt, and d_img behind them)
    jpeg: bool = False       # coefficient planes share the d_filt slots
    flow_out: bool = False   # every pair has a host flow destination (d_fstage)
    init: bool = False       # some pair has a host initial field (d_istage)
    sized: bool = False      # some host target comes at another size (d_tsrc)
    regions: bool = False    # TW_OPT_REGIONS (d_regof, d_lab)
    ramp: bool = False       # the batch goes out in the cold-start ramp's three pieces (slots / 4, slots / 4, the rest)
    filt_slot: int = 0       # bytes of a d_filt slot when the first filtered image of the batch is not rows_ch rows


Launch = collections.namedtuple("Launch", "base slots")  # index i of the launch holds batch slot slots[i], at base + i * bpp
Row = collections.namedtuple("Row", "name bytes_per_pair max_index max_offset alloc_bytes launches source")
Part = collections.namedtuple("Part", "lo hi lane plan rows")


class Table(list):
    """the rows, and `allocs`: {array: device bytes of its allocation} — every array the engine allocates for the batch,
    whether a launch of this batch indexes it or not (M[1] exists even where every level runs tw_flow_iter)"""
    allocs = None


def crossings(row):
    """the powers of two the row's largest offset has reached"""
    return tuple(p for p in POWERS if row.max_offset >= p)


def _row(name, bpp, launches, alloc, source, table=None):
    if table is not None:
        table.allocs[name.split("@")[0].split(" as ")[0]] = int(alloc)
    launches = [Launch(int(b), list(s)) for b, s in launches if len(s)]
    mi = max(len(l.slots) for l in launches) - 1
    mo = max(l.base + (len(l.slots) - 1) * bpp for l in launches)
    return Row(name, int(bpp), mi, int(mo), int(alloc), launches, source)


def batch_parts(engine, w, h, span, npairs, form):
    """[Part]: the parts of the batch as enqueue_batch_levels walks them (a lane's half with TW_LANES=2, a piece of the
    ramp, or the whole batch), each with the engine's own level plan for it."""
    kw = dict(any_fout=form.flow_out, any_init=form.init)
    if form.ramp:
        q = engine.slots // 4
        bounds = [0, q, 2 * q, npairs]
        parts = []
        for lo, hi in zip(bounds, bounds[1:]):
            plan = engine.level_plan(w, h, span, hi - lo, **kw)
            assert len(plan.parts) == 1, "the ramp is the one-lane schedule's"
            parts.append(Part(lo, hi, 0, plan, plan.parts[0]))
        return parts
    plan = engine.level_plan(w, h, span, npairs, **kw)
    n, parts = len(plan.parts), []
    for lane, rows in enumerate(plan.parts):
        lo, hi = npairs * lane // n, npairs * (lane + 1) // n  # (enqueue_batch_levels: n * lane / nlanes)
        assert rows[0].pairs == hi - lo, (rows[0], lo, hi)
        parts.append(Part(lo, hi, lane, plan, rows))
    return parts


def level_launches(part, k):
    """[(j0, nc)] of level k in this part: `per` pairs a launch, the last one the tail"""
    r = part.rows[k]
    out = [(j0, min(r.per, part.hi - j0)) for j0 in range(part.lo, part.hi, r.per)]
    assert len(out) == r.launches and out[-1][1] == r.tail, (r, out)
    return out


def byte_table(engine, w, h, span, npairs, form, level_sizes=None):
    """One Row per batch-indexed device array of a batch of `npairs` pairs of w x h at `span` on this engine.
    level_sizes: [(w_k, h_k)] of the pyramid, level 0 first (default: the oracle's level plan; the engine exports the count only)."""
    p, cap = engine.params, min(engine.slots, CAP_MAX)
    if level_sizes is None:
        import oracle
        level_sizes = [(lv.width, lv.height) for lv in oracle.level_plan(w, h, p.pyrScale, p.pyrLevels)]
    levels = engine.num_levels(w, h)
    assert levels == len(level_sizes) - 1 and tuple(level_sizes[0]) == (w, h)
    parts = batch_parts(engine, w, h, span, npairs, form)
    lanes = len(parts) if not form.ramp else 1
    lanes_alloc = 2 if lanes == 2 else 1  # (TW_LANES=2 engines: reserve_workspace multiplies by e->lanes)
    ps = [round_up(lw, 32) * lh for lw, lh in level_sizes]       # plan_geometry: L.ld = round_up(L.w, 32); L.ps = L.ld * L.h
    chunk = [engine.level_chunk(w, h, k) for k in range(levels + 1)]
    ws_lane = max(ps[k] * 2 * chunk[k] for k in range(levels + 1))  # choose_level_schedule: s.ws_lane (floats of I)
    need = ws_lane * lanes_alloc                                    # reserve_workspace: need *= e->lanes
    box = not (p.flags & 256)                                       # OPTFLOW_FARNEBACK_GAUSSIAN = 256; without it the box window
    it = p.pyrIterations
    rows = Table()
    rows.allocs = {"I": need * 4 + 256, "R": need * 20 + 256, "M[0]": need // 2 * 20 + 256, "M[1]": need // 2 * 20 + 256}
    if box:
        rows.allocs["Vd"] = need // 2 * 5 * 8 + 256

    def ws(name, k, planes, elem, lane_floats, alloc, source, want):
        """a lane-workspace array at level k: the launches of every part that `want`s it, index = z inside the launch"""
        ls = [(lane_floats * part.lane * elem, range(j0, j0 + nc))
              for part in parts if want(part.rows[k]) for j0, nc in level_launches(part, k)]
        if ls:
            rows.append(_row("%s@L%d" % (name, k), planes * ps[k] * elem, ls, alloc, source))

    for k in range(levels + 1):
        every = lambda r: True                      # noqa: E731
        mats = lambda r: not r.flow_iter            # noqa: E731  (tw_update_matrices + the window kernels)
        ws("I", k, 2, 4, ws_lane, need * 4 + 256, "make_chunk: e->I + ws_lane * lane; images 2z, 2z + 1 at stride ps", every)
        ws("R", k, 10, 4, ws_lane * 5, need * 20 + 256, "make_chunk: e->R + ws_lane * 5 * lane; z * 2 * 5 * ps", every)
        ws("M[0]", k, 5, 4, ws_lane // 2 * 5, need // 2 * 20 + 256, "make_chunk: e->M[0] + ws_lane / 2 * 5 * lane; z * 5 * ps", mats)
        ws("M[1]", k, 5, 4, ws_lane // 2 * 5, need // 2 * 20 + 256, "make_chunk: e->M[1] + ws_lane / 2 * 5 * lane; z * 5 * ps", mats)
        if it >= 2:  # enqueue_flow_iter_chain: the iterations ping-pong between the level's flow buffer and M0
            ws("M[0] as flow", k, 2, 4, ws_lane // 2 * 5, need // 2 * 20 + 256,
               "enqueue_flow_iter_chain: buf[1] = ch.M0, z * 2 * ps", lambda r: r.flow_iter)
        if k == 0:   # tw_pyr_k3f leaves level 0's images in the M1 region (enqueue_level_images: Iside = ch.M1)
            ws("M[1] as images", k, 2, 4, ws_lane // 2 * 5, need // 2 * 20 + 256,
               "enqueue_level_images: Iside = ch.M1, images 2z, 2z + 1 at stride ps", lambda r: r.images == 1)
        if box:
            ws("Vd", k, 5, 8, ws_lane // 2 * 5, need // 2 * 5 * 8 + 256, "make_chunk: e->Vd + ws_lane / 2 * 5 * lane; z * 5 * ps doubles", mats)
        if k == 0:   # make_chunk: flow[0] + lane * chunk * 2 * ps, index z; reserve_workspace: ps * 2 * chunk * lanes floats
            ls = [(part.lane * chunk[0] * 2 * ps[0] * 4, range(j0, j0 + nc)) for part in parts for j0, nc in level_launches(part, 0)]
            rows.append(_row("flow[0]", 2 * ps[0] * 4, ls, ps[0] * 2 * chunk[0] * lanes_alloc * 4 + 256,
                             "make_chunk: e->flow[0] + lane * chunk * 2 * ps; z * 2 * ps", rows))
        else:        # make_chunk: flow[k] + j0 * 2 * ps: the batch index
            rows.append(_row("flow[%d]" % k, 2 * ps[k] * 4, [(0, range(npairs))], ps[k] * 2 * cap * 4 + 256,
                             "make_chunk: e->flow[k] + j0 * 2 * ps; (j0 + z) * 2 * ps", rows))
    whole = [(0, range(npairs))]
    if span > 0:
        G = T.grid_capacity(w, h, span)
        rows.append(_row("d_grid", G * FLOAT2_BYTES, whole, G * cap * FLOAT2_BYTES + 256, "grid_of: e->d_grid + j0 * gw * gh", rows))
        rows.append(_row("d_rec", G * SCANREC_BYTES, whole, G * cap * SCANREC_BYTES + 256, "tw_span_scan: rec + z * rec_zs (G records)", rows))
        if form.regions:
            rows.append(_row("d_regof", G * 4, whole, G * cap * 4 + 256, "tw_hit_regions: region_of + z * G", rows))
            if G > RGN_LDS_POINTS:
                rows.append(_row("d_lab", G * 4, whole, G * cap * 4 + 256, "tw_hit_regions<false>: lab + z * G", rows))
    npx = staged_image_bytes(w, h)
    if form.images == "host":
        rows.append(_row("d_img", 2 * npx, whole, npx * 2 * cap + 256, "d_img + npx * (2 * j + q)", rows))
    if form.rows_ch or form.jpeg or form.filt_slot:
        slot = form.filt_slot or (filtered_rows_slot(w, h, form.rows_ch) if form.rows_ch else jpeg_coef_slot(w, h))
        rows.append(_row("d_filt", 2 * slot, whole, slot * 2 * cap + 512, "stage_png_rows: d_filt + filt_slot * (2 * j + q)", rows))
    if form.sized:
        slot = sized_target_slot(w, h)
        rows.append(_row("d_tsrc", slot, whole, slot * cap + 512, "stage_png_rows: d_tsrc + tsrc_slot * j", rows))
    fslot = flow_stage_slot(w, h)
    if form.flow_out:
        rows.append(_row("d_fstage", fslot, whole, fslot * cap + 256, "export_chunk: d_fstage + fslot * j", rows))
    if form.init:
        rows.append(_row("d_istage", fslot, whole, fslot * cap + 256, "stage of a host field: d_istage + fslot * jobs.size()", rows))
    return rows


def single_pair_buffers(engine, level_sizes):
    """bytes of lat_I + lat_R (reserve_workspace: need_lat = sum of 2 * ps floats; not indexed by a pair), which every
    engine with TW_LATENCY_STREAMS (the default) allocates with its first batch"""
    need_lat = sum(round_up(lw, 32) * lh * 2 for lw, lh in level_sizes)
    return (need_lat * 4 + 256) + (need_lat * 20 + 256)


def table_alloc_bytes(rows):
    """the device bytes of the arrays of a byte_table, each allocation once"""
    return sum(rows.allocs.values())


def format_table(rows, title=""):
    out = ["| array | bytes per pair | largest index | largest offset | crosses |", "|---|---|---|---|---|"]
    for r in rows:
        cr = ", ".join("2^%d" % (p.bit_length() - 1) for p in crossings(r))
        out.append("| `%s` | %d | %d | %d | %s |" % (r.name, r.bytes_per_pair, r.max_index, r.max_offset, cr or "-"))
    return (title + "\n" if title else "") + "\n".join(out)


# ---- a wrap cannot hide ----------------------------------------------------------------------------------------------------
def reductions(off):
    """what a truncated or wrapped offset may have lost: 2^31, 2^32, 2^33 and every multiple of 2^32, as far as off reaches"""
    return sorted({p for p in POWERS if p <= off} | set(range(P32, off + 1, P32)))


def hidden_wraps(rows, K):
    """[(row, launch base, index, slot, lost, the slot it lands on)]: the offsets of the table that could lose a power of two
    and still address the same distinct pair at the same place inside a slot.  Also the chunk buffers a later launch reuses
    at an index that held the same pair (a store that went astray would leave the earlier launch's equal bytes there)."""
    bad = []
    for r in rows:
        b = r.bytes_per_pair
        for li, l in enumerate(r.launches):
            for i, s in enumerate(l.slots):
                off = l.base + i * b
                if off < P31:
                    continue
                for lost in reductions(off):
                    for m in r.launches:  # where the reduced offset lands, in any launch's index space of this array
                        d = off - lost - m.base
                        if d >= 0 and d % b == 0 and d // b < len(m.slots) and m.slots[d // b] % K == s % K:
                            bad.append((r.name, l.base, i, s, lost, m.slots[d // b]))
                # the stale bytes at this index: what the latest earlier launch at the same base left there
                prev = [m for m in r.launches[:li] if m.base == l.base and i < len(m.slots)]
                if prev and prev[-1].slots[i] % K == s % K:
                    bad.append((r.name, l.base, i, s, 0, prev[-1].slots[i]))
    return bad


def assert_wrap_cannot_hide(rows, K):
    bad = hidden_wraps(rows, K)
    assert not bad, "K = %d: a wrapped offset would find the same pair (array, base, index, slot, lost, lands on): %r — choose another K" % (K, bad[:4])


# ---- the distinct pairs ----------------------------------------------------------------------------------------------------
_PAIRS = {}
WORKERS = 8  # threads for the oracle and the image synthesis (both leave the interpreter lock for most of their time)


def in_threads(fn, items):
    """[fn(x) for x in items] on a few threads"""
    import concurrent.futures
    items = list(items)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(WORKERS, len(items)))) as ex:
        return list(ex.map(fn, items))


def distinct_pairs(w, h, K):
    """synth.make_pair(i, h, w) for i < K (K odd: 5 or 7; 3 for the cases that need no identical pair): kinds 0, 1,
    2 (painted rectangle), 3 (identical: tw_pair_same), 0, ..."""
    import synth
    assert K in (3, 5, 7)
    todo = [i for i in range(K) if (w, h, i) not in _PAIRS]
    for i, pr in zip(todo, in_threads(lambda i: tuple(np.ascontiguousarray(x) for x in synth.make_pair(i, h, w)), todo)):
        for x in pr:
            x.flags.writeable = False
        _PAIRS[(w, h, i)] = pr
    ps = [_PAIRS[(w, h, i)] for i in range(K)]
    assert not np.array_equal(ps[2][0], ps[2][1]) and (K == 3 or np.array_equal(ps[3][0], ps[3][1]))
    assert len({a.tobytes() + b.tobytes() for a, b in ps}) == K, "the pairs are not distinct"
    return ps


def smallest_shape_for_images_past_2_32(slots=CAP_MAX):
    """The smallest 16:9 size at which the largest offset of d_img (2 * slots gray images) reaches 2^32: 8.4 Mpixel.  The
    coarser levels' flow[1] (indexed by the batch slot) and, at span 1, d_regof and d_lab pass 2^32 there as well."""
    k = 1
    while (slots - 1) * 2 * staged_image_bytes(16 * k, 9 * k) < P32:
        k += 1
    return 16 * k, 9 * k


def smallest_shape_for_sized_targets_past_2_32(slots=CAP_MAX):
    """The smallest 16:9 size at which the largest offset of d_tsrc (one slot of (w + 5) x (h + 5) bytes a pair) reaches
    2^32: 16.8 Mpixel."""
    k = 1
    while (slots - 1) * sized_target_slot(16 * k, 9 * k) < P32:
        k += 1
    return 16 * k, 9 * k


def smallest_shape_past_2_32(slots=CAP_MAX, ch=4):
    """The smallest 16:9 size (16 k x 9 k) at which the largest offsets of d_filt (2 * slots images of `ch`-channel rows) and
    of d_fstage (slots flow slots) both reach 2^32."""
    k = 1
    while True:
        w, h = 16 * k, 9 * k
        if (2 * slots - 1) * filtered_rows_slot(w, h, ch) >= P32 and (slots - 1) * flow_stage_slot(w, h) >= P32:
            return w, h
        k += 1


# ---- reading a batch back without a Python loop per vector -------------------------------------------------------------------
def vectors_array(vecs):
    """a list of (x, y, dx, dy) as a VEC array"""
    a = np.zeros(len(vecs), VEC)
    if vecs:
        v = np.array(vecs, np.float64)
        a["x"], a["y"], a["dx"], a["dy"] = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    return a


def wait_array(e, ticket, buf):
    """tw_wait into `buf` (a VEC array of a grid's worth): the pair's vectors as a view of it"""
    n, sec = C.c_int(), C.c_float()
    e._check(e._L.tw_wait(e._h, ticket[0], buf.ctypes.data_as(C.POINTER(T.Vector)), len(buf), C.byref(n), C.byref(sec)))
    assert 0 <= n.value <= len(buf)
    return buf[:n.value]


def wait_regions_arrays(e, ticket, buf, rof_buf, regs_buf):
    """tw_wait_regions into the caller's arrays (VEC, int32 and twflow.REGION_DTYPE): views of the pair's vectors, their
    region_of and the kept records, and the pair's true number of regions"""
    n, nreg, sec = C.c_int(), C.c_int(), C.c_float()
    e._check(e._L.tw_wait_regions(e._h, ticket[0], buf.ctypes.data_as(C.POINTER(T.Vector)), len(buf), C.byref(n),
                                  rof_buf.ctypes.data_as(C.POINTER(C.c_int)), regs_buf.ctypes.data_as(C.POINTER(T.Region)),
                                  len(regs_buf), C.byref(nreg), C.byref(sec)))
    assert 0 <= n.value <= len(buf) and nreg.value >= 0
    return buf[:n.value], rof_buf[:n.value], regs_buf[:min(nreg.value, len(regs_buf))], nreg.value


def regions_arrays(records, region_of):
    """the reference's (records, region_of) of regions_ref.regions as (kept records in twflow.REGION_DTYPE, int32 region_of)"""
    kept = np.zeros(min(len(records), T.MAX_REGIONS), T.REGION_DTYPE)
    for i, rec in enumerate(records[:len(kept)]):
        kept[i] = tuple(rec)
    return kept, np.array(region_of, np.int32)


def first_wrong_slot(got, want_of_slot, what):
    """got: per slot a VEC array (or any array); want_of_slot(s): the expected one.  Names the first slot that differs."""
    for s, g in enumerate(got):
        w_ = want_of_slot(s)
        if g.shape != w_.shape or not np.array_equal(g, w_):
            n = min(len(g), len(w_))
            diff = np.nonzero(g[:n] != w_[:n])[0]
            where = int(diff[0]) if len(diff) else n
            raise AssertionError("%s: slot %d is the first that differs from the oracle (%d values, want %d; first at %d: got %r want %r)" %
                                 (what, s, len(g), len(w_), where, g[where:where + 1], w_[where:where + 1]))
