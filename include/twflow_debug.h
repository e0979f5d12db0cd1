/*
 * twflow_debug.h — DIAGNOSTIC entry points of libtwflow.so.  NOT part of the drop-in boundary (include/twflow.h): no
 * interface of the reference corresponds to them, a consumer of the library never needs them, and they may change
 * without an ABI version bump.  They exist for this repository's own tests and tools and are declared here so that
 * every symbol the product library exports is declared in include/ (hygiene).
 */
#ifndef TWFLOW_DEBUG_H
#define TWFLOW_DEBUG_H

#include "twflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of captured single-pair schedules (hipGraphs, TW_LAT_GRAPH=1) this engine holds; -1 for a null engine.
 * tests/test_gpu_parity.py uses it to prove that the graph path is what really ran. */
int tw_debug_graphs(tw_engine* e);

/* The size predicate of every submit and every tw_stage_* entry point, without a device: TW_OK when a width x height
 * image is admitted, TW_E_BAD_PARAMETER outside 1 .. 32768 pixels per side, TW_E_UNSUPPORTED when round_up(width, 32) *
 * height exceeds (2^32 - 1) / 20 = 214 748 364 — the five float planes that one raw buffer resource with 32-bit offsets
 * addresses in the stencil kernels (tests/test_abi.py). */
tw_status tw_debug_check_size(int width, int height);

/* "kernel name: workgroups per CU" lines of the main kernels as the runtime admits them (tools/kbench.py).
 * Returns the number of bytes written to buf (at most cap, NUL-terminated). */
int tw_debug_occupancy(char* buf, int cap);

/* TW_DEBUG_STAMPS=1 runs only: the s_memtime phase stamps of the last tw_pyr_taps launch, 64 workgroups x 4 stamps
 * into out[256]; returns 256, or 0 when no stamps were taken.  No output value of the library depends on them. */
int tw_debug_stamps(tw_engine* e, unsigned long long* out);

/* The first n (<= 4096) entries of the same buffer: tw_flow_iter's phase stamps in the variants library
 * ([workgroup 0..31][wave 0 / 9][step 40..47][stamp 0..7]; tools/fi_stamps.py). */
int tw_debug_stamps_ex(tw_engine* e, unsigned long long* out, int n);

/* The yardstick of bench.py's `frac_of_measured_copy`: `reps` launches of a float4 device-to-device copy kernel over
 * `bytes` (16 B per lane per iteration, grid-stride; read + write counted) on the engine's stream, in GB/s. */
tw_status tw_debug_copy_rate(tw_engine* e, size_t bytes, int reps, double* gbps);

/* Kernel families of tw_debug_launch_counts: every kernel launch of the library is counted under exactly one of them
 * (the copy-rate yardstick excepted).  A test that claims to exercise a kernel asserts its family's count. */
enum tw_debug_family {
    TW_DF_PYR_K3 = 0,      /* tw_pyr_k3<0 / 2>: one 3-tap pyramid level */
    TW_DF_PYR_K3F,         /* tw_pyr_k3f: levels 0 + 1 from one read */
    TW_DF_PYR_23,          /* tw_pyr_23: levels 2 + 3 from one read */
    TW_DF_PYR_TAPS,        /* tw_pyr_taps<KS>: 7 .. 63-tap levels */
    TW_DF_PYR_LEVEL,       /* tw_pyr_level / tw_pyr_level_lds: the generic levels */
    TW_DF_POLYEXP,         /* tw_polyexp_pk / tw_polyexp / tw_polyexp_band */
    TW_DF_UPDATE_MATRICES, /* tw_update_matrices<UPSAMPLE, NY> */
    TW_DF_FLOW_ITER,       /* tw_flow_iter<15, 0>: a whole iteration, input flow from memory */
    TW_DF_FLOW_ITER_UPS,   /* tw_flow_iter<15, 1>: first iteration of a level, the coarser flow upsampled in place */
    TW_DF_FLOW_ITER_ZERO,  /* tw_flow_iter<15, 2>: first iteration of the coarsest level (zero flow) */
    TW_DF_BLUR_SOLVE4,     /* tw_blur_solve4<...>: 31-tap (and variants' 51-tap) window tiles */
    TW_DF_BLUR_SOLVE4Y,    /* tw_blur_solve4y: two sub-tiles per workgroup (51-tap default on wide levels) */
    TW_DF_BLUR_SOLVE8,     /* tw_blur_solve8: packed-f32 window kernel (51-tap narrow levels) */
    TW_DF_BLUR_PP,         /* tw_blur_solve_pp: plane-parallel small-grid kernel */
    TW_DF_BLUR_GENERIC,    /* tw_blur_solve_generic: any other window size */
    TW_DF_BLUR_VARIANT,    /* variants library only: tw_blur_solve4q / 4p / 6 */
    TW_DF_BLUR_GRID,       /* tw_blur_grid: scan-fused final iteration */
    TW_DF_BOX,             /* tw_box_vscan / tw_box_hscan_solve */
    TW_DF_TWIN,            /* tw_twin_*: two bodies in one launch (single-pair schedule; tw_twin_s4_poly since round 6) */
    TW_DF_SPAN_GATHER,
    TW_DF_SPAN_SCAN,
    TW_DF_PNG_UNFILTER,
    TW_DF_SPAN_SCAN_SEG,   /* tw_span_scan_seg: a single pair's ordered scan in 16 independent segments (round 6) */
    TW_DF_BAND_ROWS,       /* tw_band_rows: a batch part's row signatures of both images, 64 columns per entry (TW_OPT_SHIFT_BANDS) */
    TW_DF_BAND_SEARCH,     /* tw_band_search: each band's best vertical shift, from the signatures (TW_OPT_SHIFT_BANDS) */
    TW_DF_BAND_VERIFY,     /* tw_band_verify<0> + <1>: each band's pixel sums at (0, 0) and at its shift, then areas and `applied` — two launches per part (TW_OPT_SHIFT_BANDS) */
    TW_DF_FLOW_BAND_INIT,  /* tw_flow_band_init: a coarsest-level chunk's first flow from the bands, in tw_flow_shift_init's place (TW_OPT_SHIFT_BANDS; the
                            * four here, in front of TW_DF_BLUR_SOLVE4Q: the chain from there to TW_DF_COUNT is pinned by tests, nothing in front of it is) */
    TW_DF_BLUR_SOLVE4Q,    /* tw_blur_solve4q: solve + refresh by the horizontal item's owner — a single pair's level-0 launches (round 6) */
    TW_DF_OVERLAY_BASE,    /* tw_overlay_base: one pair's diff image, the base layer (tw_ticket_overlay) */
    TW_DF_OVERLAY_MARKS,   /* tw_overlay_marks<0> the region boxes, <1> the vectors: one launch each, only when the pair has any (both in
                            * front of TW_DF_PYR_LEVEL_LDS for the reason it stands here itself: no pinned neighbourhood moves) */
    TW_DF_PYR_LEVEL_LDS,   /* tw_pyr_level_lds: the generic level with its source region staged in LDS — ALSO counted in TW_DF_PYR_LEVEL.
                            * (Here and not at the end: the enum's tail from TW_DF_HIT_REGIONS on is pinned by the tests of the features that added it) */
    TW_DF_SHIFT_PROFILES,  /* tw_shift_profiles: a batch part's row and column sums of both images (TW_OPT_SHIFT) */
    TW_DF_SHIFT_SEARCH,    /* tw_shift_search: each pair's best integer shift per axis, from the profiles (TW_OPT_SHIFT) */
    TW_DF_SHIFT_VERIFY,    /* tw_shift_verify<0> + <1>: the pixel sums at (0, 0) and at the shift, then areas and `applied` — two launches per part (TW_OPT_SHIFT) */
    TW_DF_FLOW_SHIFT_INIT, /* tw_flow_shift_init: a coarsest-level chunk's first flow of the pairs whose shift was applied (TW_OPT_SHIFT; the four
                            * here, in front of TW_DF_WARP_RESIDUAL, for the reason TW_DF_PYR_LEVEL_LDS is: no pinned neighbourhood moves) */
    TW_DF_WARP_RESIDUAL,   /* tw_warp_residual: a level-0 chunk's differing pixels against the target sampled along the final flow (TW_OPT_RESIDUAL) */
    TW_DF_CHANGE_SCAN,     /* tw_change_scan: a batch's cells with a differing pixel, compacted in order behind its ordered scan (TW_OPT_RESIDUAL;
                            * both here for the reason TW_DF_PYR_LEVEL_LDS is) */
    TW_DF_FLOW_ITER_GRID,  /* tw_flow_iter<15, 3>: a batch's last level-0 iteration at the span-grid points only — ALSO counted in TW_DF_FLOW_ITER */
    TW_DF_HIT_REGIONS,     /* tw_hit_regions: the connected components of a batch's hits, behind its ordered scan (TW_OPT_REGIONS) */
    TW_DF_JPEG_IDCT,       /* tw_jpeg_idct: a batch's JPEG luma blocks -> gray images (tw_submit_jpeg) */
    TW_DF_MASK_RECTS,      /* tw_mask_rects: a batch's ignore rectangles, expected image -> target (tw_submit_*_ignore) */
    TW_DF_PAIR_SAME,       /* tw_pair_same: which pairs of a batch part have two byte-identical images */
    TW_DF_RESIZE_U8,       /* tw_resize_u8: a target within 5 px of its pair's size -> the pair's size (tw_submit_*_sized) */
    TW_DF_FLOW_INIT,       /* tw_flow_area_init: tw_submit_*_flow_init fields -> the coarsest level's first flow (zeros without one) */
    TW_DF_FLOW_EXPORT,     /* tw_flow_export: a level-0 chunk's final flow -> the pairs' tw_submit_*_flow destinations */
    TW_DF_COUNT
};

/* Launches per kernel family on this engine since it was created or the counts were last reset: counts[0 .. min(n,
 * TW_DF_COUNT) - 1]; last_z (may be NULL) receives the grid z (pairs or images) of each family's latest launch.
 * reset != 0 zeroes the counters after copying them.  Returns TW_DF_COUNT, -1 for a null engine. */
int tw_debug_launch_counts(tw_engine* e, unsigned long long* counts, unsigned long long* last_z, int n, int reset);

/* The geometry of one tw_flow_iter launch of npairs pairs at a level of width x height pixels, from the one function the
 * launch itself takes its grid from: out[0] strips (grid x), out[1] row segments per strip (grid y), out[2] steps of 5 rows
 * per segment, out[3] steps of the last segment.  It depends on the engine's CU count and on TW_FI_MAXSEG / TW_FI_MINSTEPS
 * as tw_engine_create read them.  Returns the number of values written (at most min(n, 4); 0 for a null `out` or a
 * non-positive size), -1 for a null engine.  tests/test_gpu_flow_iter_geometry.py proves from it which geometry ran. */
int tw_debug_flow_iter_plan(const tw_engine* e, int width, int height, int npairs, int* out, int n);

/* The choice of one window average + solve launch of npairs pairs at a level of width x height pixels, from the one function
 * the launch itself takes its kernel and grid from (choose_blur): out[0] the kernel's family (tw_debug_family), out[1] threads
 * per workgroup, out[2] tile columns, out[3] rows per workgroup, out[4] xsh (pixels the tile grid starts left of the image),
 * out[5] grid x, out[6] grid y, out[7] the 31-tap window's small-grid class (0: 224 x 8 / 96 x 8 tiles, 1: 96 x 8 two-wave tiles
 * on a wide level, 2: 96 x 4, 3: 32 x 4, 4: plane-parallel 32 x 8, 5: plane-parallel 96 x 8), out[8] 1 when TW_BLUR_SMALL /
 * TW_BLUR_SMALL_LEVELS set that class, 0 when the grid's size did.  `level` is the pyramid level (-1: a tw_stage_* call),
 * `update` whether the launch refreshes M, `quads` whether the caller is the single-pair schedule.  A launch that carries a
 * side job (TW_DF_TWIN) keeps this geometry for its own part.  The box window reports tw_box_vscan's block, columns and grid.
 * Returns the number of values written (at most min(n, 9); 0 for a null `out` or a non-positive size), -1 for a null engine.
 * tests/test_gpu_blur_dispatch.py proves from it which side of each edge of the choice ran. */
int tw_debug_blur_plan(const tw_engine* e, int width, int height, int level, int npairs, int update, int quads, int* out, int n);

/* The choice of one pyramid level's launch at `level` of a width x height image whose rows are `stride` bytes apart, from the
 * one function the launch itself takes its kernel, grid and LDS size from (choose_pyr), and the plan's two fusion decisions:
 * out[0] the kernel (0: tw_pyr_k3, 3: tw_pyr_taps, 4: tw_pyr_level_lds, 5: tw_pyr_level; 1 = tw_pyr_k3f and 2 = tw_pyr_23 are
 * never a level's own launch), out[1] its template argument (tw_pyr_k3: the resize mode 0 / 2; tw_pyr_taps: KS = 9 / 19 / 39, or
 * 0 for the any-size instantiation; 0 otherwise), out[2] the launch-count family (tw_debug_family; a tw_pyr_level_lds launch
 * is counted in TW_DF_PYR_LEVEL and in TW_DF_PYR_LEVEL_LDS, and this reports the latter), out[3] threads per workgroup,
 * out[4] output-tile columns, out[5] output-tile rows, out[6] grid x, out[7] grid y, out[8] dynamic LDS bytes, out[9] bytes per
 * staged source row (0: the kernel stages none), out[10] 1 when the kernel may load whole dwords of the source rows of
 * images at 4-byte-aligned addresses — the answer is for such images, as a tw_stage_* call's and every staged host image are, so
 * `stride` a multiple of 4 decides; a batch of device images at other addresses takes the byte path whatever this says, and no
 * launch changes the answer; always 0 for tw_pyr_level, which takes no such argument); the level: out[11] width,
 * out[12] height, out[13] taps of its smoothing kernel, out[14] resize mode (0: same size, 1: INTER_LINEAR, 2: exact 2 x 2
 * area), out[15] xmax (output columns from xmax on take a single tap), out[16] the row-buffer height the kernel is given; the
 * size: out[17] 1 when levels 3 and 2 may come from one tw_pyr_23 launch (Plan::fused23), out[18] 1 when levels 1 and 0 may come
 * from one tw_pyr_k3f launch (pyr01_fusable), out[19] / out[20] threads of a tw_pyr_23 workgroup for a launch of at most two /
 * of more images, out[21] the index of the coarsest level, out[22] the output rows whose lower source row is clipped to the image's
 * last row (only a level as high as the image but narrower has any; one as wide but lower has xmax < width).  It depends on TW_PYR_GENERIC, TW_PYR_GEN_TH and TW_PYR23_THREADS
 * as tw_engine_create read them.  Returns the number of values written (at most min(n, 23); 0 for a null `out`,
 * a size without a plan or a level the plan does not have), -1 for a null engine.  tests/test_gpu_pyr_dispatch.py proves from
 * it which side of each edge of the choice ran (tests/pyr_cases.py, profiles/pyr_dispatch.md). */
int tw_debug_pyr_plan(const tw_engine* e, int width, int height, int level, long long stride, int* out, int n);

/* The choice of the ordered scan's launch for npairs pairs of width x height pixels at `span`, from the one function the
 * launch itself takes its kernel from (choose_scan): out[0] the kernel (0: tw_span_scan, one workgroup per pair; 1:
 * tw_span_scan_seg, one workgroup per segment), out[1] gw, out[2] gh, out[3] G = gw * gh grid points, out[4] S, the points of
 * a segment, out[5] segments (S and segments are 0 for kernel 0), out[6] rounds of 32 768 points a workgroup runs (1 for
 * kernel 1).  `single_pair`: whether the batch takes the single-pair schedule (a batch of one pair of at least
 * TW_LATENCY_MIN_PX = 100 000 pixels does, unless TW_LATENCY_STREAMS=0); TW_SCAN_SEG is read at the call, as every batch reads it.  Returns the number of values
 * written (at most min(n, 7); 0 for a null `out`, a non-positive size, span or pair count), -1 for a null engine.
 * tests/test_gpu_span_scan.py takes its grids' seams from it. */
int tw_debug_scan_plan(const tw_engine* e, int width, int height, int span, int npairs, int single_pair, int* out, int n);

/* What a batch of npairs pairs of width x height pixels at `span` launches for each pyramid level, from the one function the
 * enqueue itself executes (choose_level_schedule).  traits: 1 a pair has a flow destination, 2 a pair has an initial field (or the batch was opened with TW_OPT_SHIFT on: the same schedule),
 * 4 a profiling class is selected, 8 the single-pair buffers do not exist, 16 the batch was opened with TW_OPT_RESIDUAL on.  out[0] the schedule (0: level-major batch, 1: one
 * pair on two streams, 2: one pair, twin launches), out[1] lanes, out[2] the coarsest level's index L, out[3] 1 when a single
 * pair's window launches take tw_blur_solve4q, out[4] 1 when the last level-0 iteration is the scan-fused one (tw_blur_grid),
 * out[5] 1 when level-0 launches that run tw_flow_iter end in the grid-only iteration, out[6] parts P (a lane's share of the
 * batch each; the pieces of a cold-start ramp are not known in advance), out[7] = 11 values per row; then P x (L + 1) rows,
 * part-major, level 0 first: [0] pairs of the part, [1] pairs per launch, [2] launches, [3] pairs of the last launch, [4] where
 * the level's images come from (0: a pyramid launch of its own, 1: the coarser level's launch wrote them, 2: its launch writes
 * the next finer level's too — tw_pyr_23 at level 3, tw_pyr_k3f at level 1), [5] 1 when the level starts from
 * tw_flow_area_init's output, [6] 1 when a launch of [1] pairs runs tw_flow_iter, [7] 1 when the identical-pair flags apply to
 * it, [8] / [9] the same for the last launch, [10] 1 when the flags apply to the part's tw_pyr_k3f launch.  TW_LAT_QUADS and
 * TW_GRID_FINAL are read at the call, as every batch reads them.  Returns the number of values written (at most n; 0 for a
 * null `out`, a non-positive size or pair count, a negative span or a size without a plan), -1 for a null engine.
 * tests/test_gpu_level_plan.py predicts every family's launches from it. */
int tw_debug_level_plan(const tw_engine* e, int width, int height, int span, int npairs, int traits, int* out, int n);

/* How tw_shift_search runs for a pair of width x height pixels at search radius `radius` (TW_OPT_SHIFT), a pure function of its
 * arguments (no engine): out[0] 1 when the x axis (the column profiles, length width) keeps both profiles in LDS, out[1] the
 * same for the y axis (the row profiles, length height), out[2] / out[3] the radius r = min(radius, L / 2) searched per axis,
 * out[4] grid x (the axes), out[5] threads per workgroup, out[6] the LDS budget in bytes (an axis stays in LDS while 8 * L fits
 * it), out[7] / out[8] tw_shift_profiles' grid x / y, out[9] tw_shift_verify<0>'s grid x.  Returns the number of values written
 * (at most min(n, 10); 0 for a null `out`, a non-positive size or a radius outside 1 .. 1024).  tests/test_gpu_shift.py takes
 * the lengths above the LDS limit from it. */
int tw_debug_shift_plan(int width, int height, int radius, int* out, int n);

/* How the band launches run for a pair of width x height pixels at search radius `radius` and band height `band`
 * (TW_OPT_SHIFT_BANDS), a pure function of its arguments (no engine): out[0] nb = ceil(height / band), out[1] nblk at dx = 0 =
 * ceil(width / 64), out[2] 1 when tw_band_search stages a band's signatures in LDS, out[3] the bytes that takes — 2 * nblk *
 * (rows + min(height, rows + 2 r)) with rows = min(band, height), r = min(radius, height / 2) — out[4] the LDS budget in bytes
 * (staged while out[3] <= out[4]), out[5] r, out[6] tw_band_rows' grid x (grid z = the images), out[7] tw_band_search's
 * threads per workgroup (grid: nb x pairs), out[8] tw_band_verify<0>'s grid x (chunks of 16 rows).  Returns the number of
 * values written (at most min(n, 9); 0 for a null `out`, a non-positive size, a radius outside 1 .. 1024 or a band height that
 * TW_OPT_SHIFT_BANDS refuses). */
int tw_debug_band_plan(int width, int height, int radius, int band, int* out, int n);

/* How tw_overlay_base runs for a width x height pair whose images lie at the addresses `expect` and `target` with rows `stride`
 * bytes apart, into a destination at the address `dst` with rows `pitch` bytes apart — a pure function of its arguments (no
 * engine, no device), the one the launch itself asks (choose_overlay): out[0] 1 when a lane loads one dword of each image and
 * stores three (all three addresses, the stride and the pitch are multiples of 4), 0 for the byte path; out[1] pixels per lane,
 * out[2] threads per workgroup, out[3] grid x, out[4] grid y.  Returns the number of values written (at most min(n, 5); 0 for
 * a null `out` or a non-positive size).  tests/test_gpu_overlay.py proves from it that both paths ran. */
int tw_debug_overlay_plan(unsigned long long expect, unsigned long long target, long long stride, unsigned long long dst,
                          long long pitch, int width, int height, int* out, int n);

/* A hit record as the ordered scan leaves it in device memory: what tw_stage_overlay takes. */
typedef struct tw_overlay_hit {
    int x, y;
    float dx, dy;
} tw_overlay_hit;

/* tw_overlay_base and tw_overlay_marks alone (include/twflow.h, "Diff image"), on host arrays: expect / target are height rows
 * of `stride` bytes, uploaded to device addresses `misalign` (0 .. 3) bytes behind a 256-byte boundary, so that a test reaches
 * the byte path; rects (n_rects <= TW_MAX_IGNORE) are clipped as a submit clips them; hits (n_hits >= 0, any values) and regions
 * (n_regions <= TW_MAX_REGIONS) are drawn as the header says, a hit inside a clipped rectangle left out.  `out` holds height
 * rows `pitch` bytes apart — pitch * height bytes, which go up before the launches and come back behind them, so the caller
 * sees every byte the kernels did not write as it was.  *path (nullable) receives the base kernel's path as
 * tw_debug_overlay_plan's out[0] names it.  The statuses of tw_ticket_overlay's argument check. */
tw_status tw_stage_overlay(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height, ptrdiff_t stride,
                           int misalign, const tw_rect* rects, int n_rects, const tw_overlay_hit* hits, int n_hits,
                           const tw_region* regions, int n_regions, int tol, uint8_t* out, ptrdiff_t pitch, int* path);

/* tw_pair_same's flags of the batch this engine enqueued last: out[j] = 1 where pair j's second image is byte for byte its
 * first over the visible width x height pixels (the batch schedule then computed that pair's polynomial expansions once at
 * the levels tw_flow_iter runs), 0 otherwise — and 0 for every pair of a batch that launched no tw_pair_same (TW_SAME_IMAGE=0,
 * the single-pair schedules).  Waits for the batch.  Returns the number of values written (at most min(n, pairs of that
 * batch); 0 for a null `out`), -1 for a null engine, -2 when the device refuses the wait or the copy (`out` then holds
 * zeros that are no flags).  Engine-level state: it describes whichever batch the engine enqueued LAST, not a ticket. */
int tw_debug_same_flags(tw_engine* e, unsigned* out, int n);

/* tw_png_unfilter alone on one image of any kind tw_stage_png_decode takes, event-timed: the rows go up once, the kernel
 * runs once untimed, then `iters` launches back to back between two events on the engine's stream; *avg_us = the time of
 * one (tools/e2e_files.py --kernel-time, profiles/png_kinds.md).  The statuses of tw_stage_png_decode. */
tw_status tw_debug_png_kernel_time(tw_engine* e, const tw_png_rows* img, int waves, int iters, float* avg_us);

/* Name of a family ("tw_flow_iter", ...), NULL past the end. */
const char* tw_debug_family_name(int family);

/* The library's own byte accounting of one engine (what it has allocated and still holds), for the leak test:
 *   out[0] device bytes (workspace, flow planes, batch contexts, tables, plans,
 *          the diff image's staging once a host destination was asked for)           out[1] page-locked host bytes it allocated
 *   out[2] cached plans                                                              out[3] bounce-buffer capacity (in out[1])
 *   out[4] entries of the process-wide page-lock table (tw_host_alloc / tw_host_register)   out[5] their bytes
 *   out[6] pooled profiling events                                                   out[7] captured single-pair graphs
 * Returns the number of values written (at most n), -1 for a null engine. */
int tw_debug_memory(tw_engine* e, unsigned long long* out, int n);

/* The resident image store of one engine (tw_image_*; its reserved bytes are in tw_debug_memory's out[0]):
 *   out[0] live images (blocks not yet back in the store)    out[1] bytes in use (blocks, each rounded up to 256)
 *   out[2] bytes reserved (the chunks)                        out[3] chunk allocations so far
 * Returns 4, -1 for a null engine or `out`. */
int tw_debug_resident(tw_engine* e, unsigned long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
