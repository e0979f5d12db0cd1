/*
 * twflow.h — C ABI of libtwflow.so, the MI355X (gfx950) Farneback image-diff engine.
 *
 * This is the drop-in boundary for tidal-wave's hot path.  It replaces
 *   - class OpticalFlow / OpticalFlowByCPU / OpticalFlowByGPU  (/root/reference/src/opticalflow.h:38-70,
 *     src/opticalflow.cpp:78-119) — the Farneback flow of one expect/target pair, and
 *   - the USE_GPU device selection and the span-grid threshold scan inside Consumer
 *     (/root/reference/src/consumer.cpp:18-32 and :60-76).
 * Everything is plain C: pointers and sizes, no C++/HIP/torch types.  No function throws or aborts
 * ("Node-gyp cannot use exceptions", src/opticalflow.h:18): every call returns a tw_status.
 *
 * Threading: a tw_engine is NOT thread-safe; create one per worker thread (the reference creates one
 * OpticalFlow per Consumer, src/consumer.cpp:27-35).  Different engines may be used concurrently from
 * different threads.  tw_engine_create binds the HIP device on the calling thread; every later call
 * re-binds it, so workers need not call hipSetDevice themselves (fixes the reference's main-thread
 * cv::gpu::setDevice, src/consumer.cpp:22).
 *
 * There is no CPU fallback in this library: without a HIP device every compute entry point returns
 * TW_E_DEVICE.
 */
#ifndef TWFLOW_H
#define TWFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): + tw_device_pci_bus_id, tw_host_register / tw_host_unregister, tw_has_variants, TW_OPT_POLYEXP_F32.
 * 3 (round 4): + tw_submit_png8 (PNG scanline reconstruction + gray conversion on the device).
 * 4 (rounds 5-6): + tw_stage_pyr_fused23 / tw_stage_pyr_fused01 / tw_stage_flow_iter (per-stage test entry points),
 *    tw_algorithmic_bytes_launch, tw_level_runs_flow_iter; NARROWED: tw_host_register takes whole pages only (a range that is
 *    not page-aligned or not a multiple of the page size — e.g. a malloc / cv::Mat heap block, which version 3 accepted —
 *    now answers TW_E_BAD_PARAMETER; see the declaration).
 * Additive except for that one narrowing: a consumer built against version 1 that never called tw_host_register on heap
 * blocks runs unchanged; tw_abi_version() tells the two apart. */
#define TWFLOW_ABI_VERSION 4

/* Status codes.  The first four are enum ErrorCode of /root/reference/src/opticalflow.h:9-14. */
typedef enum tw_status {
    TW_OK = 0,
    TW_E_BAD_PARAMETER = 1,    /* BadParameter   */
    TW_E_BAD_IMAGE_FORMAT = 2, /* BadImageFormat */
    TW_E_DONT_MATCH_SIZE = 3,  /* DontMatchSize  */
    TW_E_DEVICE = 4,           /* HIP failure / no device; text via tw_last_error */
    TW_E_NOMEM = 5,
    TW_E_UNSUPPORTED = 6, /* e.g. pyrScale >= 1 (OpenCV asserts), polyN > 7 */
    TW_E_BUSY = 7         /* all in-flight slots taken: tw_wait a ticket first */
} tw_status;

/* struct OpticalFlowParameter, /root/reference/src/opticalflow.h:28-36 (same fields, same order). */
typedef struct tw_params {
    double pyrScale;
    int pyrLevels;
    int winSize;
    int pyrIterations;
    int polyN;
    double polySigma;
    int flags; /* 256 = OPTFLOW_FARNEBACK_GAUSSIAN (default, src/broker.cpp:117); 0 = box window */
} tw_params;

/* struct Vector, /root/reference/src/message_queue.h:20-25. */
typedef struct tw_vector {
    int x;
    int y;
    double dx;
    double dy;
} tw_vector;

typedef struct tw_engine tw_engine;
typedef int64_t tw_ticket;

/* Defaults of Broker::createInstance, /root/reference/src/broker.cpp:111-117. */
void tw_default_params(tw_params* p);

/* TWFLOW_ABI_VERSION of the library that was loaded (a consumer compares it with the header it was built against). */
int tw_abi_version(void);

/* 1 for a `make VARIANTS=1` build (tidal-wave_amd/libtwflow_variants.so: the default library plus the measured-slower
 * A/B kernels behind TW_BLUR_VARIANT / TW_POLY_VARIANT / TW_BLUR_SMALL / TW_UPD_NY — tests and tools only), 0 for the
 * product library, which carries only kernels a launch can reach with no environment variable set. */
int tw_has_variants(void);

/* cv::gpu::getCudaEnabledDeviceCount() of src/consumer.cpp:19-20: number of usable HIP devices
 * (0 when there is none or the runtime cannot initialise). */
int tw_device_count(void);

/* PCI bus id of a device ("0000:c1:00.0", NUL-terminated, cap >= 16) — lets the host layer place consumer i and its
 * page-locked buffers on the NUMA node of GPU i (SURVEY.md 8(e) "scaling risks"; the reference's consumer i <-> device i
 * mapping is src/consumer.cpp:18-24).  TW_E_DEVICE if the device does not exist. */
tw_status tw_device_pci_bus_id(int device, char* buf, int cap);

/* new OpticalFlowByGPU() + cv::gpu::setDevice(id), src/consumer.cpp:21-30.
 * `slots` = image pairs per batch (>= 1); up to three batches may be outstanding.  Parameters are fixed per engine like Consumer::parameter (src/consumer.cpp:97). */
tw_status tw_engine_create(int device, const tw_params* params, int slots, tw_engine** out);
void tw_engine_destroy(tw_engine* e);

/* Human-readable text for a status; the four reference codes have no fixed text of their own. */
const char* tw_strerror(tw_status s);
/* Message of the last failure on this engine (e.g. hipGetErrorString), "" if none. */
const char* tw_last_error(const tw_engine* e);

/* OpticalFlow::calculateInternal, /root/reference/src/opticalflow.h:49 / src/opticalflow.cpp:97-119:
 * dense flow of one 8-bit gray pair (row stride in bytes), planar flowx/flowy out (w*h floats each,
 * either may be NULL).  `seconds` = device compute time, the meaning of OpticalFlowStatus::time
 * (src/opticalflow.cpp:112-118).  Both images have one size here: the <= 5 px reconcile of
 * src/opticalflow.cpp:52-68 is what the tw_submit_*_sized calls below do, on the device. */
tw_status tw_flow_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                     ptrdiff_t stride, float* flowx, float* flowy, float* seconds);

/* Flow + the span-grid scan of src/consumer.cpp:60-76 in one call; only the flagged grid vectors are
 * copied back.  `out` has room for `cap` vectors; *n receives the number found (may exceed cap, then
 * only cap are written).  Vectors are in the reference's row-major order (y, then x). */
tw_status tw_diff_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                     ptrdiff_t stride, int span, double threshold, tw_vector* out, int cap, int* n,
                     float* seconds);

/* Asynchronous pair of the same operation, for batching (the Manager queue keeps `slots` jobs in
 * flight per GPU).  The host images are copied to pinned staging before tw_submit_u8 returns.
 * Sizes (every submit and tw_stage_* call): 1 .. 32768 pixels per side, else TW_E_BAD_PARAMETER; and
 * round_up(width, 32) * height <= 214 748 364 = (2^32 - 1) / 20, else TW_E_UNSUPPORTED (five float planes behind one
 * buffer resource with 32-bit offsets: 16384 x 13107 is admitted, 16384 x 13108 is not). */
tw_status tw_submit_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                       ptrdiff_t stride, int span, double threshold, tw_ticket* ticket);
/* The same pair handed over HALF-DECODED (ABI 3): what cv::imread(path, GRAYSCALE) of src/opticalflow.cpp:37,44 does to
 * an 8-bit non-interlaced PNG after the inflate — scanline reconstruction (filter types 0-4 of ISO/IEC 15948 §9) and
 * libpng 1.5's RGB -> gray — runs on the device, so the host's decode threads only inflate.  For each
 * image: channels 1 (gray), 2 (gray + alpha), 3 (RGB) or 4 (RGBA) = the inflated IDAT stream, `height` rows of
 * 1 + width * channels bytes, filter type byte first; channels 0 = a plain gray image, dense rows of `width` bytes (so a
 * pair may mix a PNG with an image the host decoded).  The result equals tw_submit_u8 on the host-decoded images bit for
 * bit.  A filter type above 4 answers TW_E_BAD_IMAGE_FORMAT.  Page-locked buffers are DMA-ed in place like
 * tw_submit_u8's (keep them until tw_wait); pageable ones are copied before the call returns. */
tw_status tw_submit_png8(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                         int target_channels, int width, int height, int span, double threshold, tw_ticket* ticket);
/* Same with the images already resident in device memory (HBM) of the engine's device. */
tw_status tw_submit_dev(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                        ptrdiff_t stride, int span, double threshold, tw_ticket* ticket);
/* Submitted pairs are gathered into a batch of up to `slots` pairs and executed together, level by level
 * (every kernel launch covers as many pairs as it takes to fill the GPU).  A batch starts executing when it
 * is full, when tw_flush is called, or when one of its tickets is waited for.  `seconds` of a pair is the
 * device time of its batch divided by the pairs in it (exact for a batch of one).
 * Cold-start ramp (round 6; engines of >= 64 slots, host images): a batch that starts while nothing of an earlier
 * batch is still executing goes out in up to three pieces — the first quarter of `slots`, the second quarter, the
 * rest — each as soon as ITS uploads have arrived, instead of behind the batch's last upload; results, tickets and
 * their order are the same (environment TW_RAMP=0 turns it off). */
tw_status tw_flush(tw_engine* e);
tw_status tw_wait(tw_engine* e, tw_ticket ticket, tw_vector* out, int cap, int* n, float* seconds);

/* Dense flow fields from batched submissions (additive within ABI 4; a consumer detects them by the symbols).
 * The tw_submit_*_flow calls are tw_submit_u8 / tw_submit_png8 / tw_submit_dev plus a destination for the pair's final
 * level-0 flow.  When tw_wait returns TW_OK for the ticket, the field is in out->data, bit-identical to what tw_flow_u8
 * returns for the same pair; vectors, status and ticket order are those of the plain call (span 0: flow only, no scan).
 * Bytes of the row pitch beyond a row are never written.  `seconds` stays the batch's device compute time (the copy of
 * a field to host memory is not in it).  out == NULL is the plain call.  The destination is given at submit time
 * because a batch launches inside tw_submit_* when it fills.
 * out->data is device memory of the engine's device, or a page-locked host block the library knows (tw_host_alloc /
 * tw_host_register) that the caller keeps until tw_wait of the ticket returns.  Rejected with TW_E_BAD_PARAMETER before
 * anything is queued: a null data, a pitch below the row or not a multiple of 4, an unknown layout, any other host
 * memory (the runtime is never handed a pageable pointer), memory of another device, or a field that does not fit
 * inside the device allocation. */
enum {
    TW_FLOW_PLANAR = 0,     /* flowx rows, then flowy rows: plane y starts at data + pitch * height */
    TW_FLOW_INTERLEAVED = 1 /* (dx, dy) float pairs per pixel, CV_32FC2 — what cv::calcOpticalFlowFarneback writes */
};
typedef struct tw_flow_out {
    void* data;      /* device memory of the engine's device, or page-locked host memory the library knows */
    ptrdiff_t pitch; /* bytes between rows; >= width*4 (planar) or width*8 (interleaved), multiple of 4 */
    int layout;      /* TW_FLOW_PLANAR / TW_FLOW_INTERLEAVED */
} tw_flow_out;
tw_status tw_submit_u8_flow(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                            ptrdiff_t stride, int span, double threshold, const tw_flow_out* out, tw_ticket* ticket);
tw_status tw_submit_png8_flow(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                              int target_channels, int width, int height, int span, double threshold,
                              const tw_flow_out* out, tw_ticket* ticket);
tw_status tw_submit_dev_flow(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                             ptrdiff_t stride, int span, double threshold, const tw_flow_out* out, tw_ticket* ticket);

/* Initial flow fields (OPTFLOW_USE_INITIAL_FLOW; additive within ABI 4, detected by the symbols).
 * The tw_submit_*_flow_init calls are tw_submit_*_flow plus a full-resolution field that seeds the coarsest pyramid level,
 * as cv::calcOpticalFlowFarneback does with OPTFLOW_USE_INITIAL_FLOW: the field is resized to the coarsest level with
 * INTER_AREA and multiplied by that level's scale (pyrScale^levels); everything after is unchanged.  A non-NULL init
 * turns the initial flow on for that pair whatever params.flags says; without one (init == NULL, or the plain calls)
 * the pair starts from zero as before — flags & 4 alone still means a zero start (the reference passes an
 * uninitialised field).  init and out may each be NULL.
 * init->data is device memory of the engine's device (read in place), a page-locked host block the library knows
 * (DMA-ed from in place), or any other host memory (copied before the call returns; the runtime is never handed a
 * pageable pointer).  The field is read when its batch launches, so the caller keeps it unchanged until tw_wait of the
 * ticket returns; a field that is another ticket's destination needs that ticket waited first.  Non-finite values are
 * passed through.  Rejected with TW_E_BAD_PARAMETER before anything is queued: a null data, a pitch below the row or
 * not a multiple of 4, an unknown layout, memory of another device, or a field that does not fit inside its device
 * allocation. */
typedef struct tw_flow_in {
    const void* data; /* device memory of the engine's device, or host memory */
    ptrdiff_t pitch;  /* bytes between rows; >= width*4 (planar) or width*8 (interleaved), multiple of 4 */
    int layout;       /* TW_FLOW_PLANAR / TW_FLOW_INTERLEAVED */
} tw_flow_in;
tw_status tw_submit_u8_flow_init(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                                 ptrdiff_t stride, int span, double threshold, const tw_flow_in* init,
                                 const tw_flow_out* out, tw_ticket* ticket);
tw_status tw_submit_png8_flow_init(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                                   int target_channels, int width, int height, int span, double threshold,
                                   const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket);
tw_status tw_submit_dev_flow_init(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                                  ptrdiff_t stride, int span, double threshold, const tw_flow_in* init,
                                  const tw_flow_out* out, tw_ticket* ticket);

/* Pairs of unequal size (OpticalFlow::calculate's rule, src/opticalflow.cpp:52-68; additive within ABI 4, detected by the
 * symbols).  The tw_submit_*_sized calls are the tw_submit_*_flow_init calls plus a size (and, for gray images, a row
 * stride) of the target's own.  `width, height` is the PAIR's size — the expected image's: the flow, init, out, the span
 * grid, the vector coordinates and the batch's homogeneity all use it, and a reconciled pair joins the open batch of that
 * size like any other pair.  A target that differs by at most 5 pixels in width and in height is resized to the pair's
 * size on the device as cv::resize does it (8-bit, INTER_LINEAR: kernel tw_resize_u8) before anything else reads it; the
 * result equals tw_submit_u8 on the host-resized target bit for bit.  abs(width - target_width) > 5 or abs(height -
 * target_height) > 5 answers TW_E_DONT_MATCH_SIZE: nothing is queued, no ticket is consumed, the open batch stays as it
 * was.  The target's size goes through the same size predicate as the pair's; target_stride < target_width answers
 * TW_E_BAD_PARAMETER; the PNG call checks the filter type bytes of the target's rows at the target's row length.  With
 * equal sizes the call IS the _flow_init call: the same launches, copies and events, no tw_resize_u8 launch, no staging
 * (a device target whose stride differs from the expected image's is re-pitched by the same kernel).  `seconds` keeps its
 * meaning: the resize runs where the uploads and tw_png_unfilter run and is not in it.  A device target is read when
 * its batch launches and is never written. */
tw_status tw_submit_u8_sized(tw_engine* e, const uint8_t* expect, int width, int height, ptrdiff_t stride,
                             const uint8_t* target, int target_width, int target_height, ptrdiff_t target_stride,
                             int span, double threshold, const tw_flow_in* init, const tw_flow_out* out,
                             tw_ticket* ticket);
tw_status tw_submit_png8_sized(tw_engine* e, const uint8_t* expect, int expect_channels, int width, int height,
                               const uint8_t* target, int target_channels, int target_width, int target_height,
                               int span, double threshold, const tw_flow_in* init, const tw_flow_out* out,
                               tw_ticket* ticket);
tw_status tw_submit_dev_sized(tw_engine* e, const void* d_expect, int width, int height, ptrdiff_t stride,
                              const void* d_target, int target_width, int target_height, ptrdiff_t target_stride,
                              int span, double threshold, const tw_flow_in* init, const tw_flow_out* out,
                              tw_ticket* ticket);

/* PNG kinds on the device (additive within ABI 4, detected by the symbols).  tw_submit_png is tw_submit_png8_sized for
 * an image described by its IHDR: besides the 8-bit gray, gray + alpha, RGB and RGBA rows of tw_submit_png8 it takes,
 * non-interlaced,
 *     colour type 0 (gray)          depths 1, 2, 4 (v * 255 / (2^depth - 1)) and 16 (the high byte)
 *     colour type 3 (palette)       depths 1, 2, 4, 8 (libpng 1.5's truncating gray formula on PLTE[v], r == g == b kept)
 *     colour type 4 (gray + alpha)  depth 16 (the high byte of the gray sample)
 * each converted byte for byte as cv::imread(GRAYSCALE) converts it.  The packed kinds go through a 256-entry gray table
 * the library builds from the PLTE body (read before the call returns) or from the depth.  16-bit RGB and RGBA (pixels of
 * 6 and 8 bytes: more than the dword a kernel lane hands to its neighbour) and Adam7 files stay on the host:
 * tw_png_on_device answers 0 for them and tw_submit_png TW_E_UNSUPPORTED.
 * The pair's size is the expected image's; a target within 5 pixels is reconciled as tw_submit_png8_sized does it, one
 * further apart answers TW_E_DONT_MATCH_SIZE.  For the 8-bit kinds the call IS tw_submit_png8_sized: the same launches,
 * copies and events.  Refused before anything is queued (no ticket consumed): a colour type / depth pair IHDR does not
 * allow, a palette image without a palette or with palette_entries outside 1..256 (TW_E_BAD_IMAGE_FORMAT); a valid kind
 * the device does not take (TW_E_UNSUPPORTED); a filter type byte above 4, looked for at the kind's row length
 * (TW_E_BAD_IMAGE_FORMAT).  A palette index at or above palette_entries — what libpng refuses while it reads the rows —
 * is found by the kernel: tw_wait of THAT pair's ticket answers TW_E_BAD_IMAGE_FORMAT and tw_last_error names the image
 * ("expected" or "target"; the expected image wins, as the reference opens it first); the other pairs of the batch are
 * unaffected. */
enum { TW_PNG_PLAIN_GRAY = -1 };
typedef struct tw_png_rows {
    const uint8_t* rows;    /* inflated IDAT stream: height rows of 1 + ceil(width * channels * bit_depth / 8) bytes,
                               filter type first; TW_PNG_PLAIN_GRAY: dense gray rows of `width` bytes */
    int width, height;      /* this image's own size */
    int color_type;         /* IHDR: 0, 2, 3, 4, 6, or TW_PNG_PLAIN_GRAY */
    int bit_depth;          /* IHDR: 1, 2, 4, 8, 16 */
    const uint8_t* palette; /* PLTE body, r g b per entry; colour type 3 only; read before the call returns */
    int palette_entries;    /* 1 .. 256 */
} tw_png_rows;
/* 1: tw_submit_png takes rows of this IHDR colour type, bit depth and interlace method (the table above); 0: every other
 * triple, valid or not.  Needs no device.  The one predicate: the library and its host layer both ask it. */
int tw_png_on_device(int color_type, int bit_depth, int interlace);
tw_status tw_submit_png(tw_engine* e, const tw_png_rows* expect, const tw_png_rows* target, int span, double threshold,
                        const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket);

/* JPEG on the device (additive within ABI 4, detected by the symbols).  tw_submit_jpeg is tw_submit_u8_sized for images
 * handed over after their entropy decode: what cv::imread(path, GRAYSCALE) does to a JPEG's luma blocks after the Huffman
 * work — dequantisation, libjpeg's slow integer inverse DCT (jidctint), level shift and range limit, the crop to the
 * image — runs on the device (kernel tw_jpeg_idct, on the copy stream where tw_png_unfilter runs: it is not in `seconds`),
 * so a host decode thread stops at the coefficient plane.  The result equals tw_submit_u8 on the host-decoded images bit
 * for bit, for every int16 coefficient and uint16 table entry (a damaged file reaches the extremes).
 * An image is its coefficients (coef != NULL) or a plain gray image (coef == NULL, gray != NULL), so a pair may mix a JPEG
 * with an image the host decoded; with both coef NULL the call IS tw_submit_u8_sized: the same launches, no tw_jpeg_idct
 * launch.  The pair's size is the expected image's; a target within 5 pixels is reconciled by tw_resize_u8 as
 * tw_submit_png8_sized does it, one further apart answers TW_E_DONT_MATCH_SIZE.  Both sizes go through the size predicate
 * of every submit.  Refused with TW_E_BAD_PARAMETER before anything is queued (no ticket consumed, the open batch
 * unchanged): an image with both pointers NULL, block counts outside ceil(size / 8) .. ceil(size / 8) + 3.  Page-locked
 * coefficient planes are DMA-ed in place (keep them until tw_wait); pageable ones are copied before the call returns.  A
 * batch with JPEG images is launched as a PNG batch is: no cold-start ramp. */
typedef struct tw_jpeg_luma {
    const int16_t* coef;    /* blocks_w*blocks_h blocks, row-major, 64 quantised coefficients each, natural order;
                               NULL: `gray` is a plain gray image, dense rows of `width` bytes */
    const uint8_t* gray;
    int width, height;      /* this image's own size */
    int blocks_w, blocks_h; /* ceil(width/8) .. ceil(width/8)+3, likewise for height (whole MCUs) */
    uint16_t quant[64];     /* luma table, natural order */
} tw_jpeg_luma;
tw_status tw_submit_jpeg(tw_engine* e, const tw_jpeg_luma* expect, const tw_jpeg_luma* target, int span, double threshold,
                         const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket);

/* Resident images (additive within ABI 4, detected by the symbols).  A tw_image is a gray image the engine keeps in device
 * memory of its own, so that an image which takes part in many pairs — a baseline compared again and again, the inner frames
 * of a sequence — is read, decoded and uploaded once.  It belongs to the engine that made it; tw_engine_destroy frees all.
 * Blocks are 256-byte aligned ranges of chunks the engine allocates (at least 64 MB each) and reuses after release: no device
 * allocation per image in steady state.  TW_E_NOMEM when the device has no room; budgets and eviction are the caller's.
 * Handles are looked up in the engine's registry, never dereferenced first: a NULL, released, foreign or garbage pointer
 * answers TW_E_BAD_PARAMETER, consumes no ticket and leaves the open batch as it was.
 *
 * tw_image_keep keeps the expected (TW_KEEP_EXPECT) or target (TW_KEEP_TARGET) image of a submitted pair as its batch sees
 * it — dense gray at the pair's size, after tw_png_unfilter / tw_jpeg_idct and, for a reconciled target, after tw_resize_u8 —
 * for tickets of every submit entry point, from the submit that returned the ticket until the tw_wait that collects it (an
 * unknown or waited ticket, or `which` outside 0..1: TW_E_BAD_PARAMETER).  It is one device-to-device copy on the copy
 * stream, behind whatever writes the pair's slot and in front of whatever reuses it; when the batch has not been launched
 * and the slot is written by the batch's decode launches, the copy is queued with them.  The host never waits.  (A device
 * target that tw_submit_dev_sized reconciles is written on the compute stream when its batch launches: keeping it launches
 * the open batch.)  Keeping the expected image of a tw_submit_image_* pair returns the same handle once more and copies
 * nothing; each handle returned is released once.  The kept image of a pair that later answers TW_E_BAD_IMAGE_FORMAT (a
 * palette index without an entry) has undefined content: release it.
 * tw_image_create_u8 makes a plain gray host image resident.  A page-locked block the library knows is DMA-ed in place and
 * stays unchanged until tw_wait of the first pair submitted against the image returns; other memory is copied before the
 * call returns.
 * tw_image_release may be called at any time: the block returns to the store once every batch that reads it has been
 * collected (all its tickets waited) or dropped; the handle is refused from the call on.
 *
 * tw_submit_image_png / tw_submit_image_jpeg are tw_submit_png / tw_submit_jpeg with the expected image resident: the pair's
 * size is the image's; the target is described, checked, refused and reconciled exactly as there (TW_PNG_PLAIN_GRAY rows and
 * a coefficient-less tw_jpeg_luma are plain gray targets).  Only the target is staged.  Such a pair joins the open batch of
 * ordinary host pairs of its size, span and threshold; init and out work as for any pair; the result equals the plain call
 * on the image's bytes bit for bit. */
typedef struct tw_image tw_image; /* opaque */
enum { TW_KEEP_EXPECT = 0, TW_KEEP_TARGET = 1 };
tw_status tw_image_keep(tw_engine* e, tw_ticket ticket, int which, tw_image** out);
tw_status tw_image_create_u8(tw_engine* e, const uint8_t* gray, int width, int height, ptrdiff_t stride, tw_image** out);
tw_status tw_image_release(tw_engine* e, tw_image* img);
tw_status tw_image_size(const tw_engine* e, const tw_image* img, int* width, int* height);
tw_status tw_submit_image_png(tw_engine* e, const tw_image* expect, const tw_png_rows* target, int span, double threshold,
                              const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket);
tw_status tw_submit_image_jpeg(tw_engine* e, const tw_image* expect, const tw_jpeg_luma* target, int span, double threshold,
                               const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket);

/* Ignore regions (additive within ABI 4, detected by the symbols).  The tw_submit_*_ignore calls are tw_submit_u8_sized /
 * tw_submit_png / tw_submit_jpeg / tw_submit_image_png / tw_submit_image_jpeg plus rectangles of the pair that may differ — a
 * clock, an ad slot, a blinking cursor.  Inside every rectangle the target's pixels are replaced by the expected image's
 * pixels at the same coordinates, on the device (kernel tw_mask_rects, one launch per batch on the copy stream where
 * tw_png_unfilter runs: it is not in `seconds`), after tw_png_unfilter, tw_jpeg_idct and tw_resize_u8 and before anything
 * else reads the target: the result equals tw_submit_u8 on the host-decoded, host-resized, host-edited target bit for bit —
 * vectors, status, the dense field of `out`, the effect of `init`.  A pair that differs only inside its rectangles is an
 * identical pair to everything downstream.  Only the target is written: a resident expected image stays valid whatever
 * rectangles later pairs name.
 * Rectangles are in pair coordinates (the expected image's) and are read before the call returns.  Each is clipped to the
 * pair's image: x and y may be negative, x + width is computed in 64 bits, and a rectangle that is empty after clipping
 * (zero area, or wholly outside) is accepted and does nothing.  Rectangles may overlap or touch.
 * n_ignore == 0 (ignore may be NULL): the call IS the plain call — the same launches, copies and events, no tw_mask_rects
 * launch, a batch that may ramp as before; so is a call all of whose rectangles are empty after clipping.
 * Refused with TW_E_BAD_PARAMETER before anything is queued (no ticket consumed, the open batch unchanged): n_ignore < 0 or
 * above TW_MAX_IGNORE, n_ignore > 0 with ignore == NULL, a negative width or height.
 * A vector whose grid point (x, y) lies inside a clipped rectangle of its pair is not reported: *n of tw_wait counts what
 * is left (with out == NULL as well), and `out` of tw_wait receives the first min(*n, cap) of those.  (The flow there is
 * generally not zero — changes outside reach in through the window — but "ignore" means "do not report from here".)  The
 * dense field of a tw_flow_out is not touched.
 * A masked pair joins the open batch of ordinary host pairs of its size, span and threshold; a batch with at least one
 * masked pair is launched as a PNG batch is: no cold-start ramp.  tw_image_keep(.., TW_KEEP_TARGET, ..) of a masked pair
 * keeps the target as the batch sees it, after the mask; keeping an expected image is unaffected.  Device pairs
 * (tw_submit_dev*) are read in place and never written: they have no _ignore call, nor have tw_flow_u8 and tw_diff_u8. */
typedef struct tw_rect {
    int x, y, width, height; /* pair coordinates = the expected image's */
} tw_rect;
enum { TW_MAX_IGNORE = 32 };
tw_status tw_submit_u8_ignore(tw_engine* e, const uint8_t* expect, int width, int height, ptrdiff_t stride,
                              const uint8_t* target, int target_width, int target_height, ptrdiff_t target_stride,
                              int span, double threshold, const tw_flow_in* init, const tw_flow_out* out,
                              const tw_rect* ignore, int n_ignore, tw_ticket* ticket);
tw_status tw_submit_png_ignore(tw_engine* e, const tw_png_rows* expect, const tw_png_rows* target, int span,
                               double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                               int n_ignore, tw_ticket* ticket);
tw_status tw_submit_jpeg_ignore(tw_engine* e, const tw_jpeg_luma* expect, const tw_jpeg_luma* target, int span,
                                double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                                int n_ignore, tw_ticket* ticket);
tw_status tw_submit_image_png_ignore(tw_engine* e, const tw_image* expect, const tw_png_rows* target, int span,
                                     double threshold, const tw_flow_in* init, const tw_flow_out* out,
                                     const tw_rect* ignore, int n_ignore, tw_ticket* ticket);
tw_status tw_submit_image_jpeg_ignore(tw_engine* e, const tw_image* expect, const tw_jpeg_luma* target, int span,
                                      double threshold, const tw_flow_in* init, const tw_flow_out* out,
                                      const tw_rect* ignore, int n_ignore, tw_ticket* ticket);

/* Hit regions (additive within ABI 4, detected by the symbols).  With the engine option TW_OPT_REGIONS on (tw_set_option,
 * below), a batch groups each pair's vectors into regions on the device, so that a caller can act on "three places changed,
 * here are their boxes" instead of a flat list of grid vectors — the boxes are what a user pastes back as ignore rectangles.
 * A pair's hits are the vectors tw_wait reports for it (for a pair with ignore rectangles: what is left after them).  With
 * the option's value `gap` (1 .. 8), two hits are adjacent when their grid coordinates differ by at most gap grid steps in x
 * and in y (gap 1: 8-connectivity); a region is a connected component of that adjacency.  Regions are ordered by their first
 * hit in row-major order (y, then x).  Every field is an integer or a float copied from one sample: nothing is summed, the
 * result does not depend on the order of evaluation.
 * The kernel (tw_hit_regions: one workgroup per pair, union-find over the pair's span grid) is launched directly behind the
 * batch's ordered scan, on the same stream, for the same pairs, and is INSIDE `seconds`.  A batch takes the option's value
 * in force when its first pair is booked, and all its pairs share it; every submit entry point gains the feature unchanged
 * (tw_submit_dev* too).  With the option off — the default — every entry point launches exactly what it launched before.
 * tw_wait_regions is tw_wait plus the regions: *n_regions receives the TRUE number of regions of the pair; `regions`
 * (nullable) the first min(*n_regions, region_cap, TW_MAX_REGIONS) records — only the first TW_MAX_REGIONS are kept per
 * pair; `region_of` (nullable) min(*n, cap) entries parallel to `out`: the index of each reported vector's region in that
 * order, which may be TW_MAX_REGIONS or more (the record is then not kept, the index is still right).  On a ticket whose
 * batch was opened with the option off it answers TW_E_BAD_PARAMETER and does NOT consume the ticket.  Plain tw_wait on a
 * regions batch works as before.  A batch with span 0 has no hits: *n_regions = 0.  Errors of the pair itself (a palette
 * index, the device) are answered as tw_wait answers them. */
typedef struct tw_region {
    int x, y, width, height; /* pixel box: x = min hit x, y = min hit y,
                                width  = min(max hit x + span, pair width)  - x,
                                height = min(max hit y + span, pair height) - y
                                (each hit stands for its span x span cell, clipped to the image) */
    int count;               /* hits in the region */
    int peak_x, peak_y;      /* the hit with the largest float len = dx*dx + dy*dy, as the scan computes it;
                                among equal len the first in row-major order */
    float peak_dx, peak_dy;
} tw_region;                 /* 36 bytes */
enum { TW_MAX_REGIONS = 256 };
tw_status tw_wait_regions(tw_engine* e, tw_ticket ticket, tw_vector* out, int cap, int* n, int* region_of,
                          tw_region* regions, int region_cap, int* n_regions, float* seconds);

/* Residual (additive within ABI 4, detected by the symbols).  The vectors answer "where did something move by more than
 * threshold pixels"; a flat repaint moves nothing (no gradient: the flow solves to zero) and a moved block and a rewritten block
 * look alike.  With the engine option TW_OPT_RESIDUAL on (tw_set_option, below; its value is the tolerance `tol`, 1 .. 254), a
 * batch also compares each pair's expected image E with its target T sampled ALONG the pair's final level-0 flow — the field
 * tw_submit_*_flow exports — and reports, per cell of the span grid, how many differing pixels the flow does not explain.  T is
 * the target as the batch sees it (after decode, reconcile and ignore masking); w x h is the pair's size.  All arithmetic is
 * integer after one float -> int conversion per flow component, so the result does not depend on the order of evaluation:
 *   pixel (x, y) with float flow (dx, dy):
 *     q(d)  = 0 when d is NaN, else round-half-even of min(max(d, -16384.f), 16384.f) * 32.f as int (the product is exact)
 *     sx    = clamp(32 * x + q(dx), 0, 32 * (w - 1)),  sy = clamp(32 * y + q(dy), 0, 32 * (h - 1))
 *     ix    = sx >> 5, ax = sx & 31, x1 = min(ix + 1, w - 1);  iy, ay, y1 alike
 *     v     = (T[iy][ix]*(32-ax)*(32-ay) + T[iy][x1]*ax*(32-ay) + T[y1][ix]*(32-ax)*ay + T[y1][x1]*ax*ay + 512) >> 10
 *     diff  = |E[y][x] - T[y][x]|,  u = min(diff, |E[y][x] - v|)
 *   cell of grid point (gx, gy): pixels [gx*span, min((gx+1)*span, w)) x [gy*span, min((gy+1)*span, h)):
 *     n_diff = #(diff > tol), n_unexplained = #(u > tol), max_diff = max diff, max_unexplained = max u
 * A cell is reported iff n_diff >= 1, as a tw_change in row-major order (y, then x); a cell whose grid point lies inside a
 * clipped ignore rectangle of its pair is not reported (the rule vectors follow).  A batch with span 0 has no cells.
 * Kernels: tw_warp_residual per level-0 chunk (beside tw_flow_export, before the chunk's flow buffer is reused),
 * tw_change_scan once per batch directly behind the ordered scan (and tw_hit_regions), inside `seconds`.  A residual batch
 * needs the dense final field: it takes the schedule a batch with a flow destination takes (no grid-only last iteration, no
 * captured-graph replay of a single pair).  A batch takes the option's value in force when its first pair is booked, and all
 * its pairs share it; every submit entry point gains the feature unchanged (tw_submit_dev* too: the images are read in place
 * with their stride).  With the option off — the default — every entry point launches, copies and records exactly what it
 * did before, and the feature's buffers do not exist.
 * tw_ticket_changes is valid from the submit that returned the ticket until the wait that collects it.  It launches the open
 * batch if it has to, as tw_wait does, and waits for the batch; writes the first min(*n_changes, change_cap) records
 * (`changes` nullable); *n_changes is the TRUE count after the ignore rule.  It does NOT consume the ticket: tw_wait or
 * tw_wait_regions follows.  On a batch opened with the option off it answers TW_E_BAD_PARAMETER and the ticket stays
 * waitable; an unknown or already waited ticket answers TW_E_BAD_PARAMETER; errors of the pair itself (a palette index, the
 * device) are answered as tw_wait answers them. */
typedef struct tw_change {
    int x, y;                   /* the cell's grid point: gx * span, gy * span */
    int n_diff, n_unexplained;  /* pixels of the cell with diff > tol / with u > tol */
    int max_diff, max_unexplained;
} tw_change;                    /* 24 bytes */
tw_status tw_ticket_changes(tw_engine* e, tw_ticket ticket, tw_change* changes, int change_cap, int* n_changes);

/* Shift (additive within ABI 4, detected by the symbols).  The engine reproduces Farneback, and with it Farneback's reach: at
 * the default parameters a displacement of a few tens of pixels.  A page whose content moved as a whole by more (an inserted
 * banner, a scroll) has a flow that is garbage everywhere.  With the engine option TW_OPT_SHIFT on (tw_set_option, below; its
 * value is the search radius R in pixels, 1 .. 1024), a batch estimates one integer translation per pair on the device, checks
 * it on the pixels, and starts the pair's flow from it — after decode, reconcile and ignore masking, before the pyramid.
 * E, T are the pair's expected and target images as the batch sees them, w x h bytes (row padding is never read).  All integer:
 *   profiles  rowE[y] = sum_x E[y][x], colE[x] = sum_y E[y][x]; rowT, colT alike (uint32)
 *   search    once per axis of length L with profiles pE, pT: r = min(R, L / 2); for d in [-r, r]: n(d) = L - |d|,
 *             cost(d) = sum_{i = max(0, -d)}^{min(L, L - d) - 1} |pE[i] - pT[i + d]|.  Candidates in the order 0, -1, +1, -2, +2,
 *             ...; one replaces the best only when cost(d) * n(best) < cost(best) * n(d) in unsigned 64 bits (ties: the smaller
 *             |d|, then the negative one).  dy from the row profiles, dx from the column profiles; the sign is the flow's:
 *             E[y][x] ~ T[y + dy][x + dx]
 *   accept    sad_0 = sum |E - T| over the image, n_0 = w * h.  (dx, dy) != (0, 0): sad_s = sum |E[y][x] - T[y + dy][x + dx]|
 *             over the overlap rectangle, n_s its area, applied = sad_s * n_0 <= (sad_0 >> 1) * n_s in unsigned 64 bits (the
 *             shift at least halves the mean absolute difference).  (0, 0): applied = 0, sad_s = sad_0, n_s = n_0
 *   seed      a pair with applied = 1 and no tw_flow_in of its own computes exactly what tw_submit_*_flow_init computes for it
 *             with the full-resolution constant field ((float)dx, (float)dy), bit for bit; every other pair starts from zero.
 *             A pair with its own tw_flow_in keeps it: its shift is measured and reported with applied = 0.
 * Kernels: tw_shift_profiles, tw_shift_search, tw_shift_verify per batch part behind its uploads; tw_flow_shift_init at every
 * chunk of the coarsest level.  A shift batch takes the schedule a batch with an initial field takes (no captured-graph replay
 * of a single pair).  A batch takes the option's value in force when its first pair is booked, and all its pairs share it;
 * every submit entry point gains the feature unchanged.  With the option off — the default — every entry point launches,
 * copies and records exactly what it did before, and the feature's buffers do not exist.
 * tw_ticket_shift is valid from the submit that returned the ticket until the wait that collects it.  It launches the open
 * batch if it has to, as tw_wait does, and waits for the batch.  It does NOT consume the ticket.  On a batch opened with the
 * option off it answers TW_E_BAD_PARAMETER and the ticket stays waitable; an unknown or already waited ticket answers
 * TW_E_BAD_PARAMETER; errors of the pair itself are answered as tw_wait answers them. */
typedef struct tw_shift {
    int dx, dy;          /* the two searches' answers */
    int applied;         /* 1: the pair's flow started from (dx, dy) */
    int n_shift, n_zero; /* overlap area at (dx, dy); w * h */
    uint64_t sad_shift, sad_zero;
} tw_shift;              /* 40 bytes */
tw_status tw_ticket_shift(tw_engine* e, tw_ticket ticket, tw_shift* out);

/* Shift bands (additive within ABI 4, detected by the symbols).  One translation per pair does not explain a page with an
 * inserted banner or a grown paragraph: everything below the insertion moved, nothing above it did.  With the engine option
 * TW_OPT_SHIFT_BANDS on (its value B is the band height in rows: 32 .. 1024, a multiple of 16) in a batch that also has
 * TW_OPT_SHIFT on (whose value is the radius R), the batch estimates one vertical shift per band of B rows, checks each on the
 * pixels, and starts the pair's flow from the bands.  With TW_OPT_SHIFT off the option is ignored: no launch, no buffer.
 * E, T, w, h as in "Shift".  All integer:
 *   global    the pair's tw_shift record is computed and reported exactly as without bands (dx, dy, both sums, `applied` by
 *             the global rule); with bands on the seed comes from the bands only, and the record's `applied` is just that
 *             rule's verdict
 *   columns   dx = the pair's global dx, applied or not.  xa = max(0, -dx), xb = min(w, w - dx), nblk = ceil((xb - xa) / 64)
 *   bands     band b covers rows [b B, min((b + 1) B, h)): rows_b rows; nb = ceil(h / B) bands
 *   signature for every row y and block k < nblk: sigE[y][k] = sum of E[y][x] over x in [xa + 64 k, min(xa + 64 (k + 1), xb)),
 *             sigT[y][k] = sum of T[y][x + dx] over the same x (each at most 16 320: uint16)
 *   search    per band, r = min(R, h / 2): candidates d in the order 0, -1, +1, -2, +2, ...; lo = max(b B, -d),
 *             hi = min(b B + rows_b, h - d), n(d) = hi - lo; a candidate with n(d) < ceil(rows_b / 2) is skipped (d = 0 never
 *             is); cost(d) = sum over i in [lo, hi) and k of |sigE[i][k] - sigT[i + d][k]| in 64 bits; a candidate replaces
 *             the best only when cost(d) * n(best) < cost(best) * n(d) in unsigned 64 bits.  The winner — the least cost per
 *             row, the earliest in visit order among equals — is dy_b
 *   accept    per band: sad_zero = sum |E - T| over the band's rows and all w columns, n_zero = rows_b * w.
 *             (dx, dy_b) == (0, 0): applied = 0, sad_shift = sad_zero, n_shift = n_zero (the band did not move: a zero seed is
 *             right).  Otherwise sad_shift = sum |E[y][x] - T[y + dy_b][x + dx]| over the rows [lo, hi) of dy_b and the columns
 *             [xa, xb), n_shift = (hi - lo) * (xb - xa), applied = sad_shift * n_zero <= (sad_zero >> 2) * n_shift in unsigned
 *             64 bits: the shift must at least quarter the band's mean absolute difference (stricter than the page's halving,
 *             because a band has far fewer pixels)
 *   seed      a pair without a tw_flow_in of its own computes exactly what tw_submit_*_flow_init computes for it with the
 *             full-resolution field F[y][x] = ((float)dx, (float)dy_b) for y in a band with applied = 1 and (0, 0) elsewhere,
 *             bit for bit.  A pair with its own field keeps it: its bands are measured and all reported with applied = 0.
 *             There is no fall-back to the global shift.
 * Kernels: tw_band_rows, tw_band_search, tw_band_verify per batch part behind its tw_shift_verify; tw_flow_band_init at every
 * chunk of the coarsest level, in tw_flow_shift_init's place.  The option is read when a batch's first pair is booked, and all
 * pairs of the batch share it.  With the option off — the default — every entry point launches, copies, records and allocates
 * exactly what it did before.
 * Known limits: a band that straddles the insertion usually answers applied = 0, and so does a band whose content has left
 * the image — but a wrong shift can be accepted there (a few in a hundred such bands); the flow there is garbage either way.
 * The move is vertical only, plus the one global dx.  Bands do not constrain each other.
 * tw_ticket_shift_bands follows tw_ticket_shift's contract: valid until the wait that collects the ticket, launches the open
 * batch if it has to, waits for it, does NOT consume the ticket.  *n is the true nb; the first min(nb, cap) records are
 * written.  On a batch without bands it answers TW_E_BAD_PARAMETER and the ticket stays waitable; an unknown or already waited
 * ticket, a null n, or a null out with cap > 0 answers TW_E_BAD_PARAMETER. */
typedef struct tw_shift_band {
    int y, rows;          /* b * B, rows_b */
    int dy, applied;      /* the band's search answer; 1: the band's rows of the pair's start field are (dx, dy) */
    int n_shift, n_zero;  /* overlap area at (dx, dy); rows_b * w */
    uint64_t sad_shift, sad_zero;
} tw_shift_band;          /* 40 bytes */
tw_status tw_ticket_shift_bands(tw_engine* e, tw_ticket ticket, tw_shift_band* out, int cap, int* n);

/* Diff image (additive within ABI 4, detected by the symbols).  The engine answers a pair with lists of numbers; a user of a
 * screenshot diff wants the page with the changes marked on it.  The gray images as the batch sees them — after tw_png_unfilter,
 * tw_jpeg_idct, tw_resize_u8 and tw_mask_rects — exist only in device memory, and so do all hit records of a pair with more than
 * the eagerly copied ones.  tw_ticket_overlay renders one pair's picture there, on request, after the batch has finished: a
 * batch launches, copies and records exactly what it did before, no engine option turns anything on, and a caller who renders
 * only the suspicious pairs pays nothing for the others.
 * E, T are the pair's expected and target images as the batch sees them, w x h.  `rects` are the pair's ignore rectangles after
 * clipping; `hits` are the vectors tw_wait would report for the pair (after the ignore rule) — ALL of them, in their float
 * precision, not only the ones a small `cap` would take; `regions` are the records tw_wait_regions would return (at most
 * TW_MAX_REGIONS boxes) when the batch was opened with TW_OPT_REGIONS on, none otherwise; tol is 0 .. 255.  All arithmetic is
 * integer after one float -> int conversion per vector component, and every layer has one colour, so the result does not
 * depend on the order of evaluation.  Colours are (r, g, b):
 *   base, every pixel (x, y):  e = E[y][x], t = T[y][x], d = |e - t|, g = 128 + (t >> 1)
 *       inside a clipped ignore rectangle      (g - 48, g - 48, g)
 *       else d > tol                           (255, 192 - (d >> 1), 0)
 *       else                                   (g, g, g)
 *   boxes (over base): the one-pixel outline of every region's box [x, x+width) x [y, y+height)   (0, 160, 0)
 *       (a box of width 1 or height 1 is a line, a box without area draws nothing)
 *   vectors (over boxes): for every hit (x, y, dx, dy)                                            (0, 0, 255)
 *       q(v) = 0 when v is NaN, else (int) round-half-even of min(max(v, -1024.f), 1024.f)
 *       rx = q(dx), ry = q(dy), n = max(|rx|, |ry|)
 *       marker: the 3 x 3 square centred on (x, y)
 *       line:   for i = 0 .. n:  (x + floor((2*i*rx + n) / (2*n)), y + floor((2*i*ry + n) / (2*n)))     (n = 0: the origin only)
 *   pixels outside the image are dropped (of a box, a marker and a line alike)
 * The priority is vectors over boxes over base.  TW_OVERLAY_MAX_LEN is the clamp of q: a line has at most 1025 pixels.
 * Kernels: tw_overlay_base (2 bytes in, 3 bytes out per pixel), then tw_overlay_marks once for the boxes and once for the
 * vectors, in stream order — on the engine's device-to-host stream, where the call does not queue behind later batches.
 *
 * tw_ticket_hits and tw_ticket_overlay follow tw_ticket_changes' contract: valid from the submit that returned the ticket until
 * the wait that collects it; they launch the open batch if they have to, as tw_wait does, and wait for the batch; they do NOT
 * consume the ticket; an unknown or already waited ticket answers TW_E_BAD_PARAMETER; errors of the pair itself (a palette
 * index: TW_E_BAD_IMAGE_FORMAT; the device) are answered as tw_wait answers them, and the ticket stays waitable.  Both work
 * on every batch, whatever options it was opened with.  A batch with span 0 has no hits: *n = 0, the image is the base.
 * tw_ticket_hits: *n receives the TRUE count tw_wait would put into its *n.
 * tw_ticket_overlay is synchronous: when it returns TW_OK the image is in out->data, `height` rows of 3 * width bytes,
 * out->pitch bytes apart.  pitch >= 3 * width, any value (odd ones too); bytes of the pitch behind a row are never written.
 * out->data is device memory of the engine's device that holds the whole image (written in place), a page-locked host block
 * the library knows (tw_host_alloc / tw_host_register: written by DMA), or any other host memory (through the engine's
 * page-locked bounce buffer: the runtime is never handed a pageable pointer).  Host destinations are rendered into a device
 * staging buffer of the engine's, created by the first such call and kept until tw_engine_destroy.  Refused with
 * TW_E_BAD_PARAMETER before anything is launched: a null out or data, a pitch below 3 * width, an unknown format, tol
 * outside 0 .. 255, device memory of another device or one that does not hold the image.  Calling it twice for one ticket
 * gives the same bytes.  The images of a tw_submit_dev* pair are the caller's: the caller keeps them valid and unchanged
 * until the call returns (a device target that tw_resize_u8 reconciled lives in engine memory and needs nothing). */
#define TW_OVERLAY_MAX_LEN 1024
enum { TW_OVERLAY_RGB8 = 0 }; /* r, g, b bytes per pixel */
typedef struct tw_overlay_out {
    void* data;      /* device memory of the engine's device, or host memory */
    ptrdiff_t pitch; /* bytes between rows; >= 3 * width */
    int format;      /* TW_OVERLAY_RGB8 */
} tw_overlay_out;
tw_status tw_ticket_hits(tw_engine* e, tw_ticket ticket, int* n);
tw_status tw_ticket_overlay(tw_engine* e, tw_ticket ticket, int tol, const tw_overlay_out* out);

/* Number of grid points ceil(h/span)*ceil(w/span): the capacity that can never overflow. */
int tw_grid_capacity(int width, int height, int span);

/* Raw device memory helpers so a host without a HIP binding can keep inputs resident. */
tw_status tw_dev_alloc(tw_engine* e, size_t bytes, void** dptr);
tw_status tw_dev_free(tw_engine* e, void* dptr);
tw_status tw_dev_upload(tw_engine* e, void* dptr, const void* host, size_t bytes);
/* Counterpart of tw_dev_upload: synchronous device -> host copy into any host memory (pageable memory goes through the
 * engine's page-locked bounce buffer). */
tw_status tw_dev_download(tw_engine* e, void* host, const void* dptr, size_t bytes);

/* Engine options.
 * TW_OPT_SCAN_FUSED_FINAL (default 0): tw_submit_* / tw_diff_u8 with span 10 and winSize 30/31 evaluate the last
 *   window average + solve of level 0 only at the span-grid points the scan reads.  Status and vectors are
 *   bit-identical; the dense flow field of that last iteration is simply never materialised (tw_flow_u8 always
 *   computes the whole field).  Off by default because the reference's path — and bench.py's headline — produce
 *   the full field.
 * TW_OPT_POLYEXP_F32 (default 0): MEASUREMENT variant of the polynomial expansion with float instead of double
 *   horizontal accumulators (polyN 5 or 7; what OpenCV's CUDA module does).  NOT bit-identical to the CPU reference;
 *   exists so that "what would the kernel cost without its f64 half, and what would it do to the flow" is a number
 *   (bench.py `polyexp_f32_variant`, profiles/r03_polyexp_f32.md).  Value 2 (polyN 7) additionally fuses every
 *   multiply-add (v_pk_fma_f32).  Never on by default, never bench.py's `value`.
 * TW_OPT_REGIONS (default 0): hit regions, above.  0 is off; 1 .. 8 is the gap; any other value answers
 *   TW_E_BAD_PARAMETER and leaves the option as it was.  Read when a batch's first pair is booked.
 * TW_OPT_RESIDUAL (default 0): residual, above.  0 is off; 1 .. 254 is the tolerance; any other value answers
 *   TW_E_BAD_PARAMETER and leaves the option as it was.  Read when a batch's first pair is booked.
 * TW_OPT_SHIFT (default 0): shift, above.  0 is off; 1 .. 1024 is the search radius in pixels; any other value answers
 *   TW_E_BAD_PARAMETER and leaves the option as it was.  Read when a batch's first pair is booked.
 * TW_OPT_SHIFT_BANDS (default 0): shift bands, above.  0 is off; 32 .. 1024 and a multiple of 16 is the band height in rows;
 *   any other value answers TW_E_BAD_PARAMETER and leaves the option as it was.  Read when a batch's first pair is booked;
 *   ignored in a batch opened with TW_OPT_SHIFT off. */
enum {
    TW_OPT_SCAN_FUSED_FINAL = 1,
    TW_OPT_POLYEXP_F32 = 2,
    TW_OPT_REGIONS = 3,
    TW_OPT_RESIDUAL = 4,
    TW_OPT_SHIFT = 5,
    TW_OPT_SHIFT_BANDS = 6
};
tw_status tw_set_option(tw_engine* e, int option, int value);

/* Page-locked host memory.  Images handed to tw_submit_u8 from a block tw_host_alloc returned (or that the caller
 * page-locked through tw_host_register) are DMA-ed to the device straight from the caller's buffer on the engine's
 * copy stream — no staging copy — and must therefore stay unchanged until tw_wait() of the ticket returns.
 * Any other memory is treated as pageable: it is staged through the engine's own pinned buffers and may be reused as
 * soon as tw_submit_u8 returns (memory page-locked behind the library's back, e.g. by a direct hipHostRegister, is
 * staged too — correct, one memcpy slower).  The blocks are usable by the engines of every device and by every
 * thread (the table of them is process-wide).  Either way the upload of batch j+1 overlaps the kernels of batch j
 * (BASELINE config 3: "pinned H2D/D2H overlapped on a side stream").
 * Releasing a block: tw_host_free / tw_host_unregister wait only for the uploads of the engine they are called on.
 * The caller must have collected (tw_wait) every ticket of EVERY engine that was handed images from the block before
 * it releases it.  A block is released the way it was made: tw_host_free on a registered block, or
 * tw_host_unregister on a tw_host_alloc block, answers TW_E_BAD_PARAMETER and releases nothing. */
tw_status tw_host_alloc(tw_engine* e, size_t bytes, void** hptr);
tw_status tw_host_free(tw_engine* e, void* hptr);
/* Page-lock / release memory the caller owns (hipHostRegister / hipHostUnregister + the table above).
 * WHOLE PAGES ONLY: `hptr` must be page-aligned and `bytes` a multiple of the page size (sysconf(_SC_PAGESIZE)),
 * i.e. memory the caller owns page-wise — mmap, aligned_alloc(page, n * page), posix_memalign.  Anything else
 * (a malloc / new block, a cv::Mat's heap buffer) answers TW_E_BAD_PARAMETER with a tw_last_error text and
 * page-locks nothing: a partial page is shared with the allocator's other blocks, and page-locking / releasing it
 * next to them is what a GPU memory-access fault of round 4 traced to.  Use tw_host_alloc for
 * buffers that need not live at a given address. */
tw_status tw_host_register(tw_engine* e, void* hptr, size_t bytes);
tw_status tw_host_unregister(tw_engine* e, void* hptr);

/* ---- instrumentation (bench.py / tests) ---------------------------------------------------------- */

/* Kernel classes, in data-flow order. */
enum {
    TW_K_PYR = 0,
    TW_K_POLYEXP = 1,
    TW_K_UPDATE_MATRICES = 2,
    TW_K_BLUR_SOLVE = 3,
    TW_K_SCAN = 4,
    TW_K_COUNT = 5
};

/* Every later launch of kernel class `kclass` at pyramid level `level` (-1: every level, -2: off) is
 * bracketed by hipEvents on the stream it is launched on; several classes may be on at once;
 * kclass -1 turns all of them off.  Totals accumulate per class until read. */
tw_status tw_prof_select(tw_engine* e, int kclass, int level);
/* Sum of event-measured milliseconds and number of launches of `kclass` since the last read; resets both.
 * Synchronises the device. */
tw_status tw_prof_read(tw_engine* e, int kclass, double* ms_total, int* launches);
/* Bytes one launch of `kclass` at `level` must move for a w x h pair: every input of the kernel AS BUILT read once,
 * every output written once (blur+solve: averaged over the pyrIterations launches of a level — a launch fused with
 * the matrix refresh moves 80 B/px, the last one 28 B/px; flows that never leave the registers are not counted). */
double tw_algorithmic_bytes(const tw_engine* e, int kclass, int level, int width, int height);
/* The same for a batch of `npairs` pairs: the model reads the schedule's own choice (choose_level_schedule in csrc/twflow.hip,
 * the function the enqueue executes) — a single pair, a batch too small to fill the chip with tw_flow_iter workgroups or a level
 * whose launches do not cover the batch keeps tw_update_matrices + tw_blur_solve* (UPDATE_MATRICES 60 B/px + the coarser flow,
 * window launches 80 / 28 B/px) where a full batch runs tw_flow_iter (56 B/px, no UPDATE_MATRICES launch); a level whose images
 * the coarser level's launch wrote reads no source image.  tw_algorithmic_bytes is this with npairs = the engine's slots.
 * The batch these three views describe returns hit records only (no flow destination, no initial field), at span 10 — so the
 * scan-fused option is assumed with the one span it supports — with no profiling class selected; with TW_LANES=2 they answer
 * for the first lane's half of the batch, the part the schedule decides for.  A size the engine has no plan for (a degenerate
 * pyramid level, a smoothing kernel or tile beyond the kernels' limits: every submit of that size is refused) has no schedule:
 * tw_algorithmic_bytes_launch answers 0 for it, tw_level_runs_flow_iter and tw_level_chunk -1.  Before the engine has
 * enqueued a batch of the size, each call computes the size's plan geometry on the host (7 - 18 us); afterwards it reads the
 * engine's plan (0.5 us). */
double tw_algorithmic_bytes_launch(const tw_engine* e, int kclass, int level, int width, int height, int npairs);
/* 1 if `level` of such a batch of `npairs` pairs of width x height runs tw_flow_iter (whole iterations, no M in HBM), 0 if it
 * runs tw_update_matrices + tw_blur_solve* launches, -1 on a bad argument. */
int tw_level_runs_flow_iter(const tw_engine* e, int width, int height, int level, int npairs);
/* SURVEY.md 8(d) model of one whole pair (each named stage of the reference reads its inputs once and writes its
 * outputs once; 991.8 MB at 1080p with the defaults): the figure BASELINE.md prices a pair against. */
double tw_algorithmic_bytes_pair(const tw_engine* e, int width, int height, int span);
/* Sum of tw_algorithmic_bytes over every launch of a pair: what the kernels as built must move for a full batch (611.8 MB at 1080p with the defaults; 859.6 before tw_flow_iter). */
double tw_min_traffic_bytes_pair(const tw_engine* e, int width, int height, int span);
/* Number of pyramid levels (= index of the coarsest level) the engine uses for w x h. */
int tw_num_levels(const tw_engine* e, int width, int height);
/* Image pairs one kernel launch covers at `level` at most (the level-major batch schedule), -1 on error.  No device call. */
int tw_level_chunk(tw_engine* e, int width, int height, int level);

/* Isolated timing of one kernel class at `level` of a width x height pair, `npairs` pairs per launch, on
 * synthetic device-resident data: average microseconds per launch over `iters` back-to-back launches
 * (hipEvents on the engine's stream).  flags: 1 = rough (non-smooth) flow field, 2 = tw_blur_solve without
 * the fused matrix refresh. */
tw_status tw_bench_stage(tw_engine* e, int kclass, int width, int height, int level, int npairs, int iters,
                         int flags, float* avg_us);

/* ---- per-stage entry points (parity tests; host buffers, synchronous) --------------------------------
 * Layouts: images/planes are dense row-major; R and M are 5 planes [5][h][w]; flow is 2 planes. */
tw_status tw_stage_pyr_level(tw_engine* e, const uint8_t* img, int w0, int h0, int level, float* I, int* w,
                             int* h);
/* Levels 3 and 2 of one image from the batch path's one-read kernel (tw_pyr_23; round 5): I3 (w0/8 x h0/8) and I2
 * (w0/4 x h0/4).  TW_E_UNSUPPORTED when the size has no exact reductions by 4 and 8 (the engine then runs
 * tw_stage_pyr_level's kernels for those levels). */
tw_status tw_stage_pyr_fused23(tw_engine* e, const uint8_t* img, int w0, int h0, float* I3, float* I2);
/* Levels 0 and 1 of one image from one read (tw_pyr_k3f; round 5): I0 (w0 x h0) and I1 (w0/2 x h0/2).  TW_E_UNSUPPORTED
 * when level 1 is not an exact halving with 3-tap smoothing (pyrScale 0.5, even width and height). */
tw_status tw_stage_pyr_fused01(tw_engine* e, const uint8_t* img, int w0, int h0, float* I0, float* I1);
/* PNG scanline reconstruction + gray conversion of one image (tw_submit_png8's kernel): `rows` = h rows of
 * 1 + w * channels bytes, channels 1-4; `waves` = 0 (the engine's choice for this width), 1, 4 or 16 waves per image. */
tw_status tw_stage_png_unfilter(tw_engine* e, const uint8_t* rows, int channels, int w, int h, int waves,
                                uint8_t* gray);
/* The same kernel for every kind tw_submit_png takes (TW_PNG_PLAIN_GRAY excepted): `gray` = img->width x img->height
 * bytes.  A palette index without an entry answers TW_E_BAD_IMAGE_FORMAT. */
tw_status tw_stage_png_decode(tw_engine* e, const tw_png_rows* img, int waves, uint8_t* gray);
/* The size reconcile's kernel alone (tw_resize_u8): dense src (sw x sh) -> dense dst (dw x dh), cv::resize's 8-bit
 * INTER_LINEAR.  Sizes more than 5 pixels apart answer TW_E_DONT_MATCH_SIZE. */
tw_status tw_stage_resize_u8(tw_engine* e, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh);
/* tw_submit_jpeg's kernel alone (tw_jpeg_idct) on one image that has coefficients: `gray` receives width * height bytes.
 * `guard`, if not NULL, receives 512 bytes: the 256 device bytes in front of the image and the 256 behind it, which the
 * entry point set to 0xA5 before the launch — a byte that is not 0xA5 was written outside the image.  (Additive within
 * version 4.) */
tw_status tw_stage_jpeg_idct(tw_engine* e, const tw_jpeg_luma* img, uint8_t* gray, uint8_t* guard);
/* The tw_submit_*_ignore calls' kernel alone (tw_mask_rects) on two dense gray images of w x h, placed as a batch places
 * them (256-byte aligned slots, dense rows of w bytes): `out` receives the edited target, w * h bytes.  `guard`, if not
 * NULL, receives 512 bytes: the 256 device bytes in front of the target's slot and the 256 behind it, which the entry point
 * set to 0xA5 before the launch.  The slot's own padding behind the image is checked by the entry point (TW_E_DEVICE when
 * a byte of it was written).  The argument checks and the clipping of the submit calls; no launch when no rectangle is
 * left.  (Additive within version 4.) */
tw_status tw_stage_mask_rects(tw_engine* e, const uint8_t* expect, const uint8_t* target, int w, int h,
                              const tw_rect* ignore, int n_ignore, uint8_t* out, uint8_t* guard);
tw_status tw_stage_polyexp(tw_engine* e, const float* I, int w, int h, float* R5);
tw_status tw_stage_update_matrices(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow2,
                                   int w, int h, float* M5);
tw_status tw_stage_flow_upsample_update(tw_engine* e, const float* R0_5, const float* R1_5,
                                        const float* prevflow2, int pw, int ph, int w, int h, float* flow2,
                                        float* M5);
tw_status tw_stage_blur_solve(tw_engine* e, const float* R0_5, const float* R1_5, const float* M5, int w, int h,
                              int update_matrices, float* flow2, float* Mout5);
/* One whole iteration of the flow update WITHOUT M in memory (tw_flow_iter, round 5): flow_out = solve(window average of
 * FarnebackUpdateMatrices(R0, R1, flow)) where flow = flow_in2, or (prev2) the coarser level's flow prev2 (pw x ph)
 * resized INTER_LINEAR to w x h and scaled by 1/pyrScale, or zero (both null).  winSize 30/31 Gaussian window, levels of
 * at least 320 x 20 pixels; TW_E_UNSUPPORTED otherwise. */
tw_status tw_stage_flow_iter(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow_in2, const float* prev2,
                             int pw, int ph, int w, int h, float* flow_out2);
/* The same iteration from flow_in2, evaluated at the span-grid points only (tw_flow_iter's grid-only mode, a batch's last
 * level-0 iteration): grid_out receives ceil(w / span) x ceil(h / span) (dx, dy) pairs, row-major — the values
 * tw_stage_flow_iter's field holds at (gx * span, gy * span).  span >= 5; the sizes and statuses of tw_stage_flow_iter. */
tw_status tw_stage_flow_iter_grid(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow_in2, int w, int h,
                                  int span, float* grid_out);
/* The span-grid threshold scan alone, on the caller's own fields: `fields` = npairs dense planar flow fields
 * [npairs][2][h][w] (dx plane, dy plane), uploaded into level 0's padded planes; tw_span_gather samples them at every
 * span-th pixel and the ordered scan a submit of such a batch would launch — tw_span_scan, or tw_span_scan_seg for
 * single_pair = 1 on a grid large enough (tw_debug_scan_plan) — records every point with
 * (double)(float)(dx * dx + dy * dy) > threshold * threshold, row-major.  With G = ceil(w / span) * ceil(h / span):
 * counts[npairs]; xy[npairs][G][2] = (x, y) and dxy[npairs][G][2] = (dx, dy) as the device holds them (floats, not
 * tw_vector's doubles) — a pair's WHOLE record region: the counts and the records are set to 0xff bytes before the
 * launches, so an entry from counts[j] on that is not 0xffffffff was written beyond the hits, and a count of -1 was never
 * stored.  span >= 1; single_pair = 1 takes npairs = 1, else TW_E_BAD_PARAMETER.  (Additive within version 4.) */
tw_status tw_stage_span_scan(tw_engine* e, const float* fields, int npairs, int w, int h, int span, double threshold,
                             int single_pair, int* counts, int* xy, float* dxy);

/* tw_hit_regions alone, on the caller's own fields: `fields` as for tw_stage_span_scan — uploaded, gathered by tw_span_gather
 * and scanned by the ordered scan a batch of npairs such pairs would launch — then one tw_hit_regions launch over the same
 * grid samples with `gap` (1 .. 8) and, per pair j, the n_ignore[j] rectangles ignore[j * TW_MAX_IGNORE ..] (pair coordinates,
 * clipped as the submit calls clip them; n_ignore == NULL: none).  With G = ceil(w / span) * ceil(h / span): n_regions[npairs];
 * regions[npairs][TW_MAX_REGIONS]; region_of[npairs][G], entry k of a pair being the region of its k-th hit.  The outputs are
 * set to 0xff bytes before the launches, so an entry written beyond a pair's share shows.  The label plane lives in LDS for
 * G <= 32 768 and in device memory above.  (Additive within version 4.) */
tw_status tw_stage_hit_regions(tw_engine* e, const float* fields, int npairs, int w, int h, int span, double threshold,
                               int gap, const tw_rect* ignore, const int* n_ignore, int* n_regions, tw_region* regions,
                               int* region_of);

/* tw_warp_residual and tw_change_scan alone, on the caller's data, synchronously: `expect` and `target` (w x h bytes, rows
 * `stride` >= w bytes apart) are placed as a batch places a pair's images, `flow2` (planar [2][h][w]: dx, then dy) is uploaded
 * into level 0's padded planes as tw_stage_span_scan uploads its fields, then one launch of each kernel with `span` (>= 1) and
 * `tol` (1 .. 254).  With G = ceil(w / span) * ceil(h / span): cells[G][4] (n_diff, n_unexplained, max_diff, max_unexplained of
 * every cell, row-major), *n_changes, changes[G].  The outputs are set to 0xff bytes before the launches, so a write beyond the
 * pair's share shows.  (Additive within version 4.) */
tw_status tw_stage_warp_residual(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h,
                                 const float* flow2, int span, int tol, int* cells, int* n_changes, tw_change* changes);

/* tw_shift_profiles, tw_shift_search and tw_shift_verify alone, on the caller's pair, synchronously: `expect` and `target`
 * (w x h bytes, rows `stride` >= w bytes apart) go up as they are and are read in place with their stride, then the launches
 * a batch part makes with `radius` (1 .. 1024).  `profiles` (nullable): [colE[w], colT[w], rowE[h], rowT[h]].  *out: the pair's
 * record.  The outputs are set to 0xff bytes before the launches (the sums the kernels accumulate into are then zeroed as a
 * batch zeroes them), so a write beyond the pair's share shows.  force_global = 1 takes the search's device-memory path
 * whatever the length.  (Additive within version 4.) */
tw_status tw_stage_shift(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h, int radius,
                         int force_global, uint32_t* profiles, tw_shift* out);

/* The global estimation as tw_stage_shift runs it, then tw_band_rows, tw_band_search and tw_band_verify alone, on the caller's
 * pair, synchronously, with `radius` (1 .. 1024) and the band height `band` (32 .. 1024, a multiple of 16).  `sig` (nullable):
 * [sigE[h][nblk], sigT[h][nblk]] at the pair's dx.  *global: the pair's tw_shift record; bands[nb]: the band records;
 * *n_bands = nb.  The outputs are set to 0xff bytes before the launches (the band records are then zeroed as a batch zeroes
 * them), and the call answers TW_E_DEVICE when a launch wrote beyond the pair's share.  force_global = 1 takes the device-memory
 * path of both searches.  (Additive within version 4.) */
tw_status tw_stage_shift_bands(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h, int radius,
                               int band, int force_global, uint16_t* sig, tw_shift* global, tw_shift_band* bands, int* n_bands);

#ifdef __cplusplus
}
#endif
#endif /* TWFLOW_H */
