// twflow.hip — engine + C ABI of libtwflow.so (see include/twflow.h).
//
// One tw_engine = one worker's view of one MI355X: `slots` independent in-flight image pairs, each with
// its own HIP stream and device workspace (no allocation per job in steady state).  The host side only
// builds the small per-level tables (Gaussian taps, bilinear coordinates, polynomial-expansion constants)
// in double precision exactly as OpenCV 2.4.9 does on the CPU, and enqueues the kernels of
// twflow_kernels.hip.h.  There is no CPU compute path in this library.
#include "twflow_kernels.hip.h"

#include <hip/hip_runtime.h>
#include <unistd.h>

#include <dlfcn.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/twflow.h"
#include "../../include/twflow_debug.h"

using namespace twk;

namespace {

// ---------------------------------------------------------------------------------------------------
// Host-side scalar helpers (OpenCV 2.4.9 semantics)
// ---------------------------------------------------------------------------------------------------
inline int cv_round(double v) { return (int)lrint(v); }  // cvtsd2si: round-half-even
inline int cv_floor(double v)
{
    if (!(v > -2147483648.0 && v < 2147483648.0)) return INT32_MIN;
    int i = (int)lrint(v);
    return i - (v < (double)i);
}
inline int cv_ceil(double v)
{
    if (!(v > -2147483648.0 && v < 2147483648.0)) return INT32_MIN;
    int i = (int)lrint(v);
    return i + (i < v);
}
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// cv::getGaussianKernel(n, sigma, CV_32F) — imgproc/smooth.cpp
void gaussian_kernel(int n, double sigma, std::vector<float>& k)
{
    static const float tab[4][7] = {{1.f},
                                    {0.25f, 0.5f, 0.25f},
                                    {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                    {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    const float* fixed = (n % 2 == 1 && n <= 7 && sigma <= 0) ? tab[n >> 1] : nullptr;
    k.resize(n);
    const double sigmaX = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2X = -0.5 / (sigmaX * sigmaX);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        const double t = fixed ? (double)fixed[i] : exp(scale2X * x * x);
        k[i] = (float)t;
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) k[i] = (float)(k[i] * sum);
}

// Coordinate tables of cv::resize(INTER_LINEAR) for float data — imgproc/imgwarp.cpp
struct ResizeTab {
    std::vector<int> xofs, yofs;
    std::vector<float> alpha, beta;
    int xmax = 0;
    int mode = 1;  // 0 same size, 1 linear, 2 area-fast 2x2
};

void make_resize_tab(int sw, int sh, int dw, int dh, ResizeTab& t)
{
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    const int iscale_x = cv_round(scale_x), iscale_y = cv_round(scale_y);
    const bool is_area_fast = fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON;
    t.xofs.resize(dw);
    t.yofs.resize(dh);
    t.alpha.resize(2 * (size_t)dw);
    t.beta.resize(2 * (size_t)dh);
    t.xmax = dw;
    if (sw == dw && sh == dh) {
        // scale 1: fx = fy = 0 everywhere, the generic bilinear code copies exactly
        t.mode = 0;
        for (int x = 0; x < dw; x++) { t.xofs[x] = x; t.alpha[2 * x] = 1.f; t.alpha[2 * x + 1] = 0.f; }
        for (int y = 0; y < dh; y++) { t.yofs[y] = y; t.beta[2 * y] = 1.f; t.beta[2 * y + 1] = 0.f; }
        return;
    }
    if (is_area_fast && iscale_x == 2 && iscale_y == 2) {
        // "INTER_AREA (fast) also is equal to INTER_LINEAR" branch: sum of the 2x2 block * 0.25f
        t.mode = 2;
        for (int x = 0; x < dw; x++) { t.xofs[x] = 2 * x; t.alpha[2 * x] = 0.5f; t.alpha[2 * x + 1] = 0.5f; }
        for (int y = 0; y < dh; y++) { t.yofs[y] = 2 * y; t.beta[2 * y] = 0.5f; t.beta[2 * y + 1] = 0.5f; }
        return;
    }
    t.mode = 1;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            if (dx < t.xmax) t.xmax = dx;
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        t.xofs[dx] = sx;
        t.alpha[2 * dx] = 1.f - fx;
        t.alpha[2 * dx + 1] = fx;
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        t.yofs[dy] = sy;  // rows are clipped at use, weights are not (resizeGeneric_Invoker)
        t.beta[2 * dy] = 1.f - fy;
        t.beta[2 * dy + 1] = fy;
    }
}

// cv::resize(INTER_AREA) of a full-resolution initial flow field to the coarsest level — imgproc/imgwarp.cpp (2.4.9):
// mode 0 same size (a copy), 1 both scales integers within DBL_EPSILON (resizeAreaFast_Invoker), 2 computeResizeAreaTab's
// tables (ResizeArea_Invoker), computed in double exactly as there
struct AreaTab {
    int mode = 2, ix = 1, iy = 1;
    std::vector<int> xstart, xsi, ystart, ysi;  // output x's entries: [xstart[x], xstart[x + 1])
    std::vector<float> xalpha, ybeta;
};
void area_tab_1d(int ssize, int dsize, double scale, std::vector<int>& start, std::vector<int>& si, std::vector<float>& alpha)
{
    start.assign(dsize + 1, 0);
    si.clear();
    alpha.clear();
    for (int dx = 0; dx < dsize; dx++) {
        start[dx] = (int)si.size();
        const double fsx1 = dx * scale;
        const double fsx2 = fsx1 + scale;
        const double cellWidth = std::min(scale, ssize - fsx1);
        int sx1 = cv_ceil(fsx1), sx2 = cv_floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) {
            si.push_back(sx1 - 1);
            alpha.push_back((float)((sx1 - fsx1) / cellWidth));
        }
        for (int sx = sx1; sx < sx2; sx++) {
            si.push_back(sx);
            alpha.push_back(float(1.0 / cellWidth));
        }
        if (fsx2 - sx2 > 1e-3) {
            si.push_back(sx2);
            alpha.push_back((float)(std::min(std::min(fsx2 - sx2, 1.), cellWidth) / cellWidth));
        }
    }
    start[dsize] = (int)si.size();
}
void make_area_tab(int sw, int sh, int dw, int dh, AreaTab& t)
{
    if (sw == dw && sh == dh) {
        t.mode = 0;
        return;
    }
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    const int iscale_x = cv_round(scale_x), iscale_y = cv_round(scale_y);
    if (fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON) {
        t.mode = 1;
        t.ix = iscale_x;
        t.iy = iscale_y;
        return;
    }
    t.mode = 2;
    area_tab_1d(sw, dw, scale_x, t.xstart, t.xsi, t.xalpha);
    area_tab_1d(sh, dh, scale_y, t.ystart, t.ysi, t.ybeta);
}

// FarnebackPolyExp constants — video/optflowgf.cpp; invG = G.inv(DECOMP_CHOLESKY) — core/lapack.cpp
void polyexp_setup(int n, double sigma, PolyCoef& pc)
{
    std::vector<float> gb(2 * n + 1), xgb(2 * n + 1), xxgb(2 * n + 1);
    float *g = gb.data() + n, *xg = xgb.data() + n, *xxg = xxgb.data() + n;
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        xg[x] = (float)(x * g[x]);
        xxg[x] = (float)(x * x * g[x]);
    }
    double G[6][6] = {};
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += g[y] * g[x];
            G[1][1] += g[y] * g[x] * x * x;
            G[3][3] += g[y] * g[x] * x * x * x * x;
            G[5][5] += g[y] * g[x] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    double L[6][6], B[6][6] = {};
    memcpy(L, G, sizeof(L));
    for (int i = 0; i < 6; i++) B[i][i] = 1;
    for (int i = 0; i < 6; i++) {
        int j, k;
        double t;
        for (j = 0; j < i; j++) {
            t = L[i][j];
            for (k = 0; k < j; k++) t -= L[i][k] * L[j][k];
            L[i][j] = t * L[j][j];
        }
        t = L[i][i];
        for (k = 0; k < j; k++) {
            const double u = L[i][k];
            t -= u * u;
        }
        L[i][i] = 1. / sqrt(t);
    }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double t = B[i][j];
            for (int k = 0; k < i; k++) t -= L[i][k] * B[k][j];
            B[i][j] = t * L[i][i];
        }
    for (int i = 5; i >= 0; i--)
        for (int j = 0; j < 6; j++) {
            double t = B[i][j];
            for (int k = 5; k > i; k--) t -= L[k][i] * B[k][j];
            B[i][j] = t * L[i][i];
        }
    memset(&pc, 0, sizeof(pc));
    for (int k = 0; k <= n && k < 8; k++) {
        pc.g[k] = g[k];
        pc.xg[k] = xg[k];
        pc.xxg[k] = xxg[k];
        pc.gd[k] = (double)g[k];
        pc.xxgd[k] = (double)xxg[k];
    }
    pc.ig11 = B[1][1];
    pc.ig03 = B[0][3];
    pc.ig33 = B[3][3];
    pc.ig55 = B[5][5];
}

// window taps of FarnebackUpdateFlow_GaussianBlur
void window_kernel(int block_size, WinCoef& wc)
{
    const int m = block_size / 2;
    const double sigma = m * 0.3;
    double s = 1;
    memset(&wc, 0, sizeof(wc));
    wc.k[0] = (float)s;
    for (int i = 1; i <= m; i++) {
        const float t = (float)exp(-i * i / (2 * sigma * sigma));
        wc.k[i] = t;
        s += t * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= m; i++) wc.k[i] = (float)(wc.k[i] * s);
}

// ---------------------------------------------------------------------------------------------------
// Owners of an engine's HIP resources: a member of tw_engine, Ctx or Plan that holds device memory, page-locked memory, an
// event or a stream is one of these.  Each frees what it holds when it goes, so `delete e` is the whole of an engine's
// release; each converts to the bare pointer / handle, so kernel arguments, pointer arithmetic and HIP calls read as they
// would with one.  None can be copied.
// ---------------------------------------------------------------------------------------------------
struct DeviceMem {
    static hipError_t malloc(void** p, size_t n) { return hipMalloc(p, n); }
    static void free(void* p) { (void)hipFree(p); }
    static size_t& books(tw_engine* e);  // tw_engine::dev_bytes
};
struct PinnedMem {
    static hipError_t malloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
    static size_t& books(tw_engine* e);  // tw_engine::pin_bytes
};

// One allocation: the pointer, its capacity in the buffer's own unit (what grow() compares; 0 for a make() buffer) and its
// size in bytes as allocated, slack included.  make() and grow() enter that size in the engine's books (tw_debug_memory) at
// the moment the allocation is made and take it out when they free; alloc() leaves the books to the caller (a plan's tables
// and the resident store's chunks have totals of their own).  Defined behind tw_engine, which they need whole.
template <typename T, typename Mem>
struct Buf {
    T* p = nullptr;
    size_t cap = 0, bytes = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap), bytes(o.bytes) { o.p = nullptr, o.cap = o.bytes = 0; }
    ~Buf()
    {
        if (p) Mem::free((void*)p);
    }
    operator T*() const { return p; }
    tw_status alloc(tw_engine* e, size_t nbytes);
    tw_status make(tw_engine* e, size_t nbytes);
    tw_status grow(tw_engine* e, size_t new_cap, size_t nbytes, hipStream_t sync = nullptr);
    void release(tw_engine* e);
};
template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinBuf = Buf<T, PinnedMem>;

// An event or a stream.  It is created where it is used, with that site's flags (`&x.h` is what the create call fills).
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept
    {
        std::swap(h, o.h);
        return *this;
    }
    ~Handle()
    {
        if (h) (void)Destroy(h);
    }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// ---------------------------------------------------------------------------------------------------
// Plan: everything that depends only on (w0, h0, params)
// ---------------------------------------------------------------------------------------------------
struct LevelPlan {
    int w = 0, h = 0, ld = 0;
    long long ps = 0;  // plane stride (elements)
    double sigma = 0, scale = 1;
    int ksize = 3;
    int chunk = 1;  // image pairs per launch at this level (sized to fill the chip)
    // pyramid tables (full-res -> level)
    int *d_xofs = nullptr, *d_yofs = nullptr;
    float *d_alpha = nullptr, *d_beta = nullptr, *d_kern = nullptr;
    int mode = 1, xmax = 0, nrows_max = 0;
    float h_kern[3] = {0, 0, 0};  // host copy of the taps when ksize == 3
    std::vector<float> h_taps;    // host copy of all taps
    int pitch_b = 0;              // staged-row pitch (bytes) of tw_pyr_level_lds, 0: does not fit LDS
    int gen_th = PYR_TH, gen_nrows_max = 0;  // tile height of the UNSTAGED kernel (tw_pyr_level) and its row-buffer height
    // flow upsample tables (level k+1 -> k)
    int *d_uxofs = nullptr, *d_uyofs = nullptr;
    float *d_ualpha = nullptr, *d_ubeta = nullptr;
    int uxmax = 0;
};

struct Plan {
    int w0 = 0, h0 = 0;
    // levels 2 and 3 come from ONE launch of tw_pyr_23 (exact halving pyramid, 9- / 19-tap smoothing): set by get_plan
    // when the resize tables say so; k19 / k9 = [0, taps..., 0...] as the kernel's shared byte windows want them
    bool fused23 = false;
    float k19[24] = {0}, k9[16] = {0};
    int levels = 0;  // index of the coarsest level
    std::vector<LevelPlan> lv;
    // tw_flow_area_init (initial flow fields -> the coarsest level): make_area_tab's mode, ratios, the output columns a
    // workgroup stages through LDS (mode 1), and the device tables (mode 2)
    int init_mode = 0, init_ix = 1, init_iy = 1, init_tw = 0;
    int *d_ixs = nullptr, *d_ixi = nullptr, *d_iys = nullptr, *d_iyi = nullptr;
    float *d_ixa = nullptr, *d_iyb = nullptr;
    std::vector<DevBuf<char>> owned;  // device allocations (freed with the plan)
    size_t owned_bytes = 0;           // ... and their total size (tw_debug_memory)
    unsigned long long last_use = 0;  // engine's plan clock at the last get_plan (LRU eviction)
};

}  // namespace

// tw_image: a dense gray image in a block of the engine's resident store (ResidentStore below).  `handles` counts what
// tw_image_create_u8 / tw_image_keep handed out and tw_image_release took back; `uses` the batches (and queued keeps) that
// still read or write the block.  The block returns to the store when both are 0.
// What the caller holds is `handle`, a number that no engine of the process hands out twice (this record's address would
// come back from the allocator for the next image, and a released handle has to stay refused); it is never dereferenced.
struct tw_image {
    tw_engine* owner = nullptr;
    tw_image* handle = nullptr;
    uint8_t* d = nullptr;
    int w = 0, h = 0;
    int chunk = 0;
    size_t off = 0, bytes = 0;
    int handles = 0, uses = 0;
};

namespace {

void image_unuse(tw_image* im);

constexpr int TW_MAX_LEVELS = 60;  // the most pyramid levels below level 0 a plan may have (plan_geometry clamps pyrLevels)
constexpr int HOST_RECS = 1024;  // flagged vectors per pair copied back eagerly
constexpr int NCTX = 3;          // batches that may be in flight (host-side state only)
// tw_png_unfilter's table of a batch of `cap` pairs: per image a job, a flag word and a 256-byte gray table
constexpr size_t png_table_bytes(int cap) { return (sizeof(PngJob) + sizeof(unsigned) + 256) * 2 * (size_t)cap; }
// tw_jpeg_idct's table of such a batch: per image a job and a quantisation table
constexpr size_t jpeg_table_bytes(int cap) { return (sizeof(JpegJob) + 128) * 2 * (size_t)cap; }
// tw_mask_rects' table of such a batch: a job per rectangle
constexpr size_t mask_table_bytes(int cap) { return sizeof(MaskJob) * TW_MAX_IGNORE * (size_t)cap; }
// tw_hit_regions' table of such a batch: the pairs' rectangle counts, then TW_MAX_IGNORE clipped rectangles per pair
constexpr size_t region_rects_off(int cap) { return (sizeof(int) * (size_t)cap + 15) / 16 * 16; }
constexpr size_t region_table_bytes(int cap) { return region_rects_off(cap) + sizeof(int4) * TW_MAX_IGNORE * (size_t)cap; }
static_assert(sizeof(RegionRec) == sizeof(tw_region) && sizeof(tw_region) == 36, "tw_region is the kernel's record");
static_assert(RGN_MAX == TW_MAX_REGIONS && RGN_RECTS == TW_MAX_IGNORE, "the kernel's limits are the header's");
static_assert(sizeof(ChangeRec) == sizeof(tw_change) && sizeof(tw_change) == 24, "tw_change is the kernel's record");
static_assert(sizeof(ShiftRec) == sizeof(tw_shift) && sizeof(tw_shift) == 40 && offsetof(ShiftRec, sad_shift) == offsetof(tw_shift, sad_shift),
              "tw_shift is the kernel's record");
static_assert(sizeof(BandRec) == sizeof(tw_shift_band) && sizeof(tw_shift_band) == 40 && offsetof(BandRec, sad_shift) == offsetof(tw_shift_band, sad_shift) &&
                  offsetof(BandRec, n_zero) == offsetof(tw_shift_band, n_zero),
              "tw_shift_band is the kernel's record");

struct Job {
    const uint8_t *h_a = nullptr, *h_b = nullptr;  // host inputs already staged (null for device inputs)
    // tw_submit_image_*: the pair's expected image is this resident image (h_a null, h_b the staged target); the batch holds
    // a reference until it is collected or dropped.  keep[q]: a tw_image_keep of image q whose copy is queued when the
    // batch's decode launches are (the slot is written then), with a reference of its own until it is
    tw_image* res = nullptr;
    tw_image* keep[2] = {nullptr, nullptr};
    const uint8_t *d_a = nullptr, *d_b = nullptr;
    long long stride = 0;
    bool waited = false;
    int png_ch[2] = {0, 0};  // tw_submit_png8: channels of the filtered rows staged in Ctx::d_filt (0: plain gray)
    // tw_submit_png: PngJob::bits and ::entries of those rows, and their gray table in Ctx::png_luts (-1: not a table kind)
    int png_bits[2] = {0, 0}, png_entries[2] = {256, 256}, png_lut[2] = {-1, -1};
    // tw_submit_jpeg: blocks per block row of the coefficients staged in Ctx::d_filt (0: not a coefficient image) and their
    // table in Ctx::jpg_quants
    int jpg_bw[2] = {0, 0}, jpg_q[2] = {-1, -1};
    tw_flow_out fout = {nullptr, 0, 0};  // tw_submit_*_flow: where the pair's final flow goes (data null: nowhere)
    bool fout_host = false;              // ... page-locked host memory: through Ctx::d_fstage and the engine's d2h_stream
    tw_flow_in fin = {nullptr, 0, 0};    // tw_submit_*_flow_init: the pair's initial field (data null: zero start)
    bool fin_staged = false;             // ... host memory, uploaded to Ctx::d_istage as dense rows
    // tw_submit_*_sized: the target's own size and row stride (the pair's when equal), and who resizes it to the pair's
    // size (tw_resize_u8): RSZ_NONE nobody; RSZ_SUBMIT a gray host target, on the copy stream right behind its upload;
    // RSZ_FLUSH_COPY a tw_submit_png8_sized or tw_submit_jpeg target, on the copy stream behind its own tw_png_unfilter
    // (or the batch's tw_jpeg_idct) when the batch is launched; RSZ_FLUSH_DEV a device target (t_src: the caller's memory), on the compute stream in front of the pyramid
    int tw = 0, th = 0;
    long long tstride = 0;
    int rkind = 0;
    const uint8_t* t_src = nullptr;
    // tw_submit_*_ignore: the pair's rectangles, clipped to the pair's image, the empty ones dropped (x, y, width, height >= 1)
    std::vector<tw_rect> ign;
};
enum { RSZ_NONE = 0, RSZ_SUBMIT = 1, RSZ_FLUSH_COPY = 2, RSZ_FLUSH_DEV = 3 };

// One batch of pairs: host-side state that must outlive the asynchronous execution.
struct Ctx {
    Event ev_start, ev_stop, ev_done;
    std::vector<Job> jobs;
    int64_t first_ticket = 0;
    bool launched = false;
    int pending = 0;  // jobs not yet waited
    int w = 0, h = 0, span = 0;
    double threshold = 0;
    bool any_host = false;
    // device copy of the batch's host images (one region per context: the next batch uploads while this one
    // computes) and the event that marks its uploads complete on the copy stream
    DevBuf<uint8_t> d_img;
    Event ev_h2d;
    // cold-start ramp (round 6): the copy stream is marked when a quarter and a half of a full batch's uploads have been
    // queued (Submit::mark_ramp); a batch that is launched into an IDLE compute stream goes out in up to three pieces, each
    // behind its own mark, instead of waiting for the last upload of the whole batch (flush_ctx)
    Event ev_seg[2];
    int seg_at[2] = {0, 0};  // pairs queued when the mark was recorded
    int nseg = 0;
    // tw_submit_png8: filtered PNG rows of the batch (2 slots of filt_slot bytes per job) and the job table of
    // tw_png_unfilter, which reconstructs them into d_img on the copy stream before ev_h2d
    DevBuf<uint8_t> d_filt_raw;
    uint8_t* d_filt() const { return d_filt_raw ? d_filt_raw + 256 : nullptr; }  // (slack on both sides)
    size_t filt_slot = 0;  // bytes per image of the open batch (0: no filtered image yet)
    // Both tables are png_table_bytes(cap) long: behind the 2n jobs of a batch with table kinds (tw_submit_png: palette,
    // 1- / 2- / 4-bit gray) go one flag word per image, zero, and the batch's 256-byte gray tables — one upload, as before.
    // The flag words of a batch with palette images come back to h_pflag behind the batch's results.
    DevBuf<PngJob> d_png;
    PinBuf<PngJob> h_png;
    bool any_png = false, any_plte = false;
    std::vector<std::array<uint8_t, 256>> png_luts;  // the open batch's gray tables, in the order they were submitted
    PinBuf<unsigned> h_pflag;                        // [2*cap]
    // tw_submit_jpeg (both tables created on the first coefficient image of this context, jpeg_table_bytes(cap) long): the
    // batch's coefficient planes share the d_filt slots with filtered PNG rows; behind the 2n jobs of tw_jpeg_idct go the
    // batch's quantisation tables — one upload, as the gray tables above
    DevBuf<JpegJob> d_jpg;
    PinBuf<JpegJob> h_jpg;
    bool any_jpeg = false;
    std::vector<std::array<uint16_t, 64>> jpg_quants;  // the open batch's tables, in the order they were submitted
    long long copy_ops_at_flush = 0;  // tw_engine::copy_ops when this batch was launched
    // ordered hit records of the batch [cap][G]: tw_wait reads them late when a pair has more than HOST_RECS hits,
    // so they belong to the context, not to the engine (a later batch must not overwrite them)
    DevBuf<ScanRec> d_rec;
    // pinned host memory
    PinBuf<uint8_t> h_img;
    PinBuf<const uint8_t*> h_ptrs;  // [2*cap]
    PinBuf<int> h_count;            // [cap]
    PinBuf<ScanRec> h_rec;          // [cap][HOST_RECS]
    // tw_submit_*_flow (all created on first use): the per-pair destination table (pinned, [cap]; uploaded to
    // tw_engine::d_fdst), and for host destinations the HBM staging the export writes (cap slots of dense rows in the
    // destination's layout), the event behind each chunk's export that the device-to-host copies wait for, and the
    // event behind the batch's last copy that tw_wait waits for
    bool any_fout = false, any_fout_host = false;
    PinBuf<FlowDst> h_fdst;
    DevBuf<char> d_fstage;
    Event ev_fexp, ev_d2h;
    long long d2h_ops_at_flush = 0;  // tw_engine::d2h_ops when this batch was launched
    // tw_submit_*_flow_init (created on first use): the per-pair source table of tw_flow_area_init (pinned, [cap]; uploaded
    // to tw_engine::d_fsrc), and the HBM staging of host fields (cap slots of dense rows in the field's layout), filled on
    // the copy stream behind the same marks as the pairs' images
    bool any_init = false, any_init_host = false;
    PinBuf<FlowDst> h_fsrc;
    DevBuf<char> d_istage;
    // tw_submit_*_sized (all created on the first reconciled pair of this context): d_tsrc = `cap` slots of tsrc_slot bytes
    // for host targets of up to (w + 5) x (h + 5) pixels at their own size (256 bytes of slack in front, as d_filt), and tw_resize_u8's
    // job tables, three of [cap] each — one entry per launch at submit time, the batch's PNG targets, the batch's device
    // targets (three, because each is written while the one before may still be on its way to the device) — with the
    // table of the PNG targets' own tw_png_unfilter launches
    DevBuf<uint8_t> d_tsrc_raw;
    uint8_t* d_tsrc() const { return d_tsrc_raw ? d_tsrc_raw + 256 : nullptr; }
    size_t tsrc_slot = 0;
    DevBuf<ResizeJob> d_rsz;  // [3 * cap]
    PinBuf<ResizeJob> h_rsz;
    DevBuf<PngJob> d_rpng;  // [cap]
    PinBuf<PngJob> h_rpng;
    bool any_resize = false, any_resize_png = false, any_resize_dev = false;
    bool any_keep = false;  // a job of the open batch has a tw_image_keep copy to queue at launch
    // tw_submit_*_ignore (both tables created on the first pair with a non-empty rectangle of this context,
    // mask_table_bytes(cap) long): tw_mask_rects' jobs, one per rectangle of the batch
    DevBuf<MaskJob> d_msk;
    PinBuf<MaskJob> h_msk;
    bool any_mask = false;
    // hit regions (TW_OPT_REGIONS; all created when the first batch with the option on is launched from this context):
    // `regions` = the gap of this batch (0: off), taken when its first pair is booked.  The kernel's outputs belong to the
    // context as d_rec does (tw_wait_regions reads region_of late for a pair with more than HOST_RECS hits): counts [cap],
    // kept records [cap][TW_MAX_REGIONS], region_of [cap][G]; their eager copies and the rectangle table are pinned
    int regions = 0;
    DevBuf<int> d_nreg;
    DevBuf<RegionRec> d_regs;
    DevBuf<int> d_regof;
    PinBuf<int> h_nreg;        // [cap]
    PinBuf<RegionRec> h_regs;  // [cap][TW_MAX_REGIONS]
    PinBuf<int> h_regof;       // [cap][HOST_RECS]
    PinBuf<char> h_rgn;        // region_table_bytes(cap)
    // residual (TW_OPT_RESIDUAL; all created when the first batch with the option on is launched from this context):
    // `residual` = the tolerance of this batch (0: off), taken when its first pair is booked.  tw_change_scan's outputs
    // belong to the context as d_rec does (tw_ticket_changes reads the records behind the first HOST_RECS late): counts
    // [cap], records [cap][G]; their eager copies are pinned
    int residual = 0;
    DevBuf<int> d_nchg;
    DevBuf<ChangeRec> d_chg;
    PinBuf<int> h_nchg;       // [cap]
    PinBuf<ChangeRec> h_chg;  // [cap][HOST_RECS]
    // shift (TW_OPT_SHIFT): `shift` = the search radius of this batch (0: off), taken when its first pair is booked; the
    // pinned copy of the batch's records ([cap], created when the first batch with the option on is launched from this context)
    int shift = 0;
    PinBuf<ShiftRec> h_shift;
    // shift bands (TW_OPT_SHIFT_BANDS): `bands` = the band height of this batch (0: off — always when `shift` is), taken when
    // its first pair is booked; the pinned copy of the batch's band records ([cap][nb], grown when a batch needs more)
    int bands = 0;
    int nbands() const { return bands ? (h + bands - 1) / bands : 0; }
    PinBuf<BandRec> h_bands;

    // the batch is collected or dropped: its resident images may return to the store
    void release_images()
    {
        for (Job& jb : jobs) {
            for (tw_image*& im : jb.keep)
                if (im) image_unuse(im), im = nullptr;
            if (jb.res) image_unuse(jb.res), jb.res = nullptr;
        }
        any_keep = false;
    }

    // A new batch in this context: what describes the batch starts over; the device and pinned regions, their capacities
    // and the events survive.
    void begin_batch(int width, int height, int span_, double threshold_, int64_t first, int regions_, int residual_, int shift_, int bands_)
    {
        regions = regions_;
        residual = residual_;
        shift = shift_;
        bands = shift_ ? bands_ : 0;
        release_images();
        jobs.clear();
        launched = false;
        pending = 0;
        w = width;
        h = height;
        span = span_;
        threshold = threshold_;
        any_host = any_png = any_plte = any_fout = any_fout_host = any_init = any_init_host = false;
        png_luts.clear();  // (keeps its capacity: tw_engine_create reserved two tables per slot)
        any_jpeg = false;
        jpg_quants.clear();
        any_resize = any_resize_png = any_resize_dev = false;
        any_mask = false;
        filt_slot = 0;
        nseg = 0;
        first_ticket = first;
    }
};

struct ProfPair {
    Event a, b;
};

// what a captured single-pair schedule depends on besides the engine's (fixed) parameters and workspace addresses
struct GraphKey {
    int w, h, span;
    long long stride;
    int aligned4, scan_fused, poly_f32;
    bool operator<(const GraphKey& o) const
    {
        return std::tie(w, h, span, stride, aligned4, scan_fused, poly_f32) <
               std::tie(o.w, o.h, o.span, o.stride, o.aligned4, o.scan_fused, o.poly_f32);
    }
};

// Optional roctx ranges (TW_ROCTX=1): one range per batch and per pyramid level on the submitting thread, so that a
// rocprofv3 --marker-trace timeline shows which launches belong to which batch / level (SURVEY §5 "tracing"; the
// reference only times the call, which `seconds` preserves).  The roctx library is loaded on demand: no link dependency.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char* ev = getenv("TW_ROCTX");
        if (!ev || !atoi(ev)) return;
        // rocprofv3 (rocprofiler-sdk) listens to its own roctx library; roctracer's libroctx64 is the fallback
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
Roctx& roctx()
{
    static Roctx r;
    return r;
}
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char* fmt, int a = 0, int b = 0, int c = 0) : on(roctx().push != nullptr)
    {
        if (on) {
            char buf[96];
            snprintf(buf, sizeof(buf), fmt, a, b, c);
            roctx().push(buf);
        }
    }
    ~RoctxRange()
    {
        if (on) roctx().pop();
    }
};

// What is fixed when an engine is created: the parameters, what follows from them and from the device, and the engine's
// environment switches.  make_engine_config fills it, tw_engine holds it const, and the choice functions (choose_pyr,
// choose_blur, choose_level_schedule, ...) take it in place of the engine: they cannot read what an earlier batch left behind.
struct EngineConfig {
    tw_params p;
    int cap = 1;  // pairs per batch ("slots")
    int cu_count = 256;
    PolyCoef pc;
    WinCoef wc;
    int win_m = 15;
    int box = 0;           // flags without 256: box window (FarnebackUpdateFlow_Blur), scan kernels
    int lanes = 1;         // TW_LANES=2: the two halves of a batch run on two streams (memory-bound kernels of one
                           // half overlap the VALU-bound blur of the other); per-kernel hipEvent durations then
                           // include the co-running kernel
    int upd_ny = 2;        // TW_UPD_NY: pixels per lane of tw_update_matrices (1 or 2)
    long long mfree_min_px = 0;  // TW_MFREE_MIN_PX: smallest level (pixels) that takes tw_flow_iter
    int mfree_min_w = 320;       // TW_MFREE_MIN_W: narrowest level (columns; strips are 160 outputs wide) that takes it
    int mfree = 1;         // TW_MFREE=0: every level runs update + blur launches again (A/B; tw_flow_iter, no M in HBM, is the
                           // default); 2: tw_flow_iter also for launches of a few workgroups (tests, tools/fuzz_parity.py)
    int pyr23_threads = 0;    // TW_PYR23_THREADS=256 / 512 / 1024: waves per tw_pyr_23 workgroup (A/B); 0 = 512, and 1024 for a
                              // single pair (432 workgroups: sixteen waves cover the staging latency, -0.5 us of 10.6)
    int blur_cm = 0;       // TW_BLUR_CM=1: tw_blur_solve4y (51-tap window) walks an XCD's tiles column-major (A/B)
    int pyr_fused = 1;     // TW_PYR_FUSED=0: levels 2 and 3 as two tw_pyr_taps launches again (A/B; tw_pyr_23 is the default)
    int pyr_generic = 0;   // TW_PYR_GENERIC=1: always the generic pyramid kernel, 2: tw_pyr_level_lds for every level (A/B)
    int blur_variant = 4;  // 4: tw_blur_solve4 (default); 8: tw_blur_solve8 (packed f32) — TW_BLUR_VARIANT
    int pp_waves = 512;    // TW_PP_WAVES: below this many waves of 96x8 tiles a level takes the plane-parallel kernel
    int debug_stamps = 0;  // TW_DEBUG_STAMPS=1: tw_engine_create allocates tw_engine::dbg_stamps (diagnostic runs only)
    int blur_nomask = 0;   // TW_BLUR_NOMASK
    int blur_pipe = 0;     // TW_BLUR_PIPE: tiles a workgroup of tw_blur_solve4p walks (0: tw_blur_solve4 for every launch)
    int blur_small = -1;   // TW_BLUR_SMALL: force the small-grid tile choice of the 31-tap blur (-1: by grid size)
    int blur_small_lv[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // TW_BLUR_SMALL_LEVELS="a,b,c,d": the same per pyramid level
    int poly_variant = 1;  // 1: tw_polyexp_pk<N,8> (packed f32, default); 2: tw_polyexp_pk<N,16>; 0: tw_polyexp (scalar f32) — TW_POLY_VARIANT
    int poly_f32 = 0;      // TW_POLYEXP_F32: what EngineOptions::poly_f32 starts as (measurement runs)
    // single-pair latency schedule (BASELINE config 2): a batch of one pair runs the pyramid + polynomial expansion of
    // every level on stream2 (they depend only on the images) while the main stream walks the flow chain coarse to
    // fine; needs every level's I and R at once (TW_LATENCY_STREAMS=0: everything on one stream)
    int lat_streams = 1;
    long long lat_min_px = 100000;  // TW_LATENCY_MIN_PX
    int lat_s2_max = 1000;  // TW_LAT_S2_LEVELS: finest..this level's image-only work goes to the second stream
    int ramp = 1;  // TW_RAMP=0: no cold-start ramp (A/B)
    long long chunk_tiles = 300000;      // TW_CHUNK_TILES: tiles a launch covers before a level is split (pairs_per_launch)
    int chunk_pairs_lv[TW_MAX_LEVELS + 1] = {};  // TW_CHUNK_PAIRS_LEVELS="p0,p1,...": pairs per launch at level 0, 1, ... (0: the rule)
    int pyr_gen_th = 0;    // TW_PYR_GEN_TH: tile height of the unstaged pyramid kernel (0: by the row buffer's size; A/B)
    int lat_evtiming = 0;  // TW_LAT_EVTIMING: the single-pair schedule's hand-off events keep their timestamps (diagnostic)
    int fi_maxseg = 4, fi_minsteps = 16;  // TW_FI_MAXSEG / TW_FI_MINSTEPS: most row segments per strip / fewest steps per segment (A/B)
    int fi_skip = 0;    // TW_FI_SKIP (variants library): timing experiments on tw_flow_iter (results are wrong)
    int fi_nt = 1024;   // TW_FI_NT=512 (variants library): tw_flow_iter as two 512-thread workgroups per CU on 64-output strips (A/B)
    int lat_fused = 1;  // TW_LAT_FUSED=0: the two-stream single-pair schedule of rounds 2-4 instead of the twin launches (A/B)
    int lat_graph = 0;  // TW_LAT_GRAPH=1: replay the single-pair schedule from a captured hipGraph (measured SLOWER on
                        // ROCm 7.2: 0.55 ms vs 0.37 ms — profiles/r03_latency.md — so it is opt-in, kept for re-measuring);
                        // in use while tw_engine::graph_capture_failed is unset (tw_engine::graph_replay)
    int same_image = 1;    // TW_SAME_IMAGE=0: no tw_pair_same launch, both images of every pair processed (A/B)
};

// What tw_set_option changes between batches (its only writer besides the engine's constructor).
struct EngineOptions {
    int scan_fused = 0;    // TW_OPT_SCAN_FUSED_FINAL
    int poly_f32 = 0;      // TW_OPT_POLYEXP_F32 (measurement variant: float accumulators, not bit-exact)
    int regions_gap = 0;   // TW_OPT_REGIONS: the next batch's gap (0: off)
    int residual_tol = 0;  // TW_OPT_RESIDUAL: the next batch's tolerance (0: off)
    int shift_radius = 0;  // TW_OPT_SHIFT: the next batch's search radius (0: off)
    int shift_bands = 0;   // TW_OPT_SHIFT_BANDS: the next batch's band height in rows (0: off)
};

// the parameters an engine admits (tw_engine_create asks before it touches the device; make_engine_config asks for itself)
tw_status check_params(const tw_params& p)
{
    if (!(p.pyrScale < 1) || !(p.pyrScale > 0)) return TW_E_UNSUPPORTED;  // CV_Assert(pyr_scale < 1)
    if (p.polyN < 1 || p.polyN > 7) return TW_E_UNSUPPORTED;
    if (p.winSize < 2 || p.winSize / 2 > 32) return TW_E_UNSUPPORTED;
    if (p.pyrIterations < 0 || p.pyrLevels < 0) return TW_E_BAD_PARAMETER;
    return TW_OK;
}

// THE reader of the engine's environment switches, and the place to add one: validates the parameters, reads every TW_*
// engine switch once with its clamp, and refuses what the library as built cannot run (*why: the refusal's message).
// No HIP call and no state: the same arguments and environment give the same value.
tw_status make_engine_config(const tw_params& p, int slots, int cu_count, EngineConfig* out, std::string* why)
{
    if (const tw_status st = check_params(p)) return st;
    EngineConfig& c = *out;
    c.p = p;
    c.cap = std::min(256, std::max(1, slots));
    c.cu_count = cu_count;
    polyexp_setup(p.polyN, p.polySigma, c.pc);
    window_kernel(p.winSize, c.wc);
    c.win_m = p.winSize / 2;
    c.box = (p.flags & 256) ? 0 : 1;
    if (const char* ev = getenv("TW_BLUR_VARIANT")) c.blur_variant = atoi(ev);
    if (const char* ev = getenv("TW_PYR_GENERIC")) c.pyr_generic = atoi(ev);
    if (const char* ev = getenv("TW_PYR_FUSED")) c.pyr_fused = atoi(ev) != 0;
    if (const char* ev = getenv("TW_BLUR_CM")) c.blur_cm = atoi(ev);
    if (const char* ev = getenv("TW_PYR23_THREADS")) c.pyr23_threads = atoi(ev) == 256 ? 256 : atoi(ev) == 1024 ? 1024 : atoi(ev) == 512 ? 512 : 0;
    if (const char* ev = getenv("TW_MFREE")) c.mfree = atoi(ev);
    if (const char* ev = getenv("TW_MFREE_MIN_PX")) c.mfree_min_px = atoll(ev);
    if (const char* ev = getenv("TW_MFREE_MIN_W")) c.mfree_min_w = std::max(31, atoi(ev));
    if (c.pyr_generic) c.pyr_fused = 0;
    if (const char* ev = getenv("TW_POLY_VARIANT")) c.poly_variant = atoi(ev);
    if (const char* ev = getenv("TW_BLUR_SMALL")) c.blur_small = atoi(ev);
    if (const char* ev = getenv("TW_BLUR_SMALL_LEVELS")) {
        int k = 0;
        for (const char* q = ev; *q && k < 8; k++) {
            c.blur_small_lv[k] = atoi(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
    if (const char* ev = getenv("TW_PP_WAVES")) c.pp_waves = atoi(ev);
    if (const char* ev = getenv("TW_BLUR_NOMASK")) c.blur_nomask = atoi(ev);
    if (const char* ev = getenv("TW_BLUR_PIPE")) c.blur_pipe = atoi(ev);
    if (const char* ev = getenv("TW_POLYEXP_F32")) c.poly_f32 = atoi(ev) == 2 ? 2 : (atoi(ev) ? 1 : 0);  // = TW_OPT_POLYEXP_F32 (measurement runs)
    if (const char* ev = getenv("TW_DEBUG_STAMPS")) c.debug_stamps = atoi(ev) != 0;
    if (const char* ev = getenv("TW_UPD_NY")) c.upd_ny = atoi(ev) == 1 ? 1 : 2;
    if (const char* ev = getenv("TW_LANES")) c.lanes = std::min(2, std::max(1, atoi(ev)));
    if (const char* ev = getenv("TW_LATENCY_STREAMS")) c.lat_streams = atoi(ev) ? 1 : 0;
    if (const char* ev = getenv("TW_LATENCY_MIN_PX")) c.lat_min_px = atoll(ev);
    if (const char* ev = getenv("TW_LAT_GRAPH")) c.lat_graph = atoi(ev) ? 1 : 0;
    if (const char* ev = getenv("TW_LAT_FUSED")) c.lat_fused = atoi(ev) ? 1 : 0;
#ifdef TW_VARIANTS
    if (const char* ev = getenv("TW_FI_NT")) c.fi_nt = atoi(ev) == 512 ? 512 : 1024;
    if (const char* ev = getenv("TW_FI_SKIP")) c.fi_skip = atoi(ev);
#endif
    if (const char* ev = getenv("TW_LAT_S2_LEVELS")) c.lat_s2_max = atoi(ev);
    if (const char* ev = getenv("TW_RAMP")) c.ramp = atoi(ev) ? 1 : 0;
    if (const char* ev = getenv("TW_CHUNK_TILES")) c.chunk_tiles = std::max(1, atoi(ev));
    if (const char* ev = getenv("TW_CHUNK_PAIRS_LEVELS"))
        for (int lv = 0; lv <= TW_MAX_LEVELS && ev; lv++) {
            c.chunk_pairs_lv[lv] = std::max(0, atoi(ev));
            ev = strchr(ev, ',');
            if (ev) ev++;
        }
    if (const char* ev = getenv("TW_PYR_GEN_TH")) c.pyr_gen_th = atoi(ev);
    c.lat_evtiming = getenv("TW_LAT_EVTIMING") != nullptr;
    if (const char* ev = getenv("TW_SAME_IMAGE")) c.same_image = atoi(ev) ? 1 : 0;
    if (const char* ev = getenv("TW_FI_MAXSEG")) c.fi_maxseg = std::min(64, std::max(1, atoi(ev)));
    if (const char* ev = getenv("TW_FI_MINSTEPS")) c.fi_minsteps = std::max(2, atoi(ev));
#ifndef TW_VARIANTS
    // The measured-slower A/B kernels are compiled only into `make VARIANTS=1` builds (libtwflow_variants.so): a
    // default build refuses their switches instead of silently running something else.
    {
        bool bad_lv = false;
        for (int v : c.blur_small_lv) bad_lv = bad_lv || v == 2 || v == 3 || v == 5;
        const bool bad = bad_lv || (c.blur_variant != 4) || (c.poly_variant != 1) || (c.blur_pipe != 0) || (c.blur_small == 2 || c.blur_small == 3 ||
                         c.blur_small == 5) || c.upd_ny == 1;
        if (bad) {
            *why = "twflow: TW_BLUR_VARIANT / TW_POLY_VARIANT / TW_BLUR_PIPE / TW_BLUR_SMALL=2,3,5 / TW_UPD_NY=1 select kernels "
                   "that are only in a VARIANTS=1 build (tidal-wave_amd/libtwflow_variants.so)\n";
            return TW_E_UNSUPPORTED;
        }
    }
#endif
    return TW_OK;
}

}  // namespace

struct tw_engine {
    const EngineConfig cfg;  // fixed at creation (make_engine_config)
    EngineOptions opt;       // tw_set_option
    explicit tw_engine(const EngineConfig& c) : cfg(c) { opt.poly_f32 = c.poly_f32; }
    int device = 0;
    // what the engine has allocated, in bytes as allocated: Buf::make / grow / release keep them (tw_debug_memory reports them)
    size_t dev_bytes = 0, pin_bytes = 0;
    Stream stream;
    Ctx ctx[NCTX];
    int cur = 0;  // context accepting submissions
    int64_t next_ticket = 1;
    std::map<std::pair<int, int>, std::unique_ptr<Plan>> plans;
    unsigned long long plan_clock = 0;
    DevBuf<double> Vd;  // running column sums of the box window (5 double planes per pair of a chunk)
    int copy_sync_skipped = 0;    // batches since the host last synchronised the copy stream (tw_wait)
    long long copy_ops = 0;       // host images queued on the copy stream so far
    PinBuf<uint8_t> h_bounce;     // bounce buffer of tw_submit_png8's pageable inputs (capacity in bytes)
    Stream stream2;
    Event ev_fork, ev_join;
    DevBuf<unsigned long long> dbg_stamps;  // TW_DEBUG_STAMPS=1: phase stamps of tw_pyr_taps (diagnostic runs only)
    std::string err;
    // device workspace, shared by all batches (execution is ordered on one stream)
    size_t ws_elems = 0;                 // capacity of I (floats); R = 5x, M = 5x each
    DevBuf<float> I, R, M[2];
    std::vector<DevBuf<float>> flow;     // per level, cap (levels>=1) or chunk0 (level 0) pairs x 2 planes
    DevBuf<float> lat_I, lat_R;  // the single-pair schedule's buffers: every level's I and R at once
    size_t lat_cap = 0;  // floats in lat_I (lat_R holds 5x)
    std::vector<Event> lat_ev;
    std::map<GraphKey, hipGraphExec_t> lat_graphs;  // captured single-pair schedules (dropped whenever a buffer moves)
    bool graph_capture_failed = false;  // this runtime could not capture the schedule: direct launches from then on
    bool graph_replay() const { return cfg.lat_graph && !graph_capture_failed; }  // TW_LAT_GRAPH=1 still in use
    Stream copy_stream;  // host -> device image uploads, overlapped with the compute stream
    // tw_submit_*_flow: device -> host copies of the flow fields (created when a host destination is first seen, so that
    // an engine that never asks for one keeps its queue use), the copies queued there so far, batches since the host last
    // synchronised it, and the device copy of a batch's destination table ([cap], created on first use)
    Stream d2h_stream;
    long long d2h_ops = 0;
    int d2h_sync_skipped = 0;
    DevBuf<FlowDst> d_fdst;
    DevBuf<FlowDst> d_fsrc;  // tw_submit_*_flow_init: the device copy of a batch's init source table ([cap], on first use)
    DevBuf<const uint8_t*> d_ptrs;  // [2*cap]
    DevBuf<int> d_count;            // [cap]
    // identical pairs (tw_pair_same): 1 where a pair's second image is byte for byte its first — the batch schedule then
    // computes that pair's pyramid levels and polynomial expansions once, at the levels tw_flow_iter runs (it reads R0 as R1)
    DevBuf<unsigned> d_same;           // [cap], of the batch enqueued last; all 0 until a batch schedule fills it
    int same_n = 0;                    // pairs of the batch enqueued last (tw_debug_same_flags)
    bool same_valid = false;           // ... and whether tw_pair_same ran for it
    DevBuf<float2> d_grid;             // [cap][G] dense grid samples (dx,dy)
    // hit regions (the next batch's gap is opt.regions_gap): the device copy of a batch's
    // rectangle table (region_table_bytes(cap), on first use), tw_hit_regions' label planes for grids that do not fit LDS
    // ([cap][G], on first use), and whether the LDS kernel's dynamic size has been announced to the runtime
    DevBuf<char> d_rgn;
    DevBuf<int> d_lab;
    bool rgn_attr = false;
    bool band_attr = false;  // ... and tw_band_search's
    // residual (the next batch's tolerance is opt.residual_tol): tw_warp_residual's dense
    // cell plane ([cap][G] cells of four ints, on first use) — the engine's, as d_grid: the batch's own tw_change_scan
    // consumes it before the next batch's launches write it
    DevBuf<int4> d_cells;
    // shift (the next batch's radius is opt.shift_radius): the records of the batch being enqueued ([cap]) and the four
    // profiles of each of its pairs ([cap][2 (w + h)] words), both on first use and the engine's, as d_cells: the batch's own
    // launches consume them, and its result copy reads the records, before the next batch's launches write them
    DevBuf<ShiftRec> d_shift;
    DevBuf<unsigned> d_sprof;
    // shift bands (the next batch's band height is opt.shift_bands): the band records of the batch being enqueued ([cap][nb])
    // and its pairs' row signatures ([cap][2][h][ceil(w / 64)] uint16), on first use and the engine's, as d_shift and d_sprof
    DevBuf<BandRec> d_bands;
    DevBuf<unsigned short> d_bsig;
    // diff image (tw_ticket_overlay): the staging a picture for a HOST destination is rendered into (dense rows of
    // round_up(3 w, 4) bytes), created by the first such call and grown on demand; device destinations are written in place
    DevBuf<uint8_t> d_ovl;
    // profiling: per kernel class, -2 = off, -1 = every level, k = level k only
    int prof_level[TW_K_COUNT] = {-2, -2, -2, -2, -2};
    std::vector<ProfPair> prof_pending[TW_K_COUNT];
    std::vector<Event> prof_free;
    // diagnostics (include/twflow_debug.h: tw_debug_launch_counts): launches per kernel family since the engine was created /
    // the counts were last reset, and the pairs (grid z) of each family's latest launch — what lets a test prove WHICH kernel ran
    unsigned long long launches[TW_DF_COUNT] = {};
    unsigned long long last_grid_z[TW_DF_COUNT] = {};
    // resident images (tw_image_*): the store's chunks (each one hipMalloc of at least RES_CHUNK bytes, kept until the engine
    // goes; `free` = offset -> length of its unused ranges, neighbours merged), every image that still owns a block, and the
    // handles a caller may pass in — a handle is looked up here, never dereferenced first
    struct ResChunk {
        DevBuf<uint8_t> base;
        size_t bytes = 0;
        std::map<size_t, size_t> free;
    };
    std::vector<ResChunk> res_chunks;
    std::set<tw_image*> res_images;         // own a block (handles > 0 or uses > 0)
    std::map<const tw_image*, tw_image*> res_handles;  // tw_image::handle -> the record, while handles > 0
    size_t res_in_use = 0, res_reserved = 0;
    unsigned long long res_chunk_allocs = 0;
};

namespace {

// every kernel launch of the library goes through here (tw_copy_f4, the copy-rate yardstick, excepted)
#define TW_LAUNCH(e, fam, kern, grid, ...)                         \
    do {                                                           \
        const dim3 _g = (grid);                                    \
        if (e) {                                                   \
            (e)->launches[fam]++;                                  \
            (e)->last_grid_z[fam] = _g.z;                          \
        }                                                          \
        hipLaunchKernelGGL(kern, _g, __VA_ARGS__);                 \
    } while (0)

#define TW_HIP(e, call)                                                                   \
    do {                                                                                  \
        hipError_t _err = (call);                                                         \
        if (_err != hipSuccess) {                                                         \
            (void)hipGetLastError(); /* the failure is reported here: do not leave it for a later launch check */ \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_err);               \
            return _err == hipErrorOutOfMemory ? TW_E_NOMEM : TW_E_DEVICE;                \
        }                                                                                 \
    } while (0)

#define TW_TRY(call)                      \
    do {                                  \
        const tw_status _st = (call);     \
        if (_st != TW_OK) return _st;     \
    } while (0)

size_t staged_image_bytes(int w, int h);

// ---- the resident image store (tw_image_*) ---------------------------------------------------------------------------
// Blocks are multiples of 256 bytes at multiples of 256 in a chunk (hipMalloc's own alignment is at least that), so a
// resident image is aligned as a d_img slot is and BatchEnqueue::aligned4 and every alignment-dependent kernel choice come out the same.
constexpr size_t RES_CHUNK = (size_t)64 << 20;  // a chunk is at least this large

void res_free(tw_engine* e, int chunk, size_t off, size_t bytes)
{
    std::map<size_t, size_t>& fr = e->res_chunks[chunk].free;
    auto it = fr.emplace(off, bytes).first;
    auto nx = std::next(it);
    if (nx != fr.end() && it->first + it->second == nx->first) {
        it->second += nx->second;
        fr.erase(nx);
    }
    if (it != fr.begin()) {
        auto pv = std::prev(it);
        if (pv->first + pv->second == it->first) {
            pv->second += it->second;
            fr.erase(it);
        }
    }
    e->res_in_use -= bytes;
}

// first fit over the chunks' free ranges, otherwise a new chunk (256 bytes of slack behind it, as every image region has)
tw_status res_alloc(tw_engine* e, size_t bytes, int* chunk, size_t* off)
{
    for (int pass = 0; pass < 2; pass++) {
        for (size_t k = 0; k < e->res_chunks.size(); k++) {
            std::map<size_t, size_t>& fr = e->res_chunks[k].free;
            for (auto it = fr.begin(); it != fr.end(); ++it) {
                if (it->second < bytes) continue;
                const size_t o = it->first, len = it->second;
                fr.erase(it);
                if (len > bytes) fr[o + bytes] = len - bytes;
                *chunk = (int)k;
                *off = o;
                e->res_in_use += bytes;
                return TW_OK;
            }
        }
        if (pass) break;
        tw_engine::ResChunk ch;
        ch.bytes = std::max(RES_CHUNK, bytes);
        TW_TRY(ch.base.alloc(e, ch.bytes + 256));  // (the store's own total: res_reserved)
        ch.free[0] = ch.bytes;
        e->res_reserved += ch.bytes + 256;
        e->res_chunk_allocs++;
        e->res_chunks.push_back(std::move(ch));
    }
    e->err = "resident store: no block";
    return TW_E_NOMEM;
}

// a new image of w x h with one handle; its content is whatever the caller queues on the copy stream next
tw_status image_new(tw_engine* e, int w, int h, tw_image** out)
{
    int chunk = 0;
    size_t off = 0;
    const size_t bytes = staged_image_bytes(w, h);
    TW_TRY(res_alloc(e, bytes, &chunk, &off));
    tw_image* im = new tw_image();
    im->owner = e;
    im->d = e->res_chunks[chunk].base + off;
    im->w = w;
    im->h = h;
    im->chunk = chunk;
    im->off = off;
    im->bytes = bytes;
    im->handles = 1;
    static std::atomic<uintptr_t> next_handle{0x1000};
    im->handle = (tw_image*)next_handle.fetch_add(16);
    e->res_images.insert(im);
    e->res_handles[im->handle] = im;
    *out = im;
    return TW_OK;
}

// the block returns to the store when no handle and no batch is left
void image_settle(tw_image* im)
{
    if (im->handles > 0 || im->uses > 0) return;
    tw_engine* e = im->owner;
    res_free(e, im->chunk, im->off, im->bytes);
    e->res_images.erase(im);
    delete im;
}

void image_unuse(tw_image* im)
{
    im->uses--;
    image_settle(im);
}

// tw_image_keep's copy: w x h bytes at src (rows `pitch` apart) to the image's dense rows, device to device on the copy stream
tw_status queue_keep_copy(tw_engine* e, tw_image* im, const uint8_t* src, long long pitch)
{
    const size_t w = (size_t)im->w, h = (size_t)im->h;
    if ((size_t)pitch == w) TW_HIP(e, hipMemcpyAsync(im->d, src, w * h, hipMemcpyDeviceToDevice, e->copy_stream));
    else TW_HIP(e, hipMemcpy2DAsync(im->d, w, src, (size_t)pitch, w, h, hipMemcpyDeviceToDevice, e->copy_stream));
    e->copy_ops++;
    return TW_OK;
}

// tw_jpeg_idct's grid for `nimg` images of up to w x h pixels: a workgroup takes JPEG_WG_BLOCKS adjacent blocks of a block row
dim3 jpeg_idct_grid(int w, int h, int nimg)
{
    return dim3((unsigned)((w + 8 * JPEG_WG_BLOCKS - 1) / (8 * JPEG_WG_BLOCKS)), (unsigned)((h + 7) / 8), (unsigned)nimg);
}

// tw_mask_rects' grid for `nrect` rectangles of up to w x h pixels: a workgroup takes 64 aligned dwords of MASK_ROWS rows; a
// row of w bytes that starts anywhere in a dword touches at most (w + 6) / 4 dwords
dim3 mask_rects_grid(int w, int h, int nrect)
{
    return dim3((unsigned)(((w + 6) / 4 + 63) / 64), (unsigned)((h + MASK_ROWS - 1) / MASK_ROWS), (unsigned)nrect);
}

// The rectangles of a tw_submit_*_ignore / tw_stage_mask_rects call, clipped to a w x h image; the empty ones are dropped.
// Refuses what the calls refuse (include/twflow.h); no HIP call.
tw_status clip_ignore(tw_engine* e, const tw_rect* ignore, int n_ignore, int w, int h, std::vector<tw_rect>* out)
{
    out->clear();
    if (n_ignore < 0 || n_ignore > TW_MAX_IGNORE || (n_ignore > 0 && !ignore)) {
        e->err = "bad ignore rectangles (a count outside 0 .. TW_MAX_IGNORE, or a null table)";
        return TW_E_BAD_PARAMETER;
    }
    for (int i = 0; i < n_ignore; i++)
        if (ignore[i].width < 0 || ignore[i].height < 0) {
            e->err = "bad ignore rectangle (negative width or height)";
            return TW_E_BAD_PARAMETER;
        }
    for (int i = 0; i < n_ignore; i++) {
        const tw_rect& r = ignore[i];
        const long long x0 = std::max<long long>(r.x, 0), x1 = std::min<long long>((long long)r.x + r.width, w);
        const long long y0 = std::max<long long>(r.y, 0), y1 = std::min<long long>((long long)r.y + r.height, h);
        if (x0 < x1 && y0 < y1) out->push_back(tw_rect{(int)x0, (int)y0, (int)(x1 - x0), (int)(y1 - y0)});
    }
    return TW_OK;
}

// One row of tw_resize_u8's job table: sw x sh at src -> dw x dh at dst, with cv::resize's scales (inv_scale = (double)dsize /
// ssize, scale = 1. / inv_scale: computed here, in double, once per job)
ResizeJob resize_job(const uint8_t* src, int sw, int sh, long long spitch, uint8_t* dst, int dw, int dh, long long dpitch)
{
    ResizeJob rj;
    rj.src = src;
    rj.dst = dst;
    rj.spitch = spitch;
    rj.dpitch = dpitch;
    rj.scale_x = 1. / ((double)dw / sw);
    rj.scale_y = 1. / ((double)dh / sh);
    rj.sw = sw;
    rj.sh = sh;
    rj.dw = dw;
    rj.dh = dh;
    return rj;
}

// ---- Buf: the engine's allocations and its books ---------------------------------------------------------------------
size_t& DeviceMem::books(tw_engine* e) { return e->dev_bytes; }
size_t& PinnedMem::books(tw_engine* e) { return e->pin_bytes; }

template <typename T, typename Mem>
tw_status Buf<T, Mem>::alloc(tw_engine* e, size_t nbytes)
{
    TW_HIP(e, Mem::malloc((void**)&p, nbytes));
    bytes = nbytes;
    return TW_OK;
}
// A buffer that is made once: `nbytes` (the caller's size, slack included) unless it exists already.
template <typename T, typename Mem>
tw_status Buf<T, Mem>::make(tw_engine* e, size_t nbytes)
{
    if (p) return TW_OK;
    TW_TRY(alloc(e, nbytes));
    Mem::books(e) += bytes;
    return TW_OK;
}
template <typename T, typename Mem>
void Buf<T, Mem>::release(tw_engine* e)
{
    if (p) Mem::free((void*)p);
    Mem::books(e) -= bytes;
    p = nullptr;
    cap = bytes = 0;
}
// The one "grow this buffer" step (buffers grow, never shrink): when `new_cap` (in the buffer's own unit) exceeds `cap`,
// wait for `sync` if one is given (the stream whose queued work may still touch the old buffer), free the buffer and
// allocate `nbytes`.  Pointer and capacity are cleared BEFORE the allocation, so that a failed one leaves an empty buffer,
// not a dangling one, and the next call tries again.
template <typename T, typename Mem>
tw_status Buf<T, Mem>::grow(tw_engine* e, size_t new_cap, size_t nbytes, hipStream_t sync)
{
    if (new_cap <= cap) return TW_OK;
    if (sync) TW_HIP(e, hipStreamSynchronize(sync));
    release(e);
    TW_TRY(make(e, nbytes));
    cap = new_cap;
    return TW_OK;
}

// ---- the runtime is never handed a pageable host pointer ------------------------------------------------
// Round 4 recorded a GPU memory-access fault on a malloc-heap address inside a synchronous copy, right after a
// hipHostRegister / hipHostUnregister cycle on a neighbouring, non-page-aligned heap block: for a
// pageable operand the runtime pins the enclosing pages on the fly, and that pinning raced with the pages a partial-page
// registration had just released.  Two rules close it at the source: tw_host_register only takes whole pages the
// caller owns (below), and EVERY synchronous copy of this library whose host side is not a page-locked range the
// library knows goes through the engine's own page-locked bounce buffer, in bounded chunks.
bool host_range_is_page_locked(const void* p, size_t n);  // PinRegistry::covers (defined below)
constexpr size_t BOUNCE_CHUNK = 8u << 20;
tw_status bounce_reserve(tw_engine* e, size_t bytes)
{
    return e->h_bounce.grow(e, bytes, bytes);
}
// synchronous host -> device / device -> host copies of any host pointer (null stream, like the hipMemcpy they replace)
tw_status h2d_sync(tw_engine* e, void* d, const void* h, size_t n)
{
    if (!n) return TW_OK;
    if (host_range_is_page_locked(h, n)) {
        TW_HIP(e, hipMemcpy(d, h, n, hipMemcpyHostToDevice));
        return TW_OK;
    }
    tw_status r = bounce_reserve(e, std::min(n, BOUNCE_CHUNK));
    if (r) return r;
    for (size_t o = 0; o < n; o += BOUNCE_CHUNK) {
        const size_t k = std::min(BOUNCE_CHUNK, n - o);
        memcpy(e->h_bounce, (const uint8_t*)h + o, k);
        TW_HIP(e, hipMemcpy((uint8_t*)d + o, e->h_bounce, k, hipMemcpyHostToDevice));
    }
    return TW_OK;
}
tw_status d2h_sync(tw_engine* e, void* h, const void* d, size_t n)
{
    if (!n) return TW_OK;
    if (host_range_is_page_locked(h, n)) {
        TW_HIP(e, hipMemcpy(h, d, n, hipMemcpyDeviceToHost));
        return TW_OK;
    }
    tw_status r = bounce_reserve(e, std::min(n, BOUNCE_CHUNK));
    if (r) return r;
    for (size_t o = 0; o < n; o += BOUNCE_CHUNK) {
        const size_t k = std::min(BOUNCE_CHUNK, n - o);
        TW_HIP(e, hipMemcpy(e->h_bounce, (const uint8_t*)d + o, k, hipMemcpyDeviceToHost));
        memcpy((uint8_t*)h + o, e->h_bounce, k);
    }
    return TW_OK;
}
// scoped device allocations (per-stage test entry points, slow paths)
struct Tmp {
    std::vector<void*> v;
    ~Tmp()
    {
        for (void* p : v) (void)hipFree(p);
    }
    template <typename T>
    T* alloc(size_t n)
    {
        void* p = nullptr;
        if (hipMalloc(&p, n * sizeof(T) + 256) != hipSuccess) return nullptr;
        v.push_back(p);
        return (T*)p;
    }
};
template <typename T>
tw_status upload_vec(tw_engine* e, Plan* pl, const std::vector<T>& v, T** out)
{
    DevBuf<char> d;
    TW_TRY(d.alloc(e, v.size() * sizeof(T) + 16));  // (the plan's own total: owned_bytes)
    pl->owned_bytes += d.bytes;
    TW_TRY(h2d_sync(e, d.p, v.data(), v.size() * sizeof(T)));
    *out = (T*)d.p;
    pl->owned.push_back(std::move(d));
    return TW_OK;
}

int plan_levels(int w0, int h0, double pyr_scale, int levels)
{
    const int min_size = 32;
    int k;
    double scale;
    for (k = 0, scale = 1; k < levels; k++) {
        scale *= pyr_scale;
        if (w0 * scale < min_size || h0 * scale < min_size) break;
    }
    return k;
}

void level_geometry(int w0, int h0, double pyr_scale, int k, int* w, int* h, double* sigma, int* ksize,
                    double* scale_out)
{
    double scale = 1;
    for (int i = 0; i < k; i++) scale *= pyr_scale;
    const double sg = (1. / scale - 1) * 0.5;
    int smooth_sz = cv_round(sg * 5) | 1;
    if (smooth_sz < 3) smooth_sz = 3;
    *w = cv_round(w0 * scale);
    *h = cv_round(h0 * scale);
    *sigma = sg;
    *ksize = smooth_sz;
    *scale_out = scale;
}

int pyr_nrows_max(const ResizeTab& t, int h, int h0, int r, int th = PYR_TH)
{
    int mx = 0;
    for (int y0 = 0; y0 < h; y0 += th) {
        const int yB = std::min(y0 + th - 1, h - 1);
        const int ylo = std::min(std::max(t.yofs[y0], 0), h0 - 1) - r;
        const int yhi = std::min(std::max(t.yofs[yB] + 1, 0), h0 - 1) + r;
        mx = std::max(mx, yhi - ylo + 1);
    }
    return mx;
}

// captured schedules hold workspace and table addresses: whenever one of those may move, they go
void drop_graphs(tw_engine* e)
{
    for (auto& kv : e->lat_graphs) (void)hipGraphExecDestroy(kv.second);
    e->lat_graphs.clear();
}

// pairs one launch covers at a level of w x h pixels (level index k): enough 8-row x 240-column tiles of two images to cover
// the 256 CUs many times over.  plan_geometry is its one caller: every reader takes LevelPlan::chunk.
int pairs_per_launch(const EngineConfig& cfg, int w, int h, int k)
{
    const long long tiles = (long long)((w + PE_TW - 1) / PE_TW) * ((h + PE_TH - 1) / PE_TH) * 2;
    // measured at 1080p: 4096 -> 16384 tiles per launch is +11 % pairs/s (fewer tails and gaps), 16384 -> 34000
    // (16 pairs per level-0 launch) another +2.5 %, 34000 -> a whole 64-pair batch per launch +1.5 %, a whole
    // 128-pair batch +4 % (round 2): every kernel boundary costs a drain, a fill and an L2 write-back of the dirty
    // M planes, and 288 GB of HBM make the workspace of a whole batch (23 GB at 128 x 1080p) a non-issue.  So a
    // launch covers the whole batch unless that exceeds 300 000 tiles (TW_CHUNK_TILES).
    long long c = (cfg.chunk_tiles + tiles - 1) / tiles;
    // TW_CHUNK_PAIRS_LEVELS: the round-4 Infinity-Cache experiment (does a level's chain run faster when a chunk's R / M
    // planes fit the 256 MB memory-side cache between its kernels?  profiles/r04_mall_chunks.md)
    if (cfg.chunk_pairs_lv[k] > 0) c = cfg.chunk_pairs_lv[k];
    return (int)std::min<long long>(std::max<long long>(c, 1), cfg.cap);
}

// The host tables of a plan on their way to the device: what plan_geometry computes and get_plan uploads.
struct PlanTables {
    std::vector<ResizeTab> pyr;  // full resolution -> level k
    std::vector<ResizeTab> ups;  // level k + 1 -> level k (flow upsampling; none at the coarsest level)
    AreaTab init;                // full resolution -> the coarsest level (tw_flow_area_init)
};

// The pure part of a plan: everything that depends only on (parameters, engine switches, cap, w0, h0), with no HIP call
// and no engine state written.  get_plan uploads `tabs` behind it; tw_level_chunk, tw_level_runs_flow_iter, the byte model
// and tw_debug_level_plan read the geometry as it stands (device pointers null).  *why: the reason of a refusal.
tw_status plan_geometry(const EngineConfig& cfg, int w0, int h0, Plan* pl, PlanTables* tabs, const char** why)
{
    pl->w0 = w0;
    pl->h0 = h0;
    pl->levels = plan_levels(w0, h0, cfg.p.pyrScale, std::min(std::max(cfg.p.pyrLevels, 0), TW_MAX_LEVELS));
    pl->lv.resize(pl->levels + 1);
    tabs->pyr.resize(pl->levels + 1);
    tabs->ups.resize(pl->levels + 1);
    for (int k = 0; k <= pl->levels; k++) {
        LevelPlan& L = pl->lv[k];
        level_geometry(w0, h0, cfg.p.pyrScale, k, &L.w, &L.h, &L.sigma, &L.ksize, &L.scale);
        if (L.w < 1 || L.h < 1 || L.ksize > PYR_MAXK - 1) {
            *why = "pyramid level degenerate or smoothing kernel too large";
            return TW_E_UNSUPPORTED;
        }
        L.ld = round_up(L.w, 32);
        L.ps = (long long)L.ld * L.h;
        L.chunk = pairs_per_launch(cfg, L.w, L.h, k);
    }
    for (int k = 0; k <= pl->levels; k++) {
        LevelPlan& L = pl->lv[k];
        ResizeTab& t = tabs->pyr[k];
        make_resize_tab(w0, h0, L.w, L.h, t);
        gaussian_kernel(L.ksize, L.sigma, L.h_taps);
        L.mode = t.mode;
        L.xmax = t.xmax;
        if (L.ksize == 3) memcpy(L.h_kern, L.h_taps.data(), sizeof(L.h_kern));
        L.nrows_max = pyr_nrows_max(t, L.h, h0, L.ksize / 2);
        // Round 6: the unstaged kernel takes 4-row tiles when an 8-row tile's row buffer is more than 32 KB (a deep level of a
        // large image: BASELINE configs[4]'s 39- / 79-tap levels of a 4K pyramid).  Twice the workgroups at 0.6 of the work
        // each, five / three of them per CU instead of three / two, and the last round of a launch no longer a quarter full
        // (TW_PYR_GEN_TH=8: the old tiles, A/B).
        {
            const size_t rb8 = (size_t)L.nrows_max * (t.mode == 0 ? PYR_TW : 2 * PYR_TW) * 4;
            L.gen_th = cfg.pyr_gen_th >= 1 && cfg.pyr_gen_th <= PYR_TH ? cfg.pyr_gen_th : (rb8 > 32 * 1024 ? 4 : PYR_TH);
            L.gen_nrows_max = L.gen_th == PYR_TH ? L.nrows_max : pyr_nrows_max(t, L.h, h0, L.ksize / 2, L.gen_th);
        }
        const size_t lds = (size_t)(PYR_MAXK + (size_t)L.nrows_max * (t.mode == 0 ? PYR_TW : 2 * PYR_TW)) * 4;
        if (lds > 160 * 1024) {
            *why = "pyramid tile does not fit LDS (scale/kernel too large)";
            return TW_E_UNSUPPORTED;
        }
        {
            // widest staged source span over the tiles of this level (same formulas as the kernel)
            const int r = L.ksize / 2;
            int span = 0;
            for (int x0 = 0; x0 < L.w; x0 += PYR_TW) {
                const int xl = std::min(x0, L.w - 1), xr = std::min(x0 + PYR_TW - 1, L.w - 1);
                const int Xfirst = t.mode == 0 ? xl : t.xofs[xl];
                const int Xlast = t.mode == 0 ? xr : t.xofs[xr] + 1;
                const int xlo_a = (Xfirst - r) & ~3;
                span = std::max(span, ((Xlast + r - xlo_a) / 4 + 1) * 4);
            }
            const size_t lds2 = lds + (size_t)L.nrows_max * span;
            L.pitch_b = (lds2 + (size_t)L.nrows_max * 8 + 64 <= 64 * 1024 && L.ksize <= 63) ? span : 0;
        }
        if (k < pl->levels) {
            const LevelPlan& P = pl->lv[k + 1];
            ResizeTab& u = tabs->ups[k];
            make_resize_tab(P.w, P.h, L.w, L.h, u);
            if (u.mode == 2) {
                // cannot happen for pyr_scale < 1 (the previous level is never twice as large)
                *why = "unexpected area-fast flow resize";
                return TW_E_UNSUPPORTED;
            }
            L.uxmax = u.xmax;
        }
    }
    {
        // tw_flow_area_init: full resolution -> the coarsest level (INTER_AREA).  Mode 1 stages a tile of tw output columns'
        // iy source rows (both channels) in at most 32 KB of LDS; blocks too large for that read memory directly (tw = 0)
        const LevelPlan& C = pl->lv[pl->levels];
        AreaTab& t = tabs->init;
        make_area_tab(w0, h0, C.w, C.h, t);
        pl->init_mode = t.mode;
        pl->init_ix = t.ix;
        pl->init_iy = t.iy;
        if (t.mode == 1) {
            const int fit = 32768 / (t.ix * t.iy * 8);
            pl->init_tw = fit >= 4 ? std::min(128, fit / 4 * 4) : 0;
        }
    }
    // tw_pyr_23 eligibility: both levels are exact INTER_LINEAR reductions by 4 and 8 (sample columns s*x + s/2 - 1 and
    // + 1 with weights 0.5 / 0.5, no single-tap tail, rows alike) with the 9- / 19-tap kernels of pyr_scale = 0.5
    if (pl->levels >= 3 && pl->lv[2].ksize == 9 && pl->lv[3].ksize == 19 && pl->lv[2].w == 2 * pl->lv[3].w &&
        pl->lv[2].h == 2 * pl->lv[3].h && w0 >= 64 && h0 >= 64) {
        bool exact = true;
        for (int k = 2; k <= 3 && exact; k++) {
            const LevelPlan& L = pl->lv[k];
            const ResizeTab& t = tabs->pyr[k];
            const int sc = 1 << k;
            exact = t.mode == 1 && t.xmax == L.w && L.w * sc == w0 && L.h * sc == h0;
            for (int x = 0; x < L.w && exact; x++)
                exact = t.xofs[x] == sc * x + sc / 2 - 1 && t.alpha[2 * x] == 0.5f && t.alpha[2 * x + 1] == 0.5f;
            for (int y = 0; y < L.h && exact; y++)
                exact = t.yofs[y] == sc * y + sc / 2 - 1 && t.beta[2 * y] == 0.5f && t.beta[2 * y + 1] == 0.5f;
        }
        if (exact) {
            pl->fused23 = true;
            memcpy(pl->k19 + 1, pl->lv[3].h_taps.data(), sizeof(float) * 19);
            memcpy(pl->k9 + 1, pl->lv[2].h_taps.data(), sizeof(float) * 9);
        }
    }
    return TW_OK;
}

// the device part of a plan: the tables plan_geometry made, uploaded
tw_status upload_plan_tables(tw_engine* e, Plan* pl, const PlanTables& tabs)
{
    for (int k = 0; k <= pl->levels; k++) {
        LevelPlan& L = pl->lv[k];
        const ResizeTab& t = tabs.pyr[k];
        TW_TRY(upload_vec(e, pl, t.xofs, &L.d_xofs));
        TW_TRY(upload_vec(e, pl, t.yofs, &L.d_yofs));
        TW_TRY(upload_vec(e, pl, t.alpha, &L.d_alpha));
        TW_TRY(upload_vec(e, pl, t.beta, &L.d_beta));
        TW_TRY(upload_vec(e, pl, L.h_taps, &L.d_kern));
        if (k < pl->levels) {
            const ResizeTab& u = tabs.ups[k];
            TW_TRY(upload_vec(e, pl, u.xofs, &L.d_uxofs));
            TW_TRY(upload_vec(e, pl, u.yofs, &L.d_uyofs));
            TW_TRY(upload_vec(e, pl, u.alpha, &L.d_ualpha));
            TW_TRY(upload_vec(e, pl, u.beta, &L.d_ubeta));
        }
    }
    const AreaTab& t = tabs.init;
    if (t.mode == 2) {
        TW_TRY(upload_vec(e, pl, t.xstart, &pl->d_ixs));
        TW_TRY(upload_vec(e, pl, t.xsi, &pl->d_ixi));
        TW_TRY(upload_vec(e, pl, t.xalpha, &pl->d_ixa));
        TW_TRY(upload_vec(e, pl, t.ystart, &pl->d_iys));
        TW_TRY(upload_vec(e, pl, t.ysi, &pl->d_iyi));
        TW_TRY(upload_vec(e, pl, t.ybeta, &pl->d_iyb));
    }
    return TW_OK;
}

tw_status get_plan(tw_engine* e, int w0, int h0, Plan** out)
{
    auto key = std::make_pair(w0, h0);
    auto it = e->plans.find(key);
    if (it != e->plans.end()) {
        it->second->last_use = ++e->plan_clock;
        *out = it->second.get();
        return TW_OK;
    }
    if (e->plans.size() >= 64) {
        // a long-running service that sees arbitrary image sizes must not collect plans (and their device tables) for
        // ever: the 65th size evicts the least recently used one (emptying the whole cache made a service
        // that cycles through 65 sizes rebuild all of them on every wrap).  Queued launches may still read the evicted
        // plan's tables, so the streams are drained first — once per new size, and only beyond 64 sizes.
        auto victim = e->plans.begin();
        for (auto jt = e->plans.begin(); jt != e->plans.end(); ++jt)
            if (jt->second->last_use < victim->second->last_use) victim = jt;
        TW_HIP(e, hipStreamSynchronize(e->stream));
        TW_HIP(e, hipStreamSynchronize(e->stream2));
        drop_graphs(e);
        e->plans.erase(victim);
    }
    std::unique_ptr<Plan> pl(new Plan());
    pl->last_use = ++e->plan_clock;
    PlanTables tabs;
    const char* why = "";
    tw_status s = plan_geometry(e->cfg, w0, h0, pl.get(), &tabs, &why);
    if (s) e->err = why;
    else s = upload_plan_tables(e, pl.get(), tabs);
    if (s) return s;
    *out = pl.get();
    e->plans[key] = std::move(pl);
    return TW_OK;
}

// Device workspace for a plan (grown, never shrunk).  Safe to reallocate only when nothing is queued.
tw_status reserve_workspace(tw_engine* e, const Plan* pl, int span)
{
    size_t need = 0;
    for (const LevelPlan& L : pl->lv) need = std::max(need, (size_t)L.ps * 2 * L.chunk);
    need *= e->cfg.lanes;  // one workspace per lane, carved from the same allocations
    bool grow = need > e->ws_elems || e->flow.size() < pl->lv.size() || (e->cfg.box && need / 2 * 5 > e->Vd.cap);
    if (!grow)
        for (size_t k = 0; k < pl->lv.size(); k++) {
            const size_t fc = (size_t)pl->lv[k].ps * 2 * (k == 0 ? pl->lv[0].chunk * e->cfg.lanes : e->cfg.cap);
            if (fc > e->flow[k].cap) grow = true;
        }
    const size_t G = span > 0 ? (size_t)tw_grid_capacity(pl->w0, pl->h0, span) : 0;
    if (G * e->cfg.cap > e->d_grid.cap) grow = true;
    size_t need_lat = 0;
    for (const LevelPlan& L : pl->lv) need_lat += (size_t)L.ps * 2;
    if (e->cfg.lat_streams && (need_lat > e->lat_cap || e->lat_ev.size() < pl->lv.size())) grow = true;
    if (!grow) return TW_OK;
    TW_HIP(e, hipStreamSynchronize(e->stream));
    TW_HIP(e, hipStreamSynchronize(e->stream2));
    drop_graphs(e);
    if (need > e->ws_elems) {  // (all four go before the first comes back; ws_elems stands for all four)
        e->ws_elems = 0;
        for (DevBuf<float>* b : {&e->I, &e->R, &e->M[0], &e->M[1]}) b->release(e);
        TW_TRY(e->I.make(e, need * 4 + 256));
        TW_TRY(e->R.make(e, need * 5 * 4 + 256));
        TW_TRY(e->M[0].make(e, need / 2 * 5 * 4 + 256));
        TW_TRY(e->M[1].make(e, need / 2 * 5 * 4 + 256));
        e->ws_elems = need;
    }
    if (e->cfg.lat_streams && need_lat > e->lat_cap) {
        e->lat_cap = 0;
        for (DevBuf<float>* b : {&e->lat_I, &e->lat_R}) b->release(e);
        TW_TRY(e->lat_I.make(e, need_lat * 4 + 256));
        TW_TRY(e->lat_R.make(e, need_lat * 5 * 4 + 256));
        e->lat_cap = need_lat;
    }
    while (e->cfg.lat_streams && e->lat_ev.size() < pl->lv.size()) {
        Event ev;
        TW_HIP(e, hipEventCreateWithFlags(&ev.h, e->cfg.lat_evtiming ? hipEventDefault : hipEventDisableTiming));
        e->lat_ev.push_back(std::move(ev));
    }
    if (e->cfg.box) TW_TRY(e->Vd.grow(e, need / 2 * 5, need / 2 * 5 * sizeof(double) + 256));
    if (e->flow.size() < pl->lv.size()) e->flow.resize(pl->lv.size());
    for (size_t k = 0; k < pl->lv.size(); k++) {
        const size_t fc = (size_t)pl->lv[k].ps * 2 * (k == 0 ? pl->lv[0].chunk * e->cfg.lanes : e->cfg.cap);
        TW_TRY(e->flow[k].grow(e, fc, fc * 4 + 256));
    }
    return e->d_grid.grow(e, G * e->cfg.cap, G * e->cfg.cap * sizeof(float2) + 256);
}

// ---- profiling hooks -------------------------------------------------------------------------------
Event prof_event(tw_engine* e)
{
    Event ev;
    if (!e->prof_free.empty()) {
        ev = std::move(e->prof_free.back());
        e->prof_free.pop_back();
    } else (void)hipEventCreate(&ev.h);
    return ev;
}

struct ProfScope {
    tw_engine* e;
    hipStream_t st;
    bool on;
    int kc;
    ProfPair pp;
    ProfScope(tw_engine* e_, hipStream_t st_, int kclass, int level) : e(e_), st(st_), kc(kclass)
    {
        on = (e->prof_level[kclass] == -1 || (e->prof_level[kclass] >= 0 && e->prof_level[kclass] == level));
        if (on) {
            pp.a = prof_event(e);
            pp.b = prof_event(e);
            (void)hipEventRecord(pp.a, st);
        }
    }
    ~ProfScope()
    {
        if (on) {
            (void)hipEventRecord(pp.b, st);
            e->prof_pending[kc].push_back(std::move(pp));
        }
    }
};

// A side job of the single-pair schedule: image-only work (a band of a level's polynomial expansion, or the level 0 / 1
// images) that rides in the same launch as a kernel of the dependent flow chain (the twin kernels of twflow_kernels.hip.h).
// A launcher that has a twin for its kernel sets *used; the caller launches the job by itself otherwise.
struct SideJob {
    int kind = 0;        // 1: polynomial-expansion band (tw_polyexp_pk<7, 8, 0>), 2: tw_pyr_k3f
    int need_level = 0;  // the finest level whose flow chain reads what the job writes
    int carry_level = -1;       // >= 0: only a chain launch of this level carries the job
    bool windows_only = false;  // ... and only its window launches, not its FarnebackUpdateMatrices launch
    PolyArgs pa;
    PyrK3fArgs ka;
    VGrid g;             // the job's workgroups
    unsigned n() const { return g.gx * g.gy * g.gz; }
};
TwinGrid make_twin(const dim3& ga, const SideJob& s)
{
    TwinGrid t;
    t.a = VGrid{ga.x, ga.y, ga.z, 0u, 0u};
    t.b = s.g;
    t.nA = ga.x * ga.y * ga.z;
    t.nA8 = (t.nA + 7u) & ~7u;
    return t;
}
void launch_side_alone(tw_engine* e, hipStream_t st, const SideJob& s)
{
    if (s.kind == 1) TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp_band, dim3(s.n()), dim3(256), 0, st, s.pa, s.g);
    else if (s.kind == 2) TW_LAUNCH(e, TW_DF_PYR_K3F, tw_pyr_k3f, dim3(s.g.gx, s.g.gy, s.g.gz), dim3(256), 0, st, s.ka);
}

// tw_update_matrices<UPSAMPLE, NY>: NY pixels of a column per lane (TW_UPD_NY, default 2)
template <bool UP>
void launch_upd_kernel(tw_engine* e, hipStream_t st, int w, int h, int npairs, const UpdArgs& a, const SideJob* side = nullptr,
                       bool* side_used = nullptr)
{
#ifdef TW_VARIANTS
    if (e->cfg.upd_ny == 1) {
        TW_LAUNCH(e, TW_DF_UPDATE_MATRICES, (tw_update_matrices<UP, 1>), dim3((w + 63) / 64, (h + 3) / 4, npairs), dim3(256), 0, st, a);
        return;
    }
#endif
    const dim3 grid((w + 63) / 64, (h + 7) / 8, npairs);
    if (side && side_used && side->kind == 1) {
        const TwinGrid t = make_twin(grid, *side);
        TW_LAUNCH(e, TW_DF_TWIN, tw_twin_upd_poly<UP>, dim3(t.nA8 + side->n()), dim3(256), 0, st, a, side->pa, t);
        *side_used = true;
        return;
    }
    TW_LAUNCH(e, TW_DF_UPDATE_MATRICES, (tw_update_matrices<UP, 2>), grid, dim3(256), 0, st, a);
}

// ---- kernel launch helpers (nz = images or pairs in this launch) -------------------------------------
// The choice of one pyramid level's launch — the ONE place it is made: launch_pyr launches it and tw_debug_pyr_plan shows it
// to the tests.  The register kernel for 3-tap levels that copy or halve exactly, the shared-window row filter for staged
// levels of 7 .. 63 taps that resize, the staged generic kernel where the tile's source region fits plan_geometry's 64 KB LDS
// budget, the unstaged one otherwise.  (The two launches that write two levels each, tw_pyr_23 and tw_pyr_k3f, are the
// plan's decisions: Plan::fused23, pyr01_fusable; pyr23_threads is the former's workgroup size.)
enum PyrKernel { PYR_KN_K3 = 0, PYR_KN_K3F, PYR_KN_23, PYR_KN_TAPS, PYR_KN_LEVEL_LDS, PYR_KN_LEVEL };
struct PyrChoice {
    int kernel;     // PyrKernel
    int targ;       // the template argument: tw_pyr_k3's MODE (0 / 2), tw_pyr_taps' KS (9 / 19 / 39, 0: any size); 0 otherwise
    int family;     // tw_debug_family (a staged generic launch is ALSO counted in TW_DF_PYR_LEVEL_LDS)
    int block;      // threads per workgroup
    int tw, th;     // output-tile columns and rows
    unsigned gx, gy;
    size_t lds;     // dynamic LDS bytes
    int pitch;      // bytes per staged source row as the kernel lays them out (0: nothing is staged)
    int aligned4;   // whole-dword loads of the source rows allowed
    int nrows_max;  // row-buffer height the kernel is given
};
// img_al4: every image address of the launch is 4-byte aligned (the row stride decides with it)
PyrChoice choose_pyr(const EngineConfig& cfg, const Plan* pl, int k, long long stride, int img_al4)
{
    const LevelPlan& L = pl->lv[k];
    const int P = (L.mode == 0) ? PYR_TW : 2 * PYR_TW;
    const int aligned4 = (stride % 4 == 0) ? img_al4 : 0;
    PyrChoice c{PYR_KN_LEVEL, 0, TW_DF_PYR_LEVEL, 256, PYR_TW, PYR_TH, (unsigned)((L.w + PYR_TW - 1) / PYR_TW),
                (unsigned)((L.h + PYR_TH - 1) / PYR_TH), 0, 0, aligned4, L.nrows_max};
    if (L.ksize == 3 && (L.mode == 0 || L.mode == 2) && pl->w0 >= 16 && !cfg.pyr_generic) {
        // register-only fast path (3 taps, same-size or exact 2x2 area resize)
        c.kernel = PYR_KN_K3;
        c.targ = L.mode;
        c.family = TW_DF_PYR_K3;
        c.tw = 256;
        c.th = L.mode == 0 ? 8 : 4;
        c.gx = (L.w + 255) / 256;
        c.gy = (L.h + c.th - 1) / c.th;
        return c;
    }
    if (L.pitch_b > 0 && L.mode != 0 && L.ksize >= 7 && cfg.pyr_generic == 0) {
        // coarse levels: shared-window row filter (tw_pyr_taps)
        const int pd = (L.pitch_b / 4 + 1) | 1;
        c.kernel = PYR_KN_TAPS;
        c.targ = (L.ksize == 9 || L.ksize == 19 || L.ksize == 39) ? L.ksize : 0;
        c.family = TW_DF_PYR_TAPS;
        c.lds = ((size_t)L.nrows_max * (2 * PYR_TW) + (size_t)L.nrows_max * pd + 4) * 4;
        c.pitch = pd * 4;
        return c;
    }
    if (L.pitch_b > 0 && cfg.pyr_generic != 1) {
        c.kernel = PYR_KN_LEVEL_LDS;
        c.lds = (size_t)(PYR_MAXK + (size_t)L.nrows_max * P) * 4 + (size_t)L.nrows_max * L.pitch_b;
        c.pitch = L.pitch_b;
        return c;
    }
    c.th = L.gen_th;
    c.gy = (L.h + L.gen_th - 1) / L.gen_th;
    c.nrows_max = L.gen_nrows_max;
    c.lds = (size_t)(PYR_MAXK + (size_t)L.gen_nrows_max * P) * 4;
    c.aligned4 = 0;  // (the unstaged kernel takes no such argument: it reads bytes, and unaligned dwords of interior taps)
    return c;
}
// threads of a tw_pyr_23 workgroup: TW_PYR23_THREADS, or 1024 for a launch of one pair's images and 512 for more
int pyr23_threads(const EngineConfig& cfg, int nimg) { return cfg.pyr23_threads ? cfg.pyr23_threads : nimg <= 2 ? 1024 : 512; }

// same: tw_pair_same's flags of the launch's pairs where the level's only reader of the second images honours them (null:
// every image) — the 3-tap register kernel skips those images, the other kernels compute them as ever
void launch_pyr(tw_engine* e, hipStream_t st, const Plan* pl, int k, const uint8_t* const* d_srcs, long long stride, int img_al4,
                float* I, int nimg, const unsigned* same = nullptr)
{
    const LevelPlan& L = pl->lv[k];
    const PyrChoice c = choose_pyr(e->cfg, pl, k, stride, img_al4);
    PyrArgs a;
    a.srcs = d_srcs;
    a.dst = I;
    a.dst_zs = L.ps;
    a.stride = stride;
    a.w0 = pl->w0;
    a.h0 = pl->h0;
    a.w = L.w;
    a.h = L.h;
    a.ld = L.ld;
    a.xofs = L.d_xofs;
    a.alpha = L.d_alpha;
    a.yofs = L.d_yofs;
    a.beta = L.d_beta;
    a.kern = L.d_kern;
    a.ksize = L.ksize;
    a.mode = L.mode;
    a.xmax = L.xmax;
    a.nrows_max = c.nrows_max;
    a.th = c.th;
    const dim3 grid(c.gx, c.gy, nimg), block(c.block);
    ProfScope ps(e, st, TW_K_PYR, k);
    switch (c.kernel) {
        case PYR_KN_K3: {
            PyrK3Args b;
            b.srcs = d_srcs;
            b.dst = I;
            b.dst_zs = L.ps;
            b.stride = stride;
            b.w0 = pl->w0;
            b.h0 = pl->h0;
            b.w = L.w;
            b.h = L.h;
            b.ld = L.ld;
            b.k0 = L.h_kern[1];
            b.k1 = L.h_kern[0];
            b.aligned4 = c.aligned4;
            b.same = same;
            if (c.targ == 0) TW_LAUNCH(e, TW_DF_PYR_K3, tw_pyr_k3<0>, grid, block, c.lds, st, b);
            else TW_LAUNCH(e, TW_DF_PYR_K3, tw_pyr_k3<2>, grid, block, c.lds, st, b);
            return;
        }
        case PYR_KN_TAPS: {
            PyrTapsArgs b;
            b.p = a;
            b.pd = c.pitch / 4;
            b.aligned4 = c.aligned4;
            b.dbg = e->dbg_stamps;
            memset(b.kext, 0, sizeof(b.kext));
            memcpy(b.kext + 1, L.h_taps.data(), sizeof(float) * L.ksize);
            switch (c.targ) {
                case 9: TW_LAUNCH(e, TW_DF_PYR_TAPS, tw_pyr_taps<9>, grid, block, c.lds, st, b); break;
                case 19: TW_LAUNCH(e, TW_DF_PYR_TAPS, tw_pyr_taps<19>, grid, block, c.lds, st, b); break;
                case 39: TW_LAUNCH(e, TW_DF_PYR_TAPS, tw_pyr_taps<39>, grid, block, c.lds, st, b); break;
                default: TW_LAUNCH(e, TW_DF_PYR_TAPS, tw_pyr_taps<0>, grid, block, c.lds, st, b); break;
            }
            return;
        }
        case PYR_KN_LEVEL_LDS: {
            PyrLdsArgs b;
            b.p = a;
            b.pitch_b = c.pitch;
            b.aligned4 = c.aligned4;
            // counted as the generic level launch that it is, and in a family of its own
            e->launches[TW_DF_PYR_LEVEL_LDS]++;
            e->last_grid_z[TW_DF_PYR_LEVEL_LDS] = grid.z;
            TW_LAUNCH(e, TW_DF_PYR_LEVEL, tw_pyr_level_lds, grid, block, c.lds, st, b);
            return;
        }
        default: TW_LAUNCH(e, TW_DF_PYR_LEVEL, tw_pyr_level, grid, block, c.lds, st, a); return;
    }
}

// levels 3 and 2 of `nimg` images from one read of each image (tw_pyr_23; pl->fused23): I3 / I2 = the level images,
// z-th at + z * ps of the level
void launch_pyr23(tw_engine* e, hipStream_t st, const Plan* pl, const uint8_t* const* d_srcs, long long stride, int img_al4, float* I3,
                  float* I2, int nimg)
{
    const LevelPlan &L3 = pl->lv[3], &L2 = pl->lv[2];
    Pyr23Args a;
    a.srcs = d_srcs;
    a.dst3 = I3;
    a.dst2 = I2;
    a.zs3 = L3.ps;
    a.zs2 = L2.ps;
    a.stride = stride;
    a.w0 = pl->w0;
    a.h0 = pl->h0;
    a.w3 = L3.w;
    a.h3 = L3.h;
    a.ld3 = L3.ld;
    a.w2 = L2.w;
    a.h2 = L2.h;
    a.ld2 = L2.ld;
    a.aligned4 = (stride % 4 == 0) ? img_al4 : 0;
    memcpy(a.k19, pl->k19, sizeof(a.k19));
    memcpy(a.k9, pl->k9, sizeof(a.k9));
    ProfScope ps(e, st, TW_K_PYR, 3);
    const dim3 grid((L3.w + P23_T3W - 1) / P23_T3W, (L3.h + P23_T3H - 1) / P23_T3H, nimg);
    const int nt = pyr23_threads(e->cfg, nimg);
    if (nt == 256) TW_LAUNCH(e, TW_DF_PYR_23, tw_pyr_23<256>, grid, dim3(256), 0, st, a);
    else if (nt == 1024) TW_LAUNCH(e, TW_DF_PYR_23, tw_pyr_23<1024>, grid, dim3(1024), 0, st, a);
    else TW_LAUNCH(e, TW_DF_PYR_23, tw_pyr_23<512>, grid, dim3(512), 0, st, a);
}

tw_status launch_polyexp(tw_engine* e, hipStream_t st, int w, int h, int ld, long long ps, const float* I, float* R,
                         int nimg, int level, const SideJob* side = nullptr, bool* side_used = nullptr,
                         const unsigned* same = nullptr)
{
    PolyArgs a;
    a.same = same;
    a.src = I;
    a.dst = R;
    a.w = w;
    a.h = h;
    a.ld = ld;
    a.ps = ps;
    a.c = e->cfg.pc;
    dim3 grid((w + PE_TW - 1) / PE_TW, (h + PE_TH - 1) / PE_TH, nimg);
    ProfScope pscope(e, st, TW_K_POLYEXP, level);
#ifdef TW_VARIANTS
    if (e->cfg.poly_variant == 0) {
        // scalar-f32 kernel (A/B: TW_POLY_VARIANT=0)
        switch (e->cfg.p.polyN) {
            case 1: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<1>, grid, dim3(256), 0, st, a); break;
            case 2: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<2>, grid, dim3(256), 0, st, a); break;
            case 3: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<3>, grid, dim3(256), 0, st, a); break;
            case 4: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<4>, grid, dim3(256), 0, st, a); break;
            case 5: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<5>, grid, dim3(256), 0, st, a); break;
            case 6: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<6>, grid, dim3(256), 0, st, a); break;
            case 7: TW_LAUNCH(e, TW_DF_POLYEXP, tw_polyexp<7>, grid, dim3(256), 0, st, a); break;
            default: e->err = "polyN must be 1..7"; return TW_E_UNSUPPORTED;
        }
        return TW_OK;
    }
#endif
    if (e->opt.poly_f32) {
        // measurement variant (TW_OPT_POLYEXP_F32): float horizontal accumulators — NOT bit-exact, never the default
        switch (e->cfg.p.polyN) {
            case 5: TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<5, 8, 1>), grid, dim3(256), 0, st, a); break;
            case 7:
                if (e->opt.poly_f32 == 2) TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<7, 8, 2>), grid, dim3(256), 0, st, a);
                else TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<7, 8, 1>), grid, dim3(256), 0, st, a);
                break;
            default: e->err = "TW_OPT_POLYEXP_F32 needs polyN 5 or 7"; return TW_E_UNSUPPORTED;
        }
        return TW_OK;
    }
    // packed-f32 kernel, 240 x 8 tiles; TW_POLY_VARIANT=2 selects 240 x 16 tiles (960 two-by-two items = 15 full
    // waves of the horizontal pass, 30-row window per 16 output rows, 48 KB LDS: measured equal within the noise)
#ifdef TW_VARIANTS
    const bool t16 = e->cfg.poly_variant == 2;
    if (t16) grid.y = (h + 15) / 16;
#define TW_PK_CASE(n)                                                                        \
    case n:                                                                                  \
        if (t16) TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<n, 16, 0>), grid, dim3(256), 0, st, a);      \
        else TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<n, 8, 0>), grid, dim3(256), 0, st, a);           \
        break;
#else
#define TW_PK_CASE(n)                                                                        \
    case n: TW_LAUNCH(e, TW_DF_POLYEXP, (tw_polyexp_pk<n, 8, 0>), grid, dim3(256), 0, st, a); break;
#endif
    if (side && side_used && side->kind == 2 && e->cfg.p.polyN == 7 && e->cfg.poly_variant == 1) {
        const TwinGrid t = make_twin(grid, *side);
        TW_LAUNCH(e, TW_DF_TWIN, tw_twin_poly_k3f, dim3(t.nA8 + side->n()), dim3(256), 0, st, a, side->ka, t);
        *side_used = true;
        return TW_OK;
    }
    switch (e->cfg.p.polyN) {
        TW_PK_CASE(1) TW_PK_CASE(2) TW_PK_CASE(3) TW_PK_CASE(4) TW_PK_CASE(5) TW_PK_CASE(6) TW_PK_CASE(7)
        default: e->err = "polyN must be 1..7"; return TW_E_UNSUPPORTED;
    }
#undef TW_PK_CASE
    return TW_OK;
}

// levels 1 and 0 of `nimg` images from one read of each image (tw_pyr_k3f): both 3-tap levels of an exact halving
bool pyr01_fusable(const Plan* pl)
{
    return pl->levels >= 1 && pl->lv[0].ksize == 3 && pl->lv[1].ksize == 3 && pl->lv[0].mode == 0 && pl->lv[1].mode == 2 &&
           pl->w0 == 2 * pl->lv[1].w && pl->h0 == 2 * pl->lv[1].h && pl->w0 >= 16;
}
void launch_pyr01(tw_engine* e, hipStream_t st, const Plan* pl, const uint8_t* const* d_srcs, long long stride, int img_al4, float* I1,
                  float* I0, int nimg, const unsigned* same = nullptr)
{
    const LevelPlan &L0 = pl->lv[0], &L1 = pl->lv[1];
    PyrK3fArgs a;
    a.srcs = d_srcs;
    a.dst0 = I0;
    a.dst1 = I1;
    a.zs0 = L0.ps;
    a.zs1 = L1.ps;
    a.stride = stride;
    a.w0 = pl->w0;
    a.h0 = pl->h0;
    a.ld0 = L0.ld;
    a.w1 = L1.w;
    a.h1 = L1.h;
    a.ld1 = L1.ld;
    a.a0 = L0.h_kern[1];
    a.a1 = L0.h_kern[0];
    a.b0 = L1.h_kern[1];
    a.b1 = L1.h_kern[0];
    a.aligned4 = (stride % 4 == 0) ? img_al4 : 0;
    a.same = same;
    ProfScope ps(e, st, TW_K_PYR, 1);
    TW_LAUNCH(e, TW_DF_PYR_K3F, tw_pyr_k3f, dim3((L1.w + 255) / 256, (L1.h + 3) / 4, nimg), dim3(256), 0, st, a);
}

// One whole iteration of the flow update without M in HBM (tw_flow_iter; round 5): flow_out = solve(window average of
// FarnebackUpdateMatrices(R0, R1, flow_in)).  flow_in: a flow buffer, or (prev != nullptr) the bilinear upsample x
// 1/pyr_scale of the coarser level's flow computed in place of the load, or zero (both null: the coarsest level).
bool flow_iter_eligible(const EngineConfig& cfg, int w, int h)
{
    return cfg.win_m == 15 && !cfg.box && w >= cfg.mfree_min_w && h >= 4 * FI_TH;
}
// The predicate of choose_level_schedule, its one caller (the byte model reads the choice): does a launch of nc
// pairs at a level of w x h pixels run tw_flow_iter?  lat: the batch takes the single-pair schedule; grid_only: the level's
// last iteration is evaluated at the span-grid points only (TW_OPT_SCAN_FUSED_FINAL, level 0).  A launch of fewer workgroups
// than ~3/4 of the CUs — one or two 1080p pairs — leaves the chip to the 224 x 8 tiles of tw_blur_solve4, of which a single
// pair already makes 1 215 (TW_MFREE=2 lifts that gate: tests, tools/fuzz_parity.py).
bool level_runs_flow_iter(const EngineConfig& cfg, int w, int h, int nc, bool lat, bool grid_only)
{
    const int it = cfg.p.pyrIterations;
    const int fi_out = (cfg.fi_nt == 512 ? FI_SC_512 : FI_SC) - 30;
    const long long fi_wgs = (long long)((w + fi_out - 1) / fi_out) * std::min(4, std::max(1, h / (16 * FI_TH))) * nc;
    return cfg.mfree && !lat && it > (grid_only ? 1 : 0) && flow_iter_eligible(cfg, w, h) &&
           (fi_wgs * 4 >= (long long)cfg.cu_count * 3 || cfg.mfree == 2) &&
           (cfg.mfree_min_px <= 0 || (long long)w * h >= cfg.mfree_min_px);
}
// does a batch of n pairs of w0 x h0 pixels take the single-pair schedule (its image-only work beside the flow chain)?
bool single_pair_schedule(const EngineConfig& cfg, int n, int w0, int h0, int levels)
{
    return n == 1 && cfg.lat_streams && levels >= 1 && (long long)w0 * h0 >= cfg.lat_min_px;
}
// the last level-0 iteration at the span-grid points only?
bool scan_fused_level0(const EngineConfig& cfg, int scan_fused, int span)
{
    return cfg.p.pyrIterations > 0 && scan_fused && span == 10 && cfg.win_m == 15 && !cfg.box;
}
// pairs per launch when n pairs are split into balanced launches of at most `chunk` (64 pairs with a 63-pair chunk are 32 + 32)
int balanced_launch_pairs(int n, int chunk)
{
    const int nlaunch = (n + chunk - 1) / chunk;
    return nlaunch > 0 ? (n + nlaunch - 1) / nlaunch : 1;
}
struct FlowUps {  // the coarser level's flow and the resize tables to this level (UpdArgs' upsample fields)
    const float* prev;
    int pw, ph, pld;
    long long pfps;
    const int *xofs, *yofs;
    const float *alpha, *beta;
    int xmax;
    float scale;
};
// the common block of UpdArgs (everything else zero) and, with `ups`, its upsample source
template <typename A>
void set_upsample(A& a, const FlowUps& u)  // UpdArgs and FlowIterArgs name these fields alike
{
    a.prev = u.prev;
    a.pw = u.pw;
    a.ph = u.ph;
    a.pld = u.pld;
    a.pfps = u.pfps;
    a.xofs = u.xofs;
    a.alpha = u.alpha;
    a.yofs = u.yofs;
    a.beta = u.beta;
    a.xmax = u.xmax;
    a.scale = u.scale;
}
UpdArgs upd_args(const float* R, float* flow, float* M, int w, int h, int ld, long long ps, const FlowUps* ups = nullptr)
{
    UpdArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.flow = flow;
    a.M = M;
    a.w = w;
    a.h = h;
    a.ld = ld;
    a.ps = ps;
    a.fps = ps;
    if (ups) set_upsample(a, *ups);
    return a;
}
// The geometry of one tw_flow_iter launch — the ONE place the strip / row-segment rule lives: launch_flow_iter takes its
// grid (strips, segments, pairs) and the kernel's steps per segment from it, and tw_debug_flow_iter_plan shows it to the tests.
struct FlowIterPlan {
    int strips, segments, nt, nt_last;  // nt: steps of FI_TH rows per segment; nt_last: steps of the last segment
};
FlowIterPlan flow_iter_plan(const EngineConfig& cfg, int w, int h, int npairs)
{
    const int OUT = (cfg.fi_nt == 512 ? FI_SC_512 : FI_SC) - 30;
    const int slots = cfg.cu_count * (cfg.fi_nt == 512 ? 2 : 1);  // workgroups resident at once
    const int nstrips = (w + OUT - 1) / OUT, nsteps = (h + FI_TH - 1) / FI_TH;
    // Row segments per strip: one 1024-thread workgroup per CU is resident, so the launch runs in rounds of (CU count)
    // workgroups; a segment pays NCH = 7 chunks of M for its window's warm-up.  Take the split (1 .. 4) with the least
    // (rounds x (steps + warm-up)) — 128 pairs x 12 strips of 1080p: 2 segments = 12.0 rounds of 108 + 7 steps.
    int best_seg = 1;
    double best_cost = 1e300;
    for (int sg = 1; sg <= cfg.fi_maxseg; sg++) {
        const int nt = (nsteps + sg - 1) / sg;
        if (sg > 1 && nt < cfg.fi_minsteps) break;
        const long long wgs = (long long)nstrips * sg * npairs;
        const long long rounds = (wgs + slots - 1) / slots;
        const double cost = (double)rounds * (nt + 7 * 0.25);  // a warm-up chunk is a quarter of a step (phase C only)
        if (cost < best_cost) {
            best_cost = cost;
            best_seg = sg;
        }
    }
    FlowIterPlan fp;
    fp.strips = nstrips;
    fp.nt = (nsteps + best_seg - 1) / best_seg;
    fp.segments = (nsteps + fp.nt - 1) / fp.nt;
    fp.nt_last = nsteps - (fp.segments - 1) * fp.nt;
    return fp;
}
// grid_pts != null: the grid-only iteration (tw_flow_iter<15, 3>) — flow_in's iteration evaluated at the span-grid points
// alone, into grid_pts->g; flow_out is not written.  The caller has checked span >= FI_TH (at most one grid row per step).
struct FlowIterGrid {
    float2* g;  // pair z: gw * gh points at g + z * gw * gh
    int span, gw, gh;
};
void launch_flow_iter(tw_engine* e, hipStream_t st, int w, int h, int ld, long long ps, const float* R, const float* flow_in,
                      long long fps_in, float* flow_out, long long fps_out, const FlowUps* ups, int npairs, int level,
                      const unsigned* same = nullptr, const FlowIterGrid* grid_pts = nullptr)
{
    FlowIterArgs a;
    memset(&a, 0, sizeof(a));
    a.same = same;
    a.R = R;
    a.flow_in = flow_in;
    a.flow_out = flow_out;
    a.w = w;
    a.h = h;
    a.ld = ld;
    a.ps = ps;
    a.fps_in = fps_in;
    a.fps_out = fps_out;
    a.zero_flow = (!flow_in && !ups) ? 1 : 0;
    a.c = e->cfg.wc;
#ifdef TW_VARIANTS
    a.dbg_skip = e->cfg.fi_skip;                     // TW_FI_SKIP (timing experiments)
    a.dbg = (unsigned long long*)e->dbg_stamps;  // TW_DEBUG_STAMPS=1
#endif
    const FlowIterPlan fp = flow_iter_plan(e->cfg, w, h, npairs);
    a.nt = fp.nt;
    const dim3 grid(fp.strips, fp.segments, npairs);
    ProfScope pscope(e, st, TW_K_BLUR_SOLVE, level);
    if (ups) set_upsample(a, *ups);
    if (grid_pts) {
        // counted as the level's MODE 0 iteration that it is, and in a family of its own
        a.span = grid_pts->span;
        a.gw = grid_pts->gw;
        a.gh = grid_pts->gh;
        a.gzs = (long long)a.gw * a.gh;
        a.g = grid_pts->g;
        e->launches[TW_DF_FLOW_ITER_GRID]++;
        e->last_grid_z[TW_DF_FLOW_ITER_GRID] = grid.z;
        TW_LAUNCH(e, TW_DF_FLOW_ITER, (tw_flow_iter<15, 3>), grid, dim3(1024), 0, st, a);
        return;
    }
#ifdef TW_VARIANTS
    if (e->cfg.fi_nt == 512) {  // measured 23 % slower (profiles/r05_m_free.md): variants library only
        if (ups) TW_LAUNCH(e, TW_DF_FLOW_ITER_UPS, (tw_flow_iter<15, 1, 512>), grid, dim3(512), 0, st, a);
        else if (a.zero_flow) TW_LAUNCH(e, TW_DF_FLOW_ITER_ZERO, (tw_flow_iter<15, 2, 512>), grid, dim3(512), 0, st, a);
        else TW_LAUNCH(e, TW_DF_FLOW_ITER, (tw_flow_iter<15, 0, 512>), grid, dim3(512), 0, st, a);
        return;
    }
#endif
    if (ups) {
        TW_LAUNCH(e, TW_DF_FLOW_ITER_UPS, (tw_flow_iter<15, 1>), grid, dim3(1024), 0, st, a);
    } else if (a.zero_flow) {
        TW_LAUNCH(e, TW_DF_FLOW_ITER_ZERO, (tw_flow_iter<15, 2>), grid, dim3(1024), 0, st, a);
    } else {
        TW_LAUNCH(e, TW_DF_FLOW_ITER, (tw_flow_iter<15, 0>), grid, dim3(1024), 0, st, a);
    }
}

// ---- the window average + solve launches ------------------------------------------------------------------------------
// One row per fixed-window kernel: what it is (kernel, counter family, block, the tile a workgroup owns) and when it runs.
// choose_blur takes the first row whose predicate holds, the variants rows before the product rows.
#ifndef TW_4Y_ILP  // (A/B builds: vertical / horizontal interleave and solve unroll of the 51-tap kernel)
#define TW_4Y_ILP 2, 2, 2
#endif
struct BlurKernel {
    void (*kern)(BlurArgs);
    int family;      // TW_DF_*
    int block;       // threads
    int tw, th;      // tile columns, rows per workgroup
    bool shift;      // the tile grid may start 16 px left of the image (tile_shift)
    bool grid_out;   // stores the span-grid samples next to the flow when asked to (GridOut)
    int twin;        // carries a side job as 1: tw_twin_s4_poly, 2: tw_twin_pp_poly (0: never)
    // -- the predicate: every field that is not "any" must hold
    int m;           // winSize / 2
    int wide;        // 1: w > 480, 0: narrower, -1: any
    int small;       // the small-grid class (choose_blur), -1: any
    bool quads;      // only when the caller asks for the quad kernel (the single-pair schedule)
    int variant;     // TW_BLUR_VARIANT, 0: any
    int pipe;        // TW_BLUR_PIPE on a refreshing launch, 0: any
    int min_w;
};
constexpr int ANY = -1;
const BlurKernel kBlurKernels[] = {
    // small grids: 96 x 8 tiles of two waves, plane-parallel 32 x 8 tiles of five waves
    {tw_blur_solve4<15, 128, 16, 8, true>, TW_DF_BLUR_SOLVE4, 128, 96, 8, true, true, 1, 15, ANY, 1, false, 0, 0, 0},
    {tw_blur_solve_pp<15, 64, 16, 8>, TW_DF_BLUR_PP, 320, 32, 8, true, false, 2, 15, ANY, 4, false, 0, 0, 0},
    // quads (the single-pair schedule): the launch is bound by its workgroups' serial chain, not by throughput — the kernel
    // that solves and refreshes in the horizontal item's owner (two barriers and an LDS round trip fewer) is 6 % shorter there
    {tw_blur_solve4q<15, 256, 16, 8, true>, TW_DF_BLUR_SOLVE4Q, 256, 224, 8, true, true, 0, 15, 1, 0, true, 0, 0, 0},
    // 224-column tiles; narrow levels use 96-column tiles (less edge waste)
    {tw_blur_solve4<15, 256, 16, 8, true>, TW_DF_BLUR_SOLVE4, 256, 224, 8, true, true, 0, 15, 1, 0, false, 0, 0, 0},
    {tw_blur_solve4<15, 128, 16, 8, true>, TW_DF_BLUR_SOLVE4, 128, 96, 8, true, true, 0, 15, 0, 0, false, 0, 0, 0},
    // winSize 50/51 (BASELINE config 5).  Wide levels: two vertically adjacent 8-row sub-tiles share one 66-row register window
    // (round 3: -7 % against the one-sub-tile kernel with its 58-row window per 8 rows, which TW_BLUR_VARIANT=41 selects);
    // narrow levels: packed-f32 structure, single 58-row register window
    {tw_blur_solve4y<25, 256, 32, 8, 2, TW_4Y_ILP>, TW_DF_BLUR_SOLVE4Y, 256, 192, 16, false, false, 0, 25, 1, ANY, false, 0, 0, 0},
    {tw_blur_solve8<25, 128, 32, 8, true, false>, TW_DF_BLUR_SOLVE8, 128, 64, 8, false, false, 0, 25, 0, ANY, false, 0, 0, 0},
#ifdef TW_VARIANTS
    // packed-f32 structure (same speed as v4 at 1080p, lower VALU load); TW_BLUR_VARIANT=8 for A/B
    {tw_blur_solve8<15, 256, 16, 8, true, true>, TW_DF_BLUR_SOLVE8, 256, 224, 8, false, false, 0, 15, 1, ANY, false, 8, 0, 0},
    {tw_blur_solve8<15, 128, 16, 8, true, true>, TW_DF_BLUR_SOLVE8, 128, 96, 8, false, false, 0, 15, 0, ANY, false, 8, 0, 0},
    // small-grid classes 2 (96 x 4, 128 threads), 3 (32 x 4, 64 threads) and 5 (plane-parallel 96 x 8, 640 threads)
    {tw_blur_solve4<15, 128, 16, 4, true>, TW_DF_BLUR_SOLVE4, 128, 96, 4, true, false, 0, 15, ANY, 2, false, 0, 0, 0},
    {tw_blur_solve4<15, 64, 16, 4, true>, TW_DF_BLUR_SOLVE4, 64, 32, 4, true, false, 0, 15, ANY, 3, false, 0, 0, 0},
    {tw_blur_solve_pp<15, 128, 16, 8>, TW_DF_BLUR_PP, 640, 96, 8, true, false, 0, 15, ANY, 5, false, 0, 0, 0},
    // plane pipeline through a two-plane LDS ring (tw_blur_solve6), A/B
    {tw_blur_solve6<15, 256, 16, 8, 5>, TW_DF_BLUR_VARIANT, 256, 224, 8, true, false, 0, 15, 1, 0, false, 60, 0, 0},
    {tw_blur_solve6<15, 256, 16, 8, 4>, TW_DF_BLUR_VARIANT, 256, 224, 8, true, false, 0, 15, 1, 0, false, 61, 0, 0},
    // 480-column tiles (512 threads, 80 KB LDS, two workgroups per CU): 93.75 % of the columns of the vertical pass and of
    // the lanes of the horizontal pass are useful (87.5 % with 224-column tiles), and 1920 / 960 / 3840-pixel rows are
    // covered exactly (nine 224-column tiles cover 2016)
    {tw_blur_solve4<15, 512, 16, 8, true>, TW_DF_BLUR_SOLVE4, 512, 480, 8, true, false, 0, 15, 1, 0, false, 5, 0, 960},
    // round 4: solve + refresh by the horizontal item's owner, 16-byte R0 / M accesses
    {tw_blur_solve4q<15, 256, 16, 8, true>, TW_DF_BLUR_VARIANT, 256, 224, 8, true, false, 0, 15, 1, 0, false, 9, 0, 0},
    {tw_blur_solve4q<15, 128, 16, 8, true>, TW_DF_BLUR_VARIANT, 128, 96, 8, true, false, 0, 15, 0, 0, false, 9, 0, 0},
    {tw_blur_solve4y<15, 256, 16, 8, 2>, TW_DF_BLUR_SOLVE4Y, 256, 224, 16, true, false, 0, 15, 1, 0, false, 2, 0, 0},
    {tw_blur_solve4<15, 256, 16, 8, true, 2, 2, 2, true, false>, TW_DF_BLUR_SOLVE4, 256, 224, 8, true, false, 0, 15, 1, 0, false, 7, 0, 0},
    {tw_blur_solve4<15, 256, 16, 8, true, 2, 2, 2, false>, TW_DF_BLUR_SOLVE4, 256, 224, 8, true, false, 0, 15, 1, 0, false, 6, 0, 0},
    // refreshing launch as a cross-tile pipeline: a workgroup walks TW_BLUR_PIPE vertically adjacent tiles (109: 9 tiles, WPE 3)
    {tw_blur_solve4p<15, 256, 16, 8, 3>, TW_DF_BLUR_VARIANT, 256, 224, 8 * 3, true, false, 0, 15, 1, 0, false, 0, 3, 0},
    {tw_blur_solve4p<15, 256, 16, 8, 5>, TW_DF_BLUR_VARIANT, 256, 224, 8 * 5, true, false, 0, 15, 1, 0, false, 0, 5, 0},
    {tw_blur_solve4p<15, 256, 16, 8, 9>, TW_DF_BLUR_VARIANT, 256, 224, 8 * 9, true, false, 0, 15, 1, 0, false, 0, 9, 0},
    {tw_blur_solve4p<15, 256, 16, 8, 15>, TW_DF_BLUR_VARIANT, 256, 224, 8 * 15, true, false, 0, 15, 1, 0, false, 0, 15, 0},
    {tw_blur_solve4p<15, 256, 16, 8, 9, 3>, TW_DF_BLUR_VARIANT, 256, 224, 8 * 9, true, false, 0, 15, 1, 0, false, 0, 109, 0},
    // winSize 50/51: the packed-f32 kernel on wide levels too, and round 3's trials for config 5: shorter
    // tiles make room for the R0 prefetch (QPRE)
    {tw_blur_solve8<25, 256, 32, 8, true, false>, TW_DF_BLUR_SOLVE8, 256, 192, 8, false, false, 0, 25, 1, ANY, false, 8, 0, 0},
    {tw_blur_solve4<25, 256, 32, 6, true, 2, 2, 2, true, false>, TW_DF_BLUR_SOLVE4, 256, 192, 6, false, false, 0, 25, 1, ANY, false, 256, 0, 0},
    {tw_blur_solve4<25, 256, 32, 5, true, 2, 2, 2, true, false>, TW_DF_BLUR_SOLVE4, 256, 192, 5, false, false, 0, 25, 1, ANY, false, 255, 0, 0},
    {tw_blur_solve4<25, 256, 32, 4, true, 2, 2, 2, true, false>, TW_DF_BLUR_SOLVE4, 256, 192, 4, false, false, 0, 25, 1, ANY, false, 254, 0, 0},
    {tw_blur_solve4<25, 256, 32, 8, true, 2, 2, 2, true, false>, TW_DF_BLUR_SOLVE4, 256, 192, 8, false, false, 0, 25, 1, ANY, false, 258, 0, 0},
    {tw_blur_solve4<25, 256, 32, 8, true, 2, 2, 2, false, false>, TW_DF_BLUR_SOLVE4, 256, 192, 8, false, false, 0, 25, 1, ANY, false, 41, 0, 0},
    {tw_blur_solve4<25, 256, 32, 5, true, 2, 2, 2, false, false>, TW_DF_BLUR_SOLVE4, 256, 192, 5, false, false, 0, 25, 1, ANY, false, 259, 0, 0},
#endif
};
constexpr int kBlurKernelRows = (int)(sizeof(kBlurKernels) / sizeof(kBlurKernels[0])), kProductBlurRows = 7;
static_assert(kBlurKernelRows >= kProductBlurRows, "the product rows come first");
// ... and the two window launches that are no table kernel: any other window size (same arithmetic, runtime loops, dynamic
// LDS) and the box window (launch_box_window; block / tile of tw_box_vscan)
const BlurKernel kGenericWindow = {tw_blur_solve_generic, TW_DF_BLUR_GENERIC, 256, 64, BS_TH, false, false, 0, ANY, ANY, ANY, false, 0, 0, 0};
const BlurKernel kBoxWindow = {nullptr, TW_DF_BOX, 64, 64, 1, false, false, 0, ANY, ANY, ANY, false, 0, 0, 0};

// shift the tile grid 16 px left when that costs no extra tile column (see tw_blur_solve4)
int tile_shift(int w, int tw) { return ((w + 16 + tw - 1) / tw == (w + tw - 1) / tw) ? 16 : 0; }

// The choice of one window launch — the ONE place it is made: launch_blur launches it, plan_twin_side_jobs asks it which
// tiles level 1 takes, and tw_debug_blur_plan shows it to the tests.
struct BlurChoice {
    const BlurKernel* k;  // a row of kBlurKernels, kGenericWindow or kBoxWindow
    int xsh;
    dim3 grid;            // (box window: of tw_box_vscan)
    size_t lds;           // dynamic LDS bytes (the generic kernel)
    int small;            // 31-tap window: 0: 224x8 / 96x8 tiles, 1: 96x8 (128 threads), 2: 96x4 (128 threads), 3: 32x4 (64 threads),
                          // 4: plane-parallel 32x8 (320 threads), 5: plane-parallel 96x8 (640 threads)
    bool forced;          // ... set by TW_BLUR_SMALL_LEVELS / TW_BLUR_SMALL, not by the grid's size
};
BlurChoice choose_blur(const EngineConfig& cfg, int w, int h, int npairs, int level, bool update, bool quads)
{
    BlurChoice c{&kGenericWindow, 0, dim3(), 0, 0, false};
    if (cfg.box) {
        c.k = &kBoxWindow;
        c.grid = dim3((w + 63) / 64, 5, npairs);
        return c;
    }
    const bool wide = w > 480;
    if (cfg.win_m == 15) {
        // Small grids (a single pair, the coarse levels): a level that would launch fewer than two workgroups per
        // CU takes smaller tiles, so that more CUs share it and each workgroup's serial V -> H -> S chain is shorter
        // (BASELINE config 2, single-pair latency).  Batched launches always have enough tiles and keep the big ones.
        auto nwg = [&](int tw, int th) { return (long long)((w + tw - 1) / tw) * ((h + th - 1) / th) * npairs; };
        c.forced = true;
        if (level >= 0 && level < 8 && cfg.blur_small_lv[level] >= 0) c.small = cfg.blur_small_lv[level];
        else if (cfg.blur_small >= 0) c.small = cfg.blur_small;
        else {
            c.forced = false;
            if (wide && nwg(224, 8) >= 1024) c.small = 0;  // four 256-thread workgroups per CU: throughput regime
            else if (nwg(96, 8) * 2 >= cfg.pp_waves) c.small = wide ? 1 : 0;  // enough 2-wave workgroups to keep every SIMD busy
            else c.small = 4;  // otherwise many small plane-parallel workgroups (5 waves per 32x8 pixels)
        }
        if (c.small > 5) c.small = 4;
    }
    for (int i = 0; i < kBlurKernelRows; i++) {
        const BlurKernel& r = kBlurKernels[(kProductBlurRows + i) % kBlurKernelRows];  // the variants rows first
        if (r.m == cfg.win_m && (r.wide == ANY || r.wide == (int)wide) && (r.small == ANY || r.small == c.small) && (!r.quads || quads) &&
            (!r.variant || r.variant == cfg.blur_variant) && (!r.pipe || (update && r.pipe == cfg.blur_pipe)) && w >= r.min_w) {
            c.k = &r;
            break;
        }
    }
    if (c.k->shift) c.xsh = tile_shift(w, c.k->tw);
    c.grid = dim3((w + c.xsh + c.k->tw - 1) / c.k->tw, (h + c.k->th - 1) / c.k->th, npairs);
    if (c.k == &kGenericWindow) c.lds = (size_t)5 * BS_TH * (64 + 2 * cfg.win_m) * 4;
    return c;
}

// span-grid samples a tw_blur_solve4 launch stores next to the flow (the single-pair schedule's last level-0 launch)
struct GridOut {
    float2* g;
    int span, gw, gh;
    bool* used;  // set if the launch took a kernel that stores them (the caller launches tw_span_gather otherwise)
};
// one window launch: the level's buffers and geometry, and what only some callers have
struct BlurLaunch {
    int w, h, ld;
    long long ps;
    const float* Min;
    float* Mout;
    float* flow;
    const float* R;
    int update;               // refresh M for the next iteration
    int level;                // (ProfScope, TW_BLUR_SMALL_LEVELS; -1: a per-stage entry point)
    int npairs;
    int store_flow = 0;       // store the flow of a refreshing launch too
    double* Vbox = nullptr;   // box window: the column sums' workspace, [5 ps npairs] (null: the engine's)
    const SideJob* side = nullptr;  // the twin schedule: a side job this launch may carry, *side_used set if it did
    bool* side_used = nullptr;
    const GridOut* go = nullptr;
    bool quads = false;
};
// box window: sequential double running sums (two scan kernels) + the standard refresh kernel
void launch_box_window(tw_engine* e, hipStream_t st, const BlurLaunch& in)
{
    double* V = in.Vbox ? in.Vbox : e->Vd;  // TW_LANES=2: each lane (stream) has its own column sums
    const BoxArgs b{in.Min, V, in.flow, in.w, in.h, in.ld, in.ps, in.ps, e->cfg.win_m, 1. / ((double)e->cfg.p.winSize * e->cfg.p.winSize)};
    {
        ProfScope pscope(e, st, TW_K_BLUR_SOLVE, in.level);
        TW_LAUNCH(e, TW_DF_BOX, tw_box_vscan, dim3((in.w + 63) / 64, 5, in.npairs), dim3(64), 0, st, b);
        TW_LAUNCH(e, TW_DF_BOX, tw_box_hscan_solve, dim3((in.h + 11) / 12, 1, in.npairs), dim3(64), 0, st, b);
    }
    if (in.update) {
        const UpdArgs u = upd_args(in.R, in.flow, in.Mout, in.w, in.h, in.ld, in.ps);
        ProfScope pscope(e, st, TW_K_UPDATE_MATRICES, in.level);
        launch_upd_kernel<false>(e, st, in.w, in.h, in.npairs, u);
    }
}
void launch_blur(tw_engine* e, hipStream_t st, const BlurLaunch& in)
{
    BlurArgs a;
    a.Min = in.Min;
    a.Mout = in.Mout;
    a.flow = in.flow;
    a.R = in.R;
    a.w = in.w;
    a.h = in.h;
    a.ld = in.ld;
    a.ps = in.ps;
    a.fps = in.ps;
    a.update = in.update;
    a.store_flow = in.store_flow;
    a.m = e->cfg.win_m;
    a.nomask = e->cfg.blur_nomask;
    a.cm = e->cfg.blur_cm;
    a.grid = nullptr;
    a.gspan = a.gw = a.gh = 0;
    a.gmagic = 0;
    a.c = e->cfg.wc;
    const BlurChoice c = choose_blur(e->cfg, in.w, in.h, in.npairs, in.level, in.update != 0, in.quads);
    if (c.k == &kBoxWindow) return launch_box_window(e, st, in);
    a.xsh = a.rot = c.xsh;
    if (c.k->grid_out && in.go && in.go->span > 1 && in.w < 65536 && in.h < 65536) {
        a.grid = in.go->g;
        a.gspan = in.go->span;
        a.gw = in.go->gw;
        a.gh = in.go->gh;
        a.gmagic = (unsigned)((0x100000000ull + (unsigned)in.go->span - 1) / (unsigned)in.go->span);
        *in.go->used = true;
    }
    ProfScope pscope(e, st, TW_K_BLUR_SOLVE, in.level);
    if (c.k->twin && in.side && in.side_used && in.side->kind == 1) {
        // workgroups that leave most of the chip idle: a band of a finer level's expansion rides along
        const TwinGrid t = make_twin(c.grid, *in.side);
        if (c.k->twin == 1) TW_LAUNCH(e, TW_DF_TWIN, tw_twin_s4_poly, dim3(t.nA8 + in.side->n()), dim3(256), 0, st, a, in.side->pa, t);
        else TW_LAUNCH(e, TW_DF_TWIN, tw_twin_pp_poly, dim3(t.nA8 + in.side->n()), dim3(320), 0, st, a, in.side->pa, t);
        *in.side_used = true;
    } else {
        void (*const kern)(BlurArgs) = c.k->kern;
        TW_LAUNCH(e, c.k->family, kern, c.grid, dim3(c.k->block), c.lds, st, a);
    }
}

// init_flow: the coarsest level's flow buffer already holds the pairs' first flow (tw_flow_area_init), not zero
void launch_update(tw_engine* e, hipStream_t st, const Plan* pl, int k, const float* R, float* flow,
                   const float* prev, float* M, int npairs, const SideJob* side = nullptr, bool* side_used = nullptr,
                   bool init_flow = false)
{
    const LevelPlan& L = pl->lv[k];
    const bool up = k < pl->levels;
    FlowUps ups;
    if (up) {
        const LevelPlan& P = pl->lv[k + 1];
        ups = FlowUps{prev, P.w, P.h, P.ld, P.ps, L.d_uxofs, L.d_uyofs, L.d_ualpha, L.d_ubeta, L.uxmax, (float)(1. / e->cfg.p.pyrScale)};
    }
    UpdArgs a = upd_args(R, flow, M, L.w, L.h, L.ld, L.ps, up ? &ups : nullptr);
    a.store_flow = e->cfg.p.pyrIterations == 0 ? 1 : 0;
    ProfScope pscope(e, st, TW_K_UPDATE_MATRICES, k);
    if (up) {
        launch_upd_kernel<true>(e, st, L.w, L.h, npairs, a, side, side_used);
    } else {
        a.zero_flow = init_flow ? 0 : 1;
        launch_upd_kernel<false>(e, st, L.w, L.h, npairs, a, side, side_used);
    }
}

// tw_submit_*_flow_init: the first flow of pairs [j0, j0 + nc) at the coarsest level — each pair's init field resized and
// scaled (tw_flow_area_init), zeros for a pair without one — into `flow` (planar, the level's ld / ps), the buffer the
// level's first FarnebackUpdateMatrices or first tw_flow_iter reads
AreaInitArgs area_init_args(const tw_engine* e, const Plan* pl, float* flow, int j0)
{
    const LevelPlan& L = pl->lv[pl->levels];
    AreaInitArgs a;
    memset(&a, 0, sizeof(a));
    a.src = e->d_fsrc ? e->d_fsrc + j0 : nullptr;
    a.flow = flow;
    a.fps = L.ps;
    a.ld = L.ld;
    a.w = L.w;
    a.h = L.h;
    a.h0 = pl->h0;
    a.mode = pl->init_mode;
    a.ix = pl->init_ix;
    a.iy = pl->init_iy;
    a.inv_area = 1.f / (float)(pl->init_ix * pl->init_iy);  // (resizeAreaFast_Invoker: float scale = 1.f/(area))
    a.tw = pl->init_tw;
    a.scaled = fabs(L.scale - 1) >= DBL_EPSILON ? 1 : 0;  // convertTo's noScale: a copy
    a.scale = (float)L.scale;
    a.xstart = pl->d_ixs;
    a.xsi = pl->d_ixi;
    a.xalpha = pl->d_ixa;
    a.ystart = pl->d_iys;
    a.ysi = pl->d_iyi;
    a.ybeta = pl->d_iyb;
    return a;
}
void launch_area_init(tw_engine* e, hipStream_t st, const Plan* pl, float* flow, int j0, int nc)
{
    const LevelPlan& L = pl->lv[pl->levels];
    const AreaInitArgs a = area_init_args(e, pl, flow, j0);
    if (a.mode == 1 && a.tw > 0) {
        const size_t lds = (size_t)a.tw * a.ix * a.iy * 2 * sizeof(float);
        TW_LAUNCH(e, TW_DF_FLOW_INIT, tw_flow_area_init, dim3((L.w + a.tw - 1) / a.tw, L.h, nc), dim3(256), lds, st, a);
    } else {
        TW_LAUNCH(e, TW_DF_FLOW_INIT, tw_flow_area_init, dim3((L.w + 63) / 64, (L.h + 3) / 4, nc), dim3(256), 0, st, a);
    }
}

// TW_OPT_SHIFT: the first flow of the pairs [j0, j0 + nc) whose shift was applied, with tw_flow_area_init's arithmetic on their
// constant field; `zero_rest`: zeros for the others too (no tw_flow_area_init launch wrote the chunk)
void launch_shift_init(tw_engine* e, hipStream_t st, const Plan* pl, float* flow, int j0, int nc, bool zero_rest)
{
    const LevelPlan& L = pl->lv[pl->levels];
    ShiftInitArgs a;
    a.g = area_init_args(e, pl, flow, j0);
    a.rec = e->d_shift + j0;
    a.zero_rest = zero_rest ? 1 : 0;
    TW_LAUNCH(e, TW_DF_FLOW_SHIFT_INIT, tw_flow_shift_init, dim3((L.w + 63) / 64, (L.h + 3) / 4, nc), dim3(256), 0, st, a);
}

// TW_OPT_SHIFT_BANDS: the first flow of the pairs [j0, j0 + nc) from their bands' shifts, in tw_flow_shift_init's place
void launch_band_init(tw_engine* e, hipStream_t st, const Plan* pl, float* flow, int j0, int nc, int band, int nb, bool zero_rest)
{
    const LevelPlan& L = pl->lv[pl->levels];
    BandInitArgs a;
    a.g = area_init_args(e, pl, flow, j0);
    a.rec = e->d_shift + j0;
    a.bands = e->d_bands + (size_t)j0 * nb;
    a.band = band;
    a.nb = nb;
    a.magic = (unsigned)((1ull << 32) / (unsigned)band) + 1u;
    a.zero_rest = zero_rest ? 1 : 0;
    TW_LAUNCH(e, TW_DF_FLOW_BAND_INIT, tw_flow_band_init, dim3((L.w + 63) / 64, (L.h + 3) / 4, nc), dim3(256), 0, st, a);
}

// a flow field's rows in either layout: bytes of a row of w pixels, rows of a field of h pixel rows
size_t flow_row_bytes(int w, int layout) { return (size_t)w * (layout == TW_FLOW_INTERLEAVED ? 8 : 4); }
size_t flow_rows(int h, int layout) { return (size_t)h * (layout == TW_FLOW_INTERLEAVED ? 1 : 2); }

// bytes of one pair's slot in a context's flow staging: the field as dense rows of either layout
size_t flow_stage_slot(int w, int h) { return ((size_t)w * h * 8 + 255) / 256 * 256; }

// tw_submit_*_flow: pairs [j0, j0 + nc) of the batch have their final flow in the level-0 chunk buffer `flow` (before the
// next chunk reuses it): tw_flow_export copies it to the pairs' destinations, and the fields of host destinations go on
// from the context's staging to the caller's page-locked memory on the device-to-host stream, behind this export only
tw_status export_chunk(tw_engine* e, Ctx& c, hipStream_t st, const LevelPlan& L, const float* flow, int j0, int nc, size_t fslot)
{
    bool any = false, host = false;
    for (int j = j0; j < j0 + nc; j++) {
        any = any || c.jobs[j].fout.data;
        host = host || c.jobs[j].fout_host;
    }
    if (!any) return TW_OK;
    ExportArgs a;
    a.flow = flow;
    a.fzs = 2 * L.ps;
    a.fps = L.ps;
    a.ld = L.ld;
    a.w = L.w;
    a.h = L.h;
    a.qpr = (L.w + 3) / 4;
    a.dst = e->d_fdst + j0;
    const unsigned nq = (unsigned)a.qpr * (unsigned)L.h;
    TW_LAUNCH(e, TW_DF_FLOW_EXPORT, tw_flow_export, dim3((nq + 255) / 256, 1, nc), dim3(256), 0, st, a);
    if (!host) return TW_OK;
    TW_HIP(e, hipEventRecord(c.ev_fexp, st));
    TW_HIP(e, hipStreamWaitEvent(e->d2h_stream, c.ev_fexp, 0));
    for (int j = j0; j < j0 + nc; j++) {
        const Job& jb = c.jobs[j];
        if (!jb.fout_host) continue;
        const size_t row = flow_row_bytes(L.w, jb.fout.layout), rows = flow_rows(L.h, jb.fout.layout);
        const char* src = c.d_fstage + fslot * j;
        if ((size_t)jb.fout.pitch == row)  // dense rows: one plain transfer (the DMA engines)
            TW_HIP(e, hipMemcpyAsync(jb.fout.data, src, row * rows, hipMemcpyDeviceToHost, e->d2h_stream));
        else
            TW_HIP(e, hipMemcpy2DAsync(jb.fout.data, (size_t)jb.fout.pitch, src, row, row, rows, hipMemcpyDeviceToHost,
                                       e->d2h_stream));
        e->d2h_ops++;
    }
    return TW_OK;
}

// ---- environment switches of the enqueue path ---------------------------------------------------------
// Three classes, by WHEN a variable is read: (1) per engine, EngineConfig: read once by make_engine_config when the engine
// is created and const afterwards (TW_LANES, TW_MFREE, TW_RAMP, TW_LAT_FUSED, TW_LAT_GRAPH, TW_CHUNK_TILES, ...); (2) per
// batch, below: read at the start of every flush_ctx call, because the tests switch them between two batches of one
// engine; (3) per process, further below: measurement and diagnostic switches read once, when the process enqueues its
// first batch (and TW_ROCTX, by Roctx).  What tw_set_option changes between batches is no environment switch: EngineOptions.
struct BatchSwitches {
    bool lat_quads;  // TW_LAT_QUADS=0: a single pair's 224 x 8-tile window launches take tw_blur_solve4 as in a batch
    int lat_plan;    // TW_LAT_PLAN: which launches carry the twin schedule's side jobs (plan_twin_side_jobs)
    bool scan_seg;   // TW_SCAN_SEG=0: a single pair's ordered scan as one workgroup (tw_span_scan) — a test compares the two
    bool grid_final; // TW_GRID_FINAL=0: a batch's last level-0 iteration stores the whole field and tw_span_gather samples it
    BatchSwitches()
        : lat_quads(!getenv("TW_LAT_QUADS") || atoi(getenv("TW_LAT_QUADS")) != 0),
          lat_plan(getenv("TW_LAT_PLAN") ? atoi(getenv("TW_LAT_PLAN")) : 1),
          scan_seg(!getenv("TW_SCAN_SEG") || atoi(getenv("TW_SCAN_SEG")) != 0),
          grid_final(!getenv("TW_GRID_FINAL") || atoi(getenv("TW_GRID_FINAL")) != 0)
    {
    }
    BatchSwitches(bool lat_quads_, int lat_plan_, bool scan_seg_, bool grid_final_)  // (no environment read)
        : lat_quads(lat_quads_), lat_plan(lat_plan_), scan_seg(scan_seg_), grid_final(grid_final_)
    {
    }
};
struct ProcessSwitches {
    int side_alone;    // TW_LAT_ALONE — measurement: 1 every side job as its own launch; 2 also the chain kernels through
                       // their twins (empty side)
    int bands;         // TW_LAT_BANDS=n: n bands per level-0 image and level 1 per image (plan_twin_side_jobs)
    bool host_time;    // TW_DEBUG_HOSTTIME — diagnostic: print the host cost of every direct enqueue
    bool scan_direct;  // TW_SCAN_DIRECT (variants library): tw_span_scan<true> samples the flow planes itself
};
const ProcessSwitches& process_switches()
{
    static const ProcessSwitches s = {getenv("TW_LAT_ALONE") ? atoi(getenv("TW_LAT_ALONE")) : 0,
                                      getenv("TW_LAT_BANDS") ? atoi(getenv("TW_LAT_BANDS")) : 0,
                                      getenv("TW_DEBUG_HOSTTIME") != nullptr, getenv("TW_SCAN_DIRECT") != nullptr};
    return s;
}

// ---- the ordered scan's kernel -----------------------------------------------------------------------------
// Which kernel compacts the hits of npairs span grids of gw x gh points, as one pure function: enqueue_scan and
// tw_stage_span_scan launch what it names (launch_scan), and tw_debug_scan_plan shows it to the tests.
//   kernel 0: tw_span_scan<false>, one workgroup per pair, `rounds` rounds of SCAN_IT * 1024 points each (S and segments 0)
//   kernel 1: tw_span_scan_seg, a single pair (single_pair: the batch takes the single-pair schedule) of more than 2 048
//             points in `segments` workgroups of S points — a sixteenth of the grid rounded up to whole iterations of 1 024,
//             at most one round, so the last segment may hold as little as one point — unless TW_SCAN_SEG=0 (scan_seg)
struct ScanChoice {
    int kernel;
    long long G;
    int S, segments, rounds;
};
ScanChoice choose_scan(int npairs, bool single_pair, int gw, int gh, bool scan_seg)
{
    ScanChoice c;
    c.G = (long long)gw * gh;
    const int round = SCAN_IT * 1024;
    const int S = (int)(((c.G + 15) / 16 + 1023) / 1024 * 1024);
    if (npairs == 1 && single_pair && scan_seg && c.G > 2048 && S <= round) {
        c.kernel = 1;
        c.S = S;
        c.segments = (int)((c.G + S - 1) / S);
        c.rounds = 1;
    } else {
        c.kernel = 0;
        c.S = 0;
        c.segments = 0;
        c.rounds = (int)((c.G + round - 1) / round);
    }
    return c;
}
void launch_scan(tw_engine* e, hipStream_t st, const ScanArgs& a, const ScanChoice& sc, int npairs)
{
    if (sc.kernel == 1)
        TW_LAUNCH(e, TW_DF_SPAN_SCAN_SEG, tw_span_scan_seg, dim3((unsigned)sc.segments), dim3(1024), 0, st, a, sc.S);
    else
        TW_LAUNCH(e, TW_DF_SPAN_SCAN, tw_span_scan<false>, dim3(npairs), dim3(1024), 0, st, a);
}
// The span-grid chain's arguments, filled in one place each: a batch (enqueue_span_gather, enqueue_scan), the stage entry
// points and tw_bench_stage launch what these three build, so a stage test runs the batch's own arguments.
// tw_span_gather: npairs fields of two planes in level L's layout, one behind the other at `flow`, sampled every `span`
// pixels into gw x gh points per pair at `grid`
void launch_span_gather(tw_engine* e, hipStream_t st, const float* flow, const LevelPlan& L, int span, int gw, int gh, float2* grid,
                        int npairs)
{
    GatherArgs g;
    g.flow = flow;
    g.fzs = 2 * L.ps;
    g.fps = L.ps;
    g.ld = L.ld;
    g.span = span;
    g.gw = gw;
    g.gh = gh;
    g.g = grid;
    TW_LAUNCH(e, TW_DF_SPAN_GATHER, tw_span_gather, dim3((gw + 63) / 64, (gh + 3) / 4, npairs), dim3(256), 0, st, g);
}
// the scan of those grids: a pair's records lie its whole grid apart; flow, fps and ld are read by tw_span_scan<true> alone
ScanArgs scan_args(const float2* grid, int span, int gw, int gh, double thr2, int* count, ScanRec* rec, const float* flow, long long fps,
                   int ld)
{
    ScanArgs a;
    a.g = grid;
    a.span = span;
    a.gw = gw;
    a.gh = gh;
    a.thr2 = thr2;
    a.count = count;
    a.rec_zs = (long long)gw * gh;
    a.rec = rec;
    a.flow = flow;
    a.fps = fps;
    a.ld = ld;
    return a;
}
// tw_hit_regions behind the scan `a` of w x h images: nrect null when no pair has a rectangle
RegionArgs region_args(const ScanArgs& a, int w, int h, int gap, const int* nrect, const int4* rects, int* lab, int* n_regions,
                       RegionRec* regions, int* region_of)
{
    RegionArgs ra;
    ra.g = a.g;
    ra.span = a.span;
    ra.gw = a.gw;
    ra.gh = a.gh;
    ra.w = w;
    ra.h = h;
    ra.gap = gap;
    ra.thr2 = a.thr2;
    ra.nrect = nrect;
    ra.rects = rects;
    ra.lab = lab;
    ra.n_regions = n_regions;
    ra.regions = regions;
    ra.region_of = region_of;
    return ra;
}
// tw_hit_regions behind a scan of the same pairs: the label plane in LDS when the grid fits, in a.lab otherwise
tw_status launch_hit_regions(tw_engine* e, hipStream_t st, const RegionArgs& a, int npairs)
{
    const size_t G = (size_t)a.gw * a.gh;
    if (G <= (size_t)RGN_LDS_POINTS) {
        if (!e->rgn_attr) {
            // (more than the 64 KB a launch may take unannounced)
            TW_HIP(e, hipFuncSetAttribute((const void*)tw_hit_regions<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          RGN_LDS_POINTS * (int)sizeof(int)));
            e->rgn_attr = true;
        }
        TW_LAUNCH(e, TW_DF_HIT_REGIONS, tw_hit_regions<true>, dim3(npairs), dim3(1024), (G * sizeof(int) + 15) / 16 * 16, st, a);
    } else {
        TW_LAUNCH(e, TW_DF_HIT_REGIONS, tw_hit_regions<false>, dim3(npairs), dim3(1024), 0, st, a);
    }
    return TW_OK;
}

// tw_png_unfilter over nimages jobs of a.w x a.h pixels, one workgroup per image.  waves 0: as many waves per image as the
// 128 KB of LDS row buffers allow for this width; 1, 4 or 16: that many (a.w <= PNG_LDS_PIXELS / waves is the caller's check)
void launch_png_unfilter(tw_engine* e, hipStream_t st, const PngArgs& a, int nimages, int waves = 0)
{
    if (waves == 0) waves = a.w <= PNG_LDS_PIXELS / 16 ? 16 : (a.w <= PNG_LDS_PIXELS / 4 ? 4 : 1);
    const dim3 grid((unsigned)nimages);
    if (waves == 16) TW_LAUNCH(e, TW_DF_PNG_UNFILTER, tw_png_unfilter<16>, grid, dim3(1024), 0, st, a);
    else if (waves == 4) TW_LAUNCH(e, TW_DF_PNG_UNFILTER, tw_png_unfilter<4>, grid, dim3(256), 0, st, a);
    else TW_LAUNCH(e, TW_DF_PNG_UNFILTER, tw_png_unfilter<1>, grid, dim3(64), 0, st, a);
}

// tw_warp_residual over pairs whose images are srcs[2z], srcs[2z + 1] and whose final level-0 flow lies in `flow`
void launch_warp_residual(tw_engine* e, hipStream_t st, const uint8_t* const* srcs, long long stride, const float* flow,
                          const LevelPlan& L, int span, int tol, int4* cells, int npairs)
{
    WarpResidualArgs a;
    a.srcs = srcs;
    a.stride = stride;
    a.flow = flow;
    a.fzs = 2 * L.ps;
    a.fps = L.ps;
    a.ld = L.ld;
    a.w = L.w;
    a.h = L.h;
    a.span = span;
    a.gw = (L.w + span - 1) / span;
    a.gh = (L.h + span - 1) / span;
    a.cx = std::max(1, WR_COLS / span);
    a.cy = std::max(1, WR_ROWS / span);
    a.tol = tol;
    a.cells = cells;
    TW_LAUNCH(e, TW_DF_WARP_RESIDUAL, tw_warp_residual, dim3((a.gw + a.cx - 1) / a.cx, (a.gh + a.cy - 1) / a.cy, npairs), dim3(256),
              sizeof(int4) * (size_t)a.cx * a.cy, st, a);
}
void launch_change_scan(tw_engine* e, hipStream_t st, const int4* cells, int span, int gw, int gh, int* count, ChangeRec* rec,
                        int npairs)
{
    ChangeScanArgs a;
    a.cells = cells;
    a.span = span;
    a.gw = gw;
    a.gh = gh;
    a.count = count;
    a.rec = rec;
    TW_LAUNCH(e, TW_DF_CHANGE_SCAN, tw_change_scan, dim3(npairs), dim3(1024), 0, st, a);
}

// The plan of the shift estimation's launches (tw_debug_shift_plan shows it to the tests): whether an axis of length L keeps both
// profiles in LDS, and the grids
bool shift_axis_in_lds(int L) { return (size_t)L * 2 * sizeof(unsigned) <= (size_t)SS_LDS_BYTES; }
dim3 shift_profiles_grid(int w, int h, int nimages) { return dim3((w + 1023) / 1024, (h + SP_ROWS - 1) / SP_ROWS, nimages); }
// tw_shift_profiles, tw_shift_search, tw_shift_verify<0> and <1> over npairs pairs whose images are srcs[2z], srcs[2z + 1]:
// their profiles into `prof`, their records into `rec` (both zeroed here first, in stream order: the kernels accumulate).
// `own`: the pairs' rows of the initial-field table (a pair with a field of its own is never applied), null when no pair has
tw_status launch_shift_estimate(tw_engine* e, hipStream_t st, const uint8_t* const* srcs, long long stride, int aligned4, int w,
                                int h, int radius, bool force_global, unsigned* prof, ShiftRec* rec, const FlowDst* own, int npairs)
{
    const size_t P = 2 * ((size_t)w + h);
    TW_HIP(e, hipMemsetAsync(prof, 0, P * sizeof(unsigned) * npairs, st));
    TW_HIP(e, hipMemsetAsync(rec, 0, sizeof(ShiftRec) * npairs, st));
    ShiftProfArgs pa;
    pa.srcs = srcs;
    pa.stride = stride;
    pa.w = w;
    pa.h = h;
    pa.aligned4 = aligned4;
    pa.prof = prof;
    TW_LAUNCH(e, TW_DF_SHIFT_PROFILES, tw_shift_profiles, shift_profiles_grid(w, h, 2 * npairs), dim3(256), 0, st, pa);
    ShiftSearchArgs sa;
    sa.prof = prof;
    sa.w = w;
    sa.h = h;
    sa.radius = radius;
    sa.lds[0] = !force_global && shift_axis_in_lds(w) ? 1 : 0;
    sa.lds[1] = !force_global && shift_axis_in_lds(h) ? 1 : 0;
    sa.rec = rec;
    const size_t lds = sizeof(unsigned) * 2 * (size_t)std::max(sa.lds[0] ? w : 0, sa.lds[1] ? h : 0);
    TW_LAUNCH(e, TW_DF_SHIFT_SEARCH, tw_shift_search, dim3(2, npairs), dim3(1024), lds, st, sa);
    ShiftVerifyArgs va;
    va.srcs = srcs;
    va.stride = stride;
    va.w = w;
    va.h = h;
    va.npairs = npairs;
    va.rec = rec;
    va.own = own;
    TW_LAUNCH(e, TW_DF_SHIFT_VERIFY, tw_shift_verify<0>, dim3((h + SV_ROWS - 1) / SV_ROWS, npairs), dim3(256), 0, st, va);
    TW_LAUNCH(e, TW_DF_SHIFT_VERIFY, tw_shift_verify<1>, dim3((npairs + 255) / 256), dim3(256), 0, st, va);
    return TW_OK;
}

// The plan of the band launches (tw_debug_band_plan shows it to the tests): bands, signature blocks per row at dx = 0, and
// whether tw_band_search stages a band's signatures in LDS — the band's rows of sigE and the rows of sigT within the radius,
// clipped to the image, at the widest rows (dx = 0), two bytes each
int band_count(int h, int band) { return (h + band - 1) / band; }
int band_blocks(int w) { return (w + 63) / 64; }
size_t band_search_lds_bytes(int w, int h, int radius, int band)
{
    const int rows = std::min(band, h), r = std::min(radius, h / 2);
    return sizeof(unsigned short) * (size_t)band_blocks(w) * ((size_t)rows + std::min(h, rows + 2 * r));
}
bool band_search_in_lds(int w, int h, int radius, int band) { return band_search_lds_bytes(w, h, radius, band) <= (size_t)BS_LDS_BYTES; }
// tw_band_rows, tw_band_search, tw_band_verify<0> and <1> over npairs pairs, behind launch_shift_estimate on the same stream
// (`rec` holds the pairs' dx): their signatures into `sig`, their band records into `bands` (zeroed here first, in stream
// order: tw_band_verify<0> accumulates)
tw_status launch_band_estimate(tw_engine* e, hipStream_t st, const uint8_t* const* srcs, long long stride, int w, int h, int radius,
                               int band, bool force_global, const ShiftRec* rec, unsigned short* sig, BandRec* bands,
                               const FlowDst* own, int npairs)
{
    const int nb = band_count(h, band), nblk0 = band_blocks(w);
    TW_HIP(e, hipMemsetAsync(bands, 0, sizeof(BandRec) * (size_t)nb * npairs, st));
    BandRowsArgs ra;
    ra.srcs = srcs;
    ra.stride = stride;
    ra.w = w;
    ra.h = h;
    ra.nblk0 = nblk0;
    ra.rec = rec;
    ra.sig = sig;
    TW_LAUNCH(e, TW_DF_BAND_ROWS, tw_band_rows, dim3((unsigned)(((size_t)h * nblk0 + 255) / 256), 1, 2 * npairs), dim3(256), 0, st, ra);
    BandSearchArgs sa;
    sa.sig = sig;
    sa.rec = rec;
    sa.w = w;
    sa.h = h;
    sa.nblk0 = nblk0;
    sa.radius = radius;
    sa.band = band;
    sa.nb = nb;
    sa.lds = !force_global && band_search_in_lds(w, h, radius, band) ? 1 : 0;
    sa.bands = bands;
    if (sa.lds && !e->band_attr) {
        // (more than the 64 KB a launch may take unannounced)
        TW_HIP(e, hipFuncSetAttribute((const void*)tw_band_search, hipFuncAttributeMaxDynamicSharedMemorySize, BS_LDS_BYTES));
        e->band_attr = true;
    }
    TW_LAUNCH(e, TW_DF_BAND_SEARCH, tw_band_search, dim3(nb, npairs), dim3(1024), sa.lds ? band_search_lds_bytes(w, h, radius, band) : 0, st, sa);
    BandVerifyArgs va;
    va.srcs = srcs;
    va.stride = stride;
    va.w = w;
    va.h = h;
    va.npairs = npairs;
    va.band = band;
    va.nb = nb;
    va.rec = rec;
    va.bands = bands;
    va.own = own;
    TW_LAUNCH(e, TW_DF_BAND_VERIFY, tw_band_verify<0>, dim3((h + BV_ROWS - 1) / BV_ROWS, npairs), dim3(256), 0, st, va);
    TW_LAUNCH(e, TW_DF_BAND_VERIFY, tw_band_verify<1>, dim3((npairs * nb + 255) / 256), dim3(256), 0, st, va);
    return TW_OK;
}

// One row of tw_flow_export's destination table / tw_flow_area_init's source table: the caller's device memory in place,
// or (staged != null) this context's staging slot — dense rows in the field's own layout; null for a pair without a field
FlowDst flow_table_row(const void* data, ptrdiff_t pitch, int layout, char* staged, int w)
{
    FlowDst d;
    d.p = !data ? nullptr : staged ? staged : (char*)data;
    d.pitch = staged ? (long long)flow_row_bytes(w, layout) : (long long)pitch;
    d.layout = layout;
    d.pad = 0;
    return d;
}

// ---- the level schedule ------------------------------------------------------------------------------------
// What a batch launches for each pyramid level, as one pure function of the plan's geometry, the engine's configuration, the
// batch's switches and traits, and the pairs of the part (a lane's half of the batch, a piece of the cold-start ramp, or
// the whole batch): BatchEnqueue executes it, the byte model and tw_level_runs_flow_iter / tw_level_chunk are views of it,
// and tw_debug_level_plan shows it to the tests.
enum { LS_BATCH = 0, LS_TWO_STREAM = 1, LS_TWIN = 2 };  // level-major batch; one pair on two streams; one pair, twin launches
// where a level's images come from: a pyramid launch of its own; the coarser level's launch wrote them; the level's launch
// writes the next finer level's too (tw_pyr_23 at level 3, tw_pyr_k3f at level 1 — in the twin schedule the head's launches)
enum { IMG_OWN = 0, IMG_FROM_COARSER = 1, IMG_WITH_FINER = 2 };
struct BatchTraits {
    int n, span;
    bool any_fout, any_init;  // a pair has a flow destination / an initial field
    bool prof_on;             // a profiling class is selected
    bool lat_buffers;         // the single-pair buffers (lat_I, lat_R) exist
    // the batch reads its dense final level-0 field itself (TW_OPT_RESIDUAL: tw_warp_residual): the schedule a batch with
    // a flow destination takes, without being one
    bool residual = false;
    // what the schedule reads of the engine besides its configuration (with_engine_state): TW_OPT_SCAN_FUSED_FINAL and
    // TW_OPT_POLYEXP_F32 as tw_set_option left them, and whether single pairs replay a captured graph (TW_LAT_GRAPH=1)
    int scan_fused = 0, poly_f32 = 0;
    bool graph_replay = false;
};
struct LaunchChoice {
    bool flow_iter;  // the launch's iterations are tw_flow_iter (no tw_update_matrices, no M planes)
    bool same;       // the identical-pair flags apply to the launches of the level
};
struct LevelChoice {
    int per, launches, tail;  // pairs per launch (balanced: 64 pairs with a 63-pair chunk are 32 + 32), launches of the part,
                              // and the pairs of the last one
    int images;               // IMG_*
    bool init;                // the level starts from tw_flow_area_init's output (the coarsest level of a batch with initial fields)
    LaunchChoice full, last;  // of a launch of `per` pairs / of the last launch's `tail` pairs
    const LaunchChoice& of(int nc) const { return nc == per ? full : last; }
};
struct LevelSchedule {
    int kind = LS_BATCH, nlanes = 1, levels = 0;
    bool lat_quads = false;    // a single pair's 224 x 8-tile window launches take tw_blur_solve4q (launch_blur)
    bool fused_final = false;  // the last level-0 iteration at the span-grid points only (TW_OPT_SCAN_FUSED_FINAL: tw_blur_grid)
    bool grid_final = false;   // level-0 launches that run tw_flow_iter end in the grid-only iteration (tw_flow_iter<15, 3>)
    bool same01 = false;       // the identical-pair flags apply to the launch that writes levels 1 and 0 (tw_pyr_k3f)
    size_t ws_lane = 0;        // a lane's share of the workspace (floats of I)
    LevelChoice lv[TW_MAX_LEVELS + 1];
    bool single_pair() const { return kind != LS_BATCH; }
};
// TW_LANES=2: the two halves of a batch of at least two pairs on two streams
int batch_lanes(const EngineConfig& cfg, int n) { return (cfg.lanes > 1 && n >= 2) ? cfg.lanes : 1; }
LevelSchedule choose_level_schedule(const EngineConfig& cfg, const Plan& g, const BatchSwitches& sw, const BatchTraits& t, int npart)
{
    LevelSchedule s;
    const int it = cfg.p.pyrIterations;
    s.levels = g.levels;
    s.nlanes = batch_lanes(cfg, t.n);
    for (const LevelPlan& L : g.lv) s.ws_lane = std::max(s.ws_lane, (size_t)L.ps * 2 * L.chunk);
    // one pair: image-only work (pyramid, polynomial expansion) of all levels on the second stream
    // (only worth its cross-stream hand-offs when the image-only work is tens of microseconds: >= 0.1 Mpixel)
    const bool lat = s.nlanes == 1 && t.lat_buffers && single_pair_schedule(cfg, t.n, g.w0, g.h0, g.levels);
    // ... or, for the default parameters at sizes whose pyramid halves exactly (1080p: BASELINE config 2), ONE stream of twin
    // launches: every coarse-level chain kernel carries a piece of the finer levels' image-only work in its own launch
    // (twflow_kernels.hip.h: tw_twin_*) — no cross-queue hand-off anywhere in the pair
    const bool twin = lat && cfg.lat_fused && !t.graph_replay && !t.prof_on && g.levels == 3 && g.fused23 && cfg.pyr_fused &&
                      pyr01_fusable(&g) && !cfg.pyr_generic && cfg.p.polyN == 7 && !t.poly_f32 && cfg.poly_variant == 1 &&
                      cfg.upd_ny == 2 && cfg.win_m == 15 && !cfg.box && it >= 1;
    s.kind = twin ? LS_TWIN : lat ? LS_TWO_STREAM : LS_BATCH;
    s.lat_quads = lat && sw.lat_quads;  // (TW_LAT_QUADS=0: tw_blur_solve4 as in a batch)
    // (a batch with a flow destination needs the last level-0 field itself: never the scan-fused final iteration)
    s.fused_final = scan_fused_level0(cfg, t.scan_fused, t.span) && !t.any_fout && !t.residual;
    // the grid-only last level-0 iteration: a batch that returns hit records alone reads the last field at the span-grid
    // points only.  (it >= 2: a single iteration is the upsampling one; span >= FI_TH: at most one grid row per step)
    s.grid_final = sw.grid_final && !lat && !t.scan_fused && !t.any_fout && !t.residual && it >= 2 && t.span >= FI_TH && cfg.fi_nt == 1024;
    for (int k = 0; k <= g.levels; k++) {
        const LevelPlan& L = g.lv[k];
        LevelChoice& c = s.lv[k];
        c.per = lat ? 1 : balanced_launch_pairs(npart, L.chunk);
        c.launches = (npart + c.per - 1) / c.per;
        c.tail = npart - c.per * (c.launches - 1);
        c.images = IMG_OWN;
        c.init = t.any_init && k == g.levels;
        const bool grid_only = k == 0 && s.fused_final;
        for (LaunchChoice* lc : {&c.full, &c.last}) {
            // THE place "this level runs tw_flow_iter" is decided (level_runs_flow_iter: the CU gate counts the launch's pairs)
            lc->flow_iter = level_runs_flow_iter(cfg, L.w, L.h, lc == &c.full ? c.per : c.tail, lat, grid_only);
            // ... and "the identical-pair flags apply here": only where EVERY reader of the level's second expansions takes the
            // first in their place — tw_flow_iter does, the update / window kernels (and the scan-fused last iteration's
            // tw_update_matrices at level 0) do not, and their levels get both expansions
            lc->same = cfg.same_image && lc->flow_iter && !grid_only;
        }
    }
    if (twin) {  // tw_pyr_23, then tw_pyr_k3f carried by the coarsest level's expansion (enqueue_twin_head launches exactly
                 // these; the labels are what the byte model prices a single pair's levels 2 and 0 by)
        s.lv[3].images = s.lv[1].images = IMG_WITH_FINER;
        s.lv[2].images = s.lv[0].images = IMG_FROM_COARSER;
    } else if (!lat) {
        // levels 3 and 2 from one read of the images (tw_pyr_23): level 3's launch also writes level 2's images, behind its own
        // in the workspace (sized for level 0: there is room — the last condition), and level 2 skips its pyramid launch.  Only
        // when one launch covers the part at both levels: the loop is level-major, a second chunk of level 3 would overwrite
        // the first chunk's level-2 images before level 2 reads them.  (fused23: the plan has at least four levels)
        if (g.fused23 && cfg.pyr_fused && g.lv[3].chunk >= npart && g.lv[2].chunk >= npart &&
            (size_t)(g.lv[3].ps + g.lv[2].ps) * 2 * npart <= s.ws_lane) {
            s.lv[3].images = IMG_WITH_FINER;
            s.lv[2].images = IMG_FROM_COARSER;
        }
        // levels 1 and 0 likewise (tw_pyr_k3f): level 0's images wait in the M1 region, which nothing else touches while levels
        // 1 and 0 both run tw_flow_iter (their iterations ping-pong through M0 only) and which is large enough (5 planes per
        // pair against 2 images of one)
        if (cfg.pyr_fused && pyr01_fusable(&g) && !cfg.pyr_generic && g.lv[1].chunk >= npart && g.lv[0].chunk >= npart &&
            s.lv[0].full.flow_iter && s.lv[1].full.flow_iter) {
            s.lv[1].images = IMG_WITH_FINER;
            s.lv[0].images = IMG_FROM_COARSER;
            // (tw_pyr_k3f writes both levels: it may skip an image only when both levels skip its expansion)
            s.same01 = s.lv[0].full.same && s.lv[1].full.same;
        }
    }
    return s;
}
// The traits a schedule takes from the engine's options and state, the ONE place they are read: what tw_set_option left, and
// whether TW_LAT_GRAPH=1 is still in use.  Its callers are BatchEnqueue's choose step and the two views below it.
BatchTraits with_engine_state(const tw_engine* e, BatchTraits t)
{
    t.scan_fused = e->opt.scan_fused;
    t.poly_f32 = e->opt.poly_f32;
    t.graph_replay = e->graph_replay();
    return t;
}
// The geometry of a size for the exports: the engine's own plan when a batch has built one (its geometry is plan_geometry's,
// fixed at engine creation), else computed into *scratch — 0.5 us against 7 - 18 us a call (profiles/level_schedule.md).
// Null when the size has no plan.
const Plan* plan_geometry_of(const tw_engine* e, int width, int height, Plan* scratch)
{
    const auto it = e->plans.find(std::make_pair(width, height));
    if (it != e->plans.end()) return it->second.get();
    PlanTables tabs;
    const char* why = "";
    if (width < 1 || height < 1 || plan_geometry(e->cfg, width, height, scratch, &tabs, &why) != TW_OK) return nullptr;
    return scratch;
}
// The choice as the exports see it (tw_level_runs_flow_iter, the byte model): a batch of npairs pairs that returns hit records
// at span 10 and nothing else, no profiling class selected, the single-pair buffers in place; the per-level answers are those
// of the batch's first part (the whole batch, or the first lane's half with TW_LANES=2).  Returns the geometry, null without one.
const Plan* level_schedule_view(const tw_engine* e, int width, int height, int npairs, Plan* scratch, LevelSchedule* s)
{
    const Plan* g = plan_geometry_of(e, width, height, scratch);
    if (!g) return nullptr;
    const BatchTraits t = with_engine_state(e, BatchTraits{npairs, 10, false, false, false, true});
    *s = choose_level_schedule(e->cfg, *g, BatchSwitches(true, 1, true, true), t, npairs / batch_lanes(e->cfg, npairs));
    return g;
}

// One launch group of the level loop: pairs [j0, j0 + nc) of the batch at level k, on stream ls with lane's workspace
struct LevelChunk {
    int k, lane, j0, nc;
    LaunchChoice lc;   // of this launch (choose_level_schedule)
    hipStream_t ls;
    float* I;          // the lane's image workspace (batch schedule)
    float* R;          // polynomial expansions of the chunk's images
    float *M0, *M1;
    double* Vbox;      // running column sums of the box window (null: Gaussian window)
    float* flow_cur;   // levels >= 1 keep every pair of the batch, level 0 only the lane's current chunk
    const float* flow_prev;  // the coarser level's flow of the same pairs (null at the coarsest level)
    // scan-fused final iteration (option TW_OPT_SCAN_FUSED_FINAL): nothing but the span grid of the last level-0 flow is
    // read afterwards, so the last window average + solve runs at the grid points only
    bool grid_only;
    // the grid-only last iteration (tw_flow_iter<15, 3>; LevelSchedule::grid_final): the chunk's last tw_flow_iter launch writes
    // the span-grid samples and no field — no tw_span_gather launch
    bool grid_last;
    // a batch with initial flow fields: every chunk of the coarsest level starts from tw_flow_area_init's output (zeros
    // for its pairs without a field) through the non-zero-flow kernels
    bool init_lv;
};

// Everything flush_ctx enqueues for one batch: the steps in the order flush_ctx calls them, then the three schedules
// of the level loop (enqueue_levels) and the launches they share.  Every step returns on the first error status; the
// batch's context then stays un-launched and Submit / tw_wait drop it (drop_batch).
struct BatchEnqueue {
    tw_engine* const e;
    Ctx& c;
    const BatchSwitches sw;  // (read here: once per flush_ctx call)
    const hipStream_t st;
    const int n, it;
    const size_t npx;    // staged images are 256-byte aligned
    const size_t fslot;  // bytes of a pair's slot in the flow staging regions
    Plan* pl = nullptr;
    long long stride;
    int aligned4 = 0;    // every image pointer and the row stride of the batch are 4-byte aligned (upload_tables)
    int gw = 0, gh = 0;  // the span grid of level 0 (span > 0)
    int ramp_b[4] = {0, 0, 0, 0}, ramp_n = 1;  // cold-start ramp: piece i = pairs [ramp_b[i], ramp_b[i + 1]); ramp_n - 1 pieces
    // the schedule (choose_schedule): the batch-wide fields hold for the whole batch, the per-level ones for the part being
    // enqueued (enqueue_batch_levels asks again for every part)
    BatchTraits traits = {};
    LevelSchedule sched;
    std::vector<size_t> lat_off;  // a level's offset in lat_I (x 5 in lat_R)
    // the side jobs of the twin schedule, in the order the chain needs their results (empty in every other schedule)
    std::vector<SideJob> sideq;
    size_t side_next = 0;
    SideJob empty_side;  // (a member: engines of several host threads enqueue at once)

    BatchEnqueue(tw_engine* e_, Ctx& c_)
        : e(e_), c(c_), st(e_->stream), n((int)c_.jobs.size()), it(e_->cfg.p.pyrIterations), npx(staged_image_bytes(c_.w, c_.h)),
          fslot(flow_stage_slot(c_.w, c_.h)), stride(c_.jobs[0].stride)
    {
        empty_side.kind = 1;
        empty_side.g = VGrid{0u, 0u, 0u, 0u, 0u};
    }

    // ---- the steps of a batch, in order ------------------------------------------------------------------

    tw_status reserve_batch_buffers()
    {
        TW_TRY(get_plan(e, c.w, c.h, &pl));
        TW_TRY(reserve_workspace(e, pl, c.span));
        if (c.span > 0) {
            gw = (pl->lv[0].w + c.span - 1) / c.span;
            gh = (pl->lv[0].h + c.span - 1) / c.span;
            // this context has no results outstanding (it is being launched), nothing on the stream uses its records
            const size_t need_rec = (size_t)tw_grid_capacity(c.w, c.h, c.span) * e->cfg.cap;
            TW_TRY(c.d_rec.grow(e, need_rec, need_rec * sizeof(ScanRec) + 256));
            if (c.regions) TW_TRY(reserve_region_buffers(need_rec));
            if (c.residual) TW_TRY(reserve_residual_buffers(need_rec));
        }
        if (c.shift) TW_TRY(reserve_shift_buffers());
        if (c.bands) TW_TRY(reserve_band_buffers());
        // as d_rec above: nothing outstanding reads this context's staging (tw_wait waited for its copies)
        if (c.any_fout_host) TW_TRY(c.d_fstage.grow(e, fslot * e->cfg.cap, fslot * e->cfg.cap + 256));
        return TW_OK;
    }

    // what tw_hit_regions needs: once per engine, once per context, and per grid size (`need_rec` = cap x G, as d_rec)
    tw_status reserve_region_buffers(size_t need_rec)
    {
        const size_t cap = (size_t)e->cfg.cap;
        TW_TRY(e->d_rgn.make(e, region_table_bytes(e->cfg.cap) + 256));
        TW_TRY(c.h_rgn.make(e, region_table_bytes(e->cfg.cap)));
        TW_TRY(c.d_nreg.make(e, sizeof(int) * cap + 256));
        TW_TRY(c.d_regs.make(e, sizeof(RegionRec) * TW_MAX_REGIONS * cap + 256));
        TW_TRY(c.h_nreg.make(e, sizeof(int) * cap));
        TW_TRY(c.h_regs.make(e, sizeof(RegionRec) * TW_MAX_REGIONS * cap));
        TW_TRY(c.h_regof.make(e, sizeof(int) * HOST_RECS * cap));
        // (this context has no results outstanding, as for d_rec)
        TW_TRY(c.d_regof.grow(e, need_rec, need_rec * sizeof(int) + 256));
        // the label planes are the engine's: an earlier batch's launch may still be using them
        if ((size_t)gw * gh > (size_t)RGN_LDS_POINTS)
            TW_TRY(e->d_lab.grow(e, need_rec, need_rec * sizeof(int) + 256, e->stream));
        return TW_OK;
    }

    // what the residual kernels need: once per context, and per grid size (`need_rec` = cap x G, as d_rec)
    tw_status reserve_residual_buffers(size_t need_rec)
    {
        const size_t cap = (size_t)e->cfg.cap;
        TW_TRY(c.d_nchg.make(e, sizeof(int) * cap + 256));
        TW_TRY(c.h_nchg.make(e, sizeof(int) * cap));
        TW_TRY(c.h_chg.make(e, sizeof(ChangeRec) * HOST_RECS * cap));
        // (this context has no results outstanding, as for d_rec)
        TW_TRY(c.d_chg.grow(e, need_rec, need_rec * sizeof(ChangeRec) + 256));
        // the cell plane is the engine's: an earlier batch's launches may still be using it
        TW_TRY(e->d_cells.grow(e, need_rec, need_rec * sizeof(int4) + 256, e->stream));
        return TW_OK;
    }

    // what the shift kernels need: the engine's records and profiles (an earlier batch's launches may still be using them),
    // the context's pinned copy of the records
    tw_status reserve_shift_buffers()
    {
        const size_t cap = (size_t)e->cfg.cap;
        TW_TRY(e->d_shift.make(e, sizeof(ShiftRec) * cap + 256));
        TW_TRY(c.h_shift.make(e, sizeof(ShiftRec) * cap));
        const size_t need = 2 * ((size_t)c.w + c.h) * cap;
        TW_TRY(e->d_sprof.grow(e, need, need * sizeof(unsigned) + 256, e->stream));
        return TW_OK;
    }

    // what the band kernels need, as the shift kernels' buffers: the engine's records and signatures, the context's pinned copy
    tw_status reserve_band_buffers()
    {
        const size_t cap = (size_t)e->cfg.cap;
        const size_t nrec = (size_t)c.nbands() * cap, nsig = 2 * (size_t)c.h * band_blocks(c.w) * cap;
        TW_TRY(e->d_bands.grow(e, nrec, nrec * sizeof(BandRec) + 256, e->stream));
        TW_TRY(c.h_bands.grow(e, nrec, nrec * sizeof(BandRec)));
        TW_TRY(e->d_bsig.grow(e, nsig, nsig * sizeof(unsigned short) + 256, e->stream));
        return TW_OK;
    }

    // tw_submit_png8: reconstruct the filtered rows into the gray image slots, on the copy stream behind the
    // uploads — it runs beside the previous batch's kernels like the uploads themselves
    tw_status enqueue_png_unfilter()
    {
        if (!c.any_png) return enqueue_png_target_resizes();  // (a tw_submit_jpeg batch may have targets of another size)
        for (int j = 0; j < n; j++)
            for (int q = 0; q < 2; q++) {
                PngJob& pj = c.h_png[2 * j + q];
                // (a target of another size has a launch of its own below: the batch-wide one sees a gray image)
                pj.ch = q && c.jobs[j].rkind == RSZ_FLUSH_COPY ? 0 : c.jobs[j].png_ch[q];
                pj.src = c.d_filt() ? c.d_filt() + c.filt_slot * (size_t)(2 * j + q) : nullptr;
                pj.dst = c.d_img + npx * (size_t)(2 * j + q);
                fill_png_kind(pj, j, q);
            }
        // a batch with table kinds: the flag words (zero) and the gray tables ride behind the jobs in the same upload
        size_t nbytes = sizeof(PngJob) * 2 * (size_t)n;
        if (!c.png_luts.empty()) {
            memset(c.h_png + 2 * (size_t)n, 0, sizeof(unsigned) * 2 * (size_t)n);
            memcpy((char*)(c.h_png + 2 * (size_t)n) + sizeof(unsigned) * 2 * (size_t)n, c.png_luts.data(), 256 * c.png_luts.size());
            nbytes += sizeof(unsigned) * 2 * (size_t)n + 256 * c.png_luts.size();
        }
        TW_HIP(e, hipMemcpyAsync(c.d_png, c.h_png, nbytes, hipMemcpyHostToDevice, e->copy_stream));
        PngArgs pa;
        pa.jobs = c.d_png;
        pa.w = c.w;
        pa.h = c.h;
        launch_png_unfilter(e, e->copy_stream, pa, 2 * n);
        return enqueue_png_target_resizes();
    }

    // tw_submit_jpeg: the batch's coefficient planes through the inverse DCT into the gray image slots — a target of another
    // size into its d_tsrc slot, where the batch's tw_resize_u8 launch expects it — in one launch on the copy stream, in
    // front of enqueue_png_unfilter's launches
    tw_status enqueue_jpeg_idct()
    {
        if (!c.any_jpeg) return TW_OK;
        const uint16_t* d_quants = (const uint16_t*)(c.d_jpg + 2 * (size_t)n);
        int wmax = 1, hmax = 1;
        for (int j = 0; j < n; j++)
            for (int q = 0; q < 2; q++) {
                const Job& jb = c.jobs[j];
                JpegJob& jj = c.h_jpg[2 * j + q];
                jj = JpegJob{};
                if (jb.jpg_bw[q] == 0) continue;
                const bool own_size = q && jb.rkind == RSZ_FLUSH_COPY;
                jj.coef = (const int16_t*)(c.d_filt() + c.filt_slot * (size_t)(2 * j + q));
                jj.dst = own_size ? c.d_tsrc() + c.tsrc_slot * (size_t)j : c.d_img + npx * (size_t)(2 * j + q);
                jj.quant = d_quants + 64 * (size_t)jb.jpg_q[q];
                jj.w = own_size ? jb.tw : c.w;
                jj.h = own_size ? jb.th : c.h;
                jj.bw = jb.jpg_bw[q];
                wmax = std::max(wmax, jj.w);
                hmax = std::max(hmax, jj.h);
            }
        memcpy(c.h_jpg + 2 * (size_t)n, c.jpg_quants.data(), 128 * c.jpg_quants.size());
        TW_HIP(e, hipMemcpyAsync(c.d_jpg, c.h_jpg, sizeof(JpegJob) * 2 * (size_t)n + 128 * c.jpg_quants.size(),
                                 hipMemcpyHostToDevice, e->copy_stream));
        JpegArgs ja;
        ja.jobs = c.d_jpg;
        TW_LAUNCH(e, TW_DF_JPEG_IDCT, tw_jpeg_idct, jpeg_idct_grid(wmax, hmax, 2 * n), dim3(8 * JPEG_WG_BLOCKS), 0, e->copy_stream, ja);
        return TW_OK;
    }

    // the kind of image q of pair j, as tw_png_unfilter reads it; the flag words and the gray tables of the batch lie
    // behind the 2n jobs of Ctx::d_png (enqueue_png_unfilter uploads them)
    void fill_png_kind(PngJob& pj, int j, int q) const
    {
        const Job& jb = c.jobs[j];
        unsigned* d_flags = (unsigned*)(c.d_png + 2 * (size_t)n);
        pj.bits = jb.png_bits[q];
        pj.entries = jb.png_entries[q];
        pj.flag = d_flags + (2 * j + q);
        pj.lut = jb.png_lut[q] >= 0 ? (const uint8_t*)(d_flags + 2 * (size_t)n) + 256 * (size_t)jb.png_lut[q] : nullptr;
        pj.pad = 0;
    }

    void launch_resize(hipStream_t ls, const ResizeJob* jobs, int nz)
    {
        ResizeArgs ra;
        ra.jobs = jobs;
        TW_LAUNCH(e, TW_DF_RESIZE_U8, tw_resize_u8, dim3((c.w + 255) / 256, (c.h + RSZ_ROWS - 1) / RSZ_ROWS, nz),
                  dim3(64, RSZ_ROWS), 0, ls, ra);
    }
    // tw_submit_png8_sized: the targets of another size get one more launch of tw_png_unfilter per distinct size, at that
    // size, into their d_tsrc slots (a target that came as gray is there already); one tw_resize_u8 launch then takes them
    // all to their d_img slots — on the copy stream, behind the batch-wide launch and in front of ev_h2d
    tw_status enqueue_png_target_resizes()
    {
        if (!c.any_resize_png) return TW_OK;
        ResizeJob* hr = c.h_rsz + e->cfg.cap;
        // the filtered targets in order of their size: targets of one size share a launch (a page that grew by a few
        // pixels grew in every screenshot of a run), one workgroup per image as in the batch-wide launch
        std::vector<int> order;
        for (int j = 0; j < n; j++) {
            const Job& jb = c.jobs[j];
            const bool on = jb.rkind == RSZ_FLUSH_COPY;
            hr[j] = ResizeJob{};
            if (on) hr[j] = resize_job(c.d_tsrc() + c.tsrc_slot * (size_t)j, jb.tw, jb.th, jb.tw,
                                       c.d_img + npx * (size_t)(2 * j + 1), c.w, c.h, c.w);
            if (on && jb.png_ch[1] > 0) order.push_back(j);
        }
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            return std::make_pair(c.jobs[x].tw, c.jobs[x].th) < std::make_pair(c.jobs[y].tw, c.jobs[y].th);
        });
        for (size_t k = 0; k < order.size(); k++) {
            const int j = order[k];
            PngJob& pj = c.h_rpng[k];
            pj.ch = c.jobs[j].png_ch[1];
            pj.src = c.d_filt() + c.filt_slot * (size_t)(2 * j + 1);
            pj.dst = c.d_tsrc() + c.tsrc_slot * (size_t)j;
            fill_png_kind(pj, j, 1);
        }
        if (!order.empty())
            TW_HIP(e, hipMemcpyAsync(c.d_rpng, c.h_rpng, sizeof(PngJob) * order.size(), hipMemcpyHostToDevice, e->copy_stream));
        TW_HIP(e, hipMemcpyAsync(c.d_rsz + e->cfg.cap, hr, sizeof(ResizeJob) * (size_t)n, hipMemcpyHostToDevice, e->copy_stream));
        for (size_t k0 = 0; k0 < order.size();) {
            const Job& jb = c.jobs[order[k0]];
            size_t k1 = k0 + 1;
            while (k1 < order.size() && c.jobs[order[k1]].tw == jb.tw && c.jobs[order[k1]].th == jb.th) k1++;
            PngArgs pa;
            pa.jobs = c.d_rpng + k0;
            pa.w = jb.tw;
            pa.h = jb.th;
            launch_png_unfilter(e, e->copy_stream, pa, (int)(k1 - k0));
            k0 = k1;
        }
        launch_resize(e->copy_stream, c.d_rsz + e->cfg.cap, n);
        return TW_OK;
    }

    // tw_submit_dev_sized: the batch's device targets of another size (or row pitch) from the caller's memory into their
    // d_img slots, on the compute stream in front of the batch's start event: everything downstream reads a finished slot
    tw_status enqueue_device_target_resizes()
    {
        if (!c.any_resize_dev) return TW_OK;
        ResizeJob* hr = c.h_rsz + 2 * (size_t)e->cfg.cap;
        for (int j = 0; j < n; j++) {
            const Job& jb = c.jobs[j];
            hr[j] = ResizeJob{};
            if (jb.rkind == RSZ_FLUSH_DEV)
                hr[j] = resize_job(jb.t_src, jb.tw, jb.th, jb.tstride, const_cast<uint8_t*>(jb.d_b), c.w, c.h, jb.stride);
        }
        TW_HIP(e, hipMemcpyAsync(c.d_rsz + 2 * (size_t)e->cfg.cap, hr, sizeof(ResizeJob) * (size_t)n, hipMemcpyHostToDevice, st));
        launch_resize(st, c.d_rsz + 2 * (size_t)e->cfg.cap, n);
        return TW_OK;
    }

    // tw_submit_*_ignore: inside every rectangle of the batch the target becomes the expected image, in one launch on the copy
    // stream — behind the uploads, tw_jpeg_idct, tw_png_unfilter and the targets' resizes, in front of the kept copies and of
    // ev_h2d: whatever reads a target afterwards (tw_pair_same first) reads the masked one.  Only targets are written: a
    // resident expected image stays what it is.
    // A frame sequence inside one batch: the expected image of a masked pair may be an image that tw_image_keep is still to
    // copy out of an earlier pair's slot (Job::keep: queued behind this step).  The source is then that slot itself; and when
    // the slot is a masked TARGET, this pair's rectangles wait for that pair's: they go into a later launch (round = that
    // pair's round + 1).  Every other batch has one round, one launch.
    tw_status enqueue_mask_rects()
    {
        if (!c.any_mask) return TW_OK;
        std::vector<int> round(n, 0);
        std::vector<const uint8_t*> src(n, nullptr);
        int rounds = 1;
        for (int j = 0; j < n; j++) {
            const Job& jb = c.jobs[j];
            if (jb.ign.empty()) continue;
            src[j] = jb.res ? jb.res->d : c.d_img + npx * (size_t)(2 * j);
            for (int k = 0; jb.res && c.any_keep && k < j; k++)
                for (int q = 0; q < 2; q++)
                    if (c.jobs[k].keep[q] == jb.res) {
                        src[j] = c.d_img + npx * (size_t)(2 * k + q);
                        if (q == 1 && !c.jobs[k].ign.empty()) round[j] = round[k] + 1;
                    }
            rounds = std::max(rounds, round[j] + 1);
        }
        int nr = 0;
        std::vector<int> first(rounds + 1, 0), wmax(rounds, 1), hmax(rounds, 1);
        for (int r = 0; r < rounds; r++) {
            first[r] = nr;
            for (int j = 0; j < n; j++) {
                if (round[j] != r) continue;
                for (const tw_rect& rc : c.jobs[j].ign) {
                    c.h_msk[nr++] = MaskJob{c.d_img + npx * (size_t)(2 * j + 1), src[j], rc.x, rc.y, rc.x + rc.width, rc.y + rc.height,
                                            (long long)c.w};
                    wmax[r] = std::max(wmax[r], rc.width);
                    hmax[r] = std::max(hmax[r], rc.height);
                }
            }
        }
        first[rounds] = nr;
        TW_HIP(e, hipMemcpyAsync(c.d_msk, c.h_msk, sizeof(MaskJob) * (size_t)nr, hipMemcpyHostToDevice, e->copy_stream));
        for (int r = 0; r < rounds; r++) {
            MaskArgs ma;
            ma.jobs = c.d_msk + first[r];
            TW_LAUNCH(e, TW_DF_MASK_RECTS, tw_mask_rects, mask_rects_grid(wmax[r], hmax[r], first[r + 1] - first[r]),
                      dim3(64, MASK_ROWS), 0, e->copy_stream, ma);
        }
        return TW_OK;
    }

    // tw_image_keep of images this batch's decode launches write: their copies, on the copy stream behind those launches
    // and in front of ev_h2d (a pair of this very batch may read the kept image)
    tw_status enqueue_kept_copies()
    {
        if (!c.any_keep) return TW_OK;
        for (int j = 0; j < n; j++)
            for (int q = 0; q < 2; q++) {
                tw_image*& im = c.jobs[j].keep[q];
                if (!im) continue;
                TW_TRY(queue_keep_copy(e, im, c.d_img + npx * (size_t)(2 * j + q), c.w));
                image_unuse(im);
                im = nullptr;
            }
        c.any_keep = false;
        return TW_OK;
    }

    tw_status mark_uploads_and_plan_ramp()
    {
        c.copy_ops_at_flush = e->copy_ops;
        if (!c.any_host && !c.any_init_host) return TW_OK;
        // the uploads (images, and host initial flow fields) were queued on the copy stream as the jobs came in (Submit)
        TW_HIP(e, hipEventRecord(c.ev_h2d, e->copy_stream));
        // cold-start ramp: nothing of an earlier batch is still running on the compute stream (the first batch after a
        // pause, or a pipeline the host cannot keep filled) — the pairs whose uploads are already marked start now, the
        // rest behind their own marks, instead of all of them behind the batch's last upload (531 MB for 128 pairs of
        // 1080p: ~14 ms of an idle GPU).  A busy stream takes the whole batch in one launch per kernel and level, as before.
        if (e->cfg.ramp && e->cfg.lanes == 1 && !c.any_png && !c.any_jpeg && !c.any_mask && c.nseg > 0 && c.seg_at[0] < n) {
            bool idle = true;
            for (Ctx& o : e->ctx)
                if (&o != &c && o.launched && hipEventQuery(o.ev_done) == hipErrorNotReady) idle = false;
            (void)hipGetLastError();  // (a "not ready" answer is not an error to report later)
            if (idle) {
                for (int i = 0; i < c.nseg; i++)
                    if (c.seg_at[i] < n) ramp_b[ramp_n++] = c.seg_at[i];
            }
        }
        ramp_b[ramp_n++] = n;
        if (ramp_n == 2) TW_HIP(e, hipStreamWaitEvent(st, c.ev_h2d, 0));  // (no ramp: the whole batch behind its last upload)
        if (c.any_host) stride = c.w;
        return TW_OK;
    }

    // the batch's tables on the main stream: image pointers, flow destinations, initial-field sources
    tw_status upload_tables()
    {
        bool al4 = (stride % 4) == 0;
        for (int j = 0; j < n; j++) {
            const Job& jb = c.jobs[j];
            if (jb.h_b) {
                c.h_ptrs[2 * j] = jb.res ? jb.res->d : c.d_img + npx * (2 * j);
                c.h_ptrs[2 * j + 1] = c.d_img + npx * (2 * j + 1);
            } else {
                c.h_ptrs[2 * j] = jb.d_a;
                c.h_ptrs[2 * j + 1] = jb.d_b;
            }
            al4 = al4 && ((uintptr_t)c.h_ptrs[2 * j] % 4 == 0) && ((uintptr_t)c.h_ptrs[2 * j + 1] % 4 == 0);
        }
        aligned4 = al4 ? 1 : 0;
        TW_HIP(e, hipMemcpyAsync((void*)e->d_ptrs, c.h_ptrs, sizeof(void*) * 2 * n, hipMemcpyHostToDevice, st));
        if (c.any_fout) {
            for (int j = 0; j < n; j++) {
                const Job& jb = c.jobs[j];
                c.h_fdst[j] = flow_table_row(jb.fout.data, jb.fout.pitch, jb.fout.layout,
                                             jb.fout_host ? c.d_fstage + fslot * j : nullptr, c.w);
            }
            TW_HIP(e, hipMemcpyAsync((void*)e->d_fdst, c.h_fdst, sizeof(FlowDst) * n, hipMemcpyHostToDevice, st));
        }
        if (c.any_init) {
            for (int j = 0; j < n; j++) {
                const Job& jb = c.jobs[j];
                c.h_fsrc[j] = flow_table_row(jb.fin.data, jb.fin.pitch, jb.fin.layout,
                                             jb.fin_staged ? c.d_istage + fslot * j : nullptr, c.w);
            }
            TW_HIP(e, hipMemcpyAsync((void*)e->d_fsrc, c.h_fsrc, sizeof(FlowDst) * n, hipMemcpyHostToDevice, st));
        }
        if (c.regions && c.any_mask && c.span > 0) {
            // tw_hit_regions leaves out the grid points tw_wait leaves out: the pairs' clipped rectangles, one upload
            int* cnt = (int*)c.h_rgn.p;
            tw_rect* rects = (tw_rect*)(c.h_rgn + region_rects_off(e->cfg.cap));
            for (int j = 0; j < n; j++) {
                const std::vector<tw_rect>& ign = c.jobs[j].ign;
                cnt[j] = (int)ign.size();
                std::copy(ign.begin(), ign.end(), rects + (size_t)j * TW_MAX_IGNORE);
            }
            TW_HIP(e, hipMemcpyAsync(e->d_rgn, c.h_rgn, region_rects_off(e->cfg.cap) + sizeof(tw_rect) * TW_MAX_IGNORE * (size_t)n,
                                     hipMemcpyHostToDevice, st));
        }
        return TW_OK;
    }

    // which of the three schedules the level loop takes, and what it launches per level: choose_level_schedule's answer for
    // the whole batch (the parts of the batch schedule get their own in enqueue_batch_levels)
    tw_status choose_schedule()
    {
        traits = with_engine_state(e, BatchTraits{n, c.span, c.any_fout, c.any_init || c.shift != 0, false, e->lat_I != nullptr, c.residual != 0 && c.span > 0});
        for (int i = 0; i < TW_K_COUNT; i++) traits.prof_on = traits.prof_on || e->prof_level[i] != -2;
        sched = choose_level_schedule(e->cfg, *pl, sw, traits, n);
        if (sched.nlanes > 1) {
            TW_HIP(e, hipEventRecord(e->ev_fork, st));  // uploads + whatever ran before on the main stream
            TW_HIP(e, hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
        }
        lat_off.assign(pl->lv.size(), 0);
        if (sched.single_pair()) {
            size_t off = 0;
            for (size_t k = 0; k < pl->lv.size(); k++) {
                lat_off[k] = off;
                off += (size_t)pl->lv[k].ps * 2;
            }
        }
        return TW_OK;
    }

    // Single pair (BASELINE config 2): ~26 launches and ~10 event operations, half of them kernels of 5-10 us.  With
    // TW_LAT_GRAPH=1 the whole DAG — both streams, their hand-offs — is captured once per (size, span, stride,
    // alignment, options) and replayed with one hipGraphLaunch; the ordered scan and the result copies stay outside
    // (their targets belong to the batch context).  Round 3 measured it: the host is NOT what holds the schedule back
    // (the direct enqueue takes 110 us of host time for 375 us of GPU time, TW_DEBUG_HOSTTIME), and the replayed graph
    // is slower (0.55 ms: kernels of the forked branch stretch to ~40 us quanta behind cross-queue signals), so the
    // direct path is the default and the graph an opt-in A/B switch (profiles/r03_latency.md).
    tw_status enqueue_or_replay_graph()
    {
        // (destinations / fields would be baked into the graph; a reconciled pair's slots are not what the key describes)
        // (a residual batch's launches read the context's cell plane and the batch's tolerance: direct as well; a shift batch is
        // a batch with an initial field: traits.any_init)
        if (sched.single_pair() && traits.graph_replay && !traits.prof_on && !c.any_fout && !traits.any_init && !c.any_resize &&
            !traits.residual) {
            const GraphKey key{c.w, c.h, c.span, stride, aligned4, traits.scan_fused, traits.poly_f32};
            auto git = e->lat_graphs.find(key);
            if (git == e->lat_graphs.end()) {
                hipGraph_t graph = nullptr;
                hipGraphExec_t exec = nullptr;
                bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) == hipSuccess;
                tw_status br = TW_OK;
                if (ok) {
                    br = enqueue_levels();
                    ok = hipStreamEndCapture(st, &graph) == hipSuccess && graph != nullptr && br == TW_OK;
                }
                if (br != TW_OK) {
                    if (graph) (void)hipGraphDestroy(graph);
                    (void)hipGetLastError();
                    return br;
                }
                ok = ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph) (void)hipGraphDestroy(graph);
                if (ok) {
                    git = e->lat_graphs.emplace(key, exec).first;
                } else {
                    (void)hipGetLastError();
                    e->graph_capture_failed = true;  // this runtime cannot capture the schedule: direct launches from now on
                }
            }
            if (git != e->lat_graphs.end()) {
                TW_HIP(e, hipGraphLaunch(git->second, st));
                return TW_OK;
            }
        }
        const auto t_h0 = std::chrono::steady_clock::now();
        TW_TRY(enqueue_levels());
        if (process_switches().host_time)
            fprintf(stderr, "twflow: enqueue of %d pair(s) %dx%d took %.1f us on the host\n", n, c.w, c.h,
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_h0).count());
        return TW_OK;
    }

    // the ordered scan of the whole batch's span grids, and the stop event
    tw_status enqueue_scan()
    {
        if (c.span > 0) {
            const LevelPlan& L = pl->lv[0];
            const ScanArgs a = scan_args(e->d_grid, c.span, gw, gh, c.threshold * c.threshold, e->d_count, c.d_rec, e->flow[0], L.ps, L.ld);
            ProfScope pscope(e, st, TW_K_SCAN, 0);
#ifdef TW_VARIANTS
            // (scan_fused_level0, not fused_final: a batch with a flow destination keeps its gathered grid either way)
            // (a regions batch keeps the gathered grid: tw_hit_regions reads the samples the scan read)
            if (sched.single_pair() && !scan_fused_level0(e->cfg, traits.scan_fused, c.span) && process_switches().scan_direct && !c.regions) {
                TW_LAUNCH(e, TW_DF_SPAN_SCAN, tw_span_scan<true>, dim3(n), dim3(1024), 0, st, a);
            } else
#endif
            {
                // a single pair: 16 segments, each workgroup counting the hits before its own (tw_span_scan_seg: -5 us of one CU's VALU time)
                launch_scan(e, st, a, choose_scan(n, sched.single_pair(), a.gw, a.gh, sw.scan_seg), n);
            }
            if (c.regions) {
                // the hits' connected components, directly behind the scan and inside `seconds`
                const RegionArgs ra = region_args(a, c.w, c.h, c.regions, c.any_mask ? (const int*)e->d_rgn.p : nullptr,
                                                  (const int4*)(e->d_rgn + region_rects_off(e->cfg.cap)), e->d_lab, c.d_nreg, c.d_regs,
                                                  c.d_regof);
                TW_TRY(launch_hit_regions(e, st, ra, n));
            }
            // the batch's cells with a differing pixel, in order: inside `seconds` too
            if (c.residual) launch_change_scan(e, st, e->d_cells, c.span, gw, gh, c.d_nchg, c.d_chg, n);
        }
        TW_HIP(e, hipEventRecord(c.ev_stop, st));
        return TW_OK;
    }

    tw_status enqueue_result_copies()
    {
        if (c.span > 0) {
            const size_t G = (size_t)tw_grid_capacity(c.w, c.h, c.span);
            const size_t nrec = std::min((size_t)HOST_RECS, G);
            TW_HIP(e, hipMemcpyAsync(c.h_count, e->d_count, sizeof(int) * n, hipMemcpyDeviceToHost, st));
            TW_HIP(e, hipMemcpy2DAsync(c.h_rec, HOST_RECS * sizeof(ScanRec), c.d_rec, G * sizeof(ScanRec),
                                       nrec * sizeof(ScanRec), n, hipMemcpyDeviceToHost, st));
            if (c.regions) {
                // with the hits: every pair's region count, kept records and the region of its first HOST_RECS hits
                TW_HIP(e, hipMemcpyAsync(c.h_nreg, c.d_nreg, sizeof(int) * n, hipMemcpyDeviceToHost, st));
                TW_HIP(e, hipMemcpyAsync(c.h_regs, c.d_regs, sizeof(RegionRec) * TW_MAX_REGIONS * (size_t)n, hipMemcpyDeviceToHost, st));
                TW_HIP(e, hipMemcpy2DAsync(c.h_regof, HOST_RECS * sizeof(int), c.d_regof, G * sizeof(int), nrec * sizeof(int), n,
                                           hipMemcpyDeviceToHost, st));
            }
            if (c.residual) {
                // as the hits: every pair's count and its first HOST_RECS change records
                TW_HIP(e, hipMemcpyAsync(c.h_nchg, c.d_nchg, sizeof(int) * n, hipMemcpyDeviceToHost, st));
                TW_HIP(e, hipMemcpy2DAsync(c.h_chg, HOST_RECS * sizeof(ChangeRec), c.d_chg, G * sizeof(ChangeRec),
                                           nrec * sizeof(ChangeRec), n, hipMemcpyDeviceToHost, st));
            }
        }
        // the shift records come back with the batch's other results (tw_ticket_shift)
        if (c.shift) TW_HIP(e, hipMemcpyAsync(c.h_shift, e->d_shift, sizeof(ShiftRec) * n, hipMemcpyDeviceToHost, st));
        if (c.bands) TW_HIP(e, hipMemcpyAsync(c.h_bands, e->d_bands, sizeof(BandRec) * (size_t)c.nbands() * n, hipMemcpyDeviceToHost, st));
        // a batch with palette images: the flag words tw_png_unfilter set for an index without a PLTE entry (tw_wait)
        if (c.any_plte)
            TW_HIP(e, hipMemcpyAsync(c.h_pflag, c.d_png + 2 * (size_t)n, sizeof(unsigned) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
        if (c.any_fout_host) {
            TW_HIP(e, hipEventRecord(c.ev_d2h, e->d2h_stream));
            c.d2h_ops_at_flush = e->d2h_ops;
        }
        TW_HIP(e, hipGetLastError());
        TW_HIP(e, hipEventRecord(c.ev_done, st));
        return TW_OK;
    }

    // ---- the level loop -----------------------------------------------------------------------------------
    // Everything between the batch's start event and the ordered scan: the single-pair schedule may replay it from a
    // captured hipGraph (enqueue_or_replay_graph), every other batch enqueues it directly.
    tw_status enqueue_levels()
    {
        if (sched.single_pair()) TW_TRY(enqueue_shift_estimate(st, 0, n));  // (the flow chain's stream: behind the uploads)
        if (sched.kind == LS_TWIN) return enqueue_twin_pair();
        if (sched.kind == LS_TWO_STREAM) return enqueue_two_stream_pair();
        return enqueue_batch_levels();
    }

    LevelChunk make_chunk(int k, int lane, int j0, int nc) const
    {
        const LevelPlan& L = pl->lv[k];
        LevelChunk ch;
        ch.k = k;
        ch.lane = lane;
        ch.j0 = j0;
        ch.nc = nc;
        ch.lc = sched.lv[k].of(nc);
        ch.ls = lane == 0 ? st : e->stream2;
        const size_t ws_lane = sched.ws_lane;
        ch.I = e->I + ws_lane * lane;
        ch.R = e->R + ws_lane * 5 * lane;
        ch.M0 = e->M[0] + ws_lane / 2 * 5 * lane;
        ch.M1 = e->M[1] + ws_lane / 2 * 5 * lane;
        ch.Vbox = e->Vd ? e->Vd + ws_lane / 2 * 5 * lane : nullptr;
        ch.flow_cur = e->flow[k] + (k == 0 ? (size_t)lane * L.chunk * 2 * L.ps : (size_t)j0 * 2 * L.ps);
        ch.flow_prev = k < pl->levels ? e->flow[k + 1] + (size_t)j0 * 2 * pl->lv[k + 1].ps : nullptr;
        ch.grid_only = k == 0 && sched.fused_final;
        ch.grid_last = k == 0 && sched.grid_final && ch.lc.flow_iter;
        ch.init_lv = sched.lv[k].init;
        return ch;
    }
    // a single pair's only chunk of level k: every level's R stays in lat_R until the pair is done
    LevelChunk pair_chunk(int k) const
    {
        LevelChunk ch = make_chunk(k, 0, 0, 1);
        ch.R = e->lat_R + 5 * lat_off[k];
        return ch;
    }
    float2* grid_of(int j0) const { return e->d_grid + (size_t)j0 * gw * gh; }

    // -- the batch schedule: level-major, every level for all pairs of a part before the next finer level starts.  A part
    // is a lane's half of the batch (TW_LANES=2), or a piece of the cold-start ramp (only with nlanes == 1 and never for a
    // single pair: see where ramp_b is filled)
    tw_status enqueue_batch_levels()
    {
        const bool ramp = ramp_n > 2;
        const int nlanes = sched.nlanes;
        const int nparts = ramp ? ramp_n - 1 : nlanes;
        for (int part = 0; part < nparts; part++) {
            const int lane = ramp ? 0 : part;
            const int lo = ramp ? ramp_b[part] : (int)((long long)n * lane / nlanes);
            const int hi = ramp ? ramp_b[part + 1] : (int)((long long)n * (lane + 1) / nlanes);
            if (ramp) TW_HIP(e, hipStreamWaitEvent(st, part + 1 < nparts ? c.ev_seg[part] : c.ev_h2d, 0));
            sched = choose_level_schedule(e->cfg, *pl, sw, traits, hi - lo);
            TW_TRY(enqueue_pair_same(lane == 0 ? st : e->stream2, lo, hi));
            TW_TRY(enqueue_shift_estimate(lane == 0 ? st : e->stream2, lo, hi));
            for (int k = pl->levels; k >= 0; k--) {
                const LevelPlan& L = pl->lv[k];
                RoctxRange level_range("tw_level %d (%dx%d)", k, L.w, L.h);
                const int per = sched.lv[k].per;
                for (int j0 = lo; j0 < hi; j0 += per) {
                    const LevelChunk ch = make_chunk(k, lane, j0, std::min(per, hi - j0));
                    TW_TRY(enqueue_level_images(ch));
                    bool grid_stored = false;
                    if (ch.lc.flow_iter) enqueue_flow_iter_chain(ch);
                    else enqueue_update_blur_chain(ch, &grid_stored);
                    TW_TRY(enqueue_level0_outputs(ch, grid_stored));
                }
            }
        }
        if (nlanes > 1) {
            TW_HIP(e, hipEventRecord(e->ev_join, e->stream2));
            TW_HIP(e, hipStreamWaitEvent(st, e->ev_join, 0));
        }
        return TW_OK;
    }

    // which pairs [lo, hi) of a part have two byte-identical images: the flags every later launch of the part may read
    // (behind the part's uploads, on the part's stream)
    tw_status enqueue_pair_same(hipStream_t ls, int lo, int hi)
    {
        if (!e->cfg.same_image || hi <= lo) return TW_OK;
        TW_HIP(e, hipMemsetD32Async((hipDeviceptr_t)(e->d_same + lo), 1, hi - lo, ls));
        PairSameArgs a;
        a.srcs = e->d_ptrs + 2 * lo;
        a.same = e->d_same + lo;
        a.stride = stride;
        a.w = c.w;
        a.h = c.h;
        TW_LAUNCH(e, TW_DF_PAIR_SAME, tw_pair_same, dim3((c.h + PS_ROWS - 1) / PS_ROWS, 1, hi - lo), dim3(256), 0, ls, a);
        e->same_valid = true;
        return TW_OK;
    }
    // TW_OPT_SHIFT: the translation of the pairs [lo, hi) of a part, estimated and checked where the images are (behind the
    // part's uploads, on the part's stream) — the records every coarsest-level chunk of the part reads (enqueue_first_flow)
    tw_status enqueue_shift_estimate(hipStream_t ls, int lo, int hi)
    {
        if (!c.shift || hi <= lo) return TW_OK;
        ProfScope pscope(e, ls, TW_K_SCAN, 0);  // (tw_prof_select(TW_K_SCAN): tools/shift_prof.py times the feature's launches)
        const FlowDst* own = c.any_init ? e->d_fsrc + lo : nullptr;
        TW_TRY(launch_shift_estimate(e, ls, e->d_ptrs + 2 * lo, stride, aligned4, c.w, c.h, c.shift, false,
                                     e->d_sprof + 2 * ((size_t)c.w + c.h) * lo, e->d_shift + lo, own, hi - lo));
        if (!c.bands) return TW_OK;
        // TW_OPT_SHIFT_BANDS: a shift per band of rows behind it, from the pairs' dx
        return launch_band_estimate(e, ls, e->d_ptrs + 2 * lo, stride, c.w, c.h, c.shift, c.bands, false, e->d_shift + lo,
                                    e->d_bsig + 2 * (size_t)c.h * band_blocks(c.w) * lo, e->d_bands + (size_t)c.nbands() * lo, own,
                                    hi - lo);
    }
    // a chunk of the coarsest level of a batch that starts from a first flow: the pairs' own fields resized (zeros without
    // one), then the applied shifts of the others
    void enqueue_first_flow(const LevelChunk& ch, float* flow)
    {
        if (c.any_init) launch_area_init(e, ch.ls, pl, flow, ch.j0, ch.nc);
        if (c.shift) {
            ProfScope pscope(e, ch.ls, TW_K_SCAN, 0);
            if (c.bands) launch_band_init(e, ch.ls, pl, flow, ch.j0, ch.nc, c.bands, c.nbands(), !c.any_init);
            else launch_shift_init(e, ch.ls, pl, flow, ch.j0, ch.nc, !c.any_init);
        }
    }
    // the identical-pair flags of a chunk's pairs, where the schedule lets the chunk's launches read them
    const unsigned* same_flags_of(const LevelChunk& ch) const { return ch.lc.same ? e->d_same + ch.j0 : nullptr; }

    // pyramid + polynomial expansion of a chunk's images (batch schedule), from where the schedule says they come
    tw_status enqueue_level_images(const LevelChunk& ch)
    {
        const int k = ch.k, nc = ch.nc;
        const LevelPlan& L = pl->lv[k];
        const int images = sched.lv[k].images;
        // tw_pyr_23 writes level 2's images behind level 3's in the lane's workspace; tw_pyr_k3f leaves level 0's in the M1
        // region (choose_level_schedule has checked that both fit and stay untouched)
        float* Iside = images == IMG_OWN ? nullptr : k >= 2 ? ch.I + (size_t)pl->lv[3].ps * 2 * nc : ch.M1;
        const uint8_t* const* srcs = e->d_ptrs + 2 * ch.j0;
        const unsigned* same = same_flags_of(ch);
        if (images == IMG_WITH_FINER && k == 3) launch_pyr23(e, ch.ls, pl, srcs, stride, aligned4, ch.I, Iside, 2 * nc);
        else if (images == IMG_WITH_FINER) launch_pyr01(e, ch.ls, pl, srcs, stride, aligned4, ch.I, Iside, 2 * nc, sched.same01 ? same : nullptr);
        else if (images == IMG_OWN) launch_pyr(e, ch.ls, pl, k, srcs, stride, aligned4, ch.I, 2 * nc, same);
        const float* Isrc = images == IMG_FROM_COARSER ? Iside : ch.I;
        return launch_polyexp(e, ch.ls, L.w, L.h, L.ld, L.ps, Isrc, ch.R, 2 * nc, k, nullptr, nullptr, same);
    }

    // -- one pair, two streams: the flow chain walks the levels on the main stream, the image-only work of the finer
    // levels runs beside it on the second
    tw_status enqueue_two_stream_pair()
    {
        TW_HIP(e, hipEventRecord(e->ev_fork, st));  // pointer table + uploads + the previous batch's use of lat_I / lat_R
        TW_HIP(e, hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
        TW_TRY(enqueue_pair_images(pl->levels));
        if (pl->levels >= 1) TW_TRY(enqueue_pair_images(pl->levels - 1));
        for (int k = pl->levels; k >= 0; k--) {
            RoctxRange level_range("tw_level %d (%dx%d)", k, pl->lv[k].w, pl->lv[k].h);
            if (k < pl->levels && k <= e->cfg.lat_s2_max) TW_HIP(e, hipStreamWaitEvent(st, e->lat_ev[k], 0));
            const LevelChunk ch = pair_chunk(k);
            bool grid_stored = false;
            enqueue_update_blur_chain(ch, &grid_stored);
            TW_TRY(enqueue_level0_outputs(ch, grid_stored));
            // the image-only work two levels below goes out once this level's chain is enqueued
            if (k >= 2) TW_TRY(enqueue_pair_images(k - 2));
        }
        return TW_OK;
    }
    // image-only work of level k in the two-stream schedule: the coarsest level's is needed at once and stays on the
    // main stream (no hand-off to wait for); the finer levels' go to the second stream.  It is ENQUEUED one level
    // ahead of the flow chain that consumes it (round 3: with all of it enqueued up front the host needed ~40 us for
    // those launches before the first flow-chain kernel was even submitted — the GPU sat idle behind the host).
    tw_status enqueue_pair_images(int k)
    {
        const LevelPlan& L = pl->lv[k];
        const bool second = k < pl->levels && k <= e->cfg.lat_s2_max;
        hipStream_t ws = second ? e->stream2 : st;
        launch_pyr(e, ws, pl, k, e->d_ptrs, stride, aligned4, e->lat_I + lat_off[k], 2);
        TW_TRY(launch_polyexp(e, ws, L.w, L.h, L.ld, L.ps, e->lat_I + lat_off[k], e->lat_R + 5 * lat_off[k], 2, k));
        if (second) TW_HIP(e, hipEventRecord(e->lat_ev[k], e->stream2));
        return TW_OK;
    }

    // -- one pair, twin launches: one stream; the chain launches of levels 3..1 carry the side jobs (side queue below)
    tw_status enqueue_twin_pair()
    {
        TW_TRY(enqueue_twin_head());
        plan_twin_side_jobs();
        for (int k = pl->levels; k >= 0; k--) {
            RoctxRange level_range("tw_level %d (%dx%d)", k, pl->lv[k].w, pl->lv[k].h);
            // whatever this level reads and no chain kernel was left to carry goes out by itself
            while (side_next < sideq.size() && sideq[side_next].need_level >= k) side_done(false);
            const LevelChunk ch = pair_chunk(k);
            bool grid_stored = false;
            enqueue_update_blur_chain(ch, &grid_stored);
            TW_TRY(enqueue_level0_outputs(ch, grid_stored));
        }
        return TW_OK;
    }
    // levels 3 and 2 of both images (tw_pyr_23), then the coarsest level's expansion, which carries the level 0 / 1 images
    tw_status enqueue_twin_head()
    {
        launch_pyr23(e, st, pl, e->d_ptrs, stride, aligned4, e->lat_I + lat_off[3], e->lat_I + lat_off[2], 2);
        const LevelPlan &L0 = pl->lv[0], &L1 = pl->lv[1], &L3 = pl->lv[3];
        SideJob j;
        j.kind = 2;
        j.need_level = 1;
        PyrK3fArgs& a = j.ka;
        a.srcs = e->d_ptrs;
        a.dst0 = e->lat_I + lat_off[0];
        a.dst1 = e->lat_I + lat_off[1];
        a.zs0 = L0.ps;
        a.zs1 = L1.ps;
        a.stride = stride;
        a.w0 = pl->w0;
        a.h0 = pl->h0;
        a.ld0 = L0.ld;
        a.w1 = L1.w;
        a.h1 = L1.h;
        a.ld1 = L1.ld;
        a.a0 = L0.h_kern[1];
        a.a1 = L0.h_kern[0];
        a.b0 = L1.h_kern[1];
        a.b1 = L1.h_kern[0];
        a.aligned4 = (stride % 4 == 0) ? aligned4 : 0;
        j.g = VGrid{(unsigned)((L1.w + 255) / 256), (unsigned)((L1.h + 3) / 4), 2u, 0u, 0u};
        bool used = false;
        TW_TRY(launch_polyexp(e, st, L3.w, L3.h, L3.ld, L3.ps, e->lat_I + lat_off[3], e->lat_R + 5 * lat_off[3], 2, 3, &j, &used));
        if (!used) launch_side_alone(e, st, j);
        return TW_OK;
    }
    // The expansions of levels 2, 1 and 0 as side jobs.  The carriers: the update + `it` window launches of levels 3 and 2,
    // and level 1's update.
    void plan_twin_side_jobs()
    {
        sideq.clear();
        side_next = 0;
        const int gy2 = (pl->lv[2].h + PE_TH - 1) / PE_TH, gy1 = (pl->lv[1].h + PE_TH - 1) / PE_TH, gy0 = (pl->lv[0].h + PE_TH - 1) / PE_TH;
        // Few, large jobs on the coarsest level's launches: a chain launch stretches to its side job's own duration plus
        // ~2 us when it has CUs to spare (level 3: 136 workgroups), but by ~0.7 of the job's when it fills the chip itself
        // (level 2's window launches: 510 five-wave workgroups) — profiles/r05_single_pair.md.  TW_LAT_BANDS=n: n bands per
        // level-0 image and level 1 per image (n = 3: the first version's nine jobs on nine carriers)
        const int bands_env = process_switches().bands;
        push_side_poly(2, 0, 2, 0, gy2);
        // TW_LAT_PLAN=0: round 5's plan — everything on level 3's launches (level 1's expansion, then level 0's image by image).
        // 1 (default, round 6): level 1's expansion in `it` bands on level 3's window launches, level 0's in `it` bands (of both
        // images) on LEVEL 1's window launches (tw_twin_s4_poly: 680 two-wave workgroups leave the chip three quarters idle);
        // levels 2's launches and level 1's update carry nothing (they fill the chip: a carried job costs 0.7 of itself there).
        const BlurChoice c1 = choose_blur(e->cfg, pl->lv[1].w, pl->lv[1].h, 1, 1, true, false);
        const bool l1_twin = c1.small == 1 && !c1.forced;  // level 1 takes the 96 x 8 tiles by its size, not by a switch
        if (sw.lat_plan >= 1 && l1_twin && bands_env == 0) {
            push_side_bands(1, gy1, it, 3);
            push_side_bands(0, gy0, it, 1);  // (unequal bands, two of five bands on level 3's launches: all within the noise of this,
                                             //  profiles/r06_single_pair.md)
            return;
        }
        if (bands_env >= 2) {
            push_side_poly(1, 0, 1, 0, gy1);
            push_side_poly(1, 1, 1, 0, gy1);
        } else {
            push_side_poly(1, 0, 2, 0, gy1);
        }
        const int nb = std::min(8, std::max(1, bands_env));  // bands per level-0 image
        const int rows = (gy0 + nb - 1) / nb;
        for (int z = 0; z < 2; z++)
            for (int y0 = 0; y0 < gy0; y0 += rows) push_side_poly(0, z, 1, y0, std::min(rows, gy0 - y0));
    }
    // a side job: tile rows [y0, y0 + ny) of images [z0, z0 + nz) of level k's polynomial expansion
    void push_side_poly(int k, int z0, int nz, int y0, int ny, int carry_level = -1, bool windows_only = false)
    {
        const LevelPlan& L = pl->lv[k];
        SideJob j;
        j.kind = 1;
        j.need_level = k;
        j.carry_level = carry_level;
        j.windows_only = windows_only;
        j.pa.src = e->lat_I + lat_off[k];
        j.pa.dst = e->lat_R + 5 * lat_off[k];
        j.pa.w = L.w;
        j.pa.h = L.h;
        j.pa.ld = L.ld;
        j.pa.ps = L.ps;
        j.pa.c = e->cfg.pc;
        j.g = VGrid{(unsigned)((L.w + PE_TW - 1) / PE_TW), (unsigned)ny, (unsigned)nz, (unsigned)y0, (unsigned)z0};
        sideq.push_back(j);
    }
    // level k's expansion (both images) as nb bands of tile rows, on the window launches of level `carry`
    void push_side_bands(int k, int gy, int nb, int carry)
    {
        const int rows = (gy + nb - 1) / nb;
        for (int y0 = 0; y0 < gy; y0 += rows) push_side_poly(k, 0, 2, y0, std::min(rows, gy - y0), carry, true);
    }
    // the next side job, for the launcher of a chain kernel; side_done launches it by itself if the launcher had no twin
    const SideJob* side_peek() const
    {
        if (side_next >= sideq.size()) return nullptr;
        const int alone = process_switches().side_alone;
        return alone == 2 ? &empty_side : alone ? nullptr : &sideq[side_next];
    }
    // may a launch of level k's chain (its update launch / one of its window launches) carry the next job?
    bool side_ok(int k, bool window) const
    {
        if (side_next >= sideq.size()) return false;
        const SideJob& j = sideq[side_next];
        return (j.carry_level < 0 || j.carry_level == k) && (window || !j.windows_only);
    }
    void side_done(bool used)
    {
        if (side_next >= sideq.size()) return;
        if (!used || process_switches().side_alone) launch_side_alone(e, st, sideq[side_next]);
        side_next++;
    }

    // ---- the launches of a chunk's flow chain (shared by the schedules) ------------------------------------

    // M-free iterations (tw_flow_iter; TW_MFREE): the level's iterations read the previous flow and recompute M
    // inside the kernel — no FarnebackUpdateMatrices launch, no M planes.  Flows ping-pong between the level's
    // flow buffer and the (now unused) M0 workspace so that the last iteration lands in the flow buffer.
    // (with the scan-fused last iteration: it - 1 iterations here, then the M of the last flow from
    // tw_update_matrices<false> into M1 — tw_blur_grid evaluates the window average + solve at the span-grid
    // points from it; a single iteration has no flow of this level to start from and takes the old launches)
    void enqueue_flow_iter_chain(const LevelChunk& ch)
    {
        const int k = ch.k, nc = ch.nc;
        const LevelPlan& L = pl->lv[k];
        const int nfi = ch.grid_only ? it - 1 : it;
        float* buf[2] = {ch.flow_cur, ch.M0};  // iteration i writes buf[(nfi - 1 - i) & 1]: the last one the flow buffer
        if (ch.init_lv) enqueue_first_flow(ch, buf[nfi & 1]);  // (what iteration 0 reads)
        FlowUps ups;
        if (k < pl->levels) {
            const LevelPlan& Pv = pl->lv[k + 1];
            ups = FlowUps{ch.flow_prev, Pv.w, Pv.h, Pv.ld, Pv.ps, L.d_uxofs, L.d_uyofs, L.d_ualpha, L.d_ubeta, L.uxmax,
                          (float)(1. / e->cfg.p.pyrScale)};
        }
        for (int i = 0; i < nfi; i++) {
            float* out = buf[(nfi - 1 - i) & 1];
            const float* in = i == 0 ? (ch.init_lv ? buf[nfi & 1] : nullptr) : buf[(nfi - i) & 1];
            if (ch.grid_last && i == nfi - 1) {  // (i >= 1: `in` is the field of iteration i - 1)
                const FlowIterGrid gp{grid_of(ch.j0), c.span, gw, gh};
                launch_flow_iter(e, ch.ls, L.w, L.h, L.ld, L.ps, ch.R, in, L.ps, nullptr, L.ps, nullptr, nc, k, same_flags_of(ch), &gp);
                break;
            }
            launch_flow_iter(e, ch.ls, L.w, L.h, L.ld, L.ps, ch.R, in, L.ps, out, L.ps,
                             (i == 0 && k < pl->levels) ? &ups : nullptr, nc, k, same_flags_of(ch));
        }
        if (!ch.grid_only) return;
        UpdArgs u;
        memset(&u, 0, sizeof(u));
        u.R = ch.R;
        u.flow = ch.flow_cur;
        u.M = ch.M1;
        u.w = L.w;
        u.h = L.h;
        u.ld = L.ld;
        u.ps = L.ps;
        u.fps = L.ps;
        {
            ProfScope pscope(e, ch.ls, TW_K_UPDATE_MATRICES, k);
            launch_upd_kernel<false>(e, ch.ls, L.w, L.h, nc, u);
        }
        enqueue_grid_tail(ch, ch.M1);
    }

    // FarnebackUpdateMatrices, then `it` window launches ping-ponging M0 / M1.  In the twin schedule a launch of levels
    // 3..1 carries the next side job when it may; a single pair's last level-0 launch stores the span-grid samples too
    // (*grid_stored: no tw_span_gather launch needed)
    void enqueue_update_blur_chain(const LevelChunk& ch, bool* grid_stored)
    {
        const int k = ch.k, nc = ch.nc;
        const LevelPlan& L = pl->lv[k];
        if (ch.init_lv) enqueue_first_flow(ch, ch.flow_cur);
        if (k >= 1 && side_ok(k, false)) {
            bool used = false;
            launch_update(e, ch.ls, pl, k, ch.R, ch.flow_cur, ch.flow_prev, ch.M0, nc, side_peek(), &used, ch.init_lv);
            side_done(used);
        } else {
            launch_update(e, ch.ls, pl, k, ch.R, ch.flow_cur, ch.flow_prev, ch.M0, nc, nullptr, nullptr, ch.init_lv);
        }
        for (int i = 0; i < it; i++) {
            const float* Min = (i & 1) ? ch.M1 : ch.M0;
            float* Mout = (i & 1) ? ch.M0 : ch.M1;
            const bool last = i == it - 1;
            if (ch.grid_only && last) {
                enqueue_grid_tail(ch, Min);
                continue;
            }
            BlurLaunch b{L.w, L.h, L.ld, L.ps, Min, Mout, ch.flow_cur, ch.R, !last, k, nc};
            if (k >= 1 && side_ok(k, true)) {
                bool used = false;
                b.side = side_peek();
                b.side_used = &used;
                launch_blur(e, ch.ls, b);
                side_done(used);
                continue;
            }
            b.Vbox = ch.Vbox;
            b.quads = sched.lat_quads;
            GridOut go;
            if (sched.single_pair() && k == 0 && last && c.span > 0) {
                // the launch that stores the final flow stores its span-grid samples too: no tw_span_gather launch
                go = GridOut{grid_of(ch.j0), c.span, gw, gh, grid_stored};
                b.go = &go;
            }
            launch_blur(e, ch.ls, b);
        }
    }

    // the scan-fused final iteration: window average + solve of M at the span-grid points only (the one tw_blur_grid launch)
    void enqueue_grid_tail(const LevelChunk& ch, const float* Min)
    {
        const LevelPlan& L = pl->lv[ch.k];
        BlurGridArgs g;
        g.Min = Min;
        g.w = L.w;
        g.h = L.h;
        g.ld = L.ld;
        g.ps = L.ps;
        g.gw = gw;
        g.gh = gh;
        g.gzs = (long long)g.gw * g.gh;
        g.g = grid_of(ch.j0);
        g.c = e->cfg.wc;
        ProfScope pscope(e, ch.ls, TW_K_BLUR_SOLVE, 0);
        TW_LAUNCH(e, TW_DF_BLUR_GRID, (tw_blur_grid<15, 10, 2>), dim3((g.gw + 21) / 22, (g.gh + 1) / 2, ch.nc), dim3(256), 0, ch.ls, g);
    }

    // grid samples of this chunk -> dense per-pair buffer (the ordered scan runs once per batch).
    // (A scan that samples the flow planes itself — tw_span_scan<true>, TW_SCAN_DIRECT=1 of the variants library — saves this launch and
    // costs more than it: one workgroup's 41 472 scattered dwords are 19.5 us on one CU's memory pipe against
    // 4.8 + 7.3 us for the gather on 81 workgroups + the scan; gpurun_out/r7lat)
    void enqueue_span_gather(const LevelChunk& ch)
    {
        ProfScope pscope(e, ch.ls, TW_K_SCAN, 0);
        launch_span_gather(e, ch.ls, ch.flow_cur, pl->lv[ch.k], c.span, gw, gh, grid_of(ch.j0), ch.nc);
    }

    // what leaves a level-0 chunk once its chain is enqueued: the span-grid samples, the flow fields
    tw_status enqueue_level0_outputs(const LevelChunk& ch, bool grid_stored)
    {
        if (ch.k != 0) return TW_OK;
        if (c.span > 0 && !ch.grid_only && !ch.grid_last && !grid_stored) enqueue_span_gather(ch);
        // (before the next chunk reuses flow_cur, on the chunk's stream)
        if (c.residual && c.span > 0) {
            ProfScope pscope(e, ch.ls, TW_K_SCAN, 0);
            launch_warp_residual(e, ch.ls, e->d_ptrs + 2 * ch.j0, stride, ch.flow_cur, pl->lv[0], c.span, c.residual,
                                 e->d_cells + (size_t)ch.j0 * gw * gh, ch.nc);
        }
        if (c.any_fout) return export_chunk(e, c, ch.ls, pl->lv[0], ch.flow_cur, ch.j0, ch.nc, fslot);
        return TW_OK;
    }
};

// Enqueue a whole batch, level-major: every level is processed for all pairs (in chunks sized to fill the
// chip) before the next finer level starts; level 0 chunks are scanned as soon as their flow exists.
tw_status flush_ctx(tw_engine* e, Ctx& c)
{
    if (c.launched || c.jobs.empty()) return TW_OK;
    BatchEnqueue b(e, c);
    TW_TRY(b.reserve_batch_buffers());
    RoctxRange batch_range("tw_batch %dx%d pairs=%d", c.w, c.h, b.n);
    TW_TRY(b.enqueue_jpeg_idct());
    TW_TRY(b.enqueue_png_unfilter());
    TW_TRY(b.enqueue_mask_rects());
    TW_TRY(b.enqueue_kept_copies());
    TW_TRY(b.mark_uploads_and_plan_ramp());
    TW_TRY(b.upload_tables());
    TW_TRY(b.enqueue_device_target_resizes());
    TW_HIP(e, hipEventRecord(c.ev_start, e->stream));
    TW_TRY(b.choose_schedule());
    e->same_n = b.n;
    e->same_valid = false;  // (until the batch schedule launches tw_pair_same)
    TW_TRY(b.enqueue_or_replay_graph());
    TW_TRY(b.enqueue_scan());
    TW_TRY(b.enqueue_result_copies());
    c.launched = true;
    return TW_OK;
}

size_t staged_image_bytes(int w, int h) { return ((size_t)w * h + 255) / 256 * 256; }

// The one size predicate (check_dims: every submit; every tw_stage_* entry point; tw_debug_check_size).  The stencil
// kernels reach the five planes of R0, R1 or M through ONE raw buffer resource (make_rsrc: num_records 0xFFFFFFFF) and
// pick a plane by a 32-bit scalar byte offset c * ps * 4 next to a 32-bit row / column offset, ps = round_up(w, 32) * h.
// Every byte of the five planes, 20 * ps bytes, must therefore stay inside that 32-bit range: with ps >= 2^28 plane 4's
// offset wraps to 0, and above (2^32 - 1) / 20 the offsets leave the resource's range (whether the range check counts
// the scalar offset was never measured on gfx950; the bound keeps both sides).  ld * h <= 214 748 364: 16384 x 13107
// is admitted, 16384 x 13108 is not.
const long long TW_MAX_PLANE_ELEMS = 0xFFFFFFFFll / 20;

tw_status size_status(int width, int height, const char** why)
{
    if (width < 1 || height < 1 || width > 32768 || height > 32768) {
        *why = "bad image size";
        return TW_E_BAD_PARAMETER;
    }
    if ((long long)round_up(width, 32) * height > TW_MAX_PLANE_ELEMS) {
        *why = "image too large: five float planes of round_up(width, 32) x height must fit 32-bit buffer offsets "
               "(round_up(width, 32) * height <= 214748364)";
        return TW_E_UNSUPPORTED;
    }
    return TW_OK;
}

tw_status check_dims(tw_engine* e, int width, int height)
{
    const char* why = "";
    const tw_status r = size_status(width, height, &why);
    if (r) e->err = why;
    return r;
}

// Page-locked host ranges this library handed out (tw_host_alloc) or was told about (tw_host_register): process-wide,
// because such memory is portable across devices and one engine may free what another one uploads from (a
// per-engine cache of hipPointerGetAttributes answers went stale exactly then, and a stale "pinned" answer turns the
// safe staged upload into a DMA from pageable memory).  Any pointer outside these ranges is treated as pageable and
// staged — always correct, at the cost of one memcpy.  No runtime query per submit (each one also cost ~1 KB of host
// memory that never came back: DESIGN.md §7 "Soak").
struct PinRegistry {
    enum Kind { ALLOC = 1, REGISTERED = 2 };  // how the range was page-locked: decides which HIP call releases it
    struct Range {
        size_t bytes;
        int kind;
    };
    std::mutex m;
    std::map<uintptr_t, Range> ranges;  // start -> bytes, kind
    void add(const void* p, size_t n, int kind)
    {
        std::lock_guard<std::mutex> lk(m);
        ranges[(uintptr_t)p] = Range{n, kind};
    }
    // removes the range that STARTS at p if it was made the same way; 0 = removed, 1 = unknown, 2 = the other kind
    // (tw_host_free on a registered block must not reach hipHostFree on the caller's malloc memory)
    int remove(const void* p, int kind)
    {
        std::lock_guard<std::mutex> lk(m);
        auto it = ranges.find((uintptr_t)p);
        if (it == ranges.end()) return 1;
        if (it->second.kind != kind) return 2;
        ranges.erase(it);
        return 0;
    }
    bool covers(const void* p, size_t n)
    {
        std::lock_guard<std::mutex> lk(m);
        auto it = ranges.upper_bound((uintptr_t)p);
        if (it == ranges.begin()) return false;
        --it;
        return (uintptr_t)p >= it->first && (uintptr_t)p + n <= it->first + it->second.bytes;
    }
};
PinRegistry& pin_registry()
{
    static PinRegistry r;
    return r;
}
bool host_range_is_page_locked(const void* p, size_t n) { return pin_registry().covers(p, n); }

// bytes of `height` filtered rows: the filter type byte and `width` units of ch bytes — or, for a table kind of less than
// 8 bits per pixel (PngJob::bits 1, 2, 4), the ceil(width * bits / 8) bytes the pixels are packed into
size_t png_row_bytes(int width, int ch, int bits = 0)
{
    return 1 + (bits == 1 || bits == 2 || bits == 4 ? ((size_t)width * (size_t)bits + 7) / 8 : (size_t)width * (size_t)ch);
}
size_t png_rows_bytes(int width, int height, int ch, int bits = 0) { return (size_t)height * png_row_bytes(width, ch, bits); }

// libpng 1.5.12 png_do_rgb_to_gray as OpenCV 2.4.9 configures it (the kernel's formula, for the palette's gray table)
uint8_t png_rgb_to_gray(unsigned r, unsigned g, unsigned b)
{
    return (uint8_t)(r == g && g == b ? r : (9797u * r + 19234u * g + 3737u * b) >> 15);
}

// One image of a tw_submit_png / tw_stage_png_decode call as tw_png_unfilter takes it: PngJob's ch, bits and entries, and for
// a table kind (palette, 1- / 2- / 4-bit gray) its 256 gray values in lut.  Refuses what IHDR does not allow and what the
// device does not take (tw_png_on_device: the one predicate).
struct PngKind {
    int ch = 0, bits = 0, entries = 256;
    bool table = false;
};
tw_status describe_png(tw_engine* e, const tw_png_rows* r, const char* what, PngKind* k, uint8_t* lut)
{
    *k = PngKind();
    if (!r || !r->rows) return TW_E_BAD_PARAMETER;
    const int ct = r->color_type, d = r->bit_depth;
    if (ct == TW_PNG_PLAIN_GRAY) return TW_OK;
    const bool pow2 = d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
    const bool ihdr_ok = pow2 && ((ct == 0) || (ct == 3 && d <= 8) || ((ct == 2 || ct == 4 || ct == 6) && d >= 8));
    if (!ihdr_ok || (ct == 3 && (!r->palette || r->palette_entries < 1 || r->palette_entries > 256))) {
        e->err = std::string(what) + (ihdr_ok ? " image: a palette image needs 1 to 256 palette entries"
                                              : " image: IHDR allows no such colour type and bit depth");
        return TW_E_BAD_IMAGE_FORMAT;
    }
    if (!tw_png_on_device(ct, d, 0)) {
        e->err = std::string(what) + " image: this PNG kind is not decoded on the device (16-bit RGB / RGBA)";
        return TW_E_UNSUPPORTED;
    }
    if (ct == 3 || (ct == 0 && d < 8)) {
        k->ch = 1;
        k->bits = d;
        k->table = true;
        memset(lut, 0, 256);
        if (ct == 3) {
            k->entries = r->palette_entries;
            for (int i = 0; i < k->entries; i++) lut[i] = png_rgb_to_gray(r->palette[3 * i], r->palette[3 * i + 1], r->palette[3 * i + 2]);
        } else {
            for (int v = 0; v < (1 << d); v++) lut[v] = (uint8_t)(v * 255 / ((1 << d) - 1));
        }
        return TW_OK;
    }
    const int samples = ct == 0 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
    k->ch = samples * d / 8;              // 16-bit gray: the two-byte unit whose byte 0 is the high byte
    k->bits = ct == 4 && d == 16 ? 16 : 0;  // 16-bit gray + alpha: a four-byte unit without the RGB formula
    return TW_OK;
}

// A flow field of w x h at (data, pitch, layout) — a tw_submit_*_flow destination or a tw_submit_*_flow_init source —
// checked before anything is queued.  *kind = 1: a page-locked host block the library knows; 0: device memory of this
// engine's device that holds the whole field; 2: any other host memory (the caller decides: a destination refuses it).
// A bad pitch or layout, memory of another device, or a device field that overruns its allocation is refused here.
tw_status check_flow_field(tw_engine* e, const void* data, ptrdiff_t pitch, int layout, int w, int h, const char* what,
                           int* kind)
{
    const size_t row = flow_row_bytes(w, layout);
    if (!data || (layout != TW_FLOW_PLANAR && layout != TW_FLOW_INTERLEAVED) || pitch < (ptrdiff_t)row || pitch % 4 != 0) {
        e->err = std::string("bad ") + what + " (null data, unknown layout, or a pitch below the row or not a multiple of 4)";
        return TW_E_BAD_PARAMETER;
    }
    const size_t extent = (size_t)pitch * (flow_rows(h, layout) - 1) + row;
    if (pin_registry().covers(data, extent)) {
        *kind = 1;
        return TW_OK;
    }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, data) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        *kind = 2;
        return TW_OK;
    }
    if (at.device != e->device) {
        e->err = std::string(what) + " is memory of another device";
        return TW_E_BAD_PARAMETER;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(data)) != hipSuccess ||
        (uintptr_t)data + extent > (uintptr_t)base + size) {
        (void)hipGetLastError();
        e->err = std::string(what) + " does not hold the whole field";
        return TW_E_BAD_PARAMETER;
    }
    *kind = 0;
    return TW_OK;
}

// A tw_submit_*_flow destination: *host = a page-locked block the library knows (the export goes through the context's
// staging), otherwise device memory of this engine's device.  Anything else — pageable memory above all
// — is refused.
tw_status check_flow_out(tw_engine* e, const tw_flow_out* o, int w, int h, bool* host)
{
    int kind = 0;
    TW_TRY(check_flow_field(e, o->data, o->pitch, o->layout, w, h, "flow destination", &kind));
    if (kind == 2) {
        e->err = "flow destination is neither device memory nor a page-locked block of tw_host_alloc / tw_host_register";
        return TW_E_BAD_PARAMETER;
    }
    *host = kind == 1;
    return TW_OK;
}

// What a tw_submit_* entry point hands over: one pair as host images (h_a, h_b) or device images (d_a, d_b).
struct Submission {
    const uint8_t *h_a = nullptr, *h_b = nullptr;
    const void *d_a = nullptr, *d_b = nullptr;
    tw_image* res = nullptr;  // tw_submit_image_*: the expected image is this resident image (h_a and d_a null, h_b the target)
    int width = 0, height = 0;
    ptrdiff_t stride = 0;
    int span = 0;
    double threshold = 0;
    int ch_a = 0, ch_b = 0;  // > 0 (tw_submit_png8): that image is `height` filtered PNG rows of 1 + width * ch bytes
    // tw_submit_png: PngJob::bits of those rows; for a table kind its 256 gray values and the number of valid ones
    int bits_a = 0, bits_b = 0;
    const uint8_t *lut_a = nullptr, *lut_b = nullptr;
    int entries_a = 256, entries_b = 256;
    // tw_submit_jpeg: an image that is its luma coefficients (h_a / h_b point at them), null for every other image
    const tw_jpeg_luma *jl_a = nullptr, *jl_b = nullptr;
    // tw_submit_*_sized: the target's own size and row stride; 0 = same as the pair (every other entry point)
    int t_width = 0, t_height = 0;
    ptrdiff_t t_stride = 0;
    const tw_flow_out* fo = nullptr;  // tw_submit_*_flow: where the pair's final flow goes, null for the plain calls
    const tw_flow_in* fi = nullptr;   // tw_submit_*_flow_init: the field the pair starts from, null for a zero start
    // tw_submit_*_ignore: rectangles (pair coordinates) inside which the target becomes the expected image; 0 = the plain call
    const tw_rect* ignore = nullptr;
    int n_ignore = 0;
    tw_ticket* ticket = nullptr;
};

// A batch that cannot be launched (unsupported plan, out of memory) is dropped, not retried by every later submit or
// wait, so that the engine stays usable; its tickets are unknown from then on (find_ticket).
void drop_batch(Ctx& c)
{
    c.release_images();
    c.pending = 0;
    c.jobs.clear();
}

// One submission on its way into a batch: the steps in the order submit() calls them.  Every step returns on the first
// error status, and what it leaves behind then is the step's own business: nothing before book_job books the job, so a
// refused submission consumes no ticket and leaves the open batch as it was.
struct Submit {
    tw_engine* const e;
    const Submission& s;
    const bool png;
    const bool jpeg;             // tw_submit_jpeg with at least one coefficient image
    const bool host;             // a host pair: both images staged, or (tw_submit_image_*) a resident image and a staged target
    const long long eff_stride;  // host images are staged densely; device images are read in place with their stride
    const int tw, th;            // the target's own size (the pair's unless a _sized call says otherwise)
    const ptrdiff_t tstride;
    const bool resize;           // the target goes through tw_resize_u8 (a device target also to change its row pitch)
    Ctx* c = nullptr;
    bool fo_host = false;
    int fi_kind = 0;  // tw_submit_*_flow_init: 0 device memory (read in place), 1 page-locked, 2 other host memory
    Job jb;

    Submit(tw_engine* e_, const Submission& s_)
        : e(e_), s(s_), png(s_.ch_a > 0 || s_.ch_b > 0), jpeg(s_.jl_a || s_.jl_b), host(s_.h_a || s_.res),
          eff_stride(host ? (long long)s_.width : (long long)s_.stride),
          tw(s_.t_width ? s_.t_width : s_.width), th(s_.t_height ? s_.t_height : s_.height),
          tstride(s_.t_stride ? s_.t_stride : s_.stride),
          resize(tw != s_.width || th != s_.height || (!host && tstride != s_.stride))
    {
    }

    static size_t jpeg_coef_bytes(const tw_jpeg_luma* l) { return (size_t)l->blocks_w * (size_t)l->blocks_h * 128; }
    // bytes of a filtered image's (or a coefficient plane's) slot in Ctx::d_filt (each image at its own size)
    size_t filt_need() const
    {
        const size_t need = std::max(s.jl_a ? jpeg_coef_bytes(s.jl_a) : png_rows_bytes(s.width, s.height, s.ch_a, s.bits_a),
                                     s.jl_b ? jpeg_coef_bytes(s.jl_b) : png_rows_bytes(tw, th, s.ch_b, s.bits_b));
        return (need + 255) / 256 * 256;
    }

    // ---- host memory to dense rows at dst, on the copy stream: `rows` rows of `row` bytes, `pitch` apart ----------
    // Page-locked caller memory (tw_host_alloc / tw_host_register): DMA straight from it.  The caller keeps the block
    // unchanged until tw_wait() of this ticket returns.  Dense rows are a plain 1-D transfer (the DMA engines; a
    // pitched 2-D copy may run as a blit kernel on the CUs the flow kernels are using).
    tw_status upload_in_place(void* dst, const void* src, size_t pitch, size_t row, size_t rows)
    {
        if (pitch == row) TW_HIP(e, hipMemcpyAsync(dst, src, row * rows, hipMemcpyHostToDevice, e->copy_stream));
        else TW_HIP(e, hipMemcpy2DAsync(dst, row, src, pitch, row, rows, hipMemcpyHostToDevice, e->copy_stream));
        return TW_OK;
    }

    // Pageable memory: the caller may reuse it as soon as this call returns, and the runtime is never handed a pointer
    // it would have to page-lock on the fly: the rows go through the engine's own pinned bounce buffer,
    // in groups of whole rows of at most BOUNCE_CHUNK bytes (at least one row), and each copy is over before the next
    // one starts (the host layer hands over page-locked arenas; this is the slow, always-correct path)
    tw_status upload_through_bounce(char* dst, const void* src, size_t pitch, size_t row, size_t rows)
    {
        const size_t per = std::max<size_t>(1, BOUNCE_CHUNK / row);  // rows per bounce transfer
        TW_TRY(bounce_reserve(e, std::min(rows, per) * row));
        for (size_t r0 = 0; r0 < rows; r0 += per) {
            const size_t nr = std::min(per, rows - r0);
            for (size_t y = 0; y < nr; y++) memcpy(e->h_bounce + y * row, (const char*)src + (r0 + y) * pitch, row);
            TW_HIP(e, hipMemcpyAsync(dst + r0 * row, e->h_bounce, nr * row, hipMemcpyHostToDevice, e->copy_stream));
            TW_HIP(e, hipStreamSynchronize(e->copy_stream));
        }
        return TW_OK;
    }

    // ---- the steps of a submission, in order ---------------------------------------------------------------

    // no HIP call, nothing booked
    tw_status check_arguments()
    {
        TW_TRY(check_dims(e, s.width, s.height));
        // OpticalFlow::calculate's rule (src/opticalflow.cpp:52-68): more than 5 pixels apart is DontMatchSize
        if (std::abs(s.width - tw) > 5 || std::abs(s.height - th) > 5) {
            e->err = "Don't match image size";
            return TW_E_DONT_MATCH_SIZE;
        }
        if (tw != s.width || th != s.height) TW_TRY(check_dims(e, tw, th));
        const bool png_ok = host && s.h_b && s.ch_a >= 0 && s.ch_a <= 4 && s.ch_b >= 0 && s.ch_b <= 4;
        if (s.span < 0 || s.stride < s.width || tstride < tw || (!host && !s.d_a) || (!s.h_b && !s.d_b) || (s.res && !s.h_b) ||
            ((png || jpeg) && (!png_ok || s.stride != s.width || tstride != tw))) {
            e->err = "bad argument";
            return TW_E_BAD_PARAMETER;
        }
        // (the rectangles are read here, before the call returns; only host pairs have an _ignore call)
        TW_TRY(clip_ignore(e, s.ignore, s.n_ignore, s.width, s.height, &jb.ign));
        if (!jb.ign.empty() && !host) {
            e->err = "bad argument";
            return TW_E_BAD_PARAMETER;
        }
        if (!png) return TW_OK;
        // the filter type byte of every row (ISO/IEC 15948 §9.2: 0-4): checked here, on the host, so that the kernel
        // never has to answer for a damaged stream (libpng: "bad adaptive filter value" -> imread fails)
        const uint8_t* img[2] = {s.h_a, s.h_b};
        const int chs[2] = {s.ch_a, s.ch_b}, bits[2] = {s.bits_a, s.bits_b}, ws[2] = {s.width, tw}, hs[2] = {s.height, th};
        for (int q = 0; q < 2; q++)
            for (int y = 0; chs[q] && y < hs[q]; y++)
                if (img[q][(size_t)y * png_row_bytes(ws[q], chs[q], bits[q])] > 4) {
                    e->err = "bad PNG filter type";
                    return TW_E_BAD_IMAGE_FORMAT;
                }
        return TW_OK;
    }

    // the fields, and what they need once per engine: before the open batch is looked at (a failure books nothing)
    tw_status check_fields()
    {
        TW_HIP(e, hipSetDevice(e->device));
        if (s.fo) {
            TW_TRY(check_flow_out(e, s.fo, s.width, s.height, &fo_host));
            TW_TRY(e->d_fdst.make(e, sizeof(FlowDst) * (size_t)e->cfg.cap + 256));
            if (fo_host && !e->d2h_stream) TW_HIP(e, hipStreamCreateWithFlags(&e->d2h_stream.h, hipStreamNonBlocking));
        }
        if (s.fi) {
            TW_TRY(check_flow_field(e, s.fi->data, s.fi->pitch, s.fi->layout, s.width, s.height, "initial flow field",
                                    &fi_kind));
            TW_TRY(e->d_fsrc.make(e, sizeof(FlowDst) * (size_t)e->cfg.cap + 256));
        }
        return TW_OK;
    }

    // a batch is homogeneous: same size, span, threshold and row stride (and a filtered image larger than the slots
    // this batch's earlier filtered images were given starts a new batch)
    bool fits(const Ctx& b) const
    {
        return !b.launched && !b.jobs.empty() && b.w == s.width && b.h == s.height && b.span == s.span &&
               b.threshold == s.threshold && b.jobs[0].stride == eff_stride && (int)b.jobs.size() < e->cfg.cap &&
               (!(png || jpeg) || b.filt_slot == 0 || filt_need() <= b.filt_slot);
    }

    // c = the context whose open batch takes the pair: the current one's if the pair fits, otherwise a new batch
    tw_status open_batch()
    {
        c = &e->ctx[e->cur];
        if (fits(*c)) return TW_OK;
        const tw_status r = flush_ctx(e, *c);  // (launches an open batch, nothing else)
        if (r) {
            drop_batch(*c);
            return r;
        }
        if (c->pending > 0) {  // still owed to the caller: move on to the next context
            const int nxt = (e->cur + 1) % NCTX;
            if (e->ctx[nxt].pending > 0) return TW_E_BUSY;
            e->cur = nxt;
            c = &e->ctx[nxt];
        }
        c->begin_batch(s.width, s.height, s.span, s.threshold, e->next_ticket, e->opt.regions_gap, e->opt.residual_tol, e->opt.shift_radius,
                       e->opt.shift_bands);
        return TW_OK;
    }

    // what the fields need once per context
    tw_status reserve_context_tables()
    {
        if (s.fo) {
            TW_TRY(c->h_fdst.make(e, sizeof(FlowDst) * (size_t)e->cfg.cap));
            if (!c->ev_fexp) TW_HIP(e, hipEventCreateWithFlags(&c->ev_fexp.h, hipEventDisableTiming));
            if (!c->ev_d2h) TW_HIP(e, hipEventCreateWithFlags(&c->ev_d2h.h, hipEventDisableTiming));
        }
        if (s.fi) TW_TRY(c->h_fsrc.make(e, sizeof(FlowDst) * (size_t)e->cfg.cap));
        return TW_OK;
    }

    // a host field: to this context's staging slot on the copy stream, queued before the pair's ramp mark (a device
    // field is read in place)
    tw_status stage_init_field()
    {
        if (!s.fi || fi_kind == 0) return TW_OK;
        const size_t fslot = flow_stage_slot(s.width, s.height);
        // (grows only on the first host field of a batch: one size per batch; this context's earlier ones are waited)
        TW_TRY(c->d_istage.grow(e, fslot * e->cfg.cap, fslot * e->cfg.cap + 256, e->copy_stream));
        char* dst = c->d_istage + fslot * c->jobs.size();
        const size_t row = flow_row_bytes(s.width, s.fi->layout), rows = flow_rows(s.height, s.fi->layout);
        TW_TRY(fi_kind == 1 ? upload_in_place(dst, s.fi->data, (size_t)s.fi->pitch, row, rows)
                            : upload_through_bounce(dst, s.fi->data, (size_t)s.fi->pitch, row, rows));
        e->copy_ops++;
        return TW_OK;
    }

    // host images go to the pair's two slots of d_img; device inputs only fill the job
    tw_status stage_images()
    {
        jb.stride = eff_stride;
        jb.d_a = (const uint8_t*)s.d_a;
        jb.d_b = (const uint8_t*)s.d_b;
        jb.tw = tw;
        jb.th = th;
        jb.tstride = s.h_a ? (long long)tw : (long long)tstride;
        if (resize) TW_TRY(reserve_resize_tables());
        if (jpeg) TW_TRY(reserve_jpeg_tables());
        if (!jb.ign.empty()) TW_TRY(reserve_mask_tables());
        if (!host) return resize ? stage_device_target() : TW_OK;
        const size_t npx = staged_image_bytes(s.width, s.height);
        // (grows only on the first job of a batch: all jobs of a batch have one size)
        TW_TRY(c->d_img.grow(e, npx * 2 * e->cfg.cap, npx * 2 * e->cfg.cap + 256, e->copy_stream));
        TW_TRY(png || jpeg ? stage_png_rows(npx) : stage_gray_pair(npx));
        jb.h_a = s.h_a;
        jb.h_b = s.h_b;
        jb.res = s.res;  // (book_job takes the batch's reference)
        c->any_host = true;
        e->copy_ops++;
        return TW_OK;
    }

    // what tw_jpeg_idct needs once per context
    tw_status reserve_jpeg_tables()
    {
        TW_TRY(c->h_jpg.make(e, jpeg_table_bytes(e->cfg.cap)));
        TW_TRY(c->d_jpg.make(e, jpeg_table_bytes(e->cfg.cap) + 256));
        c->jpg_quants.reserve(2 * (size_t)e->cfg.cap);
        return TW_OK;
    }

    // what tw_mask_rects needs once per context
    tw_status reserve_mask_tables()
    {
        TW_TRY(c->h_msk.make(e, mask_table_bytes(e->cfg.cap)));
        TW_TRY(c->d_msk.make(e, mask_table_bytes(e->cfg.cap) + 256));
        return TW_OK;
    }

    // tw_submit_png8: filtered rows go to the batch's d_filt slots (tw_png_unfilter writes d_img when the batch is
    // launched), plain gray images of the pair straight to d_img.  tw_submit_jpeg: coefficient planes likewise (tw_jpeg_idct)
    tw_status stage_png_rows(size_t npx)
    {
        const size_t j = c->jobs.size();
        if (c->filt_slot == 0) {
            // first filtered image of this batch: slots as large as the region allows, at least what it needs
            const size_t slot = std::max(filt_need(), c->d_filt_raw.cap / (2 * (size_t)e->cfg.cap) / 256 * 256);
            // 256 bytes of slack on either side: tw_png_unfilter fetches whole 16-byte groups and may read a few
            // bytes before the first and after the last row of an image
            const size_t nbytes = slot * 2 * (size_t)e->cfg.cap;
            TW_TRY(c->d_filt_raw.grow(e, nbytes, nbytes + 512, e->copy_stream));
            // (only now — a failed synchronise / allocation above leaves filt_slot at 0, so that the next
            // filtered image of this batch tries again instead of copying to a null region)
            c->filt_slot = slot;
        }
        if (!c->d_filt()) {
            e->err = "tw_submit_png8: no device region for the filtered rows";
            return TW_E_NOMEM;
        }
        const uint8_t* src[2] = {s.h_a, s.h_b};
        const int chs[2] = {s.ch_a, s.ch_b}, bits[2] = {s.bits_a, s.bits_b}, entries[2] = {s.entries_a, s.entries_b};
        const uint8_t* luts[2] = {s.lut_a, s.lut_b};
        const tw_jpeg_luma* jl[2] = {s.jl_a, s.jl_b};
        for (int q = s.res ? 1 : 0; q < 2; q++) {  // (a resident expected image is where it is)
            // an image is handed over as ONE row: it goes through the bounce buffer whole, whatever its size
            const int wq = q ? tw : s.width, hq = q ? th : s.height;
            const size_t nb = jl[q] ? jpeg_coef_bytes(jl[q]) : chs[q] ? png_rows_bytes(wq, hq, chs[q], bits[q]) : (size_t)wq * hq;
            // (a gray target of another size waits in its d_tsrc slot for the batch's tw_resize_u8 launch)
            uint8_t* dst = chs[q] || jl[q] ? c->d_filt() + c->filt_slot * (2 * j + q)
                                  : (q && resize) ? c->d_tsrc() + c->tsrc_slot * j : c->d_img + npx * (2 * j + q);
            TW_TRY(pin_registry().covers(src[q], nb) ? upload_in_place(dst, src[q], nb, nb, 1)
                                                     : upload_through_bounce((char*)dst, src[q], nb, nb, 1));
        }
        jb.png_ch[0] = s.ch_a;
        jb.png_ch[1] = s.ch_b;
        for (int q = 0; q < 2; q++) {
            jb.png_bits[q] = bits[q];
            jb.png_entries[q] = entries[q];
            if (!luts[q]) continue;
            // (nothing after this point refuses the submission: at most two tables per booked job)
            jb.png_lut[q] = (int)c->png_luts.size();
            c->png_luts.emplace_back();
            memcpy(c->png_luts.back().data(), luts[q], 256);
            c->any_plte = c->any_plte || entries[q] < 256;
        }
        for (int q = 0; q < 2; q++) {
            if (!jl[q]) continue;
            jb.jpg_bw[q] = jl[q]->blocks_w;
            jb.jpg_q[q] = (int)c->jpg_quants.size();
            c->jpg_quants.emplace_back();
            memcpy(c->jpg_quants.back().data(), jl[q]->quant, 128);
        }
        c->any_png = c->any_png || png;
        c->any_jpeg = c->any_jpeg || jpeg;
        if (resize) {
            jb.rkind = RSZ_FLUSH_COPY;
            c->any_resize = c->any_resize_png = true;
        }
        return TW_OK;
    }

    tw_status stage_gray_pair(size_t npx)
    {
        const size_t at = npx * 2 * c->jobs.size();  // the pair's two slots, in d_img and in h_img
        uint8_t *dst_a = c->d_img + at, *dst_b = dst_a + npx;
        const size_t w = (size_t)s.width, h = (size_t)s.height, span_bytes = (size_t)s.stride * (h - 1) + w;
        if (resize) return stage_gray_pair_resized(dst_a, dst_b);
        const size_t span_b = (size_t)tstride * (h - 1) + w;
        if (s.res) {
            // only the target: page-locked in place, pageable through its slot of the pinned ring (the expected image is resident)
            if (pin_registry().covers(s.h_b, span_b)) return upload_in_place(dst_b, s.h_b, (size_t)tstride, w, h);
            TW_TRY(c->h_img.grow(e, npx * 2 * e->cfg.cap, npx * 2 * e->cfg.cap));
            uint8_t* db = c->h_img + at + npx;
            for (size_t y = 0; y < h; y++) memcpy(db + y * w, s.h_b + y * (size_t)tstride, w);
            TW_HIP(e, hipMemcpyAsync(dst_b, db, w * h, hipMemcpyHostToDevice, e->copy_stream));
            return TW_OK;
        }
        if (pin_registry().covers(s.h_a, span_bytes) && pin_registry().covers(s.h_b, span_b)) {
            TW_TRY(upload_in_place(dst_a, s.h_a, (size_t)s.stride, w, h));
            return upload_in_place(dst_b, s.h_b, (size_t)tstride, w, h);
        }
        // pageable: not through the bounce buffer — the pair is copied to its own slots of the context's pinned ring
        // (nothing to wait for) and goes up as one transfer of both images, queued now: it overlaps the caller's next
        // submit and whatever the compute stream is still doing for the previous batch
        TW_TRY(c->h_img.grow(e, npx * 2 * e->cfg.cap, npx * 2 * e->cfg.cap));
        uint8_t* da = c->h_img + at;
        for (size_t y = 0; y < h; y++) {
            memcpy(da + y * w, s.h_a + y * (size_t)s.stride, w);
            memcpy(da + npx + y * w, s.h_b + y * (size_t)tstride, w);
        }
        TW_HIP(e, hipMemcpyAsync(dst_a, da, npx * 2, hipMemcpyHostToDevice, e->copy_stream));
        return TW_OK;
    }

    // ---- tw_submit_*_sized: a target of another size ---------------------------------------------------------
    // what tw_resize_u8 needs once per context, and the staging region at this batch's size (it grows only on the first
    // reconciled pair of a batch: all of a batch's slots have one size; this context's earlier batches are waited)
    tw_status reserve_resize_tables()
    {
        const size_t n = (size_t)e->cfg.cap;
        TW_TRY(c->h_rsz.make(e, sizeof(ResizeJob) * 3 * n));
        TW_TRY(c->d_rsz.make(e, sizeof(ResizeJob) * 3 * n + 256));
        TW_TRY(c->h_rpng.make(e, sizeof(PngJob) * n));
        TW_TRY(c->d_rpng.make(e, sizeof(PngJob) * n + 256));
        if (!host) return TW_OK;  // (a device target is read in place)
        const size_t slot = staged_image_bytes(s.width + 5, s.height + 5), nbytes = slot * n;
        TW_TRY(c->d_tsrc_raw.grow(e, nbytes, nbytes + 512, e->copy_stream));
        c->tsrc_slot = slot;
        return TW_OK;
    }

    // one host image as dense rows, DMA-ed in place when page-locked, through the bounce buffer otherwise
    tw_status upload_rows(uint8_t* dst, const uint8_t* src, size_t pitch, size_t row, size_t rows)
    {
        return pin_registry().covers(src, pitch * (rows - 1) + row) ? upload_in_place(dst, src, pitch, row, rows)
                                                                    : upload_through_bounce((char*)dst, src, pitch, row, rows);
    }

    // a gray host pair whose target has another size: the expected image to its d_img slot, the target to its d_tsrc slot
    // and, right behind that upload on the copy stream, tw_resize_u8 into the pair's second d_img slot — in front of the
    // pair's ramp mark and of ev_h2d, so that everything downstream sees a finished slot
    tw_status stage_gray_pair_resized(uint8_t* dst_a, uint8_t* dst_b)
    {
        const size_t j = c->jobs.size();
        uint8_t* tsrc = c->d_tsrc() + c->tsrc_slot * j;
        if (!s.res) TW_TRY(upload_rows(dst_a, s.h_a, (size_t)s.stride, (size_t)s.width, (size_t)s.height));
        TW_TRY(upload_rows(tsrc, s.h_b, (size_t)tstride, (size_t)tw, (size_t)th));
        c->h_rsz[j] = resize_job(tsrc, tw, th, tw, dst_b, s.width, s.height, s.width);
        TW_HIP(e, hipMemcpyAsync(c->d_rsz + j, c->h_rsz + j, sizeof(ResizeJob), hipMemcpyHostToDevice, e->copy_stream));
        ResizeArgs ra;
        ra.jobs = c->d_rsz + j;
        TW_LAUNCH(e, TW_DF_RESIZE_U8, tw_resize_u8, dim3((s.width + 255) / 256, (s.height + RSZ_ROWS - 1) / RSZ_ROWS, 1),
                  dim3(64, RSZ_ROWS), 0, e->copy_stream, ra);
        jb.rkind = RSZ_SUBMIT;
        c->any_resize = true;
        return TW_OK;
    }

    // a device target of another size (or row pitch): read in place when the batch launches, resized into the pair's
    // second d_img slot, whose pitch is the batch's row stride — the slot is sized for the stride, not the width
    tw_status stage_device_target()
    {
        const size_t dslot = ((size_t)eff_stride * (size_t)s.height + 255) / 256 * 256;
        TW_TRY(c->d_img.grow(e, dslot * 2 * e->cfg.cap, dslot * 2 * e->cfg.cap + 256, e->copy_stream));
        jb.t_src = (const uint8_t*)s.d_b;
        jb.d_b = c->d_img + dslot * (2 * c->jobs.size() + 1);
        jb.rkind = RSZ_FLUSH_DEV;
        c->any_resize = c->any_resize_dev = true;
        return TW_OK;
    }

    // cold-start ramp: mark the copy stream behind the first quarter / half of a full batch's uploads
    // (before the job is booked: a failure here leaves the batch as it was)
    tw_status mark_ramp()
    {
        const int sz = (int)c->jobs.size() + 1;
        if (host && !png && !jpeg && e->cfg.ramp && e->cfg.cap >= 64 && c->nseg < 2 && (sz == e->cfg.cap / 4 || sz == e->cfg.cap / 2)) {
            TW_HIP(e, hipEventRecord(c->ev_seg[c->nseg], e->copy_stream));
            c->seg_at[c->nseg++] = sz;
        }
        return TW_OK;
    }

    // from here on the submission cannot be refused: the job, its ticket
    void book_job()
    {
        if (s.fo) jb.fout = *s.fo;
        if (s.fi) jb.fin = *s.fi;
        jb.fout_host = fo_host;  // (false, and fi_kind 0, without the field)
        jb.fin_staged = fi_kind != 0;
        c->any_fout = c->any_fout || s.fo;
        c->any_fout_host = c->any_fout_host || fo_host;
        c->any_init = c->any_init || s.fi;
        c->any_init_host = c->any_init_host || fi_kind != 0;
        c->any_mask = c->any_mask || !jb.ign.empty();
        if (jb.res) jb.res->uses++;
        c->jobs.push_back(jb);
        c->pending++;
        if (s.ticket) *s.ticket = e->next_ticket;
        e->next_ticket++;
    }

    tw_status launch_if_full()
    {
        const tw_status r = (int)c->jobs.size() == e->cfg.cap ? flush_ctx(e, *c) : TW_OK;
        if (r) drop_batch(*c);
        return r;
    }
};

// Every tw_submit_* entry point: one pair into the engine's open batch, its uploads queued on the copy stream
tw_status submit(tw_engine* e, const Submission& s)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    Submit b(e, s);
    TW_TRY(b.check_arguments());
    TW_TRY(b.check_fields());
    TW_TRY(b.open_batch());
    TW_TRY(b.reserve_context_tables());
    TW_TRY(b.stage_init_field());
    TW_TRY(b.stage_images());
    TW_TRY(b.mark_ramp());
    b.book_job();
    return b.launch_if_full();
}

// The batch context and job index of a ticket that is out and not yet collected; any other ticket is refused.  A call that
// belongs to an option names the batch's setting of it and what it says of a batch opened with the option off (such a
// refusal leaves the ticket waitable).
tw_status find_ticket(tw_engine* e, tw_ticket t, Ctx** ctx, int* idx, int Ctx::*option = nullptr, const char* off = nullptr)
{
    for (Ctx& c : e->ctx) {
        const int64_t j = t - c.first_ticket;
        if (c.pending > 0 && j >= 0 && j < (int64_t)c.jobs.size() && !c.jobs[j].waited) {
            if (option && !(c.*option)) {
                e->err = off;
                return TW_E_BAD_PARAMETER;
            }
            *ctx = &c;
            *idx = (int)j;
            return TW_OK;
        }
    }
    e->err = "unknown ticket";
    return TW_E_BAD_PARAMETER;
}
// ---- what the calls on a ticket share (tw_wait, tw_wait_regions, tw_ticket_*) ------------------------------------------
// A pair's own error, which every call on its ticket answers once the batch has finished: what libpng refuses while it reads
// the rows (the reference opens the expected image first: it wins)
tw_status pair_error(tw_engine* e, const Ctx* c, int j)
{
    if (c->any_plte && (c->h_pflag[2 * j] || c->h_pflag[2 * j + 1])) {
        e->err = std::string("bad palette index in the ") + (c->h_pflag[2 * j] ? "expected" : "target") + " image";
        return TW_E_BAD_IMAGE_FORMAT;
    }
    return TW_OK;
}
// What the calls that leave a ticket waitable share (tw_ticket_changes, _shift, _shift_bands, _hits, _overlay): the ticket's
// batch is launched if it has to be and waited for, the pair's own errors are answered as tw_wait answers them, and the ticket
// is NOT consumed (the wait that collects it does the per-batch bookkeeping of the copy streams).
tw_status ticket_finished(tw_engine* e, Ctx* c, int j)
{
    tw_status r;
    if (!c->launched && (r = flush_ctx(e, *c))) {
        drop_batch(*c);
        return r;
    }
    const hipError_t herr = hipEventSynchronize(c->ev_done);
    if (herr != hipSuccess) {
        e->err = std::string("hipEventSynchronize: ") + hipGetErrorString(herr);
        return TW_E_DEVICE;
    }
    return pair_error(e, c, j);
}
// *recs = the first `want` records of pair j of a finished batch.  The eager copy (`eager`: [cap][HOST_RECS]) holds a pair's
// first HOST_RECS; more than that is rare and comes in one synchronous copy from the context's own plane (`plane`: [cap][G],
// untouched until the batch is collected) into `storage`.
template <typename Rec>
tw_status pair_records(tw_engine* e, const Ctx* c, int j, const Rec* eager, const Rec* plane, int want, std::vector<Rec>& storage,
                       const Rec** recs)
{
    *recs = eager + (size_t)j * HOST_RECS;
    if (want <= HOST_RECS) return TW_OK;
    const size_t G = (size_t)tw_grid_capacity(c->w, c->h, c->span);
    storage.resize(want);
    *recs = storage.data();
    return d2h_sync(e, storage.data(), plane + (size_t)j * G, (size_t)want * sizeof(Rec));
}
// The ignore rule on a pair's records: one whose point lies inside one of the pair's clipped rectangles is not reported.
// keep(record, its index among the kept) for every other record, in order; returns how many those are.
template <typename Rec, typename F>
int outside_rects(const std::vector<tw_rect>& ign, const Rec* rec, int cnt, F keep)
{
    int kept = 0;
    for (int i = 0; i < cnt; i++) {
        bool inside = false;
        for (const tw_rect& r : ign)
            inside = inside || (rec[i].x >= r.x && rec[i].x < r.x + r.width && rec[i].y >= r.y && rec[i].y < r.y + r.height);
        if (!inside) keep(rec[i], kept++);
    }
    return kept;
}
tw_vector to_tw_vector(const ScanRec& r)
{
    return {r.x, r.y, r.dx, r.dy};  // (float widened to double, src/consumer.cpp:72-73)
}
static_assert(sizeof(BandRec) == sizeof(tw_shift_band) && offsetof(BandRec, y) == offsetof(tw_shift_band, y) &&
                  offsetof(BandRec, rows) == offsetof(tw_shift_band, rows) && offsetof(BandRec, dy) == offsetof(tw_shift_band, dy) &&
                  offsetof(BandRec, applied) == offsetof(tw_shift_band, applied) &&
                  offsetof(BandRec, n_shift) == offsetof(tw_shift_band, n_shift) &&
                  offsetof(BandRec, n_zero) == offsetof(tw_shift_band, n_zero) &&
                  offsetof(BandRec, sad_shift) == offsetof(tw_shift_band, sad_shift) &&
                  offsetof(BandRec, sad_zero) == offsetof(tw_shift_band, sad_zero),
              "band records go to the caller as bytes");
// a shift record into the caller's tw_shift, field by field: the caller's padding word stays as it is
void to_tw_shift(const ShiftRec& s, tw_shift* o)
{
    o->dx = s.dx;
    o->dy = s.dy;
    o->applied = s.applied;
    o->n_shift = s.n_shift;
    o->n_zero = s.n_zero;
    o->sad_shift = s.sad_shift;
    o->sad_zero = s.sad_zero;
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

void tw_default_params(tw_params* p)
{
    if (!p) return;
    p->pyrScale = 0.5;
    p->pyrLevels = 3;
    p->winSize = 30;
    p->pyrIterations = 3;
    p->polyN = 7;
    p->polySigma = 1.5;
    p->flags = 256;
}

int tw_abi_version(void) { return TWFLOW_ABI_VERSION; }

int tw_has_variants(void)
{
#ifdef TW_VARIANTS
    return 1;
#else
    return 0;
#endif
}

int tw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

tw_status tw_device_pci_bus_id(int device, char* buf, int cap)
{
    if (!buf || cap < 16) return TW_E_BAD_PARAMETER;
    buf[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return TW_E_DEVICE;
    if (hipDeviceGetPCIBusId(buf, cap, device) != hipSuccess) {
        (void)hipGetLastError();
        buf[0] = 0;
        return TW_E_DEVICE;
    }
    for (char* c = buf; *c; c++)
        if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');  // sysfs names are lower case
    return TW_OK;
}

const char* tw_strerror(tw_status s)
{
    switch (s) {
        case TW_OK: return "OK";
        case TW_E_BAD_PARAMETER: return "BadParameter";
        case TW_E_BAD_IMAGE_FORMAT: return "BadImageFormat";
        case TW_E_DONT_MATCH_SIZE: return "Don't match image size";
        case TW_E_DEVICE: return "HIP device error";
        case TW_E_NOMEM: return "out of device memory";
        case TW_E_UNSUPPORTED: return "unsupported parameter";
        case TW_E_BUSY: return "all slots busy";
    }
    return "unknown";
}

const char* tw_last_error(const tw_engine* e) { return e ? e->err.c_str() : ""; }

int tw_grid_capacity(int width, int height, int span)
{
    if (span <= 0 || width <= 0 || height <= 0) return 0;
    return ((height + span - 1) / span) * ((width + span - 1) / span);
}

tw_status tw_engine_create(int device, const tw_params* params, int slots, tw_engine** out)
{
    if (!out) return TW_E_BAD_PARAMETER;
    *out = nullptr;
    tw_params p;
    if (params) p = *params;
    else tw_default_params(&p);
    // the statuses in this order: parameters (before the device is touched), device, what the configuration refuses
    if (const tw_status st = check_params(p)) return st;
    int n = 0, cus = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return TW_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return TW_E_DEVICE;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    EngineConfig cfg;
    std::string why;
    if (const tw_status st = make_engine_config(p, slots, cus, &cfg, &why)) {
        fputs(why.c_str(), stderr);
        return st;
    }
    slots = cfg.cap;  // (clamped to 1 .. 256)
    tw_engine* e = new tw_engine(cfg);
    e->device = device;
    if (cfg.debug_stamps && e->dbg_stamps.make(e, 4096 * sizeof(unsigned long long)) == TW_OK)
        (void)hipMemset(e->dbg_stamps, 0, 4096 * sizeof(unsigned long long));
    // the main stream carries the dependent flow chain: highest priority, so that its small launches are not queued
    // behind the second stream's image-only work
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    bool ok = hipStreamCreateWithPriority(&e->stream.h, hipStreamNonBlocking, prio_hi) == hipSuccess &&
              hipStreamCreateWithPriority(&e->stream2.h, hipStreamNonBlocking, e->cfg.lanes > 1 ? prio_hi : prio_lo) == hipSuccess &&
              hipStreamCreateWithFlags(&e->copy_stream.h, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&e->ev_fork.h, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&e->ev_join.h, hipEventDisableTiming) == hipSuccess &&
              e->d_ptrs.make(e, sizeof(void*) * 2 * slots + 256) == TW_OK &&
              e->d_count.make(e, sizeof(int) * slots + 256) == TW_OK &&
              e->d_same.make(e, sizeof(unsigned) * slots + 256) == TW_OK &&
              hipMemset(e->d_same, 0, sizeof(unsigned) * slots + 256) == hipSuccess;
    for (Ctx& c : e->ctx) {
        ok = ok && hipEventCreate(&c.ev_start.h) == hipSuccess && hipEventCreate(&c.ev_stop.h) == hipSuccess &&
             hipEventCreateWithFlags(&c.ev_done.h, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c.ev_h2d.h, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c.ev_seg[0].h, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c.ev_seg[1].h, hipEventDisableTiming) == hipSuccess &&
             c.h_ptrs.make(e, sizeof(void*) * 2 * slots) == TW_OK &&
             c.h_count.make(e, sizeof(int) * slots) == TW_OK &&
             (c.png_luts.reserve(2 * (size_t)slots), true) &&
             c.h_png.make(e, png_table_bytes(slots)) == TW_OK &&
             c.h_pflag.make(e, sizeof(unsigned) * 2 * (size_t)slots) == TW_OK &&
             c.d_png.make(e, png_table_bytes(slots) + 256) == TW_OK &&
             c.h_rec.make(e, sizeof(ScanRec) * HOST_RECS * (size_t)slots) == TW_OK;
    }
    if (!ok) {
        tw_engine_destroy(e);
        return TW_E_DEVICE;
    }
    *out = e;
    return TW_OK;
}

void tw_engine_destroy(tw_engine* e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    drop_graphs(e);
    for (tw_image* im : e->res_images) delete im;
    delete e;
}

tw_status tw_submit_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                       ptrdiff_t stride, int span, double threshold, tw_ticket* ticket)
{
    if (!expect || !target) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = stride, .span = span,
                      .threshold = threshold, .ticket = ticket});
}

// (the png8 calls: two plain gray images, both channel counts 0, take the ordinary host path with stride == width)
tw_status tw_submit_png8(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                         int target_channels, int width, int height, int span, double threshold, tw_ticket* ticket)
{
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = width, .span = span,
                      .threshold = threshold, .ch_a = expect_channels, .ch_b = target_channels, .ticket = ticket});
}

tw_status tw_submit_dev(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                        ptrdiff_t stride, int span, double threshold, tw_ticket* ticket)
{
    if (!d_expect || !d_target) return TW_E_BAD_PARAMETER;
    return submit(e, {.d_a = d_expect, .d_b = d_target, .width = width, .height = height, .stride = stride,
                      .span = span, .threshold = threshold, .ticket = ticket});
}

tw_status tw_submit_u8_flow(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                            ptrdiff_t stride, int span, double threshold, const tw_flow_out* out, tw_ticket* ticket)
{
    if (!expect || !target) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = stride, .span = span,
                      .threshold = threshold, .fo = out, .ticket = ticket});
}

tw_status tw_submit_png8_flow(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                              int target_channels, int width, int height, int span, double threshold,
                              const tw_flow_out* out, tw_ticket* ticket)
{
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = width, .span = span,
                      .threshold = threshold, .ch_a = expect_channels, .ch_b = target_channels, .fo = out,
                      .ticket = ticket});
}

tw_status tw_submit_dev_flow(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                             ptrdiff_t stride, int span, double threshold, const tw_flow_out* out, tw_ticket* ticket)
{
    if (!d_expect || !d_target) return TW_E_BAD_PARAMETER;
    return submit(e, {.d_a = d_expect, .d_b = d_target, .width = width, .height = height, .stride = stride,
                      .span = span, .threshold = threshold, .fo = out, .ticket = ticket});
}

tw_status tw_submit_u8_flow_init(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                                 ptrdiff_t stride, int span, double threshold, const tw_flow_in* init,
                                 const tw_flow_out* out, tw_ticket* ticket)
{
    if (!expect || !target) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = stride, .span = span,
                      .threshold = threshold, .fo = out, .fi = init, .ticket = ticket});
}

tw_status tw_submit_png8_flow_init(tw_engine* e, const uint8_t* expect, int expect_channels, const uint8_t* target,
                                   int target_channels, int width, int height, int span, double threshold,
                                   const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = width, .span = span,
                      .threshold = threshold, .ch_a = expect_channels, .ch_b = target_channels, .fo = out, .fi = init,
                      .ticket = ticket});
}

tw_status tw_submit_dev_flow_init(tw_engine* e, const void* d_expect, const void* d_target, int width, int height,
                                  ptrdiff_t stride, int span, double threshold, const tw_flow_in* init,
                                  const tw_flow_out* out, tw_ticket* ticket)
{
    if (!d_expect || !d_target) return TW_E_BAD_PARAMETER;
    return submit(e, {.d_a = d_expect, .d_b = d_target, .width = width, .height = height, .stride = stride,
                      .span = span, .threshold = threshold, .fo = out, .fi = init, .ticket = ticket});
}

// (equal sizes: t_width / t_height name the pair's own size, and the call is the _flow_init call)
tw_status tw_submit_u8_sized(tw_engine* e, const uint8_t* expect, int width, int height, ptrdiff_t stride,
                             const uint8_t* target, int target_width, int target_height, ptrdiff_t target_stride,
                             int span, double threshold, const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    if (!expect || !target || target_width < 1 || target_height < 1 || target_stride < 1) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = stride, .span = span,
                      .threshold = threshold, .t_width = target_width, .t_height = target_height,
                      .t_stride = target_stride, .fo = out, .fi = init, .ticket = ticket});
}

// (without rectangles: exactly the Submission tw_submit_u8_sized builds)
tw_status tw_submit_u8_ignore(tw_engine* e, const uint8_t* expect, int width, int height, ptrdiff_t stride,
                              const uint8_t* target, int target_width, int target_height, ptrdiff_t target_stride, int span,
                              double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                              int n_ignore, tw_ticket* ticket)
{
    if (!expect || !target || target_width < 1 || target_height < 1 || target_stride < 1) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = stride, .span = span,
                      .threshold = threshold, .t_width = target_width, .t_height = target_height,
                      .t_stride = target_stride, .fo = out, .fi = init, .ignore = ignore, .n_ignore = n_ignore,
                      .ticket = ticket});
}

tw_status tw_submit_png8_sized(tw_engine* e, const uint8_t* expect, int expect_channels, int width, int height,
                               const uint8_t* target, int target_channels, int target_width, int target_height,
                               int span, double threshold, const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    if (target_width < 1 || target_height < 1) return TW_E_BAD_PARAMETER;
    return submit(e, {.h_a = expect, .h_b = target, .width = width, .height = height, .stride = width, .span = span,
                      .threshold = threshold, .ch_a = expect_channels, .ch_b = target_channels, .t_width = target_width,
                      .t_height = target_height, .t_stride = target_width, .fo = out, .fi = init, .ticket = ticket});
}

int tw_png_on_device(int color_type, int bit_depth, int interlace)
{
    if (interlace != 0) return 0;
    switch (color_type) {
        case 0: return bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8 || bit_depth == 16;
        case 3: return bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8;
        case 4: return bit_depth == 8 || bit_depth == 16;
        case 2:
        case 6: return bit_depth == 8;
        default: return 0;
    }
}

// (the 8-bit kinds: exactly the Submission tw_submit_png8_sized builds)
tw_status tw_submit_png(tw_engine* e, const tw_png_rows* expect, const tw_png_rows* target, int span, double threshold,
                        const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    return tw_submit_png_ignore(e, expect, target, span, threshold, init, out, nullptr, 0, ticket);
}

tw_status tw_submit_png_ignore(tw_engine* e, const tw_png_rows* expect, const tw_png_rows* target, int span, double threshold,
                               const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore, int n_ignore,
                               tw_ticket* ticket)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    PngKind ka, kb;
    uint8_t lut_a[256], lut_b[256];
    TW_TRY(describe_png(e, expect, "expected", &ka, lut_a));
    TW_TRY(describe_png(e, target, "target", &kb, lut_b));
    if (target->width < 1 || target->height < 1) return TW_E_BAD_PARAMETER;
    Submission s;
    s.h_a = expect->rows;
    s.h_b = target->rows;
    s.width = expect->width;
    s.height = expect->height;
    s.stride = expect->width;
    s.span = span;
    s.threshold = threshold;
    s.ch_a = ka.ch;
    s.ch_b = kb.ch;
    s.bits_a = ka.bits;
    s.bits_b = kb.bits;
    s.lut_a = ka.table ? lut_a : nullptr;
    s.lut_b = kb.table ? lut_b : nullptr;
    s.entries_a = ka.entries;
    s.entries_b = kb.entries;
    s.t_width = target->width;
    s.t_height = target->height;
    s.t_stride = target->width;
    s.fo = out;
    s.fi = init;
    s.ignore = ignore;
    s.n_ignore = n_ignore;
    s.ticket = ticket;
    return submit(e, s);
}

// one image of a tw_submit_jpeg / tw_stage_jpeg_idct call: no HIP call
static tw_status check_jpeg_luma(const tw_jpeg_luma* l)
{
    if (!l || (!l->coef && !l->gray) || l->width < 1 || l->height < 1) return TW_E_BAD_PARAMETER;
    if (!l->coef) return TW_OK;
    const int nbx = (int)(((long long)l->width + 7) / 8), nby = (int)(((long long)l->height + 7) / 8);
    if (l->blocks_w < nbx || l->blocks_w > nbx + 3 || l->blocks_h < nby || l->blocks_h > nby + 3) return TW_E_BAD_PARAMETER;
    return TW_OK;
}

// (both images gray: exactly the Submission tw_submit_u8_sized builds for dense rows)
tw_status tw_submit_jpeg(tw_engine* e, const tw_jpeg_luma* expect, const tw_jpeg_luma* target, int span, double threshold,
                         const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    return tw_submit_jpeg_ignore(e, expect, target, span, threshold, init, out, nullptr, 0, ticket);
}

tw_status tw_submit_jpeg_ignore(tw_engine* e, const tw_jpeg_luma* expect, const tw_jpeg_luma* target, int span,
                                double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                                int n_ignore, tw_ticket* ticket)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    TW_TRY(check_jpeg_luma(expect));
    TW_TRY(check_jpeg_luma(target));
    Submission s;
    s.h_a = expect->coef ? (const uint8_t*)expect->coef : expect->gray;
    s.h_b = target->coef ? (const uint8_t*)target->coef : target->gray;
    s.jl_a = expect->coef ? expect : nullptr;
    s.jl_b = target->coef ? target : nullptr;
    s.width = expect->width;
    s.height = expect->height;
    s.stride = expect->width;
    s.span = span;
    s.threshold = threshold;
    s.t_width = target->width;
    s.t_height = target->height;
    s.t_stride = target->width;
    s.fo = out;
    s.fi = init;
    s.ignore = ignore;
    s.n_ignore = n_ignore;
    s.ticket = ticket;
    return submit(e, s);
}

// ---- resident images ---------------------------------------------------------------------------------------------------

// the engine's own record of a handle the caller passed (null: not one of this engine's live handles)
static tw_image* find_image(const tw_engine* e, const tw_image* img)
{
    auto it = e->res_handles.find(img);
    if (it != e->res_handles.end()) return it->second;
    const_cast<tw_engine*>(e)->err = "not a resident image of this engine (null, released or foreign handle)";
    return nullptr;
}

tw_status tw_image_keep(tw_engine* e, tw_ticket ticket, int which, tw_image** out)
{
    if (!e || !out) return TW_E_BAD_PARAMETER;
    e->err.clear();
    *out = nullptr;
    if (which != TW_KEEP_EXPECT && which != TW_KEEP_TARGET) {
        e->err = "tw_image_keep: which is TW_KEEP_EXPECT or TW_KEEP_TARGET";
        return TW_E_BAD_PARAMETER;
    }
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j));
    TW_HIP(e, hipSetDevice(e->device));
    tw_image* known = which == TW_KEEP_EXPECT ? c->jobs[j].res : nullptr;  // (itself resident: the same block once more)
    if (!known) known = c->jobs[j].keep[which];                            // (kept before, its copy not yet queued)
    if (known) {
        known->handles++;
        e->res_handles[known->handle] = known;
        *out = known->handle;
        return TW_OK;
    }
    // where the image is, and when it is there: a host pair's slot of d_img is written on the copy stream — at submit time
    // (a gray image, a gray target resized there) or by the batch's decode launches; a device pair's images are the caller's,
    // except a reconciled target, which tw_resize_u8 writes on the compute stream in front of the batch's start event
    const bool host = c->jobs[j].h_b != nullptr;
    const bool dev_resized = !host && which == TW_KEEP_TARGET && c->jobs[j].rkind == RSZ_FLUSH_DEV;
    if (dev_resized && !c->launched) {
        const tw_status r = flush_ctx(e, *c);
        if (r) {
            drop_batch(*c);
            return r;
        }
    }
    Job& jb = c->jobs[j];
    // (a masked target is what the batch sees only behind the batch's tw_mask_rects launch)
    const bool at_launch = host && !c->launched &&
                           (jb.png_ch[which] > 0 || jb.jpg_bw[which] > 0 ||
                            (which == TW_KEEP_TARGET && (jb.rkind == RSZ_FLUSH_COPY || !jb.ign.empty())));
    tw_image* im = nullptr;
    TW_TRY(image_new(e, c->w, c->h, &im));
    if (at_launch) {
        jb.keep[which] = im;
        im->uses++;
        c->any_keep = true;
        *out = im->handle;
        return TW_OK;
    }
    tw_status r = TW_OK;
    if (dev_resized && hipStreamWaitEvent(e->copy_stream, c->ev_start, 0) != hipSuccess) {
        (void)hipGetLastError();
        e->err = "tw_image_keep: hipStreamWaitEvent failed";
        r = TW_E_DEVICE;
    }
    const uint8_t* src = host ? c->d_img + staged_image_bytes(c->w, c->h) * (size_t)(2 * j + which) : which ? jb.d_b : jb.d_a;
    if (!r) r = queue_keep_copy(e, im, src, host ? (long long)c->w : jb.stride);
    if (r) {
        im->handles = 0;
        e->res_handles.erase(im->handle);
        image_settle(im);
        return r;
    }
    *out = im->handle;
    return TW_OK;
}

tw_status tw_image_create_u8(tw_engine* e, const uint8_t* gray, int width, int height, ptrdiff_t stride, tw_image** out)
{
    if (!e || !out) return TW_E_BAD_PARAMETER;
    e->err.clear();
    *out = nullptr;
    if (!gray) return TW_E_BAD_PARAMETER;
    TW_TRY(check_dims(e, width, height));
    if (stride < width) {
        e->err = "bad argument";
        return TW_E_BAD_PARAMETER;
    }
    TW_HIP(e, hipSetDevice(e->device));
    tw_image* im = nullptr;
    TW_TRY(image_new(e, width, height, &im));
    const Submission none;
    Submit up(e, none);  // (for its upload step only: page-locked in place, pageable through the bounce buffer)
    const tw_status r = up.upload_rows(im->d, gray, (size_t)stride, (size_t)width, (size_t)height);
    if (r) {
        im->handles = 0;
        e->res_handles.erase(im->handle);
        image_settle(im);
        return r;
    }
    e->copy_ops++;
    *out = im->handle;
    return TW_OK;
}

tw_status tw_image_release(tw_engine* e, tw_image* img)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    tw_image* im = find_image(e, img);
    if (!im) return TW_E_BAD_PARAMETER;
    if (--im->handles == 0) e->res_handles.erase(im->handle);
    image_settle(im);
    return TW_OK;
}

tw_status tw_image_size(const tw_engine* e, const tw_image* img, int* width, int* height)
{
    if (!e) return TW_E_BAD_PARAMETER;
    const tw_image* im = find_image(e, img);
    if (!im) return TW_E_BAD_PARAMETER;
    if (width) *width = im->w;
    if (height) *height = im->h;
    return TW_OK;
}

// (tw_submit_png's Submission with the expected image a plain gray one that is already where the batch reads it)
tw_status tw_submit_image_png(tw_engine* e, const tw_image* expect, const tw_png_rows* target, int span, double threshold,
                              const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    return tw_submit_image_png_ignore(e, expect, target, span, threshold, init, out, nullptr, 0, ticket);
}

tw_status tw_submit_image_png_ignore(tw_engine* e, const tw_image* expect, const tw_png_rows* target, int span,
                                     double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                                     int n_ignore, tw_ticket* ticket)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    tw_image* im = find_image(e, expect);
    if (!im) return TW_E_BAD_PARAMETER;
    PngKind kb;
    uint8_t lut_b[256];
    TW_TRY(describe_png(e, target, "target", &kb, lut_b));
    if (target->width < 1 || target->height < 1) return TW_E_BAD_PARAMETER;
    Submission s;
    s.res = im;
    s.h_b = target->rows;
    s.width = im->w;
    s.height = im->h;
    s.stride = im->w;
    s.span = span;
    s.threshold = threshold;
    s.ch_b = kb.ch;
    s.bits_b = kb.bits;
    s.lut_b = kb.table ? lut_b : nullptr;
    s.entries_b = kb.entries;
    s.t_width = target->width;
    s.t_height = target->height;
    s.t_stride = target->width;
    s.fo = out;
    s.fi = init;
    s.ignore = ignore;
    s.n_ignore = n_ignore;
    s.ticket = ticket;
    return submit(e, s);
}

// (tw_submit_jpeg's Submission likewise)
tw_status tw_submit_image_jpeg(tw_engine* e, const tw_image* expect, const tw_jpeg_luma* target, int span, double threshold,
                               const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    return tw_submit_image_jpeg_ignore(e, expect, target, span, threshold, init, out, nullptr, 0, ticket);
}

tw_status tw_submit_image_jpeg_ignore(tw_engine* e, const tw_image* expect, const tw_jpeg_luma* target, int span,
                                      double threshold, const tw_flow_in* init, const tw_flow_out* out, const tw_rect* ignore,
                                      int n_ignore, tw_ticket* ticket)
{
    if (!e) return TW_E_BAD_PARAMETER;
    e->err.clear();
    tw_image* im = find_image(e, expect);
    if (!im) return TW_E_BAD_PARAMETER;
    TW_TRY(check_jpeg_luma(target));
    Submission s;
    s.res = im;
    s.h_b = target->coef ? (const uint8_t*)target->coef : target->gray;
    s.jl_b = target->coef ? target : nullptr;
    s.width = im->w;
    s.height = im->h;
    s.stride = im->w;
    s.span = span;
    s.threshold = threshold;
    s.t_width = target->width;
    s.t_height = target->height;
    s.t_stride = target->width;
    s.fo = out;
    s.fi = init;
    s.ignore = ignore;
    s.n_ignore = n_ignore;
    s.ticket = ticket;
    return submit(e, s);
}

tw_status tw_submit_dev_sized(tw_engine* e, const void* d_expect, int width, int height, ptrdiff_t stride,
                              const void* d_target, int target_width, int target_height, ptrdiff_t target_stride,
                              int span, double threshold, const tw_flow_in* init, const tw_flow_out* out, tw_ticket* ticket)
{
    if (!d_expect || !d_target || target_width < 1 || target_height < 1 || target_stride < 1) return TW_E_BAD_PARAMETER;
    return submit(e, {.d_a = d_expect, .d_b = d_target, .width = width, .height = height, .stride = stride,
                      .span = span, .threshold = threshold, .t_width = target_width, .t_height = target_height,
                      .t_stride = target_stride, .fo = out, .fi = init, .ticket = ticket});
}

tw_status tw_flush(tw_engine* e)
{
    if (!e) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    return flush_ctx(e, e->ctx[e->cur]);
}

namespace {
// where tw_wait_regions' extra results go (tw_wait: none)
struct RegionsOut {
    int* region_of;
    tw_region* regions;
    int region_cap;
    int* n_regions;
};
// the regions of pair j of a collected batch: `reported` = the vectors the pair reports (what is left after the ignore
// filter), of which the first min(reported, cap) went to the caller.  tw_hit_regions left the same points out, so its
// region_of is parallel to the reported vectors.
tw_status collect_regions(tw_engine* e, Ctx* c, int j, int reported, int cap, const RegionsOut& ro)
{
    const int nreg = c->span > 0 ? c->h_nreg[j] : 0;
    if (ro.n_regions) *ro.n_regions = nreg;
    if (c->span <= 0) return TW_OK;
    if (ro.regions) {
        const int k = std::max(0, std::min(std::min(nreg, ro.region_cap), (int)TW_MAX_REGIONS));
        memcpy(ro.regions, c->h_regs + (size_t)j * TW_MAX_REGIONS, sizeof(tw_region) * (size_t)k);
    }
    const int m = std::max(0, std::min(reported, cap));
    if (ro.region_of && m > 0) {
        if (m <= HOST_RECS) {
            memcpy(ro.region_of, c->h_regof + (size_t)j * HOST_RECS, sizeof(int) * (size_t)m);
        } else {
            // rare, as for the records: the context's own plane still has them
            const size_t G = (size_t)tw_grid_capacity(c->w, c->h, c->span);
            TW_TRY(d2h_sync(e, ro.region_of, c->d_regof + (size_t)j * G, sizeof(int) * (size_t)m));
        }
    }
    return TW_OK;
}

tw_status wait_ticket(tw_engine* e, tw_ticket ticket, tw_vector* out, int cap, int* n, float* seconds, const RegionsOut* ro)
{
    if (!e) return TW_E_BAD_PARAMETER;
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j, ro ? &Ctx::regions : nullptr,
                       "tw_wait_regions: the ticket's batch was opened with TW_OPT_REGIONS off"));
    TW_HIP(e, hipSetDevice(e->device));
    tw_status r;
    if (!c->launched && (r = flush_ctx(e, *c))) {
        drop_batch(*c);
        return r;
    }
    hipError_t herr = hipEventSynchronize(c->ev_done);
    if ((c->any_host || c->any_init_host) && c->pending == (int)c->jobs.size()) {
        // Once per batch the host synchronises the copy stream.  Nothing else ever waits on it from the host (the
        // compute stream does, through ev_h2d), and this runtime releases a stream's per-command bookkeeping only on
        // a host-side hipStreamSynchronize: without it the process grew by ~1 KB per uploaded image (found by a
        // 300 000-pair soak; an event wait or a stream query does not release it).  The uploads it waits for are this
        // batch's (long done) and, at most, the next batch's, which that batch needs before it can start anyway.
        // Round 4: a caller that keeps two batches in flight has the NEXT batches' uploads (and their scanline
        // reconstruction) queued there — 4-6 ms of waiting per batch for nothing.  So: synchronise when the stream is
        // idle anyway (free), and otherwise only every 16th batch (the bookkeeping stays bounded at ~1 MB).
        // (the engine counts what it queues there itself: a hipStreamQuery per batch leaves bookkeeping of its own behind)
        if (e->copy_ops == c->copy_ops_at_flush || ++e->copy_sync_skipped >= 16) {
            (void)hipStreamSynchronize(e->copy_stream);
            e->copy_sync_skipped = 0;
        }
    }
    if (herr == hipSuccess && c->any_fout_host) {
        // the batch's flow fields on their way to host memory (the compute stream never waits for these copies)
        herr = hipEventSynchronize(c->ev_d2h);
        // as for the copy stream above: a host-side synchronise of the stream releases its bookkeeping — free when no later
        // batch has queued copies behind this one's, otherwise every 16th batch
        if (herr == hipSuccess && c->pending == (int)c->jobs.size() &&
            (e->d2h_ops == c->d2h_ops_at_flush || ++e->d2h_sync_skipped >= 16)) {
            herr = hipStreamSynchronize(e->d2h_stream);
            e->d2h_sync_skipped = 0;
        }
    }
    c->jobs[j].waited = true;
    c->pending--;
    if (c->pending == 0) c->release_images();  // (the batch is collected: ev_done has passed)
    if (herr != hipSuccess) {
        e->err = std::string("hipEventSynchronize: ") + hipGetErrorString(herr);
        return TW_E_DEVICE;
    }
    TW_TRY(pair_error(e, c, j));
    if (seconds) {
        // device compute time of the batch, shared equally by its pairs (exact for a batch of one)
        float ms = 0.f;
        TW_HIP(e, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
        *seconds = ms * 1e-3f / (float)c->jobs.size();
    }
    if (c->span > 0 && !c->jobs[j].ign.empty()) {
        // a pair with ignore rectangles: a vector whose grid point lies inside one of them is not reported.  All of the
        // pair's records are read and filtered in order; *n counts what is left (with out == NULL as well)
        const int cnt = c->h_count[j];
        const ScanRec* hr = nullptr;
        std::vector<ScanRec> extra;
        TW_TRY(pair_records<ScanRec>(e, c, j, c->h_rec, c->d_rec, cnt, extra, &hr));
        const int kept = outside_rects(c->jobs[j].ign, hr, cnt, [&](const ScanRec& r, int k) {
            if (out && k < cap) out[k] = to_tw_vector(r);
        });
        if (n) *n = kept;
        if (ro) TW_TRY(collect_regions(e, c, j, kept, cap, *ro));
    } else if (c->span > 0) {
        const int cnt = c->h_count[j];
        if (n) *n = cnt;
        const int want = out ? std::min(cnt, cap) : 0;
        const ScanRec* hr = nullptr;
        std::vector<ScanRec> extra;
        TW_TRY(pair_records<ScanRec>(e, c, j, c->h_rec, c->d_rec, want, extra, &hr));
        for (int i = 0; i < want; i++) out[i] = to_tw_vector(hr[i]);
        if (ro) TW_TRY(collect_regions(e, c, j, cnt, cap, *ro));
    } else {
        if (n) *n = 0;
        if (ro) TW_TRY(collect_regions(e, c, j, 0, cap, *ro));
    }
    return TW_OK;
}
}  // namespace

tw_status tw_wait(tw_engine* e, tw_ticket ticket, tw_vector* out, int cap, int* n, float* seconds)
{
    return wait_ticket(e, ticket, out, cap, n, seconds, nullptr);
}

tw_status tw_wait_regions(tw_engine* e, tw_ticket ticket, tw_vector* out, int cap, int* n, int* region_of, tw_region* regions,
                          int region_cap, int* n_regions, float* seconds)
{
    const RegionsOut ro = {region_of, regions, region_cap, n_regions};
    return wait_ticket(e, ticket, out, cap, n, seconds, &ro);
}

tw_status tw_ticket_changes(tw_engine* e, tw_ticket ticket, tw_change* changes, int change_cap, int* n_changes)
{
    if (!e) return TW_E_BAD_PARAMETER;
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j, &Ctx::residual,
                       "tw_ticket_changes: the ticket's batch was opened with TW_OPT_RESIDUAL off"));
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(ticket_finished(e, c, j));
    if (c->span <= 0) {
        if (n_changes) *n_changes = 0;
        return TW_OK;
    }
    const int cnt = c->h_nchg[j];
    const std::vector<tw_rect>& ign = c->jobs[j].ign;
    // all of the pair's records when rectangles filter them, else what the caller takes
    const int want = ign.empty() ? std::max(0, std::min(cnt, changes ? change_cap : 0)) : cnt;
    const ChangeRec* hr = nullptr;
    std::vector<ChangeRec> extra;
    TW_TRY(pair_records<ChangeRec>(e, c, j, c->h_chg, c->d_chg, want, extra, &hr));
    int kept = cnt;
    if (ign.empty()) {
        if (want > 0) memcpy(changes, hr, sizeof(tw_change) * (size_t)want);
    } else {
        kept = outside_rects(ign, hr, cnt, [&](const ChangeRec& r, int k) {
            if (changes && k < change_cap) memcpy(changes + k, &r, sizeof(tw_change));
        });
    }
    if (n_changes) *n_changes = kept;
    return TW_OK;
}

tw_status tw_ticket_shift(tw_engine* e, tw_ticket ticket, tw_shift* out)
{
    if (!e) return TW_E_BAD_PARAMETER;
    if (!out) {
        e->err = "tw_ticket_shift: null out";
        return TW_E_BAD_PARAMETER;
    }
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j, &Ctx::shift, "tw_ticket_shift: the ticket's batch was opened with TW_OPT_SHIFT off"));
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(ticket_finished(e, c, j));
    to_tw_shift(c->h_shift[j], out);
    return TW_OK;
}

tw_status tw_ticket_shift_bands(tw_engine* e, tw_ticket ticket, tw_shift_band* out, int cap, int* n)
{
    if (!e) return TW_E_BAD_PARAMETER;
    if (!n || cap < 0 || (!out && cap > 0)) {
        e->err = "tw_ticket_shift_bands: null n, or null out with cap > 0";
        return TW_E_BAD_PARAMETER;
    }
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j, &Ctx::bands,
                       "tw_ticket_shift_bands: the ticket's batch was opened without TW_OPT_SHIFT_BANDS and TW_OPT_SHIFT on"));
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(ticket_finished(e, c, j));
    const int nb = c->nbands();
    if (std::min(nb, cap) > 0) memcpy(out, c->h_bands + (size_t)j * nb, sizeof(BandRec) * (size_t)std::min(nb, cap));
    *n = nb;
    return TW_OK;
}

namespace {
// ---- diff image (tw_ticket_overlay, tw_stage_overlay) ---------------------------------------------------------------
// How tw_overlay_base runs: a pure function of the addresses, the strides and the size (tw_debug_overlay_plan shows it).
struct OverlayChoice {
    int vec;  // 1: dword loads and stores; 0: the byte path
    int px, threads, gx, gy;
};
OverlayChoice choose_overlay(uintptr_t E, uintptr_t T, long long stride, uintptr_t dst, long long pitch, int w, int h)
{
    OverlayChoice c;
    c.vec = (E % 4 == 0 && T % 4 == 0 && dst % 4 == 0 && stride % 4 == 0 && pitch % 4 == 0) ? 1 : 0;
    c.px = OVL_PX;
    c.threads = 64 * OVL_ROWS;
    c.gx = (w + 64 * OVL_PX - 1) / (64 * OVL_PX);
    c.gy = (h + OVL_ROWS - 1) / OVL_ROWS;
    return c;
}
static_assert(OVL_RECTS == TW_MAX_IGNORE && OVL_MAX_LEN == TW_OVERLAY_MAX_LEN, "the kernel's limits are the header's");
static_assert(sizeof(tw_overlay_hit) == sizeof(ScanRec) && offsetof(tw_overlay_hit, dx) == offsetof(ScanRec, dx),
              "tw_overlay_hit is the scan's record");

// one picture: everything device memory, the rectangles clipped (clip_ignore)
struct OverlayJob {
    const uint8_t *E, *T;
    long long stride;
    uint8_t* dst;
    long long pitch;
    int w, h, tol;
    const std::vector<tw_rect>* rects;
    const RegionRec* d_regions;
    int n_regions;
    const ScanRec* d_hits;
    int n_hits;
};
// The launches of one picture on `st`, in the order that is the layers' priority: the base, the boxes when there are any,
// the vectors when there are any.  Returns the base kernel's path (OverlayChoice::vec).
int launch_overlay(tw_engine* e, hipStream_t st, const OverlayJob& j)
{
    OverlayRects rc;
    rc.n = (int)std::min<size_t>(j.rects->size(), OVL_RECTS);
    for (int i = 0; i < rc.n; i++) {
        const tw_rect& r = (*j.rects)[i];
        rc.r[i] = make_int4(r.x, r.y, r.width, r.height);
    }
    const OverlayChoice ch = choose_overlay((uintptr_t)j.E, (uintptr_t)j.T, j.stride, (uintptr_t)j.dst, j.pitch, j.w, j.h);
    OverlayBaseArgs b;
    b.E = j.E;
    b.T = j.T;
    b.stride = j.stride;
    b.dst = j.dst;
    b.pitch = j.pitch;
    b.w = j.w;
    b.h = j.h;
    b.tol = j.tol;
    b.rc = rc;
    const dim3 grid(ch.gx, ch.gy, 1);
    if (ch.vec) TW_LAUNCH(e, TW_DF_OVERLAY_BASE, tw_overlay_base<true>, grid, dim3(ch.threads), 0, st, b);
    else TW_LAUNCH(e, TW_DF_OVERLAY_BASE, tw_overlay_base<false>, grid, dim3(ch.threads), 0, st, b);
    OverlayMarksArgs m;
    m.dst = j.dst;
    m.pitch = j.pitch;
    m.w = j.w;
    m.h = j.h;
    m.regions = j.d_regions;
    m.n_regions = j.n_regions;
    m.hits = j.d_hits;
    m.n_hits = j.n_hits;
    m.rc = rc;
    if (j.n_regions > 0) {
        // a box has at most 2 (w + h) outline pixels; eight workgroups stride the largest
        const int gx = std::max(1, std::min(8, (2 * (j.w + j.h) + 255) / 256));
        TW_LAUNCH(e, TW_DF_OVERLAY_MARKS, tw_overlay_marks<0>, dim3(gx, j.n_regions, 1), dim3(256), 0, st, m);
    }
    if (j.n_hits > 0)
        TW_LAUNCH(e, TW_DF_OVERLAY_MARKS, tw_overlay_marks<1>, dim3((j.n_hits + OVL_HITS_PER_WG - 1) / OVL_HITS_PER_WG, 1, 1),
                  dim3(64 * OVL_HITS_PER_WG), 0, st, m);
    return ch.vec;
}

// A picture's destination, checked before anything is launched as check_flow_field checks a flow field.  *kind = 0: device
// memory of this engine's device that holds the whole image; 1: a page-locked host block the library knows; 2: any other
// host memory.
tw_status check_overlay_out(tw_engine* e, const void* data, ptrdiff_t pitch, int w, int h, int* kind)
{
    const size_t row = 3 * (size_t)w;
    if (!data || pitch < (ptrdiff_t)row) {
        e->err = "bad diff image destination (null data, or a pitch below 3 * width)";
        return TW_E_BAD_PARAMETER;
    }
    const size_t extent = (size_t)pitch * (size_t)(h - 1) + row;
    if (pin_registry().covers(data, extent)) {
        *kind = 1;
        return TW_OK;
    }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, data) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        *kind = 2;
        return TW_OK;
    }
    if (at.device != e->device) {
        e->err = "diff image destination is memory of another device";
        return TW_E_BAD_PARAMETER;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(data)) != hipSuccess ||
        (uintptr_t)data + extent > (uintptr_t)base + size) {
        (void)hipGetLastError();
        e->err = "diff image destination does not hold the whole image";
        return TW_E_BAD_PARAMETER;
    }
    *kind = 0;
    return TW_OK;
}
}  // namespace

tw_status tw_ticket_hits(tw_engine* e, tw_ticket ticket, int* n)
{
    if (!e || !n) return TW_E_BAD_PARAMETER;
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j));
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(ticket_finished(e, c, j));
    if (c->span <= 0) {
        *n = 0;
        return TW_OK;
    }
    const int cnt = c->h_count[j];
    const std::vector<tw_rect>& ign = c->jobs[j].ign;
    if (ign.empty()) {
        *n = cnt;
        return TW_OK;
    }
    // as tw_wait counts a pair with rectangles: over all of its records
    const ScanRec* hr = nullptr;
    std::vector<ScanRec> extra;
    TW_TRY(pair_records<ScanRec>(e, c, j, c->h_rec, c->d_rec, cnt, extra, &hr));
    *n = outside_rects(ign, hr, cnt, [](const ScanRec&, int) {});
    return TW_OK;
}

tw_status tw_ticket_overlay(tw_engine* e, tw_ticket ticket, int tol, const tw_overlay_out* out)
{
    if (!e) return TW_E_BAD_PARAMETER;
    if (!out || !out->data || out->format != TW_OVERLAY_RGB8 || tol < 0 || tol > 255) {
        e->err = "tw_ticket_overlay: a null destination, an unknown format, or tol outside 0 .. 255";
        return TW_E_BAD_PARAMETER;
    }
    int j = 0;
    Ctx* c = nullptr;
    TW_TRY(find_ticket(e, ticket, &c, &j));
    TW_HIP(e, hipSetDevice(e->device));
    const int w = c->w, h = c->h;
    int kind = 0;
    TW_TRY(check_overlay_out(e, out->data, out->pitch, w, h, &kind));
    TW_TRY(ticket_finished(e, c, j));
    // The batch is over and its context is not reused before the ticket is collected: the pair's images are where the batch
    // read them — a host pair's slots of d_img (a resident expected image in its block), a device pair's own memory (a
    // reconciled device target in its d_img slot) — and all its hit records in the context's plane.
    const Job& jb = c->jobs[j];
    const bool host = jb.h_b != nullptr;
    const size_t npx = staged_image_bytes(w, h);
    OverlayJob oj;
    oj.E = host ? (jb.res ? jb.res->d : c->d_img + npx * (size_t)(2 * j)) : jb.d_a;
    oj.T = host ? c->d_img + npx * (size_t)(2 * j + 1) : jb.d_b;
    oj.stride = host ? (long long)w : jb.stride;
    oj.w = w;
    oj.h = h;
    oj.tol = tol;
    oj.rects = &jb.ign;
    oj.n_hits = c->span > 0 ? c->h_count[j] : 0;
    oj.d_hits = oj.n_hits > 0 ? c->d_rec + (size_t)j * (size_t)tw_grid_capacity(w, h, c->span) : nullptr;
    oj.n_regions = (c->regions && c->span > 0) ? std::max(0, std::min(c->h_nreg[j], (int)TW_MAX_REGIONS)) : 0;
    oj.d_regions = oj.n_regions > 0 ? c->d_regs + (size_t)j * TW_MAX_REGIONS : nullptr;
    // on the device-to-host stream: the compute stream may hold later batches' kernels, and the process has no queue to spare
    // for a further stream
    if (!e->d2h_stream) TW_HIP(e, hipStreamCreateWithFlags(&e->d2h_stream.h, hipStreamNonBlocking));
    hipStream_t st = e->d2h_stream;
    const size_t row = 3 * (size_t)w, spitch = (row + 3) / 4 * 4;
    if (kind == 0) {
        oj.dst = (uint8_t*)out->data;
        oj.pitch = out->pitch;
    } else {
        const size_t need = spitch * (size_t)h;
        TW_TRY(e->d_ovl.grow(e, need, need + 256, st));
        oj.dst = e->d_ovl;
        oj.pitch = (long long)spitch;
    }
    (void)launch_overlay(e, st, oj);
    TW_HIP(e, hipGetLastError());
    if (kind == 1) {
        TW_HIP(e, hipMemcpy2DAsync(out->data, (size_t)out->pitch, e->d_ovl, spitch, row, (size_t)h, hipMemcpyDeviceToHost, st));
    } else if (kind == 2) {
        // pageable: whole staging rows come down into the bounce buffer, the CPU copies each row's 3 w bytes out
        const size_t per = std::max<size_t>(1, BOUNCE_CHUNK / spitch);
        TW_TRY(bounce_reserve(e, std::min((size_t)h, per) * spitch));
        for (size_t r0 = 0; r0 < (size_t)h; r0 += per) {
            const size_t nr = std::min(per, (size_t)h - r0);
            TW_HIP(e, hipMemcpyAsync(e->h_bounce, e->d_ovl + r0 * spitch, nr * spitch, hipMemcpyDeviceToHost, st));
            TW_HIP(e, hipStreamSynchronize(st));
            for (size_t y = 0; y < nr; y++)
                memcpy((uint8_t*)out->data + (r0 + y) * (size_t)out->pitch, e->h_bounce + y * spitch, row);
        }
    }
    // the call is synchronous; and a host-side synchronise is what releases the stream's per-command bookkeeping (wait_ticket)
    TW_HIP(e, hipStreamSynchronize(st));
    return TW_OK;
}

tw_status tw_diff_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                     ptrdiff_t stride, int span, double threshold, tw_vector* out, int cap, int* n, float* seconds)
{
    if (span < 1) return TW_E_BAD_PARAMETER;
    tw_ticket t;
    tw_status r = tw_submit_u8(e, expect, target, width, height, stride, span, threshold, &t);
    if (r) return r;
    return tw_wait(e, t, out, cap, n, seconds);
}

tw_status tw_flow_u8(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height,
                     ptrdiff_t stride, float* flowx, float* flowy, float* seconds)
{
    if (!e) return TW_E_BAD_PARAMETER;
    // the dense flow of a pair lives in the level-0 chunk buffer: run this pair as a batch of its own
    tw_status r = tw_flush(e);
    if (r) return r;
    tw_ticket t;
    r = tw_submit_u8(e, expect, target, width, height, stride, 0, 0.0, &t);
    if (r) return r;
    r = tw_wait(e, t, nullptr, 0, nullptr, seconds);
    if (r) return r;
    Plan* pl = nullptr;
    if ((r = get_plan(e, width, height, &pl))) return r;
    const LevelPlan& L0 = pl->lv[0];
    const float* f = e->flow[0];
    // on the engine's own stream, then one host-side synchronise of it (copies on the null stream are never
    // followed by one, and this runtime keeps a little bookkeeping per command until a stream is synchronised)
    // The planes come down into the engine's own page-locked bounce buffer and are copied out by the CPU, unless the
    // caller's planes are page-locked blocks the library knows (tw_host_alloc / tw_host_register): the runtime is never
    // handed a pageable pointer it would have to page-lock on the fly (round 4: a fault on a malloc-heap address inside
    // this call, after an earlier hipHostRegister / hipHostUnregister of a neighbouring heap block).
    const size_t plane = (size_t)width * height * 4;
    float* dst[2] = {flowx, flowy};
    float* via[2] = {flowx, flowy};
    size_t need = 0;
    for (int q = 0; q < 2; q++)
        if (dst[q] && !pin_registry().covers(dst[q], plane)) need += plane;
    if ((r = bounce_reserve(e, need))) return r;
    size_t off = 0;
    for (int q = 0; q < 2; q++) {
        if (!dst[q]) continue;
        if (!pin_registry().covers(dst[q], plane)) {
            via[q] = (float*)(e->h_bounce + off);
            off += plane;
        }
        TW_HIP(e, hipMemcpy2DAsync(via[q], (size_t)width * 4, f + (q ? L0.ps : 0), (size_t)L0.ld * 4, (size_t)width * 4,
                                   height, hipMemcpyDeviceToHost, e->stream));
    }
    TW_HIP(e, hipStreamSynchronize(e->stream));
    for (int q = 0; q < 2; q++)
        if (dst[q] && via[q] != dst[q]) memcpy(dst[q], via[q], plane);
    return TW_OK;
}

tw_status tw_dev_alloc(tw_engine* e, size_t bytes, void** dptr)
{
    if (!e || !dptr) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipMalloc(dptr, bytes));
    return TW_OK;
}
tw_status tw_dev_free(tw_engine* e, void* dptr)
{
    if (!e) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipFree(dptr));
    return TW_OK;
}
tw_status tw_dev_upload(tw_engine* e, void* dptr, const void* host, size_t bytes)
{
    if (!e || !dptr || !host) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(h2d_sync(e, dptr, host, bytes));
    return TW_OK;
}
tw_status tw_dev_download(tw_engine* e, void* host, const void* dptr, size_t bytes)
{
    if (!e || !dptr || !host) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_TRY(d2h_sync(e, host, dptr, bytes));
    return TW_OK;
}

tw_status tw_set_option(tw_engine* e, int option, int value)
{
    if (!e) return TW_E_BAD_PARAMETER;
    switch (option) {
        case TW_OPT_SCAN_FUSED_FINAL: e->opt.scan_fused = value ? 1 : 0; return TW_OK;
        case TW_OPT_POLYEXP_F32: e->opt.poly_f32 = value == 2 ? 2 : (value ? 1 : 0); return TW_OK;
        case TW_OPT_REGIONS:
            if (value < 0 || value > 8) {
                e->err = "TW_OPT_REGIONS: 0 (off) or a gap of 1 .. 8";
                return TW_E_BAD_PARAMETER;
            }
            e->opt.regions_gap = value;
            return TW_OK;
        case TW_OPT_RESIDUAL:
            if (value < 0 || value > 254) {
                e->err = "TW_OPT_RESIDUAL: 0 (off) or a tolerance of 1 .. 254";
                return TW_E_BAD_PARAMETER;
            }
            e->opt.residual_tol = value;
            return TW_OK;
        case TW_OPT_SHIFT:
            if (value < 0 || value > 1024) {
                e->err = "TW_OPT_SHIFT: 0 (off) or a search radius of 1 .. 1024";
                return TW_E_BAD_PARAMETER;
            }
            e->opt.shift_radius = value;
            return TW_OK;
        case TW_OPT_SHIFT_BANDS:
            if (value != 0 && (value < 32 || value > 1024 || value % 16 != 0)) {
                e->err = "TW_OPT_SHIFT_BANDS: 0 (off) or a band height of 32 .. 1024 rows, a multiple of 16";
                return TW_E_BAD_PARAMETER;
            }
            e->opt.shift_bands = value;
            return TW_OK;
        default: e->err = "unknown option"; return TW_E_BAD_PARAMETER;
    }
}

tw_status tw_host_alloc(tw_engine* e, size_t bytes, void** hptr)
{
    if (!e || !hptr) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipHostMalloc(hptr, bytes, hipHostMallocPortable));  // usable by the engines of every device (one queue, N consumers)
    pin_registry().add(*hptr, bytes, PinRegistry::ALLOC);
    return TW_OK;
}
tw_status tw_host_free(tw_engine* e, void* hptr)
{
    if (!e) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipStreamSynchronize(e->copy_stream));  // an upload of THIS engine may still be reading it (see twflow.h)
    if (const int why = pin_registry().remove(hptr, PinRegistry::ALLOC)) {
        e->err = why == 2 ? "tw_host_free: the block was registered (tw_host_register): release it with tw_host_unregister"
                          : "tw_host_free: not a tw_host_alloc block";
        return TW_E_BAD_PARAMETER;
    }
    TW_HIP(e, hipHostFree(hptr));
    return TW_OK;
}
tw_status tw_host_register(tw_engine* e, void* hptr, size_t bytes)
{
    if (!e || !hptr || !bytes) return TW_E_BAD_PARAMETER;
    // Whole pages only, and only pages the caller owns outright: a range that starts or ends inside a page shares
    // that page with whatever else the allocator placed there, and page-locking / releasing it behind the runtime's
    // back is what round 4's GPU fault traced to (a pageable copy of a NEIGHBOURING heap block right after such a
    // block's hipHostUnregister).  malloc / new / cv::Mat heap blocks are refused: take the memory from
    // tw_host_alloc, or from an allocation of your own that is page-aligned and a page multiple (mmap,
    // aligned_alloc(page, n * page), posix_memalign).
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    if (((uintptr_t)hptr % page) != 0 || (bytes % page) != 0) {
        e->err = "tw_host_register: the range must start on a page boundary and be a whole number of pages (" +
                 std::to_string(page) + " bytes): register memory you own page-wise (mmap / aligned_alloc) or use tw_host_alloc";
        return TW_E_BAD_PARAMETER;
    }
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipHostRegister(hptr, bytes, hipHostRegisterPortable));
    pin_registry().add(hptr, bytes, PinRegistry::REGISTERED);
    return TW_OK;
}
tw_status tw_host_unregister(tw_engine* e, void* hptr)
{
    if (!e || !hptr) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipStreamSynchronize(e->copy_stream));
    if (const int why = pin_registry().remove(hptr, PinRegistry::REGISTERED)) {
        e->err = why == 2 ? "tw_host_unregister: the block came from tw_host_alloc: release it with tw_host_free"
                          : "tw_host_unregister: not a registered block";
        return TW_E_BAD_PARAMETER;
    }
    TW_HIP(e, hipHostUnregister(hptr));
    return TW_OK;
}

// ---- instrumentation ---------------------------------------------------------------------------------
tw_status tw_prof_select(tw_engine* e, int kclass, int level)
{
    if (!e || kclass >= TW_K_COUNT) return TW_E_BAD_PARAMETER;
    if (kclass < 0) {
        for (int i = 0; i < TW_K_COUNT; i++) e->prof_level[i] = -2;
        return TW_OK;
    }
    e->prof_level[kclass] = level < -1 ? -2 : level;
    return TW_OK;
}

tw_status tw_prof_read(tw_engine* e, int kclass, double* ms_total, int* launches)
{
    if (!e || kclass < 0 || kclass >= TW_K_COUNT) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    TW_HIP(e, hipDeviceSynchronize());
    double tot = 0;
    int cnt = 0;
    for (ProfPair& pp : e->prof_pending[kclass]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pp.a, pp.b) == hipSuccess) {
            tot += ms;
            cnt++;
        }
        e->prof_free.push_back(std::move(pp.a));
        e->prof_free.push_back(std::move(pp.b));
    }
    e->prof_pending[kclass].clear();
    if (ms_total) *ms_total = tot;
    if (launches) *launches = cnt;
    return TW_OK;
}

int tw_num_levels(const tw_engine* e, int width, int height)
{
    if (!e) return -1;
    return plan_levels(width, height, e->cfg.p.pyrScale, std::min(std::max(e->cfg.p.pyrLevels, 0), TW_MAX_LEVELS));
}

int tw_level_chunk(tw_engine* e, int width, int height, int level)
{
    if (!e) return -1;
    Plan scratch;
    const Plan* g = plan_geometry_of(e, width, height, &scratch);
    return g && level >= 0 && level <= g->levels ? g->lv[level].chunk : -1;
}

int tw_level_runs_flow_iter(const tw_engine* e, int width, int height, int level, int npairs)
{
    if (!e || npairs < 1) return -1;
    Plan scratch;
    LevelSchedule s;
    const Plan* g = level_schedule_view(e, width, height, npairs, &scratch, &s);
    if (!g || level < 0 || level > g->levels) return -1;
    return s.lv[level].full.flow_iter ? 1 : 0;
}

double tw_algorithmic_bytes(const tw_engine* e, int kclass, int level, int width, int height)
{
    return e ? tw_algorithmic_bytes_launch(e, kclass, level, width, height, e->cfg.cap) : 0;
}

double tw_algorithmic_bytes_launch(const tw_engine* e, int kclass, int level, int width, int height, int npairs)
{
    if (!e || npairs < 1) return 0;
    Plan scratch;
    LevelSchedule s;
    const Plan* g = level_schedule_view(e, width, height, npairs, &scratch, &s);
    if (!g || level < 0 || level > g->levels) return 0;
    const int L = g->levels;
    const double N = (double)g->lv[level].w * g->lv[level].h, N0 = (double)width * height;
    const double Nprev = level < L ? (double)g->lv[level + 1].w * g->lv[level + 1].h : 0;  // the coarser level's pixels
    const int it = e->cfg.p.pyrIterations;
    // as built, read off the schedule's own choice (choose_level_schedule): levels that run tw_flow_iter have no
    // FarnebackUpdateMatrices launch and no M planes (flow 8N + R0 20N + R1 20N in, flow 8N out = 56N per iteration; the first
    // one reads the coarser level's flow, 8 N_{k+1}, instead of this level's); a level whose images the coarser level's launch
    // wrote (tw_pyr_23, tw_pyr_k3f) reads no source image.  A single pair, a small batch or a narrow level keeps
    // tw_update_matrices + tw_blur_solve*.
    const bool mfree = s.lv[level].full.flow_iter;
    switch (kclass) {
        case TW_K_PYR:
            if (s.lv[level].images == IMG_FROM_COARSER) return 2 * (4 * N);  // written by the coarser level's launch
            return 2 * (N0 + 4 * N);
        case TW_K_POLYEXP: return 48 * N;  // 2 images x (4 + 20) B/px
        case TW_K_UPDATE_MATRICES:
            if (mfree) return 0;
            // R0 20N + R1 20N read, M 20N written; the level's initial flow is read from the coarser level (8 N_{k+1})
            // and is only stored when no iteration follows (the first blur launch recomputes nothing from it: the
            // refresh of iteration 0 uses M, and the flow itself is rewritten by the first solve)
            return 60 * N + ((it == 0 ? 8 * N : 0) + 8 * Nprev);
        case TW_K_BLUR_SOLVE:
            // average over the `it` launches of a level.  The last one reads M (20N) and writes the flow (8N).  The
            // others are fused with the FarnebackUpdateMatrices refresh: M 20N + R0 20N + R1 20N read, M 20N
            // written = 80N — the flow they compute stays in registers and is never stored (counting
            // 28N + 68N charged 16N the kernel does not move).
            if (mfree) return (48 * N + 8 * Nprev + (it - 1) * 56 * N) / it;
            return it > 0 ? (28 * N + (it - 1) * 80 * N) / it : 0;
        default: return 0;
    }
}

// SURVEY.md 8(d) model of one pair (every named stage of the reference reads each input once and writes each output
// once: pyr 2(N0+4N), polyexp 48N, updateMatrices 68N and blur+solve 28N per iteration, flow init): the
// figure BASELINE.md prices the pair against (991.8 MB at 1080p with the default parameters).
double tw_algorithmic_bytes_pair(const tw_engine* e, int width, int height, int span)
{
    if (!e) return 0;
    const int L = tw_num_levels(e, width, height);
    const int it = e->cfg.p.pyrIterations;
    double tot = 0;
    for (int k = 0; k <= L; k++) {
        int w, h, ks;
        double sg, sc;
        level_geometry(width, height, e->cfg.p.pyrScale, k, &w, &h, &sg, &ks, &sc);
        const double N = (double)w * h, N0 = (double)width * height;
        double up = 8 * N;  // memset at the coarsest level
        if (k < L) {
            int pw, ph;
            level_geometry(width, height, e->cfg.p.pyrScale, k + 1, &pw, &ph, &sg, &ks, &sc);
            up = 8.0 * pw * ph + 8 * N;
        }
        tot += 2 * (N0 + 4 * N) + 48 * N + up + it * (68 + 28) * N;
    }
    if (span > 0) tot += 16.0 * tw_grid_capacity(width, height, span);
    return tot;
}

// What the kernels as built must move for one pair (fusion removed the flow stores between iterations): the sum of
// tw_algorithmic_bytes over all launches.  Reported beside the SURVEY figure; smaller than it.
double tw_min_traffic_bytes_pair(const tw_engine* e, int width, int height, int span)
{
    if (!e) return 0;
    const int L = tw_num_levels(e, width, height);
    const int it = e->cfg.p.pyrIterations;
    double tot = 0;
    for (int k = 0; k <= L; k++) {
        tot += tw_algorithmic_bytes(e, TW_K_PYR, k, width, height);
        tot += tw_algorithmic_bytes(e, TW_K_POLYEXP, k, width, height);
        tot += tw_algorithmic_bytes(e, TW_K_UPDATE_MATRICES, k, width, height);
        tot += it * tw_algorithmic_bytes(e, TW_K_BLUR_SOLVE, k, width, height);
    }
    if (span > 0) tot += 16.0 * tw_grid_capacity(width, height, span);
    return tot;
}

}  // extern "C"

// diagnostic: the phase stamps of the last tw_pyr_taps launch (TW_DEBUG_STAMPS=1), 64 workgroups x 4 stamps
extern "C" int tw_debug_stamps(tw_engine* e, unsigned long long* out)
{
    if (!e || !e->dbg_stamps || !out) return 0;
    if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
    return d2h_sync(e, out, e->dbg_stamps, 64 * 4 * sizeof(unsigned long long)) == TW_OK ? 256 : 0;
}

// the first n (<= 4096) stamps of the debug buffer: tw_flow_iter's phase stamps (variants library, TW_DEBUG_STAMPS=1):
// [workgroup 0..31][wave 0 / 9][step 40..47][stamp 0..7]
extern "C" int tw_debug_stamps_ex(tw_engine* e, unsigned long long* out, int n)
{
    if (!e || !e->dbg_stamps || !out || n < 1 || n > 4096) return 0;
    if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
    return d2h_sync(e, out, e->dbg_stamps, (size_t)n * sizeof(unsigned long long)) == TW_OK ? n : 0;
}

// number of captured single-pair schedules this engine holds (tests: the graph path is really the one that ran)
extern "C" int tw_debug_graphs(tw_engine* e) { return e ? (int)e->lat_graphs.size() : -1; }

extern "C" tw_status tw_debug_check_size(int width, int height)
{
    const char* why = "";
    return size_status(width, height, &why);
}

extern "C" int tw_debug_flow_iter_plan(const tw_engine* e, int width, int height, int npairs, int* out, int n)
{
    if (!e) return -1;
    if (!out || width < 1 || height < 1 || npairs < 1) return 0;
    const FlowIterPlan fp = flow_iter_plan(e->cfg, width, height, npairs);
    const int v[4] = {fp.strips, fp.segments, fp.nt, fp.nt_last};
    int i = 0;
    for (; i < n && i < 4; i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_blur_plan(const tw_engine* e, int width, int height, int level, int npairs, int update, int quads, int* out, int n)
{
    if (!e) return -1;
    if (!out || width < 1 || height < 1 || npairs < 1) return 0;
    const BlurChoice c = choose_blur(e->cfg, width, height, npairs, level, update != 0, quads != 0);
    const int v[9] = {c.k->family, c.k->block, c.k->tw, c.k->th, c.xsh, (int)c.grid.x, (int)c.grid.y, c.small, c.forced ? 1 : 0};
    int i = 0;
    for (; i < n && i < 9; i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_pyr_plan(const tw_engine* e, int width, int height, int level, long long stride, int* out, int n)
{
    if (!e) return -1;
    if (!out || width < 1 || height < 1 || level < 0) return 0;
    Plan scratch;
    const Plan* g = plan_geometry_of(e, width, height, &scratch);
    if (!g || level > g->levels) return 0;
    const PyrChoice c = choose_pyr(e->cfg, g, level, stride, 1);  // (4-byte-aligned image addresses: include/twflow_debug.h)
    const LevelPlan& L = g->lv[level];
    // output rows whose lower source row yofs + 1 lies past the image and is clipped to h0 - 1 (the level's table, made anew:
    // the plan keeps it on the device only)
    int yclip = 0;
    if (L.mode == 1) {
        ResizeTab t;
        make_resize_tab(width, height, L.w, L.h, t);
        for (int y = 0; y < L.h; y++) yclip += t.yofs[y] + 1 > height - 1;
    }
    const int v[23] = {c.kernel, c.targ, c.kernel == PYR_KN_LEVEL_LDS ? (int)TW_DF_PYR_LEVEL_LDS : c.family, c.block, c.tw, c.th,
                       (int)c.gx, (int)c.gy, (int)c.lds, c.pitch, c.aligned4, L.w, L.h, L.ksize, L.mode, L.xmax, c.nrows_max,
                       g->fused23 ? 1 : 0, pyr01_fusable(g) ? 1 : 0, pyr23_threads(e->cfg, 2), pyr23_threads(e->cfg, 3), g->levels, yclip};
    int i = 0;
    for (; i < n && i < 23; i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_scan_plan(const tw_engine* e, int width, int height, int span, int npairs, int single_pair, int* out, int n)
{
    if (!e) return -1;
    if (!out || width < 1 || height < 1 || span < 1 || npairs < 1) return 0;
    const int gw = (width + span - 1) / span, gh = (height + span - 1) / span;
    const ScanChoice c = choose_scan(npairs, single_pair != 0, gw, gh, BatchSwitches().scan_seg);
    if (c.G > INT32_MAX) return 0;
    const int v[7] = {c.kernel, gw, gh, (int)c.G, c.S, c.segments, c.rounds};
    int i = 0;
    for (; i < n && i < 7; i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_level_plan(const tw_engine* e, int width, int height, int span, int npairs, int traits, int* out, int n)
{
    if (!e) return -1;
    if (!out || width < 1 || height < 1 || span < 0 || npairs < 1) return 0;
    Plan scratch;
    const Plan* gp = plan_geometry_of(e, width, height, &scratch);
    if (!gp) return 0;
    const Plan& g = *gp;
    const BatchTraits t = with_engine_state(
        e, BatchTraits{npairs, span, (traits & 1) != 0, (traits & 2) != 0, (traits & 4) != 0, !(traits & 8), (traits & 16) != 0});
    const BatchSwitches sw;  // (read at the call, as every batch reads them)
    const int parts = batch_lanes(e->cfg, npairs);
    std::vector<int> v;
    for (int part = 0; part < parts; part++) {
        const int npart = (int)((long long)npairs * (part + 1) / parts) - (int)((long long)npairs * part / parts);
        const LevelSchedule s = choose_level_schedule(e->cfg, g, sw, t, npart);
        if (part == 0) v = {s.kind, s.nlanes, s.levels, s.lat_quads, s.fused_final, s.grid_final, parts, 11};
        for (int k = 0; k <= s.levels; k++) {
            const LevelChoice& c = s.lv[k];
            v.insert(v.end(), {npart, c.per, c.launches, c.tail, c.images, c.init, c.full.flow_iter, c.full.same, c.last.flow_iter,
                               c.last.same, s.same01});
        }
    }
    int i = 0;
    for (; i < n && i < (int)v.size(); i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_launch_counts(tw_engine* e, unsigned long long* counts, unsigned long long* last_z, int n, int reset)
{
    if (!e) return -1;
    for (int i = 0; i < n && i < TW_DF_COUNT; i++) {
        if (counts) counts[i] = e->launches[i];
        if (last_z) last_z[i] = e->last_grid_z[i];
    }
    if (reset) {
        memset(e->launches, 0, sizeof(e->launches));
        memset(e->last_grid_z, 0, sizeof(e->last_grid_z));
    }
    return TW_DF_COUNT;
}

extern "C" int tw_debug_same_flags(tw_engine* e, unsigned* out, int n)
{
    if (!e) return -1;
    if (!out || n < 1) return 0;
    const int m = std::min(n, e->same_n);
    for (int i = 0; i < m; i++) out[i] = 0;
    if (m < 1 || !e->same_valid) return std::max(m, 0);
    // (both lanes' launches are joined into the main stream before the batch's scan)
    if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
        hipMemcpy(out, e->d_same, sizeof(unsigned) * m, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -2;  // (out holds zeros, none of them a flag)
    }
    return m;
}

extern "C" int tw_debug_shift_plan(int width, int height, int radius, int* out, int n)
{
    if (!out || width < 1 || height < 1 || radius < 1 || radius > 1024) return 0;
    const dim3 pg = shift_profiles_grid(width, height, 2);
    const int v[10] = {shift_axis_in_lds(width) ? 1 : 0, shift_axis_in_lds(height) ? 1 : 0, std::min(radius, width / 2),
                       std::min(radius, height / 2), 2, 1024, SS_LDS_BYTES, (int)pg.x, (int)pg.y, (height + SV_ROWS - 1) / SV_ROWS};
    const int m = std::max(0, std::min(n, 10));
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
}

extern "C" int tw_debug_band_plan(int width, int height, int radius, int band, int* out, int n)
{
    if (!out || width < 1 || height < 1 || radius < 1 || radius > 1024 || band < 32 || band > 1024 || band % 16 != 0) return 0;
    const int v[9] = {band_count(height, band),
                      band_blocks(width),
                      band_search_in_lds(width, height, radius, band) ? 1 : 0,
                      (int)std::min<size_t>(band_search_lds_bytes(width, height, radius, band), INT_MAX),
                      BS_LDS_BYTES,
                      std::min(radius, height / 2),
                      (int)(((size_t)height * band_blocks(width) + 255) / 256),
                      1024,
                      (height + BV_ROWS - 1) / BV_ROWS};
    const int m = std::max(0, std::min(n, 9));
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
}

extern "C" int tw_debug_overlay_plan(unsigned long long expect, unsigned long long target, long long stride,
                                     unsigned long long dst, long long pitch, int width, int height, int* out, int n)
{
    if (!out || width < 1 || height < 1) return 0;
    const OverlayChoice c = choose_overlay((uintptr_t)expect, (uintptr_t)target, stride, (uintptr_t)dst, pitch, width, height);
    const int v[5] = {c.vec, c.px, c.threads, c.gx, c.gy};
    const int m = std::max(0, std::min(n, 5));
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
}

extern "C" const char* tw_debug_family_name(int family)
{
    static const char* const names[TW_DF_COUNT] = {
        "tw_pyr_k3", "tw_pyr_k3f", "tw_pyr_23", "tw_pyr_taps", "tw_pyr_level", "tw_polyexp", "tw_update_matrices",
        "tw_flow_iter", "tw_flow_iter_ups", "tw_flow_iter_zero", "tw_blur_solve4", "tw_blur_solve4y", "tw_blur_solve8",
        "tw_blur_solve_pp", "tw_blur_solve_generic", "tw_blur_variant", "tw_blur_grid", "tw_box", "tw_twin",
        "tw_span_gather", "tw_span_scan", "tw_png_unfilter", "tw_span_scan_seg",
        "tw_band_rows", "tw_band_search", "tw_band_verify", "tw_flow_band_init", "tw_blur_solve4q",
        "tw_overlay_base", "tw_overlay_marks", "tw_pyr_level_lds",
        "tw_shift_profiles", "tw_shift_search", "tw_shift_verify", "tw_flow_shift_init", "tw_warp_residual", "tw_change_scan",
        "tw_flow_iter_grid",
        "tw_hit_regions", "tw_jpeg_idct", "tw_mask_rects", "tw_pair_same",
        "tw_resize_u8", "tw_flow_area_init", "tw_flow_export"};
    return (family >= 0 && family < TW_DF_COUNT) ? names[family] : nullptr;
}

extern "C" int tw_debug_memory(tw_engine* e, unsigned long long* out, int n)
{
    if (!e || !out) return -1;
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // device and pinned: what Buf::make / grow allocated for the engine and its contexts, each allocation with the slack it
    // was made with (the bounce buffer among the pinned), plus the totals of the plans' tables and of the resident store
    v[0] = e->dev_bytes;
    v[1] = e->pin_bytes;
    for (const auto& kv : e->plans) v[0] += kv.second->owned_bytes;
    v[0] += e->res_reserved;  // (the resident store's chunks: tw_debug_resident)
    v[2] = e->plans.size();
    v[3] = e->h_bounce.cap;
    {
        PinRegistry& r = pin_registry();
        std::lock_guard<std::mutex> lk(r.m);
        v[4] = r.ranges.size();
        for (const auto& kv : r.ranges) v[5] += kv.second.bytes;
    }
    v[6] = e->prof_free.size();
    for (int i = 0; i < TW_K_COUNT; i++) v[6] += 2 * e->prof_pending[i].size();
    v[7] = e->lat_graphs.size();
    int i = 0;
    for (; i < n && i < 8; i++) out[i] = v[i];
    return i;
}

extern "C" int tw_debug_resident(tw_engine* e, unsigned long long out[4])
{
    if (!e || !out) return -1;
    out[0] = e->res_images.size();
    out[1] = e->res_in_use;
    out[2] = e->res_reserved;
    out[3] = e->res_chunk_allocs;
    return 4;
}

// occupancy report of the main kernels (workgroups per CU the runtime admits) — tools/kbench.py
extern "C" int tw_debug_occupancy(char* buf, int cap)
{
    int n = 0, o = 0;
    auto add = [&](const char* name, const void* fn, int threads, size_t dyn_lds) {
        int blocks = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, dyn_lds);
        o = snprintf(buf + n, cap - n, "%s: %d workgroups/CU of %d threads\n", name, blocks, threads);
        if (o > 0) n += o;
    };
    add("tw_blur_solve4<15,256>", (const void*)tw_blur_solve4<15, 256, 16, 8, true>, 256, 0);
#ifdef TW_VARIANTS
    add("tw_blur_solve8<15,256>", (const void*)tw_blur_solve8<15, 256, 16, 8, true, true>, 256, 0);
    add("tw_blur_solve8<15,128>", (const void*)tw_blur_solve8<15, 128, 16, 8, true, true>, 128, 0);
    add("tw_polyexp<7>", (const void*)tw_polyexp<7>, 256, 0);
    add("tw_polyexp_pk<7,16>", (const void*)tw_polyexp_pk<7, 16>, 256, 0);
#endif
    add("tw_polyexp_pk<7,8>", (const void*)tw_polyexp_pk<7, 8>, 256, 0);
    add("tw_update_matrices<true,2>", (const void*)tw_update_matrices<true, 2>, 256, 0);
    add("tw_pyr_k3<0>", (const void*)tw_pyr_k3<0>, 256, 0);
    return n;
}

// ---- the yardstick: a plain float4 device copy (SURVEY 8d "measured device-copy peak taken in the same run") -----------
// ONE 16-byte load and one 16-byte store per lane, no loop, one workgroup per 4 KiB: the shape that reaches what
// MI355X_MICROARCH.md quotes for "float4 copy" (6.29 TB/s there; 6.19 TB/s on round 5's lease, against 4.9 for a
// grid-stride loop, 4.8 for hipMemcpyDtoD and 5.5 for round 4's torch copy_: tools/ubench/copy_rate.hip,
// profiles/r05_copy_rate.txt), so that bench.py's `frac_of_measured_copy` is comparable with the guide.
__global__ __launch_bounds__(256) void tw_copy_f4(const float4* __restrict__ src, float4* __restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
extern "C" tw_status tw_debug_copy_rate(tw_engine* e, size_t bytes, int reps, double* gbps)
{
    if (!e || !gbps || bytes < 4096 || reps < 1) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    Tmp t;
    float4* a = (float4*)t.alloc<uint8_t>(bytes);
    float4* b = (float4*)t.alloc<uint8_t>(bytes);
    if (!a || !b) return TW_E_NOMEM;
    hipStream_t st = e->stream;
    TW_HIP(e, hipMemsetAsync(a, 1, bytes, st));
    const size_t n = bytes / 16;
    if ((n + 255) / 256 > 0x7fffffffu) return TW_E_BAD_PARAMETER;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipEvent_t ea, eb;
    TW_HIP(e, hipEventCreate(&ea));
    TW_HIP(e, hipEventCreate(&eb));
    hipLaunchKernelGGL(tw_copy_f4, dim3(grid), dim3(256), 0, st, a, b, n);  // warm-up
    (void)hipEventRecord(ea, st);
    for (int i = 0; i < reps; i++) hipLaunchKernelGGL(tw_copy_f4, dim3(grid), dim3(256), 0, st, a, b, n);
    (void)hipEventRecord(eb, st);
    hipError_t err = hipStreamSynchronize(st);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, ea, eb);
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    TW_HIP(e, err);
    TW_HIP(e, hipGetLastError());
    *gbps = 2.0 * (double)(n * 16) * reps / (ms * 1e-3) / 1e9;  // read + write counted
    return TW_OK;
}

// ---- isolated kernel timing on synthetic device data (bench.py, tools/kbench.py) -------------------------
extern "C" tw_status tw_bench_stage(tw_engine* e, int kclass, int width, int height, int level, int npairs,
                                    int iters, int flags, float* avg_us)
{
    if (!e || !avg_us || npairs < 1 || iters < 1 || kclass < 0 || kclass >= TW_K_COUNT) return TW_E_BAD_PARAMETER;
    TW_HIP(e, hipSetDevice(e->device));
    Plan* pl = nullptr;
    tw_status r = get_plan(e, width, height, &pl);
    if (r) return r;
    if (level < 0 || level > pl->levels) return TW_E_BAD_PARAMETER;
    const LevelPlan& L = pl->lv[level];
    const size_t ps = (size_t)L.ps, npx0 = (size_t)width * height;
    const size_t pps = level < pl->levels ? (size_t)pl->lv[level + 1].ps : 1;
    Tmp t;
    float* I = t.alloc<float>(ps * 2 * npairs);
    float* R = t.alloc<float>(ps * 10 * npairs);
    float* M0 = t.alloc<float>(ps * 5 * npairs);
    float* M1 = t.alloc<float>(ps * 5 * npairs);
    float* fl = t.alloc<float>(ps * 2 * npairs);
    float* pf = t.alloc<float>(pps * 2 * npairs);
    uint8_t* img = t.alloc<uint8_t>(npx0 * 2 * npairs);
    const uint8_t** tab = t.alloc<const uint8_t*>(2 * (size_t)npairs);
    const int span = 10;
    const size_t G = (size_t)tw_grid_capacity(width, height, span);
    int* cnt = t.alloc<int>(npairs);
    ScanRec* rec = t.alloc<ScanRec>(G * npairs);
    float2* grid = t.alloc<float2>(G * npairs);
    if (!grid || !I || !R || !M0 || !M1 || !fl || !pf || !img || !tab || !cnt || !rec) return TW_E_NOMEM;
    {
        // deterministic pseudo-random fill (host LCG), smooth small flow
        std::vector<float> hb(ps * 10);
        uint32_t sd = 12345u;
        auto rnd = [&]() { sd = sd * 1664525u + 1013904223u; return (float)((sd >> 8) & 0xFFFF) / 65536.f - 0.5f; };
        for (float& v : hb) v = rnd() * 20.f;
        // M: G = identity, h = small smooth field -> the solved flow is (h2, h1)/(1+1e-3), a few pixels
        std::vector<float> hm(ps * 5);
        for (size_t i = 0; i < ps; i++) {
            hm[i] = 1.f;
            hm[ps + i] = 0.f;
            hm[2 * ps + i] = 1.f;
            hm[3 * ps + i] = 2.5f * sinf((float)(i % 1931) * 0.004f);
            hm[4 * ps + i] = 2.0f * cosf((float)(i % 2477) * 0.003f);
        }
        for (int j = 0; j < npairs; j++) {
            TW_TRY(h2d_sync(e, R + ps * 10 * j, hb.data(), ps * 10 * 4));
            TW_TRY(h2d_sync(e, M0 + ps * 5 * j, hm.data(), ps * 5 * 4));
            TW_TRY(h2d_sync(e, M1 + ps * 5 * j, hm.data(), ps * 5 * 4));
            TW_TRY(h2d_sync(e, I + ps * 2 * j, hb.data() + 17, ps * 2 * 4));
        }
        std::vector<float> hf(std::max(ps, pps) * 2);
        for (size_t i = 0; i < hf.size(); i++) hf[i] = 3.f * sinf((float)(i % 977) * 0.01f) + (flags & 1 ? rnd() * 8.f : 0.f);
        std::vector<uint8_t> hi(npx0);
        for (uint8_t& v : hi) v = (uint8_t)((rnd() + 0.5f) * 255.f);
        std::vector<const uint8_t*> ht(2 * (size_t)npairs);
        for (int j = 0; j < npairs; j++) {
            TW_TRY(h2d_sync(e, fl + ps * 2 * j, hf.data(), ps * 2 * 4));
            TW_TRY(h2d_sync(e, pf + pps * 2 * j, hf.data(), pps * 2 * 4));
            for (int q = 0; q < 2; q++) {
                TW_TRY(h2d_sync(e, img + npx0 * (2 * j + q), hi.data(), npx0));
                ht[2 * j + q] = img + npx0 * (2 * j + q);
            }
        }
        TW_TRY(h2d_sync(e, (void*)tab, ht.data(), sizeof(void*) * ht.size()));
    }
    hipStream_t st = e->stream;
    // profiling off while the stage is timed, and two events: both given back on every way out
    struct Borrowed {
        tw_engine* e;
        int saved[TW_K_COUNT];
        hipEvent_t ea = nullptr, eb = nullptr;
        explicit Borrowed(tw_engine* e_) : e(e_)
        {
            memcpy(saved, e->prof_level, sizeof(saved));
            for (int i = 0; i < TW_K_COUNT; i++) e->prof_level[i] = -2;
        }
        ~Borrowed()
        {
            memcpy(e->prof_level, saved, sizeof(saved));
            if (ea) (void)hipEventDestroy(ea);
            if (eb) (void)hipEventDestroy(eb);
        }
    } borrowed(e);
    hipEvent_t &ea = borrowed.ea, &eb = borrowed.eb;
    TW_HIP(e, hipEventCreate(&ea));
    TW_HIP(e, hipEventCreate(&eb));
    auto once = [&](int i) -> tw_status {
        switch (kclass) {
            case TW_K_PYR:
                launch_pyr(e, st, pl, level, tab, width, npx0 % 4 == 0, I, 2 * npairs);
                break;
            case TW_K_POLYEXP: return launch_polyexp(e, st, L.w, L.h, L.ld, L.ps, I, R, 2 * npairs, level);
            case TW_K_UPDATE_MATRICES: launch_update(e, st, pl, level, R, fl, pf, M0, npairs); break;
            case TW_K_BLUR_SOLVE:
                if (flags & 12) {
                    // flags 4: one M-free iteration (tw_flow_iter) from the synthetic flow field into the M1 workspace;
                    // flags 8: the same with the upsample of the coarser level's flow fused (first iteration of a level)
                    if (!flow_iter_eligible(e->cfg, L.w, L.h)) return TW_E_UNSUPPORTED;
                    FlowUps ups;
                    const bool up = (flags & 8) && level < pl->levels;
                    if (up) {
                        const LevelPlan& Pv = pl->lv[level + 1];
                        ups = FlowUps{pf, Pv.w, Pv.h, Pv.ld, Pv.ps, L.d_uxofs, L.d_uyofs, L.d_ualpha, L.d_ubeta, L.uxmax,
                                      (float)(1. / e->cfg.p.pyrScale)};
                    }
                    if ((flags & 20) == 20) {
                        // flags 4 + 16: the grid-only iteration (tw_flow_iter's MODE 3) at span 10, samples into the scan's grid
                        const FlowIterGrid gp{grid, span, (L.w + span - 1) / span, (L.h + span - 1) / span};
                        if (level != 0) return TW_E_UNSUPPORTED;
                        launch_flow_iter(e, st, L.w, L.h, L.ld, L.ps, R, fl, L.ps, nullptr, L.ps, nullptr, npairs, level, nullptr, &gp);
                        break;
                    }
                    launch_flow_iter(e, st, L.w, L.h, L.ld, L.ps, R, up ? nullptr : fl, L.ps, M1, L.ps, up ? &ups : nullptr,
                                     npairs, level);
                    break;
                }
                launch_blur(e, st, BlurLaunch{L.w, L.h, L.ld, L.ps, (i & 1) ? M1 : M0, (i & 1) ? M0 : M1, fl, R, (flags & 2) ? 0 : 1,
                                              level, npairs});
                break;
            case TW_K_SCAN: {
                const int gw = (L.w + span - 1) / span, gh = (L.h + span - 1) / span;
                launch_span_gather(e, st, fl, L, span, gw, gh, grid, npairs);
                const ScanArgs a = scan_args(grid, span, gw, gh, 4.0, cnt, rec, nullptr, 0, 0);
                TW_LAUNCH(e, TW_DF_SPAN_SCAN, tw_span_scan<false>, dim3(npairs), dim3(1024), 0, st, a);
            } break;
        }
        return TW_OK;
    };
    for (int i = 0; i < 2; i++)
        if ((r = once(i))) return r;
    TW_HIP(e, hipEventRecord(ea, st));
    for (int i = 0; i < iters; i++)
        if ((r = once(i))) return r;
    TW_HIP(e, hipEventRecord(eb, st));
    TW_HIP(e, hipGetLastError());
    TW_HIP(e, hipEventSynchronize(eb));
    float ms = 0;
    TW_HIP(e, hipEventElapsedTime(&ms, ea, eb));
    *avg_us = ms * 1e3f / iters;
    return TW_OK;
}

// ---- per-stage entry points (tests) --------------------------------------------------------------------
#include "twflow_stage.hip.h"
