// stub_twflow.cpp — a stand-in for libtwflow.so's C ABI that computes nothing: every pair answers a canned vector
// list.  ONLY for CPU-side builds of the host layer: the ThreadSanitizer build (`make tsan`; GPU sanitizer runs are not
// available) and the host-layer ceiling measurement (`make queue_stub`, tests/test_host_queue.py): twhost.cpp's queue,
// consumers, pump and dispose path with 8 consumers on 8 pretend devices.  Never linked into the product.
//
// Two timing models:
//   default              every tw_wait sleeps 50 us (TSAN runs: just enough to interleave threads)
//   TW_STUB_BATCH_MS=T   each pretend device is a FIFO server with the MEASURED service time of the real engine:
//                        a batch of `slots` pairs takes T ms (a partial batch its share), batches of one engine run one
//                        after the other, and tw_wait returns when the batch's completion time has passed (a timer,
//                        not a sleep per call) — VERDICT r4 #5: 31.3 ms per 128 pairs per device at 1080p.
//
// Two switches for the tests of the consumer's steps (tests/test_host_consumer_steps.py, tools/consumer_trace.py):
//   TW_STUB_TRACE=<file> every call of the C ABI appends one line to <file>, under one mutex: the engine's device, the
//                        call's name, its value arguments, the ticket, an image handle's ordinal of creation, and for every
//                        host image handed over whether it lies inside a live tw_host_alloc block ("pin") and a 64-bit
//                        FNV-1a of exactly the bytes the call may read; then the status (tw_wait: the count too).
//                        tw_host_alloc logs its byte count, tw_host_free the ordinal of the block.  Pointers and times are
//                        not logged.  Off unless set: the timing models are untouched.  Not recorded: the queries that take
//                        no engine's state and may come from any thread (tw_png_on_device — the decode pool asks it —,
//                        tw_strerror, tw_last_error, tw_default_params, tw_stub_*).
//   TW_STUB_BUSY_AT=k    the k-th submit call of each engine answers TW_E_BUSY once and books nothing (the consumer's retry)
//
// What "differs" means changed with tw_submit_png: the consumer sends every half-decoded pair through it, and the stub
// finishes both images with the host layer's own code (one allocation and copy per image) and compares the GRAY of pixel
// 0, where tw_submit_png8 compares the first raw sample of the filtered rows.  Two RGBA files with equal R bytes and
// different grays (or the reverse) therefore answer differently through the two calls; the suite's fixtures do not.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/twflow.h"
#include "twhost.h"

// (weak: the stub built on its own, without twhost.cpp, still loads; tw_submit_png then takes gray images only)
namespace twhost {
bool finish_png_kind_on_host(const uint8_t* rows, int w, int h, const PngKind& kind, std::vector<uint8_t>& gray) __attribute__((weak));
void jpeg_luma_to_gray(const JpegLuma& luma, std::vector<uint8_t>& img) __attribute__((weak));
}

typedef std::chrono::steady_clock stub_clock;
// a resident image: the stub's host copy of the gray bytes it ever looks at — pixel 0 — and the size
struct tw_image {
    int w, h;
    uint8_t first;
};
struct tw_engine {
    int device, cap;
    std::mutex m;
    std::map<tw_ticket, int> open;  // ticket -> width (echoed as the vector's x)
    struct PairInfo {
        int w, h;
        uint8_t first[2];
    };
    std::map<tw_ticket, PairInfo> info;  // ticket -> what tw_image_keep keeps of the pair
    std::map<const tw_image*, tw_image> images;  // live resident images by handle (a number never handed out twice: looked up, never dereferenced)
    std::map<tw_ticket, std::string> bad;  // tw_submit_png: the image ("expected" / "target") the host's finisher refused
    int regions = 0;                       // TW_OPT_REGIONS as tw_set_option left it
    std::map<tw_ticket, int> gap_of;       // ticket -> the option's value when the pair was submitted (0: off)
    int residual = 0;                      // TW_OPT_RESIDUAL as tw_set_option left it
    std::map<tw_ticket, int> tol_of;       // ticket -> that option's value when the pair was submitted (0: off)
    int shift = 0;                         // TW_OPT_SHIFT as tw_set_option left it
    std::map<tw_ticket, tw_shift> shift_of;  // ticket -> the pair's record, computed when it was submitted with the option on
    int bands = 0;                         // TW_OPT_SHIFT_BANDS as tw_set_option left it
    std::map<tw_ticket, std::vector<tw_shift_band>> bands_of;  // ticket -> the pair's band records, likewise (both options on)
    std::string err;
    tw_ticket next = 1;
    int submit_calls = 0, busy_at = 0;  // TW_STUB_BUSY_AT
    // timer model (TW_STUB_BATCH_MS): the open batch and the completion time of every launched one
    double batch_ms = 0;
    long cur_batch = 0;
    int cur_count = 0;
    std::map<tw_ticket, long> batch_of;
    std::map<long, stub_clock::time_point> done_at;
    std::map<long, int> waiters;  // pairs of a launched batch not collected yet
    stub_clock::time_point free_at = stub_clock::now();
    void launch_locked()
    {
        if (!cur_count) return;
        const stub_clock::time_point now = stub_clock::now();
        const stub_clock::time_point start = now > free_at ? now : free_at;
        const auto service = std::chrono::nanoseconds((long long)(batch_ms * 1e6 * cur_count / (cap > 0 ? cap : 1)));
        free_at = start + service;
        done_at[cur_batch] = free_at;
        waiters[cur_batch] = cur_count;
        cur_batch++;
        cur_count = 0;
    }
};

static std::atomic<int> g_engines{0};
// calls so far, for the drivers that report them (tests/test_host_png_kinds.py): pairs that came through tw_submit_png,
// and through it images that were still PNG rows
static std::atomic<long> g_png_calls{0}, g_png_row_images{0};
// likewise pairs that came through tw_submit_jpeg, and through it images that were still coefficients
static std::atomic<long> g_jpeg_calls{0}, g_jpeg_coef_images{0};
// resident images: tw_image_keep calls that kept one, pairs that came through tw_submit_image_*, tw_image_release calls
static std::atomic<long> g_res_kept{0}, g_res_image_pairs{0}, g_res_released{0};
static const uintptr_t kFirstImage = 0x1000, kImageStep = 16;
static std::atomic<uintptr_t> g_next_image{kFirstImage};

// --- the call recorder (TW_STUB_TRACE) ---
static const char* const g_trace_path = getenv("TW_STUB_TRACE");
static std::mutex g_trace_m;
static FILE* g_trace_file = nullptr;
struct HostBlock {
    size_t bytes;
    long ordinal;
};
static std::map<const uint8_t*, HostBlock> g_blocks;  // live tw_host_alloc blocks (kept only while tracing)
static long g_block_ordinal = 0;
static inline bool tracing() { return g_trace_path && g_trace_path[0]; }
static void trace(const tw_engine* e, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void trace(const tw_engine* e, const char* fmt, ...)
{
    std::lock_guard<std::mutex> lk(g_trace_m);
    if (!g_trace_file) g_trace_file = fopen(g_trace_path, "a");
    if (!g_trace_file) return;
    if (e) fprintf(g_trace_file, "dev=%d ", e->device);
    else fputs("dev=- ", g_trace_file);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(g_trace_file, fmt, ap);
    va_end(ap);
    fputc('\n', g_trace_file);
    fflush(g_trace_file);
}
static const char* status_name(tw_status r)
{
    switch (r) {
        case TW_OK: return "OK";
        case TW_E_BUSY: return "BUSY";
        case TW_E_BAD_PARAMETER: return "BAD_PARAMETER";
        case TW_E_BAD_IMAGE_FORMAT: return "BAD_IMAGE_FORMAT";
        case TW_E_DONT_MATCH_SIZE: return "DONT_MATCH_SIZE";
        case TW_E_UNSUPPORTED: return "UNSUPPORTED";
        case TW_E_NOMEM: return "NOMEM";
        case TW_E_DEVICE: return "DEVICE";
        default: return "OTHER";
    }
}
static long image_ordinal(const tw_image* img) { return img ? (long)(((uintptr_t)img - kFirstImage) / kImageStep) : -1; }
// "pin=<0|1> fnv=<hash>" of `rows` rows of `row_bytes` at `stride`, plus `tail` bytes at `extra` (a JPEG's quant table)
static std::string bytes_seen(const void* p, size_t rows, size_t row_bytes, ptrdiff_t stride, const void* extra = nullptr,
                              size_t tail = 0)
{
    if (!p) return "null";
    const uint8_t* b = (const uint8_t*)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t y = 0; y < rows; y++)
        for (size_t x = 0; x < row_bytes; x++) h = (h ^ b[(ptrdiff_t)y * stride + (ptrdiff_t)x]) * 1099511628211ull;
    for (size_t x = 0; x < tail; x++) h = (h ^ ((const uint8_t*)extra)[x]) * 1099511628211ull;
    bool pinned = false;
    {
        std::lock_guard<std::mutex> lk(g_trace_m);
        auto it = g_blocks.upper_bound(b);
        if (it != g_blocks.begin()) {
            --it;
            const size_t last = rows ? (rows - 1) * (size_t)stride + row_bytes : 0;
            pinned = b + last <= it->first + it->second.bytes;
        }
    }
    char buf[64];
    snprintf(buf, sizeof(buf), "pin=%d fnv=%016llx", pinned ? 1 : 0, (unsigned long long)h);
    return buf;
}
static size_t png_row_bytes(int color_type, int bit_depth, int w)
{
    const size_t samples = color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 1;
    return 1 + ((size_t)w * samples * (size_t)bit_depth + 7) / 8;
}
static std::string rows_seen(const tw_png_rows* r)
{
    if (!r) return "null";
    const bool gray = r->color_type == TW_PNG_PLAIN_GRAY;
    const size_t rb = gray ? (size_t)r->width : png_row_bytes(r->color_type, r->bit_depth, r->width);
    char buf[96];
    if (gray) snprintf(buf, sizeof(buf), "%dx%d gray ", r->width, r->height);
    else snprintf(buf, sizeof(buf), "%dx%d ct=%d bd=%d plte=%d ", r->width, r->height, r->color_type, r->bit_depth, r->palette_entries);
    return buf + bytes_seen(r->rows, r->height > 0 ? (size_t)r->height : 0, r->width > 0 ? rb : 0, (ptrdiff_t)rb);
}
static std::string luma_seen(const tw_jpeg_luma* l)
{
    if (!l) return "null";
    char buf[96];
    if (l->coef) {
        snprintf(buf, sizeof(buf), "%dx%d coef blocks=%dx%d ", l->width, l->height, l->blocks_w, l->blocks_h);
        return buf + bytes_seen(l->coef, 1, (size_t)l->blocks_w * (size_t)l->blocks_h * 128, 0, l->quant, 128);
    }
    snprintf(buf, sizeof(buf), "%dx%d gray ", l->width, l->height);
    return buf + bytes_seen(l->gray, l->height > 0 ? (size_t)l->height : 0, l->width > 0 ? (size_t)l->width : 0, l->width);
}
// TW_STUB_BUSY_AT: true for the one submit call that is to answer TW_E_BUSY
static bool busy_now(tw_engine* e)
{
    if (!e) return false;
    std::lock_guard<std::mutex> lk(e->m);
    return ++e->submit_calls == e->busy_at;
}

extern "C" {
void tw_default_params(tw_params* p)
{
    p->pyrScale = 0.5; p->pyrLevels = 3; p->winSize = 30; p->pyrIterations = 3; p->polyN = 7; p->polySigma = 1.5; p->flags = 256;
}
static int stub_device_count()
{
    const char* ev = getenv("TW_STUB_DEVICES");
    return ev ? atoi(ev) : 8;
}
int tw_device_count(void)
{
    const int n = stub_device_count();
    if (tracing()) trace(nullptr, "tw_device_count -> %d", n);
    return n;
}
// TW_STUB_PCI="0000:01:00.0,0000:81:00.0,...": bus id of pretend device i (cycled); unset: "0000:<i>0:00.0"
tw_status tw_device_pci_bus_id(int device, char* buf, int cap)
{
    if (tracing()) trace(nullptr, "tw_device_pci_bus_id device=%d", device);
    if (!buf || cap < 16 || device < 0 || device >= stub_device_count()) return TW_E_DEVICE;
    const char* ev = getenv("TW_STUB_PCI");
    if (ev && ev[0]) {
        std::string s(ev);
        std::vector<std::string> ids;
        size_t p = 0;
        while (p <= s.size()) {
            const size_t q = s.find(',', p);
            ids.push_back(s.substr(p, q == std::string::npos ? std::string::npos : q - p));
            if (q == std::string::npos) break;
            p = q + 1;
        }
        snprintf(buf, (size_t)cap, "%s", ids[(size_t)device % ids.size()].c_str());
    } else {
        snprintf(buf, (size_t)cap, "0000:%x0:00.0", device & 0xf);
    }
    return TW_OK;
}
tw_status tw_host_alloc(tw_engine* e, size_t bytes, void** hptr)
{
    *hptr = malloc(bytes);
    if (tracing()) {
        long ord = -1;
        if (*hptr) {
            std::lock_guard<std::mutex> lk(g_trace_m);
            ord = g_block_ordinal++;
            g_blocks[(const uint8_t*)*hptr] = HostBlock{bytes, ord};
        }
        trace(e, "tw_host_alloc bytes=%zu -> %s block=%ld", bytes, *hptr ? "OK" : "NOMEM", ord);
    }
    return *hptr ? TW_OK : TW_E_NOMEM;
}
tw_status tw_host_free(tw_engine* e, void* hptr)
{
    if (tracing()) {
        long ord = -1;
        {
            std::lock_guard<std::mutex> lk(g_trace_m);
            auto it = g_blocks.find((const uint8_t*)hptr);
            if (it != g_blocks.end()) {
                ord = it->second.ordinal;
                g_blocks.erase(it);
            }
        }
        trace(e, "tw_host_free block=%ld -> OK", ord);
    }
    free(hptr);
    return TW_OK;
}
tw_status tw_set_option(tw_engine* e, int option, int value)
{
    tw_status r = TW_OK;
    if (option == TW_OPT_REGIONS) {
        if (value < 0 || value > 8) r = TW_E_BAD_PARAMETER;
        else if (e) {
            std::lock_guard<std::mutex> lk(e->m);
            e->regions = value;
        }
    }
    if (option == TW_OPT_RESIDUAL) {
        if (value < 0 || value > 254) r = TW_E_BAD_PARAMETER;
        else if (e) {
            std::lock_guard<std::mutex> lk(e->m);
            e->residual = value;
        }
    }
    if (option == TW_OPT_SHIFT) {
        if (value < 0 || value > 1024) r = TW_E_BAD_PARAMETER;
        else if (e) {
            std::lock_guard<std::mutex> lk(e->m);
            e->shift = value;
        }
    }
    if (option == TW_OPT_SHIFT_BANDS) {
        if (value != 0 && (value < 32 || value > 1024 || value % 16 != 0)) r = TW_E_BAD_PARAMETER;
        else if (e) {
            std::lock_guard<std::mutex> lk(e->m);
            e->bands = value;
        }
    }
    if (tracing()) trace(e, "tw_set_option option=%d value=%d -> %s", option, value, status_name(r));
    return r;
}
tw_status tw_prof_select(tw_engine* e, int kernel, int level)
{
    if (tracing()) trace(e, "tw_prof_select kernel=%d level=%d -> OK", kernel, level);
    return TW_OK;
}
tw_status tw_prof_read(tw_engine* e, int kernel, double* ms, int* n)
{
    if (tracing()) trace(e, "tw_prof_read kernel=%d -> OK", kernel);
    if (ms) *ms = 0;
    if (n) *n = 0;
    return TW_OK;
}
const char* tw_strerror(tw_status) { return "stub"; }
const char* tw_last_error(const tw_engine* e) { return e ? e->err.c_str() : ""; }
void tw_stub_png_calls(long* pairs, long* row_images)
{
    *pairs = g_png_calls;
    *row_images = g_png_row_images;
}
void tw_stub_jpeg_calls(long* pairs, long* coef_images)
{
    *pairs = g_jpeg_calls;
    *coef_images = g_jpeg_coef_images;
}
void tw_stub_resident_calls(long* kept, long* image_pairs, long* released)
{
    *kept = g_res_kept;
    *image_pairs = g_res_image_pairs;
    *released = g_res_released;
}
int tw_grid_capacity(int w, int h, int span)
{
    const int cap = span > 0 ? ((h + span - 1) / span) * ((w + span - 1) / span) : 0;
    if (tracing()) trace(nullptr, "tw_grid_capacity %dx%d span=%d -> %d", w, h, span, cap);
    return cap;
}
tw_status tw_engine_create(int device, const tw_params* p, int slots, tw_engine** out)
{
    tw_engine* e = new tw_engine();
    e->device = device;
    e->cap = slots;
    if (const char* ev = getenv("TW_STUB_BATCH_MS")) e->batch_ms = atof(ev);
    if (const char* ev = getenv("TW_STUB_BUSY_AT")) e->busy_at = atoi(ev);
    g_engines++;
    *out = e;
    if (tracing())
        trace(e, "tw_engine_create slots=%d pyrScale=%g pyrLevels=%d winSize=%d pyrIterations=%d polyN=%d polySigma=%g flags=%d -> OK",
              slots, (double)p->pyrScale, (int)p->pyrLevels, (int)p->winSize, (int)p->pyrIterations, (int)p->polyN,
              (double)p->polySigma, (int)p->flags);
    return TW_OK;
}
void tw_engine_destroy(tw_engine* e)
{
    if (tracing()) trace(e, "tw_engine_destroy");
    g_engines--;
    delete e;
}
}  // extern "C"

// TW_OPT_SHIFT on the CPU, the definition of include/twflow.h restated: the profiles, the search of one axis, the acceptance
// check.  Plain loops: the stub is where the host tests run, not a fast path.
static int stub_shift_search(const std::vector<uint32_t>& pE, const std::vector<uint32_t>& pT, int R)
{
    const int L = (int)pE.size(), r = std::min(R, L / 2);
    int best = 0;
    uint64_t bc = 0, bn = 0;
    for (int k = 0; k <= 2 * r; k++) {
        const int d = (k & 1) ? -((k + 1) / 2) : k / 2;  // 0, -1, +1, -2, +2, ...
        uint64_t c = 0;
        for (int i = std::max(0, -d); i < std::min(L, L - d); i++) c += pE[i] > pT[i + d] ? pE[i] - pT[i + d] : pT[i + d] - pE[i];
        const uint64_t n = (uint64_t)(L - abs(d));
        if (k == 0 || c * bn < bc * n) best = d, bc = c, bn = n;
    }
    return best;
}
static uint64_t stub_shift_sad(const uint8_t* a, const uint8_t* b, int w, int h, ptrdiff_t stride, int dx, int dy)
{
    uint64_t s = 0;
    for (int y = std::max(0, -dy); y < std::min(h, h - dy); y++)
        for (int x = std::max(0, -dx); x < std::min(w, w - dx); x++)
            s += (uint64_t)abs((int)a[y * stride + x] - (int)b[(y + dy) * stride + (x + dx)]);
    return s;
}
static tw_shift stub_shift(const uint8_t* a, const uint8_t* b, int w, int h, ptrdiff_t stride, int R)
{
    std::vector<uint32_t> colE(w, 0), colT(w, 0), rowE(h, 0), rowT(h, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            colE[x] += a[y * stride + x];
            rowE[y] += a[y * stride + x];
            colT[x] += b[y * stride + x];
            rowT[y] += b[y * stride + x];
        }
    tw_shift s;
    memset(&s, 0, sizeof(s));
    s.dx = stub_shift_search(colE, colT, R);
    s.dy = stub_shift_search(rowE, rowT, R);
    s.n_zero = w * h;
    s.sad_zero = stub_shift_sad(a, b, w, h, stride, 0, 0);
    s.n_shift = (w - abs(s.dx)) * (h - abs(s.dy));
    s.sad_shift = stub_shift_sad(a, b, w, h, stride, s.dx, s.dy);
    if (s.dx != 0 || s.dy != 0) s.applied = s.sad_shift * (uint64_t)s.n_zero <= (s.sad_zero >> 1) * (uint64_t)s.n_shift ? 1 : 0;
    return s;
}

// TW_OPT_SHIFT_BANDS on the CPU, the definition of include/twflow.h restated: the row signatures at the pair's global dx, the
// search of each band, its acceptance check.  sig (nullable): [sigE[h][nblk], sigT[h][nblk]].
static std::vector<tw_shift_band> stub_bands(const uint8_t* a, const uint8_t* b, int w, int h, ptrdiff_t stride, int R, int B, int dx,
                                             uint16_t* sig = nullptr)
{
    const int xa = std::max(0, -dx), xb = std::min(w, w - dx), nblk = (xb - xa + 63) / 64;
    std::vector<uint16_t> sE((size_t)h * nblk, 0), sT((size_t)h * nblk, 0);
    for (int y = 0; y < h; y++)
        for (int x = xa; x < xb; x++) {
            sE[(size_t)y * nblk + (x - xa) / 64] += a[y * stride + x];
            sT[(size_t)y * nblk + (x - xa) / 64] += b[y * stride + x + dx];
        }
    if (sig) {
        memcpy(sig, sE.data(), sE.size() * sizeof(uint16_t));
        memcpy(sig + sE.size(), sT.data(), sT.size() * sizeof(uint16_t));
    }
    const int r = std::min(R, h / 2);
    std::vector<tw_shift_band> out;
    for (int y0 = 0; y0 < h; y0 += B) {
        const int rows = std::min(B, h - y0), need = (rows + 1) / 2;
        int best = 0;
        uint64_t bc = 0, bn = 0;
        for (int k = 0; k <= 2 * r; k++) {
            const int d = (k & 1) ? -((k + 1) / 2) : k / 2;  // 0, -1, +1, -2, +2, ...
            const int lo = std::max(y0, -d), hi = std::min(y0 + rows, h - d);
            if (k != 0 && hi - lo < need) continue;
            uint64_t c = 0;
            for (int i = lo; i < hi; i++)
                for (int j = 0; j < nblk; j++) c += (uint64_t)abs((int)sE[(size_t)i * nblk + j] - (int)sT[(size_t)(i + d) * nblk + j]);
            const uint64_t n = (uint64_t)(hi - lo);
            if (k == 0 || c * bn < bc * n) best = d, bc = c, bn = n;
        }
        tw_shift_band s;
        memset(&s, 0, sizeof(s));
        s.y = y0;
        s.rows = rows;
        s.dy = best;
        s.n_zero = rows * w;
        for (int y = y0; y < y0 + rows; y++)
            for (int x = 0; x < w; x++) s.sad_zero += (uint64_t)abs((int)a[y * stride + x] - (int)b[y * stride + x]);
        s.n_shift = s.n_zero;
        s.sad_shift = s.sad_zero;
        if (dx != 0 || best != 0) {
            const int lo = std::max(y0, -best), hi = std::min(y0 + rows, h - best);
            s.n_shift = (hi - lo) * (xb - xa);
            s.sad_shift = 0;
            for (int y = lo; y < hi; y++)
                for (int x = xa; x < xb; x++) s.sad_shift += (uint64_t)abs((int)a[y * stride + x] - (int)b[(y + best) * stride + x + dx]);
            s.applied = s.sad_shift * (uint64_t)s.n_zero <= (s.sad_zero >> 2) * (uint64_t)s.n_shift ? 1 : 0;
        }
        out.push_back(s);
    }
    return out;
}

// What the entry points do once a call is recorded (and not refused by TW_STUB_BUSY_AT): they call one another through these.
// stride > 0: a and b are whole images of w x h bytes (tw_submit_u8); 0: only their first bytes are there (every other
// entry point hands on a pair's first pixels), and a shift record is then that of the 1 x 1 pair of those two bytes
static tw_status stub_u8(tw_engine* e, const uint8_t* a, const uint8_t* b, int w, int h, tw_ticket* t, ptrdiff_t stride = 0)
{
    if (!a || !b || w < 1 || h < 1) return TW_E_BAD_PARAMETER;
    if (stride && stride < w) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    const int radius = e->shift;
    tw_shift sh;
    if (radius) sh = stride ? stub_shift(a, b, w, h, stride, radius) : stub_shift(a, b, 1, 1, 1, radius);
    // (the bands take effect only with the shift on; as the shift record, on the whole images where they are there)
    std::vector<tw_shift_band> bd;
    if (radius && e->bands) bd = stride ? stub_bands(a, b, w, h, stride, radius, e->bands, sh.dx) : stub_bands(a, b, 1, 1, 1, radius, e->bands, sh.dx);
    *t = e->next++;
    e->open[*t] = w + (a[0] != b[0] ? 1000000 : 0);
    e->info[*t] = tw_engine::PairInfo{w, h, {a[0], b[0]}};
    if (e->regions) e->gap_of[*t] = e->regions;
    if (e->residual) e->tol_of[*t] = e->residual;
    if (radius) e->shift_of[*t] = sh;
    if (!bd.empty()) e->bands_of[*t] = bd;
    if (e->batch_ms > 0) {
        e->batch_of[*t] = e->cur_batch;
        if (++e->cur_count >= e->cap) e->launch_locked();  // a full batch starts by itself, like the engine's
    }
    return TW_OK;
}
// filtered rows: byte 0 is a filter type, byte 1 the first sample — compare those like tw_submit_u8 compares pixel 0
static tw_status stub_png8(tw_engine* e, const uint8_t* a, int cha, const uint8_t* b, int chb, int w, int h, tw_ticket* t)
{
    return stub_u8(e, a + (cha ? 1 : 0), b + (chb ? 1 : 0), w, h, t);
}
// the _sized calls: OpticalFlow::calculate's size rule, then what tw_submit_u8 / tw_submit_png8 do
static bool stub_sizes_match(int w, int h, int tw, int th) { return abs(w - tw) <= 5 && abs(h - th) <= 5; }
static tw_status stub_u8_sized(tw_engine* e, const uint8_t* a, int w, int h, const uint8_t* b, int tw, int th, ptrdiff_t tstride,
                               tw_ticket* t)
{
    if (tw < 1 || th < 1 || tstride < tw) return TW_E_BAD_PARAMETER;
    if (!stub_sizes_match(w, h, tw, th)) return TW_E_DONT_MATCH_SIZE;
    return stub_u8(e, a, b, w, h, t);
}
// the same table as the library's
extern "C" int tw_png_on_device(int color_type, int bit_depth, int interlace)
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
// tw_submit_png: each image is finished to gray with the host layer's own code, then the pair is what tw_submit_u8 sees.
// A palette index without an entry is remembered for the ticket: tw_wait answers it, as the engine's does.
static tw_status stub_png(tw_engine* e, const tw_png_rows* a, const tw_png_rows* b, tw_ticket* t)
{
    if (!a || !b || !a->rows || !b->rows) return TW_E_BAD_PARAMETER;
    if (!stub_sizes_match(a->width, a->height, b->width, b->height)) return TW_E_DONT_MATCH_SIZE;
    g_png_calls++;
    const tw_png_rows* im[2] = {a, b};
    uint8_t first[2] = {0, 0};
    const char* bad = nullptr;
    for (int q = 0; q < 2; q++) {
        if (im[q]->color_type == TW_PNG_PLAIN_GRAY) {
            first[q] = im[q]->rows[0];
            continue;
        }
        if (!tw_png_on_device(im[q]->color_type, im[q]->bit_depth, 0) || !twhost::finish_png_kind_on_host) return TW_E_UNSUPPORTED;
        g_png_row_images++;
        twhost::PngKind k;
        k.color_type = im[q]->color_type;
        k.bit_depth = im[q]->bit_depth;
        if (im[q]->color_type == 3) {
            if (!im[q]->palette || im[q]->palette_entries < 1 || im[q]->palette_entries > 256) return TW_E_BAD_IMAGE_FORMAT;
            k.plte.assign(im[q]->palette, im[q]->palette + 3 * (size_t)im[q]->palette_entries);
        }
        std::vector<uint8_t> g;
        if (!twhost::finish_png_kind_on_host(im[q]->rows, im[q]->width, im[q]->height, k, g)) {
            if (!bad) bad = q ? "target" : "expected";
            continue;
        }
        first[q] = g[0];
    }
    const tw_status r = stub_u8(e, &first[0], &first[1], a->width, a->height, t);
    if (r == TW_OK && bad) {
        std::lock_guard<std::mutex> lk(e->m);
        e->bad[*t] = bad;
    }
    return r;
}
// tw_submit_jpeg: the first gray pixel of a coefficient image is the host layer's own inverse DCT of its block 0, then the
// pair is what tw_submit_u8 sees
static tw_status stub_jpeg(tw_engine* e, const tw_jpeg_luma* a, const tw_jpeg_luma* b, tw_ticket* t)
{
    const tw_jpeg_luma* im[2] = {a, b};
    for (int q = 0; q < 2; q++) {
        if (!im[q] || (!im[q]->coef && !im[q]->gray) || im[q]->width < 1 || im[q]->height < 1) return TW_E_BAD_PARAMETER;
        const int nbx = (im[q]->width + 7) / 8, nby = (im[q]->height + 7) / 8;
        if (im[q]->coef && (im[q]->blocks_w < nbx || im[q]->blocks_w > nbx + 3 || im[q]->blocks_h < nby || im[q]->blocks_h > nby + 3))
            return TW_E_BAD_PARAMETER;
    }
    if (!stub_sizes_match(a->width, a->height, b->width, b->height)) return TW_E_DONT_MATCH_SIZE;
    g_jpeg_calls++;
    uint8_t first[2] = {0, 0};
    for (int q = 0; q < 2; q++) {
        if (!im[q]->coef) {
            first[q] = im[q]->gray[0];
            continue;
        }
        if (!twhost::jpeg_luma_to_gray) return TW_E_UNSUPPORTED;
        g_jpeg_coef_images++;
        twhost::JpegLuma l;
        l.w = l.h = l.bw = l.bh = 1;
        memcpy(l.quant, im[q]->quant, sizeof(l.quant));
        l.coef.assign(im[q]->coef, im[q]->coef + 64);
        std::vector<uint8_t> g;
        twhost::jpeg_luma_to_gray(l, g);
        first[q] = g[0];
    }
    return stub_u8(e, &first[0], &first[1], a->width, a->height, t);
}

extern "C" {
// every submit: refused once by TW_STUB_BUSY_AT or handed on, then recorded with its ticket
#define STUB_SUBMIT(call) (busy_now(e) ? TW_E_BUSY : (call))
static void trace_submit(tw_engine* e, const char* name, const std::string& images, int span, double thr, tw_status r, const tw_ticket* t)
{
    trace(e, "%s %s span=%d threshold=%g -> %s ticket=%lld", name, images.c_str(), span, thr, status_name(r),
          r == TW_OK ? (long long)*t : -1LL);
}
tw_status tw_submit_u8(tw_engine* e, const uint8_t* a, const uint8_t* b, int w, int h, ptrdiff_t stride, int span, double thr,
                       tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_u8(e, a, b, w, h, t, stride));
    if (tracing()) {
        char sz[64];
        snprintf(sz, sizeof(sz), "[%dx%d stride=%td ", w, h, stride);  // (one size and stride for both images)
        const size_t rows = h > 0 ? (size_t)h : 0, rb = w > 0 ? (size_t)w : 0;
        trace_submit(e, "tw_submit_u8", "a=" + (sz + bytes_seen(a, rows, rb, stride)) + "] b=" + (sz + bytes_seen(b, rows, rb, stride)) + "]",
                     span, thr, r, t);
    }
    return r;
}
tw_status tw_submit_png8(tw_engine* e, const uint8_t* a, int cha, const uint8_t* b, int chb, int w, int h, int span, double thr,
                         tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_png8(e, a, cha, b, chb, w, h, t));
    if (tracing()) {
        char sz[64];
        snprintf(sz, sizeof(sz), "%dx%d cha=%d chb=%d", w, h, cha, chb);
        const size_t rows = h > 0 ? (size_t)h : 0, ra = (size_t)(cha ? 1 + w * cha : w), rb = (size_t)(chb ? 1 + w * chb : w);
        trace_submit(e, "tw_submit_png8", std::string(sz) + " a=[" + bytes_seen(a, rows, ra, (ptrdiff_t)ra) + "] b=[" + bytes_seen(b, rows, rb, (ptrdiff_t)rb) + "]",
                     span, thr, r, t);
    }
    return r;
}
tw_status tw_submit_u8_sized(tw_engine* e, const uint8_t* a, int w, int h, ptrdiff_t stride, const uint8_t* b, int tw, int th,
                             ptrdiff_t tstride, int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_u8_sized(e, a, w, h, b, tw, th, tstride, t));
    if (tracing()) {
        char sa[64], sb[64];
        snprintf(sa, sizeof(sa), "a=[%dx%d stride=%td ", w, h, stride);
        snprintf(sb, sizeof(sb), "] b=[%dx%d stride=%td ", tw, th, tstride);
        trace_submit(e, "tw_submit_u8_sized", sa + bytes_seen(a, h > 0 ? (size_t)h : 0, w > 0 ? (size_t)w : 0, stride) + sb +
                     bytes_seen(b, th > 0 ? (size_t)th : 0, tw > 0 ? (size_t)tw : 0, tstride) + "]", span, thr, r, t);
    }
    return r;
}
tw_status tw_submit_png8_sized(tw_engine* e, const uint8_t* a, int cha, int w, int h, const uint8_t* b, int chb, int tw, int th,
                               int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(tw < 1 || th < 1 ? TW_E_BAD_PARAMETER : !stub_sizes_match(w, h, tw, th) ? TW_E_DONT_MATCH_SIZE
                                                                          : stub_png8(e, a, cha, b, chb, w, h, t));
    if (tracing()) {
        char sa[64], sb[64];
        snprintf(sa, sizeof(sa), "a=[%dx%d ch=%d ", w, h, cha);
        snprintf(sb, sizeof(sb), "] b=[%dx%d ch=%d ", tw, th, chb);
        const size_t ra = (size_t)(cha ? 1 + w * cha : w), rb = (size_t)(chb ? 1 + tw * chb : tw);
        trace_submit(e, "tw_submit_png8_sized", sa + bytes_seen(a, h > 0 ? (size_t)h : 0, ra, (ptrdiff_t)ra) + sb +
                     bytes_seen(b, th > 0 ? (size_t)th : 0, rb, (ptrdiff_t)rb) + "]", span, thr, r, t);
    }
    return r;
}
tw_status tw_submit_png(tw_engine* e, const tw_png_rows* a, const tw_png_rows* b, int span, double thr, const tw_flow_in*,
                        const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_png(e, a, b, t));
    if (tracing()) trace_submit(e, "tw_submit_png", "a=[" + rows_seen(a) + "] b=[" + rows_seen(b) + "]", span, thr, r, t);
    return r;
}
tw_status tw_submit_jpeg(tw_engine* e, const tw_jpeg_luma* a, const tw_jpeg_luma* b, int span, double thr, const tw_flow_in*,
                         const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_jpeg(e, a, b, t));
    if (tracing()) trace_submit(e, "tw_submit_jpeg", "a=[" + luma_seen(a) + "] b=[" + luma_seen(b) + "]", span, thr, r, t);
    return r;
}
// Resident images: the first gray pixel of the pair's image as tw_submit_u8 saw it (a palette image the finisher refused
// has pixel 0 = 0: undefined content, as the engine's header says)
static tw_status stub_image_keep(tw_engine* e, tw_ticket t, int which, tw_image** out)
{
    if (!e || !out) return TW_E_BAD_PARAMETER;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(e->m);
    auto it = e->info.find(t);
    if (it == e->info.end() || which < 0 || which > 1) return TW_E_BAD_PARAMETER;
    *out = (tw_image*)g_next_image.fetch_add(kImageStep);
    e->images[*out] = tw_image{it->second.w, it->second.h, it->second.first[which]};
    g_res_kept++;
    return TW_OK;
}
tw_status tw_image_keep(tw_engine* e, tw_ticket t, int which, tw_image** out)
{
    const tw_status r = stub_image_keep(e, t, which, out);
    if (tracing()) trace(e, "tw_image_keep ticket=%lld which=%d -> %s image=%ld", (long long)t, which, status_name(r), out ? image_ordinal(*out) : -1L);
    return r;
}
static tw_status stub_image_create_u8(tw_engine* e, const uint8_t* gray, int w, int h, ptrdiff_t stride, tw_image** out)
{
    if (!e || !out || !gray || w < 1 || h < 1 || stride < w) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    *out = (tw_image*)g_next_image.fetch_add(kImageStep);
    e->images[*out] = tw_image{w, h, gray[0]};
    return TW_OK;
}
tw_status tw_image_create_u8(tw_engine* e, const uint8_t* gray, int w, int h, ptrdiff_t stride, tw_image** out)
{
    const tw_status r = stub_image_create_u8(e, gray, w, h, stride, out);
    if (tracing())
        trace(e, "tw_image_create_u8 %dx%d stride=%td [%s] -> %s image=%ld", w, h, stride,
              bytes_seen(gray, h > 0 ? (size_t)h : 0, w > 0 ? (size_t)w : 0, stride).c_str(), status_name(r),
              r == TW_OK ? image_ordinal(*out) : -1L);
    return r;
}
static tw_status stub_image_release(tw_engine* e, tw_image* img)
{
    if (!e) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    if (!e->images.erase(img)) return TW_E_BAD_PARAMETER;
    g_res_released++;
    return TW_OK;
}
tw_status tw_image_release(tw_engine* e, tw_image* img)
{
    const tw_status r = stub_image_release(e, img);
    if (tracing()) trace(e, "tw_image_release image=%ld -> %s", image_ordinal(img), status_name(r));
    return r;
}
tw_status tw_image_size(const tw_engine* e, const tw_image* img, int* w, int* h)
{
    if (tracing()) trace(e, "tw_image_size image=%ld", image_ordinal(img));
    if (!e) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(const_cast<tw_engine*>(e)->m);
    auto it = e->images.find(img);
    if (it == e->images.end()) return TW_E_BAD_PARAMETER;
    if (w) *w = it->second.w;
    if (h) *h = it->second.h;
    return TW_OK;
}
// the resident image as a plain gray expected image of one known pixel, then what tw_submit_png / tw_submit_jpeg do
static bool stub_image_pixel(tw_engine* e, const tw_image* img, tw_image* copy)
{
    if (!e) return false;
    std::lock_guard<std::mutex> lk(e->m);
    auto it = e->images.find(img);
    if (it == e->images.end()) return false;
    *copy = it->second;
    return true;
}
static tw_status stub_image_png(tw_engine* e, const tw_image* img, const tw_png_rows* b, tw_ticket* t)
{
    tw_image im;
    if (!stub_image_pixel(e, img, &im)) return TW_E_BAD_PARAMETER;
    tw_png_rows a;
    a.rows = &im.first;
    a.width = im.w;
    a.height = im.h;
    a.color_type = TW_PNG_PLAIN_GRAY;
    a.bit_depth = 8;
    a.palette = nullptr;
    a.palette_entries = 0;
    const tw_status r = stub_png(e, &a, b, t);
    if (r == TW_OK) g_res_image_pairs++;
    return r;
}
tw_status tw_submit_image_png(tw_engine* e, const tw_image* img, const tw_png_rows* b, int span, double thr, const tw_flow_in*,
                              const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_image_png(e, img, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_image_png", "image=" + std::to_string(image_ordinal(img)) + " b=[" + rows_seen(b) + "]", span, thr, r, t);
    return r;
}
static tw_status stub_image_jpeg(tw_engine* e, const tw_image* img, const tw_jpeg_luma* b, tw_ticket* t)
{
    tw_image im;
    if (!stub_image_pixel(e, img, &im)) return TW_E_BAD_PARAMETER;
    tw_jpeg_luma a;
    memset(&a, 0, sizeof(a));
    a.gray = &im.first;
    a.width = im.w;
    a.height = im.h;
    const tw_status r = stub_jpeg(e, &a, b, t);
    if (r == TW_OK) g_res_image_pairs++;
    return r;
}
tw_status tw_submit_image_jpeg(tw_engine* e, const tw_image* img, const tw_jpeg_luma* b, int span, double thr, const tw_flow_in*,
                               const tw_flow_out*, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(stub_image_jpeg(e, img, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_image_jpeg", "image=" + std::to_string(image_ordinal(img)) + " b=[" + luma_seen(b) + "]", span, thr, r, t);
    return r;
}
// Ignore regions: the rectangles are checked as the engine checks them and recorded as given; the stub's one-pixel images
// have nothing to mask, so the pair is then what the plain call sees
static bool stub_rects_ok(const tw_rect* ig, int n)
{
    if (n < 0 || n > TW_MAX_IGNORE || (n > 0 && !ig)) return false;
    for (int i = 0; i < n; i++)
        if (ig[i].width < 0 || ig[i].height < 0) return false;
    return true;
}
static std::string rects_seen(const tw_rect* ig, int n)
{
    std::string s = " ignore=" + std::to_string(n) + "[";
    for (int i = 0; ig && i < n && i <= TW_MAX_IGNORE; i++) {
        char b[64];
        snprintf(b, sizeof(b), "%s%d,%d,%d,%d", i ? ";" : "", ig[i].x, ig[i].y, ig[i].width, ig[i].height);
        s += b;
    }
    return s + "]";
}
tw_status tw_submit_u8_ignore(tw_engine* e, const uint8_t* a, int w, int h, ptrdiff_t stride, const uint8_t* b, int tw, int th,
                              ptrdiff_t tstride, int span, double thr, const tw_flow_in*, const tw_flow_out*, const tw_rect* ig,
                              int n, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(!stub_rects_ok(ig, n) ? TW_E_BAD_PARAMETER : stub_u8_sized(e, a, w, h, b, tw, th, tstride, t));
    if (tracing()) {
        char sa[64], sb[64];
        snprintf(sa, sizeof(sa), "a=[%dx%d stride=%td ", w, h, stride);
        snprintf(sb, sizeof(sb), "] b=[%dx%d stride=%td ", tw, th, tstride);
        trace_submit(e, "tw_submit_u8_ignore", sa + bytes_seen(a, h > 0 ? (size_t)h : 0, w > 0 ? (size_t)w : 0, stride) + sb +
                     bytes_seen(b, th > 0 ? (size_t)th : 0, tw > 0 ? (size_t)tw : 0, tstride) + "]" + rects_seen(ig, n), span, thr, r, t);
    }
    return r;
}
tw_status tw_submit_png_ignore(tw_engine* e, const tw_png_rows* a, const tw_png_rows* b, int span, double thr, const tw_flow_in*,
                               const tw_flow_out*, const tw_rect* ig, int n, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(!stub_rects_ok(ig, n) ? TW_E_BAD_PARAMETER : stub_png(e, a, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_png_ignore", "a=[" + rows_seen(a) + "] b=[" + rows_seen(b) + "]" + rects_seen(ig, n), span, thr, r, t);
    return r;
}
tw_status tw_submit_jpeg_ignore(tw_engine* e, const tw_jpeg_luma* a, const tw_jpeg_luma* b, int span, double thr,
                                const tw_flow_in*, const tw_flow_out*, const tw_rect* ig, int n, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(!stub_rects_ok(ig, n) ? TW_E_BAD_PARAMETER : stub_jpeg(e, a, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_jpeg_ignore", "a=[" + luma_seen(a) + "] b=[" + luma_seen(b) + "]" + rects_seen(ig, n), span, thr, r, t);
    return r;
}
tw_status tw_submit_image_png_ignore(tw_engine* e, const tw_image* img, const tw_png_rows* b, int span, double thr,
                                     const tw_flow_in*, const tw_flow_out*, const tw_rect* ig, int n, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(!stub_rects_ok(ig, n) ? TW_E_BAD_PARAMETER : stub_image_png(e, img, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_image_png_ignore",
                     "image=" + std::to_string(image_ordinal(img)) + " b=[" + rows_seen(b) + "]" + rects_seen(ig, n), span, thr, r, t);
    return r;
}
tw_status tw_submit_image_jpeg_ignore(tw_engine* e, const tw_image* img, const tw_jpeg_luma* b, int span, double thr,
                                      const tw_flow_in*, const tw_flow_out*, const tw_rect* ig, int n, tw_ticket* t)
{
    const tw_status r = STUB_SUBMIT(!stub_rects_ok(ig, n) ? TW_E_BAD_PARAMETER : stub_image_jpeg(e, img, b, t));
    if (tracing())
        trace_submit(e, "tw_submit_image_jpeg_ignore",
                     "image=" + std::to_string(image_ordinal(img)) + " b=[" + luma_seen(b) + "]" + rects_seen(ig, n), span, thr, r, t);
    return r;
}
tw_status tw_submit_dev_sized(tw_engine* e, const void* a, int w, int h, ptrdiff_t stride, const void* b, int tw, int th,
                              ptrdiff_t tstride, int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    // (the stub's "device memory" is host memory: tw_submit_u8 reads pixel 0 of both)
    const tw_status r = STUB_SUBMIT(stub_u8_sized(e, (const uint8_t*)a, w, h, (const uint8_t*)b, tw, th, tstride, t));
    if (tracing()) {
        char sz[128];
        snprintf(sz, sizeof(sz), "a=[%dx%d stride=%td] b=[%dx%d stride=%td]", w, h, stride, tw, th, tstride);
        trace_submit(e, "tw_submit_dev_sized", sz, span, thr, r, t);
    }
    return r;
}
tw_status tw_flush(tw_engine* e)
{
    if (tracing()) trace(e, "tw_flush -> OK");
    if (e->batch_ms > 0) {
        std::lock_guard<std::mutex> lk(e->m);
        e->launch_locked();
    }
    return TW_OK;
}
static tw_status stub_wait(tw_engine* e, tw_ticket t, tw_vector* out, int cap, int* n, float* seconds)
{
    int w;
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->open.find(t);
        if (it == e->open.end()) return TW_E_BAD_PARAMETER;
        w = it->second;
        e->open.erase(it);
        e->info.erase(t);
        e->gap_of.erase(t);
        e->tol_of.erase(t);
        e->shift_of.erase(t);
        e->bands_of.erase(t);
    }
    if (e->batch_ms > 0) {
        stub_clock::time_point until;
        {
            std::lock_guard<std::mutex> lk(e->m);
            const long b = e->batch_of[t];
            e->batch_of.erase(t);
            if (b == e->cur_batch) e->launch_locked();  // waiting for a pair of the open batch starts it
            until = e->done_at[b];
            if (--e->waiters[b] == 0) {
                e->waiters.erase(b);
                e->done_at.erase(b);
            }
        }
        std::this_thread::sleep_until(until);  // returns at once for every later pair of a finished batch
    } else {
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->bad.find(t);
        if (it != e->bad.end()) {
            e->err = "bad palette index in the " + it->second + " image";
            e->bad.erase(it);
            return TW_E_BAD_IMAGE_FORMAT;
        }
    }
    const bool differs = w >= 1000000;
    if (n) *n = differs ? 1 : 0;
    if (differs && out && cap > 0) {
        out[0].x = w - 1000000;
        out[0].y = e->device;
        out[0].dx = 6.0;
        out[0].dy = -7.5;
    }
    if (seconds) *seconds = 1e-4f;
    return TW_OK;
}
tw_status tw_wait(tw_engine* e, tw_ticket t, tw_vector* out, int cap, int* n, float* seconds)
{
    int count = 0;
    const tw_status r = stub_wait(e, t, out, cap, &count, seconds);
    if (n) *n = count;
    if (tracing()) trace(e, "tw_wait ticket=%lld cap=%d -> %s count=%d", (long long)t, cap, status_name(r), count);
    return r;
}
// tw_wait plus a plain host flood fill over the vectors the stub reports.  Those vectors are echoes (x = the pair's width, y =
// the device), not grid points of an image: every one stands for a 1 x 1 cell, nothing is clipped, `gap` counts units of 1.
// Two differences from the library, neither visible through the stub's echoes of at most one vector per pair: the gap is the
// option's value when the PAIR was submitted (the library: when the pair's BATCH was opened), and the regions are those of the
// first cap + 1 vectors, so *n_regions would not be the true count for a pair with more vectors than cap + 1.
tw_status tw_wait_regions(tw_engine* e, tw_ticket t, tw_vector* out, int cap, int* n, int* region_of, tw_region* regions,
                          int region_cap, int* n_regions, float* seconds)
{
    if (!e) return TW_E_BAD_PARAMETER;
    int gap = 0;
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->gap_of.find(t);
        if (it != e->gap_of.end()) gap = it->second;
    }
    if (!gap) {  // (the ticket stays waitable)
        if (tracing()) trace(e, "tw_wait_regions ticket=%lld cap=%d -> %s", (long long)t, cap, status_name(TW_E_BAD_PARAMETER));
        return TW_E_BAD_PARAMETER;
    }
    int count = 0;
    std::vector<tw_vector> v((size_t)(cap > 0 ? cap : 0) + 1);
    const tw_status r = stub_wait(e, t, v.data(), (int)v.size(), &count, seconds);
    if (n) *n = count;
    const int got = r == TW_OK ? std::min(count, (int)v.size()) : 0;
    std::vector<int> of((size_t)got, -1);
    std::vector<tw_region> regs;
    for (int s = 0; s < got; s++) {
        if (of[s] >= 0) continue;
        const int id = (int)regs.size();
        std::vector<int> stack(1, s), members;
        of[s] = id;
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            members.push_back(i);
            for (int k = 0; k < got; k++)
                if (of[k] < 0 && abs(v[k].x - v[i].x) <= gap && abs(v[k].y - v[i].y) <= gap) of[k] = id, stack.push_back(k);
        }
        std::sort(members.begin(), members.end());
        int x0 = v[s].x, y0 = v[s].y, x1 = v[s].x, y1 = v[s].y, peak = members[0];
        const auto len = [&](int i) { return (float)v[i].dx * (float)v[i].dx + (float)v[i].dy * (float)v[i].dy; };
        for (int i : members) {
            x0 = std::min(x0, v[i].x), y0 = std::min(y0, v[i].y), x1 = std::max(x1, v[i].x), y1 = std::max(y1, v[i].y);
            if (len(i) > len(peak)) peak = i;
        }
        regs.push_back(tw_region{x0, y0, x1 + 1 - x0, y1 + 1 - y0, (int)members.size(), v[peak].x, v[peak].y, (float)v[peak].dx,
                                 (float)v[peak].dy});
    }
    for (int i = 0; i < got && i < cap; i++) {
        if (out) out[i] = v[i];
        if (region_of) region_of[i] = of[i];
    }
    if (n_regions) *n_regions = (int)regs.size();
    for (int i = 0; regions && i < (int)regs.size() && i < region_cap && i < TW_MAX_REGIONS; i++) regions[i] = regs[i];
    if (tracing())
        trace(e, "tw_wait_regions ticket=%lld cap=%d -> %s count=%d regions=%d", (long long)t, cap, status_name(r), count,
              (int)regs.size());
    return r;
}
// The change records of a pair that was submitted with TW_OPT_RESIDUAL on; the ticket is not consumed.  The stub compares no
// pixels: every such pair has ONE record, an echo like its vector — x = the pair's width, y = the device, n_diff =
// n_unexplained = the tolerance, max_diff = max_unexplained = |first byte of the expected image - first byte of the target|.
// As for the regions, the tolerance is the option's value when the PAIR was submitted.
tw_status tw_ticket_changes(tw_engine* e, tw_ticket t, tw_change* changes, int change_cap, int* n_changes)
{
    if (!e) return TW_E_BAD_PARAMETER;
    tw_status r = TW_OK;
    tw_change rec = {0, 0, 0, 0, 0, 0};
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->tol_of.find(t);
        auto in = e->info.find(t);
        if (it == e->tol_of.end() || in == e->info.end() || e->open.find(t) == e->open.end()) r = TW_E_BAD_PARAMETER;
        else {
            const int d = abs((int)in->second.first[0] - (int)in->second.first[1]);
            rec = tw_change{in->second.w, e->device, it->second, it->second, d, d};
        }
    }
    if (r == TW_OK) {
        if (n_changes) *n_changes = 1;
        if (changes && change_cap > 0) changes[0] = rec;
    }
    if (tracing()) trace(e, "tw_ticket_changes ticket=%lld cap=%d -> %s", (long long)t, change_cap, status_name(r));
    return r;
}
// The shift record of a pair that was submitted with TW_OPT_SHIFT on; the ticket is not consumed.  The definition of
// include/twflow.h computed on the CPU when the pair was submitted (stub_shift) — on the whole images where the entry point
// has them (tw_submit_u8), on the pair's first pixels otherwise.  The stub computes no flow, so nothing starts from the shift.
tw_status tw_ticket_shift(tw_engine* e, tw_ticket t, tw_shift* out)
{
    if (!e) return TW_E_BAD_PARAMETER;
    tw_status r = TW_OK;
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->shift_of.find(t);
        if (!out || it == e->shift_of.end() || e->open.find(t) == e->open.end()) r = TW_E_BAD_PARAMETER;
        else *out = it->second;
    }
    if (tracing()) trace(e, "tw_ticket_shift ticket=%lld -> %s", (long long)t, status_name(r));
    return r;
}
// The band records of a pair that was submitted with TW_OPT_SHIFT and TW_OPT_SHIFT_BANDS on; the ticket is not consumed.  The
// definition computed on the CPU when the pair was submitted (stub_bands), as tw_ticket_shift's record.
tw_status tw_ticket_shift_bands(tw_engine* e, tw_ticket t, tw_shift_band* out, int cap, int* n)
{
    if (!e) return TW_E_BAD_PARAMETER;
    tw_status r = TW_OK;
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->bands_of.find(t);
        if (!n || cap < 0 || (!out && cap > 0) || it == e->bands_of.end() || e->open.find(t) == e->open.end()) r = TW_E_BAD_PARAMETER;
        else {
            const int nb = (int)it->second.size();
            for (int i = 0; i < std::min(nb, cap); i++) out[i] = it->second[i];
            *n = nb;
        }
    }
    if (tracing()) trace(e, "tw_ticket_shift_bands ticket=%lld cap=%d -> %s", (long long)t, cap, status_name(r));
    return r;
}
// The stage entry on the CPU: the global record and the bands of the caller's pair (no guards to check: nothing is launched)
tw_status tw_stage_shift_bands(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h, int radius,
                               int band, int, uint16_t* sig, tw_shift* global, tw_shift_band* bands, int* n_bands)
{
    if (!e || !expect || !target || !global || !bands || !n_bands || radius < 1 || radius > 1024) return TW_E_BAD_PARAMETER;
    if (band < 32 || band > 1024 || band % 16 != 0 || w < 1 || h < 1 || stride < w) return TW_E_BAD_PARAMETER;
    *global = stub_shift(expect, target, w, h, stride, radius);
    const std::vector<tw_shift_band> bd = stub_bands(expect, target, w, h, stride, radius, band, global->dx, sig);
    for (size_t i = 0; i < bd.size(); i++) bands[i] = bd[i];
    *n_bands = (int)bd.size();
    return TW_OK;
}
// (a pure host function in the library too; the stub launches nothing: the LDS decision and the grids are the library's rule)
int tw_debug_band_plan(int width, int height, int radius, int band, int* out, int n)
{
    if (!out || width < 1 || height < 1 || radius < 1 || radius > 1024 || band < 32 || band > 1024 || band % 16 != 0) return 0;
    const int nblk = (width + 63) / 64, rows = std::min(band, height), r = std::min(radius, height / 2);
    const long long bytes = 2ll * nblk * (rows + std::min(height, rows + 2 * r));
    const int v[9] = {(height + band - 1) / band, nblk, bytes <= 96 * 1024 ? 1 : 0, (int)std::min(bytes, 2147483647ll), 96 * 1024, r,
                      (int)(((long long)height * nblk + 255) / 256), 1024, (height + 15) / 16};
    const int m = std::max(0, std::min(n, 9));
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
}
// The diff image calls; neither consumes the ticket.  tw_ticket_hits echoes the count the ticket's tw_wait will give; a pair
// whose tw_wait will answer a bad palette index answers it here too, and stays waitable.  The stub renders nothing:
// tw_ticket_overlay writes pixel (x, y) as (x & 255, y & 255, tol) into host memory, the bytes behind a row untouched.
static tw_status stub_ticket_state(tw_engine* e, tw_ticket t, int* width, int* height, int* count)
{
    std::lock_guard<std::mutex> lk(e->m);
    auto op = e->open.find(t);
    if (op == e->open.end()) return TW_E_BAD_PARAMETER;
    auto bad = e->bad.find(t);
    if (bad != e->bad.end()) {
        e->err = "bad palette index in the " + bad->second + " image";
        return TW_E_BAD_IMAGE_FORMAT;
    }
    auto in = e->info.find(t);
    if (width) *width = in != e->info.end() ? in->second.w : 0;
    if (height) *height = in != e->info.end() ? in->second.h : 0;
    if (count) *count = op->second >= 1000000 ? 1 : 0;
    return TW_OK;
}
tw_status tw_ticket_hits(tw_engine* e, tw_ticket t, int* n)
{
    if (!e || !n) return TW_E_BAD_PARAMETER;
    int count = 0;
    const tw_status r = stub_ticket_state(e, t, nullptr, nullptr, &count);
    if (r == TW_OK) *n = count;
    if (tracing()) trace(e, "tw_ticket_hits ticket=%lld -> %s count=%d", (long long)t, status_name(r), count);
    return r;
}
tw_status tw_ticket_overlay(tw_engine* e, tw_ticket t, int tol, const tw_overlay_out* out)
{
    if (!e) return TW_E_BAD_PARAMETER;
    int w = 0, h = 0;
    tw_status r = TW_OK;
    if (!out || !out->data || out->format != TW_OVERLAY_RGB8 || tol < 0 || tol > 255) r = TW_E_BAD_PARAMETER;
    if (r == TW_OK) r = stub_ticket_state(e, t, &w, &h, nullptr);
    if (r == TW_OK && out->pitch < 3 * (ptrdiff_t)w) r = TW_E_BAD_PARAMETER;
    if (r == TW_OK)
        for (int y = 0; y < h; y++) {
            uint8_t* row = (uint8_t*)out->data + (ptrdiff_t)y * out->pitch;
            for (int x = 0; x < w; x++) row[3 * x] = (uint8_t)(x & 255), row[3 * x + 1] = (uint8_t)(y & 255), row[3 * x + 2] = (uint8_t)tol;
        }
    if (tracing()) trace(e, "tw_ticket_overlay ticket=%lld tol=%d -> %s %dx%d", (long long)t, tol, status_name(r), w, h);
    return r;
}
}
