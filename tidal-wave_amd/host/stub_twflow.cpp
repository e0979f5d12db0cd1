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
// What "differs" means changed with tw_submit_png: the consumer sends every half-decoded pair through it, and the stub
// finishes both images with the host layer's own code (one allocation and copy per image) and compares the GRAY of pixel
// 0, where tw_submit_png8 compares the first raw sample of the filtered rows.  Two RGBA files with equal R bytes and
// different grays (or the reverse) therefore answer differently through the two calls; the suite's fixtures do not.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    std::string err;
    tw_ticket next = 1;
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
static std::atomic<uintptr_t> g_next_image{0x1000};

extern "C" {
void tw_default_params(tw_params* p)
{
    p->pyrScale = 0.5; p->pyrLevels = 3; p->winSize = 30; p->pyrIterations = 3; p->polyN = 7; p->polySigma = 1.5; p->flags = 256;
}
int tw_device_count(void)
{
    const char* ev = getenv("TW_STUB_DEVICES");
    return ev ? atoi(ev) : 8;
}
// TW_STUB_PCI="0000:01:00.0,0000:81:00.0,...": bus id of pretend device i (cycled); unset: "0000:<i>0:00.0"
tw_status tw_device_pci_bus_id(int device, char* buf, int cap)
{
    if (!buf || cap < 16 || device < 0 || device >= tw_device_count()) return TW_E_DEVICE;
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
tw_status tw_host_alloc(tw_engine*, size_t bytes, void** hptr)
{
    *hptr = malloc(bytes);
    return *hptr ? TW_OK : TW_E_NOMEM;
}
tw_status tw_host_free(tw_engine*, void* hptr)
{
    free(hptr);
    return TW_OK;
}
tw_status tw_set_option(tw_engine*, int, int) { return TW_OK; }
tw_status tw_prof_select(tw_engine*, int, int) { return TW_OK; }
tw_status tw_prof_read(tw_engine*, int, double* ms, int* n)
{
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
int tw_grid_capacity(int w, int h, int span) { return span > 0 ? ((h + span - 1) / span) * ((w + span - 1) / span) : 0; }
tw_status tw_engine_create(int device, const tw_params*, int slots, tw_engine** out)
{
    tw_engine* e = new tw_engine();
    e->device = device;
    e->cap = slots;
    if (const char* ev = getenv("TW_STUB_BATCH_MS")) e->batch_ms = atof(ev);
    g_engines++;
    *out = e;
    return TW_OK;
}
void tw_engine_destroy(tw_engine* e)
{
    g_engines--;
    delete e;
}
tw_status tw_submit_u8(tw_engine* e, const uint8_t* a, const uint8_t* b, int w, int h, ptrdiff_t, int, double, tw_ticket* t)
{
    if (!a || !b || w < 1 || h < 1) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    *t = e->next++;
    e->open[*t] = w + (a[0] != b[0] ? 1000000 : 0);
    e->info[*t] = tw_engine::PairInfo{w, h, {a[0], b[0]}};
    if (e->batch_ms > 0) {
        e->batch_of[*t] = e->cur_batch;
        if (++e->cur_count >= e->cap) e->launch_locked();  // a full batch starts by itself, like the engine's
    }
    return TW_OK;
}
tw_status tw_submit_png8(tw_engine* e, const uint8_t* a, int cha, const uint8_t* b, int chb, int w, int h, int span, double thr,
                         tw_ticket* t)
{
    // filtered rows: byte 0 is a filter type, byte 1 the first sample — compare those like tw_submit_u8 compares pixel 0
    return tw_submit_u8(e, a + (cha ? 1 : 0), b + (chb ? 1 : 0), w, h, w, span, thr, t);
}
// the _sized calls: OpticalFlow::calculate's size rule, then what tw_submit_u8 / tw_submit_png8 do
static bool stub_sizes_match(int w, int h, int tw, int th) { return abs(w - tw) <= 5 && abs(h - th) <= 5; }
tw_status tw_submit_u8_sized(tw_engine* e, const uint8_t* a, int w, int h, ptrdiff_t stride, const uint8_t* b, int tw, int th,
                             ptrdiff_t tstride, int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    if (tw < 1 || th < 1 || tstride < tw) return TW_E_BAD_PARAMETER;
    if (!stub_sizes_match(w, h, tw, th)) return TW_E_DONT_MATCH_SIZE;
    return tw_submit_u8(e, a, b, w, h, stride, span, thr, t);
}
tw_status tw_submit_png8_sized(tw_engine* e, const uint8_t* a, int cha, int w, int h, const uint8_t* b, int chb, int tw, int th,
                               int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    if (tw < 1 || th < 1) return TW_E_BAD_PARAMETER;
    if (!stub_sizes_match(w, h, tw, th)) return TW_E_DONT_MATCH_SIZE;
    return tw_submit_png8(e, a, cha, b, chb, w, h, span, thr, t);
}
// the same table as the library's
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
// tw_submit_png: each image is finished to gray with the host layer's own code, then the pair is what tw_submit_u8 sees.
// A palette index without an entry is remembered for the ticket: tw_wait answers it, as the engine's does.
tw_status tw_submit_png(tw_engine* e, const tw_png_rows* a, const tw_png_rows* b, int span, double thr, const tw_flow_in*,
                        const tw_flow_out*, tw_ticket* t)
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
    const tw_status r = tw_submit_u8(e, &first[0], &first[1], a->width, a->height, a->width, span, thr, t);
    if (r == TW_OK && bad) {
        std::lock_guard<std::mutex> lk(e->m);
        e->bad[*t] = bad;
    }
    return r;
}
// tw_submit_jpeg: the first gray pixel of a coefficient image is the host layer's own inverse DCT of its block 0, then the
// pair is what tw_submit_u8 sees
tw_status tw_submit_jpeg(tw_engine* e, const tw_jpeg_luma* a, const tw_jpeg_luma* b, int span, double thr, const tw_flow_in*,
                         const tw_flow_out*, tw_ticket* t)
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
    return tw_submit_u8(e, &first[0], &first[1], a->width, a->height, a->width, span, thr, t);
}
// Resident images: the first gray pixel of the pair's image as tw_submit_u8 saw it (a palette image the finisher refused
// has pixel 0 = 0: undefined content, as the engine's header says)
tw_status tw_image_keep(tw_engine* e, tw_ticket t, int which, tw_image** out)
{
    if (!e || !out) return TW_E_BAD_PARAMETER;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(e->m);
    auto it = e->info.find(t);
    if (it == e->info.end() || which < 0 || which > 1) return TW_E_BAD_PARAMETER;
    *out = (tw_image*)g_next_image.fetch_add(16);
    e->images[*out] = tw_image{it->second.w, it->second.h, it->second.first[which]};
    g_res_kept++;
    return TW_OK;
}
tw_status tw_image_create_u8(tw_engine* e, const uint8_t* gray, int w, int h, ptrdiff_t stride, tw_image** out)
{
    if (!e || !out || !gray || w < 1 || h < 1 || stride < w) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    *out = (tw_image*)g_next_image.fetch_add(16);
    e->images[*out] = tw_image{w, h, gray[0]};
    return TW_OK;
}
tw_status tw_image_release(tw_engine* e, tw_image* img)
{
    if (!e) return TW_E_BAD_PARAMETER;
    std::lock_guard<std::mutex> lk(e->m);
    if (!e->images.erase(img)) return TW_E_BAD_PARAMETER;
    g_res_released++;
    return TW_OK;
}
tw_status tw_image_size(const tw_engine* e, const tw_image* img, int* w, int* h)
{
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
tw_status tw_submit_image_png(tw_engine* e, const tw_image* img, const tw_png_rows* b, int span, double thr, const tw_flow_in* fi,
                              const tw_flow_out* fo, tw_ticket* t)
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
    const tw_status r = tw_submit_png(e, &a, b, span, thr, fi, fo, t);
    if (r == TW_OK) g_res_image_pairs++;
    return r;
}
tw_status tw_submit_image_jpeg(tw_engine* e, const tw_image* img, const tw_jpeg_luma* b, int span, double thr, const tw_flow_in* fi,
                               const tw_flow_out* fo, tw_ticket* t)
{
    tw_image im;
    if (!stub_image_pixel(e, img, &im)) return TW_E_BAD_PARAMETER;
    tw_jpeg_luma a;
    memset(&a, 0, sizeof(a));
    a.gray = &im.first;
    a.width = im.w;
    a.height = im.h;
    const tw_status r = tw_submit_jpeg(e, &a, b, span, thr, fi, fo, t);
    if (r == TW_OK) g_res_image_pairs++;
    return r;
}
tw_status tw_submit_dev_sized(tw_engine* e, const void* a, int w, int h, ptrdiff_t stride, const void* b, int tw, int th,
                              ptrdiff_t tstride, int span, double thr, const tw_flow_in*, const tw_flow_out*, tw_ticket* t)
{
    // (the stub's "device memory" is host memory: tw_submit_u8 reads pixel 0 of both)
    return tw_submit_u8_sized(e, (const uint8_t*)a, w, h, stride, (const uint8_t*)b, tw, th, tstride, span, thr, nullptr, nullptr, t);
}
tw_status tw_flush(tw_engine* e)
{
    if (e->batch_ms > 0) {
        std::lock_guard<std::mutex> lk(e->m);
        e->launch_locked();
    }
    return TW_OK;
}
tw_status tw_wait(tw_engine* e, tw_ticket t, tw_vector* out, int cap, int* n, float* seconds)
{
    int w;
    {
        std::lock_guard<std::mutex> lk(e->m);
        auto it = e->open.find(t);
        if (it == e->open.end()) return TW_E_BAD_PARAMETER;
        w = it->second;
        e->open.erase(it);
        e->info.erase(t);
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
}
