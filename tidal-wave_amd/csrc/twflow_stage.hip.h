// The per-stage entry points (tw_stage_*, twflow_debug.h) and tw_debug_png_kernel_time: one kernel, or one short chain, run
// alone on the caller's host arrays through the launchers the engine's batches use, synchronously.  The harness of the -m gpu
// stage tests.  Included at the end of twflow.hip: the same translation unit, so the launchers of its anonymous namespace are
// visible here.

namespace {
// (through the engine's page-locked bounce buffer, like tw_flow_u8: the runtime is never handed a pageable pointer for a
// pitched copy — round 4)
tw_status up_planes(tw_engine* e, float* d, int ld, long long ps, const float* h, int w, int hh, int planes)
{
    const size_t plane = (size_t)w * hh * 4;
    tw_status r = bounce_reserve(e, plane);
    if (r) return r;
    for (int c = 0; c < planes; c++) {
        memcpy(e->h_bounce, h + (size_t)c * w * hh, plane);
        TW_HIP(e, hipMemcpy2D(d + c * ps, (size_t)ld * 4, e->h_bounce, (size_t)w * 4, (size_t)w * 4, hh, hipMemcpyHostToDevice));
    }
    return TW_OK;
}
tw_status down_planes(tw_engine* e, float* h, const float* d, int ld, long long ps, int w, int hh, int planes)
{
    const size_t plane = (size_t)w * hh * 4;
    tw_status r = bounce_reserve(e, plane);
    if (r) return r;
    for (int c = 0; c < planes; c++) {
        TW_HIP(e, hipMemcpy2D(e->h_bounce, (size_t)w * 4, d + c * ps, (size_t)ld * 4, (size_t)w * 4, hh, hipMemcpyDeviceToHost));
        memcpy(h + (size_t)c * w * hh, e->h_bounce, plane);
    }
    return TW_OK;
}

// One stage call.  An entry point checks its own arguments, opens the stage on the engine and a size, takes its device memory
// from it — scoped; the first failure of an allocation, a fill or an upload sticks in `status` and turns what follows into
// nothing, so `status` is asked once, in front of the launch — launches on `st`, finishes and reads back.
struct Stage {
    tw_engine* e;
    hipStream_t st = nullptr;
    int w = 0, h = 0, ld = 0;  // the size, and the level layout of a w x h plane: rows ld floats apart, planes ps floats
    long long ps = 0;
    tw_status status = TW_OK;
    Tmp t;

    explicit Stage(tw_engine* e_) : e(e_) {}

    // open() in two steps, for an entry point that checks more of its arguments between them
    tw_status size(int w_, int h_)
    {
        TW_TRY(check_dims(e, w_, h_));
        w = w_, h = h_, ld = round_up(w_, 32), ps = (long long)ld * h_;
        return TW_OK;
    }
    tw_status device()
    {
        TW_HIP(e, hipSetDevice(e->device));
        st = e->stream;
        return TW_OK;
    }
    tw_status open(int w_, int h_)
    {
        TW_TRY(size(w_, h_));
        return device();
    }

    template <typename T>
    T* alloc(size_t n)
    {
        T* p = status == TW_OK ? t.alloc<T>(n) : nullptr;
        if (!p && status == TW_OK) status = TW_E_NOMEM;
        return p;
    }
    // n elements set to `byte` in front of the launches, on their stream: what no launch writes reads back as that
    template <typename T>
    T* guarded(size_t n, int byte = 0xff)
    {
        T* p = alloc<T>(n);
        if (status == TW_OK) status = set_bytes(p, byte, n * sizeof(T));
        return p;
    }
    tw_status set_bytes(void* p, int byte, size_t bytes)
    {
        TW_HIP(e, hipMemsetAsync(p, byte, bytes, st));
        return TW_OK;
    }
    // n elements, the first `bytes` bytes from the host
    template <typename T>
    T* from_host(size_t n, const void* src, size_t bytes)
    {
        T* p = alloc<T>(n);
        fill(p, src, bytes);
        return p;
    }
    void fill(void* d, const void* src, size_t bytes) { status = status ? status : h2d_sync(e, d, src, bytes); }
    // n planes in the level layout, filled from the host's dense w x h planes when there are any
    float* planes(int n, const float* host = nullptr)
    {
        float* p = alloc<float>((size_t)ps * n);
        if (host) up(p, host, n);
        return p;
    }
    void up(float* d, const float* host, int n) { status = status ? status : up_planes(e, d, ld, ps, host, w, h, n); }
    // R0's five planes and R1's behind them, as the kernels of a level read them
    float* planes_R(const float* R0_5, const float* R1_5)
    {
        float* p = planes(10);
        up(p, R0_5, 5);
        up(p + 5 * ps, R1_5, 5);
        return p;
    }

    tw_status finish()
    {
        TW_HIP(e, hipGetLastError());
        TW_HIP(e, hipStreamSynchronize(st));
        return TW_OK;
    }
    tw_status down(float* host, const float* d, int n) { return down_planes(e, host, d, ld, ps, w, h, n); }
    tw_status read(void* host, const void* d, size_t bytes) { return d2h_sync(e, host, d, bytes); }
};

// The pyramid stage entry points: upload the image and the one-entry pointer table the kernels read it through, run `launch`
// (table, device planes) into one plane per entry of `levels`, and download them to `out`.
template <size_t N, typename F>
tw_status run_pyr_stage(Stage& s, const Plan* pl, const uint8_t* img, const int (&levels)[N], float* const (&out)[N], F launch)
{
    tw_engine* e = s.e;
    uint8_t* d_img = s.from_host<uint8_t>((size_t)s.w * s.h, img, (size_t)s.w * s.h);
    float* d_I[N];
    for (size_t i = 0; i < N; i++) d_I[i] = s.alloc<float>((size_t)pl->lv[levels[i]].ps);
    const uint8_t* hp = d_img;
    const uint8_t** d_tab = s.from_host<const uint8_t*>(1, &hp, sizeof(hp));
    TW_TRY(s.status);
    launch(s.st, d_tab, d_I);  // (every launch with aligned4 = 1: a hipMalloc'ed image; the kernel itself checks stride % 4)
    TW_TRY(s.finish());
    for (size_t i = 0; i < N; i++) {
        const LevelPlan& L = pl->lv[levels[i]];
        TW_TRY(down_planes(e, out[i], d_I[i], L.ld, L.ps, L.w, L.h, 1));
    }
    return TW_OK;
}
// The coarser level's flow (pw x ph) and the resize tables to the stage's level, uploaded: TW_E_UNSUPPORTED for an area-fast
// resize, which no kernel upsamples
tw_status stage_flow_ups(Stage& s, const float* prev2, int pw, int ph, FlowUps* ups)
{
    const int w = s.w, h = s.h;
    ResizeTab u;
    make_resize_tab(pw, ph, w, h, u);
    if (u.mode == 2) return TW_E_UNSUPPORTED;
    const int pld = round_up(pw, 32);
    const long long pps = (long long)pld * ph;
    float* d_p = s.alloc<float>(pps * 2);
    if (s.status == TW_OK) s.status = up_planes(s.e, d_p, pld, pps, prev2, pw, ph, 2);
    int* d_xo = s.from_host<int>(w, u.xofs.data(), (size_t)w * 4);
    int* d_yo = s.from_host<int>(h, u.yofs.data(), (size_t)h * 4);
    float* d_al = s.from_host<float>(2 * (size_t)w, u.alpha.data(), (size_t)w * 8);
    float* d_be = s.from_host<float>(2 * (size_t)h, u.beta.data(), (size_t)h * 8);
    *ups = FlowUps{d_p, pw, ph, pld, pps, d_xo, d_yo, d_al, d_be, u.xmax, (float)(1. / s.e->cfg.p.pyrScale)};
    return s.status;
}
// The shift stage entry points give every output the pair's share and one more behind it, set to 0xff, which no launch may
// touch: is the share at p still that?
bool still_ff(const void* p, size_t bytes)
{
    for (size_t i = 0; i < bytes; i++)
        if (((const unsigned char*)p)[i] != 0xff) return false;
    return true;
}
// What run_shift_stage leaves on the host.
struct ShiftStage {
    size_t P = 0;                 // a pair's profile words: 2 (w + h)
    std::vector<unsigned> hprof;  // [2][P]: the pair's share, the guard share
    ShiftRec hrec[2];             // likewise
};
// Both images as they are, rows `stride` apart (the last row ends at its last pixel), each at a 256-byte boundary, behind their
// pointer table; the guarded profiles and records; launch_shift_estimate and then behind(stream, table, records) — the
// caller's further launches — under one scope; the profiles and the records read back.
template <typename F>
tw_status run_shift_stage(Stage& s, ShiftStage& o, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int radius,
                          int force_global, F behind)
{
    tw_engine* e = s.e;
    const int w = s.w, h = s.h;
    const size_t ibytes = (size_t)(h - 1) * (size_t)stride + (size_t)w, slot = (ibytes + 255) / 256 * 256;
    const size_t P = o.P = 2 * ((size_t)w + h);
    uint8_t* d_img = s.from_host<uint8_t>(2 * slot, expect, ibytes);
    s.fill(d_img + slot, target, ibytes);
    const uint8_t* hp[2] = {d_img, d_img + slot};
    const uint8_t** d_ptrs = s.from_host<const uint8_t*>(2, hp, sizeof(hp));
    unsigned* d_prof = s.guarded<unsigned>(2 * P);
    ShiftRec* d_rec = s.guarded<ShiftRec>(2);
    TW_TRY(s.status);
    hipStream_t st = s.st;
    {
        // (tw_prof_select(TW_K_SCAN): these launches alone, for measurements)
        ProfScope pscope(e, st, TW_K_SCAN, 0);
        TW_TRY(launch_shift_estimate(e, st, d_ptrs, (long long)stride, stride % 4 == 0 ? 1 : 0, w, h, radius, force_global != 0,
                                     d_prof, d_rec, nullptr, 1));
        TW_TRY(behind(st, d_ptrs, d_rec));
    }
    TW_TRY(s.finish());
    o.hprof.resize(2 * P);
    TW_TRY(s.read(o.hprof.data(), d_prof, 2 * P * sizeof(unsigned)));
    return s.read(o.hrec, d_rec, sizeof(o.hrec));
}
// What tw_stage_span_scan and tw_stage_hit_regions start with: the fields of npairs pairs (two dense w x h planes each) in level
// 0's layout, which is the stage's, one behind the other, and the grids, records and counts of their scan — with `guard` the
// records and the counts set to 0xff bytes: a count the scan did not store reads back as -1, a record it did not write as four
// 0xffffffff words
struct ScanStage {
    const LevelPlan* L;
    int gw, gh;
    size_t nrec;  // the records of all pairs: a pair's whole grid each
    float* d_f;
    float2* d_g;
    ScanRec* d_rec;
    int* d_cnt;
};
tw_status open_scan_stage(Stage& s, ScanStage& o, const float* fields, int npairs, int span, bool guard)
{
    Plan* pl = nullptr;
    TW_TRY(get_plan(s.e, s.w, s.h, &pl));
    o.L = &pl->lv[0];
    o.gw = (s.w + span - 1) / span, o.gh = (s.h + span - 1) / span;
    o.nrec = (size_t)o.gw * o.gh * (size_t)npairs;
    o.d_f = s.planes(2 * npairs);
    o.d_g = s.alloc<float2>(o.nrec);
    o.d_rec = guard ? s.guarded<ScanRec>(o.nrec) : s.alloc<ScanRec>(o.nrec);
    o.d_cnt = guard ? s.guarded<int>(npairs) : s.alloc<int>(npairs);
    for (int j = 0; j < npairs; j++) s.up(o.d_f + (size_t)j * 2 * s.ps, fields + (size_t)j * 2 * s.w * s.h, 2);
    return TW_OK;
}
// the gather and the scan as a batch of these pairs launches them; the scan's arguments
ScanArgs launch_scan_stage(Stage& s, const ScanStage& o, int npairs, int span, double threshold, bool single_pair)
{
    launch_span_gather(s.e, s.st, o.d_f, *o.L, span, o.gw, o.gh, o.d_g, npairs);
    const ScanArgs a = scan_args(o.d_g, span, o.gw, o.gh, threshold * threshold, o.d_cnt, o.d_rec, o.d_f, o.L->ps, o.L->ld);
    launch_scan(s.e, s.st, a, choose_scan(npairs, single_pair, o.gw, o.gh, BatchSwitches().scan_seg), npairs);
    return a;
}
}  // namespace

extern "C" {

tw_status tw_stage_pyr_level(tw_engine* e, const uint8_t* img, int w0, int h0, int level, float* I, int* w, int* h)
{
    if (!e || !img || !I) return TW_E_BAD_PARAMETER;
    Stage s(e);
    Plan* pl = nullptr;
    TW_TRY(s.open(w0, h0));
    TW_TRY(get_plan(e, w0, h0, &pl));
    if (level < 0 || level > pl->levels) return TW_E_BAD_PARAMETER;
    const int levels[1] = {level};
    float* const out[1] = {I};
    TW_TRY(run_pyr_stage(s, pl, img, levels, out, [&](hipStream_t st, const uint8_t** d_tab, float* const* d_I) {
        launch_pyr(e, st, pl, level, d_tab, w0, 1, d_I[0], 1);
    }));
    if (w) *w = pl->lv[level].w;
    if (h) *h = pl->lv[level].h;
    return TW_OK;
}

tw_status tw_stage_pyr_fused23(tw_engine* e, const uint8_t* img, int w0, int h0, float* I3, float* I2)
{
    if (!e || !img || !I3 || !I2) return TW_E_BAD_PARAMETER;
    Stage s(e);
    Plan* pl = nullptr;
    TW_TRY(s.open(w0, h0));
    TW_TRY(get_plan(e, w0, h0, &pl));
    if (!pl->fused23) {
        e->err = "tw_stage_pyr_fused23: levels 2 and 3 of this size are not exact reductions by 4 and 8";
        return TW_E_UNSUPPORTED;
    }
    const int levels[2] = {3, 2};
    float* const out[2] = {I3, I2};
    return run_pyr_stage(s, pl, img, levels, out, [&](hipStream_t st, const uint8_t** d_tab, float* const* d_I) {
        launch_pyr23(e, st, pl, d_tab, w0, 1, d_I[0], d_I[1], 1);
    });
}

tw_status tw_stage_pyr_fused01(tw_engine* e, const uint8_t* img, int w0, int h0, float* I0, float* I1)
{
    if (!e || !img || !I0 || !I1) return TW_E_BAD_PARAMETER;
    Stage s(e);
    Plan* pl = nullptr;
    TW_TRY(s.open(w0, h0));
    TW_TRY(get_plan(e, w0, h0, &pl));
    if (!pyr01_fusable(pl)) {
        e->err = "tw_stage_pyr_fused01: level 1 of this size / these parameters is not an exact halving with 3-tap smoothing";
        return TW_E_UNSUPPORTED;
    }
    const int levels[2] = {0, 1};
    float* const out[2] = {I0, I1};
    return run_pyr_stage(s, pl, img, levels, out, [&](hipStream_t st, const uint8_t** d_tab, float* const* d_I) {
        launch_pyr01(e, st, pl, d_tab, w0, 1, d_I[1], d_I[0], 1);
    });
}

// one image through tw_png_unfilter, synchronously (lut: the 256 gray values of a table kind, else null)
// (iters > 0: the launch is repeated that many times between two events and *avg_us is the time of one; gray may be null)
static tw_status stage_png(tw_engine* e, const uint8_t* rows, int w, int h, const PngKind& k, const uint8_t* lut, int waves,
                           uint8_t* gray, int iters = 0, float* avg_us = nullptr)
{
    Stage s(e);
    TW_TRY(s.open(w, h));
    const size_t nb = png_rows_bytes(w, h, k.ch, k.bits);
    for (int y = 0; y < h; y++)
        if (rows[(size_t)y * png_row_bytes(w, k.ch, k.bits)] > 4) {
            e->err = "bad PNG filter type";
            return TW_E_BAD_IMAGE_FORMAT;
        }
    // (waves 0 is launch_png_unfilter's choice by the width, which always fits)
    if (waves != 0 && ((waves != 1 && waves != 4 && waves != 16) || w > PNG_LDS_PIXELS / waves)) return TW_E_BAD_PARAMETER;
    uint8_t* d_rows_raw = s.alloc<uint8_t>(nb + 512);  // the kernel may read a few bytes before / after the rows
    uint8_t* d_rows = d_rows_raw ? d_rows_raw + 256 : nullptr;
    uint8_t* d_gray = s.alloc<uint8_t>(staged_image_bytes(w, h));
    PngJob* d_job = s.alloc<PngJob>(1);
    unsigned* d_tab = lut ? s.alloc<unsigned>(1 + 64) : nullptr;  // the flag word, then the gray table
    s.fill(d_rows, rows, nb);
    unsigned h_tab[1 + 64] = {0u};
    if (lut) {
        memcpy(h_tab + 1, lut, 256);
        s.fill(d_tab, h_tab, sizeof(h_tab));
    }
    const PngJob pj{d_rows, d_gray, k.ch, k.bits, lut ? (const uint8_t*)(d_tab + 1) : nullptr, d_tab, k.entries, 0};
    s.fill(d_job, &pj, sizeof(pj));
    TW_TRY(s.status);
    const PngArgs pa{d_job, w, h};
    hipStream_t st = s.st;
    launch_png_unfilter(e, st, pa, 1, waves);
    TW_TRY(s.finish());
    if (iters > 0 && avg_us) {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        TW_HIP(e, hipEventCreate(&ev0));
        if (hipEventCreate(&ev1) != hipSuccess) {
            (void)hipEventDestroy(ev0);
            return TW_E_DEVICE;
        }
        hipError_t he = hipEventRecord(ev0, st);
        for (int i = 0; i < iters; i++) launch_png_unfilter(e, st, pa, 1, waves);
        if (he == hipSuccess) he = hipEventRecord(ev1, st);
        if (he == hipSuccess) he = hipEventSynchronize(ev1);
        float ms = 0.f;
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, ev0, ev1);
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
        TW_HIP(e, he);
        *avg_us = ms * 1e3f / (float)iters;
    }
    if (gray) TW_TRY(s.read(gray, d_gray, (size_t)w * h));
    if (lut) {
        TW_TRY(s.read(h_tab, d_tab, sizeof(unsigned)));
        if (h_tab[0]) {
            e->err = "bad palette index";
            return TW_E_BAD_IMAGE_FORMAT;
        }
    }
    return TW_OK;
}

tw_status tw_stage_png_unfilter(tw_engine* e, const uint8_t* rows, int channels, int w, int h, int waves, uint8_t* gray)
{
    if (!e || !rows || !gray || channels < 1 || channels > 4) return TW_E_BAD_PARAMETER;
    PngKind k;
    k.ch = channels;
    return stage_png(e, rows, w, h, k, nullptr, waves, gray);
}

// ... an image as tw_submit_png takes it
static tw_status stage_png_image(tw_engine* e, const tw_png_rows* img, int waves, uint8_t* gray, int iters = 0, float* avg_us = nullptr)
{
    e->err.clear();
    PngKind k;
    uint8_t lut[256];
    TW_TRY(describe_png(e, img, "the", &k, lut));
    if (k.ch == 0) return TW_E_BAD_PARAMETER;  // (a plain gray image has nothing to decode)
    return stage_png(e, img->rows, img->width, img->height, k, k.table ? lut : nullptr, waves, gray, iters, avg_us);
}

tw_status tw_debug_png_kernel_time(tw_engine* e, const tw_png_rows* img, int waves, int iters, float* avg_us)
{
    if (!e || !avg_us || iters < 1) return TW_E_BAD_PARAMETER;
    return stage_png_image(e, img, waves, nullptr, iters, avg_us);
}

tw_status tw_stage_png_decode(tw_engine* e, const tw_png_rows* img, int waves, uint8_t* gray)
{
    if (!e || !gray) return TW_E_BAD_PARAMETER;
    return stage_png_image(e, img, waves, gray);
}

tw_status tw_stage_resize_u8(tw_engine* e, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh)
{
    if (!e || !src || !dst) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(sw, sh));
    TW_TRY(check_dims(e, dw, dh));
    if (std::abs(sw - dw) > 5 || std::abs(sh - dh) > 5) {
        e->err = "Don't match image size";
        return TW_E_DONT_MATCH_SIZE;
    }
    TW_TRY(s.device());
    uint8_t* d_src = s.from_host<uint8_t>(staged_image_bytes(sw, sh), src, (size_t)sw * sh);
    uint8_t* d_dst = s.alloc<uint8_t>(staged_image_bytes(dw, dh));
    const ResizeJob rj = resize_job(d_src, sw, sh, sw, d_dst, dw, dh, dw);
    ResizeJob* d_job = s.from_host<ResizeJob>(1, &rj, sizeof(rj));
    TW_TRY(s.status);
    const ResizeArgs ra{d_job};
    TW_LAUNCH(e, TW_DF_RESIZE_U8, tw_resize_u8, dim3((dw + 255) / 256, (dh + RSZ_ROWS - 1) / RSZ_ROWS, 1), dim3(64, RSZ_ROWS),
              0, s.st, ra);
    TW_TRY(s.finish());
    return s.read(dst, d_dst, (size_t)dw * dh);
}

tw_status tw_stage_jpeg_idct(tw_engine* e, const tw_jpeg_luma* img, uint8_t* gray, uint8_t* guard)
{
    if (!e || !gray) return TW_E_BAD_PARAMETER;
    e->err.clear();
    TW_TRY(check_jpeg_luma(img));
    if (!img->coef) return TW_E_BAD_PARAMETER;  // (a plain gray image has nothing to decode)
    const int w = img->width, h = img->height;
    Stage s(e);
    TW_TRY(s.open(w, h));
    const size_t ncoef = (size_t)img->blocks_w * (size_t)img->blocks_h * 64, npx = (size_t)w * h;
    int16_t* d_coef = s.from_host<int16_t>(ncoef, img->coef, ncoef * sizeof(int16_t));
    uint8_t* d_raw = s.guarded<uint8_t>(npx + 512, 0xA5);  // 256 guard bytes on either side of the image
    // the job, and the quantisation table behind it
    char h_tab[sizeof(JpegJob) + 128];
    char* d_tab = s.alloc<char>(sizeof(h_tab));
    const JpegJob jj{d_coef, d_raw + 256, (const uint16_t*)(d_tab + sizeof(JpegJob)), w, h, img->blocks_w, 0};
    memcpy(h_tab, &jj, sizeof(jj));
    memcpy(h_tab + sizeof(JpegJob), img->quant, 128);
    s.fill(d_tab, h_tab, sizeof(h_tab));
    TW_TRY(s.status);
    const JpegArgs ja{(const JpegJob*)d_tab};
    TW_LAUNCH(e, TW_DF_JPEG_IDCT, tw_jpeg_idct, jpeg_idct_grid(w, h, 1), dim3(8 * JPEG_WG_BLOCKS), 0, s.st, ja);
    TW_TRY(s.finish());
    TW_TRY(s.read(gray, d_raw + 256, npx));
    if (guard) {
        TW_TRY(s.read(guard, d_raw, 256));
        TW_TRY(s.read(guard + 256, d_raw + 256 + npx, 256));
    }
    return TW_OK;
}

tw_status tw_stage_mask_rects(tw_engine* e, const uint8_t* expect, const uint8_t* target, int w, int h, const tw_rect* ignore,
                              int n_ignore, uint8_t* out, uint8_t* guard)
{
    if (!e || !expect || !target || !out) return TW_E_BAD_PARAMETER;
    e->err.clear();
    Stage s(e);
    TW_TRY(s.size(w, h));
    std::vector<tw_rect> ign;
    TW_TRY(clip_ignore(e, ignore, n_ignore, w, h, &ign));
    TW_TRY(s.device());
    // the two images as a batch places them: 256-byte aligned slots of staged_image_bytes, dense rows of w bytes
    const size_t npx = (size_t)w * h, slot = staged_image_bytes(w, h);
    uint8_t* d_exp = s.guarded<uint8_t>(slot, 0xA5);
    uint8_t* d_raw = s.guarded<uint8_t>(slot + 512, 0xA5);  // 256 guard bytes on either side of the target's slot, and its padding
    MaskJob* d_tab = s.alloc<MaskJob>(TW_MAX_IGNORE);
    TW_TRY(s.status);
    hipStream_t st = s.st;
    TW_HIP(e, hipStreamSynchronize(st));  // (the fill is in front of the images, and of the launch)
    s.fill(d_exp, expect, npx);
    s.fill(d_raw + 256, target, npx);
    TW_TRY(s.status);
    if (!ign.empty()) {
        MaskJob h_tab[TW_MAX_IGNORE];
        int wmax = 1, hmax = 1;
        for (size_t i = 0; i < ign.size(); i++) {
            const tw_rect& r = ign[i];
            h_tab[i] = MaskJob{d_raw + 256, d_exp, r.x, r.y, r.x + r.width, r.y + r.height, (long long)w};
            wmax = std::max(wmax, r.width);
            hmax = std::max(hmax, r.height);
        }
        TW_TRY(h2d_sync(e, d_tab, h_tab, sizeof(MaskJob) * ign.size()));
        const MaskArgs ma{d_tab};
        TW_LAUNCH(e, TW_DF_MASK_RECTS, tw_mask_rects, mask_rects_grid(wmax, hmax, (int)ign.size()), dim3(64, MASK_ROWS), 0, st, ma);
        TW_TRY(s.finish());
    }
    TW_TRY(s.read(out, d_raw + 256, npx));
    // the slot's padding behind the image belongs to nobody: a byte there that is not 0xA5 was written outside the image
    std::vector<uint8_t> pad(slot - npx);
    if (!pad.empty()) TW_TRY(s.read(pad.data(), d_raw + 256 + npx, pad.size()));
    for (uint8_t b : pad)
        if (b != 0xA5) {
            e->err = "tw_mask_rects wrote the padding of the target's slot";
            return TW_E_DEVICE;
        }
    if (guard) {
        TW_TRY(s.read(guard, d_raw, 256));
        TW_TRY(s.read(guard + 256, d_raw + 256 + slot, 256));
    }
    return TW_OK;
}

tw_status tw_stage_polyexp(tw_engine* e, const float* I, int w, int h, float* R5)
{
    if (!e || !I || !R5) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.open(w, h));
    float* d_I = s.planes(1, I);
    float* d_R = s.planes(5);
    TW_TRY(s.status);
    TW_TRY(launch_polyexp(e, s.st, w, h, s.ld, s.ps, d_I, d_R, 1, -1));
    TW_TRY(s.finish());
    return s.down(R5, d_R, 5);
}

tw_status tw_stage_update_matrices(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow2, int w,
                                   int h, float* M5)
{
    if (!e || !R0_5 || !R1_5 || !flow2 || !M5) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.open(w, h));
    float *d_R = s.planes_R(R0_5, R1_5), *d_M = s.planes(5), *d_f = s.planes(2, flow2);
    TW_TRY(s.status);
    launch_upd_kernel<false>(e, s.st, w, h, 1, upd_args(d_R, d_f, d_M, w, h, s.ld, s.ps));
    TW_TRY(s.finish());
    return s.down(M5, d_M, 5);
}

tw_status tw_stage_flow_upsample_update(tw_engine* e, const float* R0_5, const float* R1_5, const float* prevflow2,
                                        int pw, int ph, int w, int h, float* flow2, float* M5)
{
    if (!e || !R0_5 || !R1_5 || !prevflow2 || !flow2 || !M5) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    TW_TRY(check_dims(e, pw, ph));
    TW_TRY(s.device());
    FlowUps ups;
    TW_TRY(stage_flow_ups(s, prevflow2, pw, ph, &ups));
    float *d_R = s.planes_R(R0_5, R1_5), *d_M = s.planes(5), *d_f = s.planes(2);
    TW_TRY(s.status);
    UpdArgs a = upd_args(d_R, d_f, d_M, w, h, s.ld, s.ps, &ups);
    a.store_flow = 1;
    launch_upd_kernel<true>(e, s.st, w, h, 1, a);
    TW_TRY(s.finish());
    TW_TRY(s.down(flow2, d_f, 2));
    return s.down(M5, d_M, 5);
}

tw_status tw_stage_blur_solve(tw_engine* e, const float* R0_5, const float* R1_5, const float* M5, int w, int h,
                              int update_matrices, float* flow2, float* Mout5)
{
    if (!e || !R0_5 || !R1_5 || !M5 || !flow2) return TW_E_BAD_PARAMETER;
    if (update_matrices && !Mout5) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.open(w, h));
    float *d_R = s.planes_R(R0_5, R1_5), *d_M = s.planes(5, M5), *d_Mo = s.planes(5), *d_f = s.planes(2);
    BlurLaunch b{w, h, s.ld, s.ps, d_M, d_Mo, d_f, d_R, update_matrices ? 1 : 0, -1, 1};
    b.store_flow = 1;  // the stage returns the flow of a refreshing launch as well
    if (e->cfg.box) b.Vbox = s.alloc<double>((size_t)s.ps * 5);  // no engine workspace here
    TW_TRY(s.status);
    launch_blur(e, s.st, b);
    TW_TRY(s.finish());
    TW_TRY(s.down(flow2, d_f, 2));
    if (update_matrices) return s.down(Mout5, d_Mo, 5);
    return TW_OK;
}

tw_status tw_stage_flow_iter(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow_in2, const float* prev2,
                             int pw, int ph, int w, int h, float* flow_out2)
{
    if (!e || !R0_5 || !R1_5 || !flow_out2 || (flow_in2 && prev2)) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    if (prev2) TW_TRY(check_dims(e, pw, ph));
    if (!flow_iter_eligible(e->cfg, w, h)) {
        e->err = "tw_stage_flow_iter: winSize 30/31 Gaussian window and a level of at least TW_MFREE_MIN_W (320) x 20 pixels";
        return TW_E_UNSUPPORTED;
    }
    TW_TRY(s.device());
    float *d_R = s.planes_R(R0_5, R1_5), *d_fi = s.planes(2, flow_in2), *d_fo = s.planes(2);
    FlowUps ups;
    if (prev2) TW_TRY(stage_flow_ups(s, prev2, pw, ph, &ups));
    TW_TRY(s.status);
    launch_flow_iter(e, s.st, w, h, s.ld, s.ps, d_R, flow_in2 ? d_fi : nullptr, s.ps, d_fo, s.ps, prev2 ? &ups : nullptr, 1, -1);
    TW_TRY(s.finish());
    return s.down(flow_out2, d_fo, 2);
}

tw_status tw_stage_flow_iter_grid(tw_engine* e, const float* R0_5, const float* R1_5, const float* flow_in2, int w, int h, int span,
                                  float* grid_out)
{
    if (!e || !R0_5 || !R1_5 || !flow_in2 || !grid_out || span < FI_TH) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    if (!flow_iter_eligible(e->cfg, w, h) || e->cfg.fi_nt != 1024) {
        e->err = "tw_stage_flow_iter_grid: winSize 30/31 Gaussian window and a level of at least TW_MFREE_MIN_W (320) x 20 pixels";
        return TW_E_UNSUPPORTED;
    }
    TW_TRY(s.device());
    const int gw = (w + span - 1) / span, gh = (h + span - 1) / span;
    const size_t npts = (size_t)gw * gh;
    float *d_R = s.planes_R(R0_5, R1_5), *d_fi = s.planes(2, flow_in2);
    float2* d_g = s.guarded<float2>(npts);  // (0xff bytes: a point the launch did not write reads back as NaN)
    TW_TRY(s.status);
    const FlowIterGrid gp{d_g, span, gw, gh};
    launch_flow_iter(e, s.st, w, h, s.ld, s.ps, d_R, d_fi, s.ps, nullptr, s.ps, nullptr, 1, -1, nullptr, &gp);
    TW_TRY(s.finish());
    TW_HIP(e, hipMemcpy(grid_out, d_g, npts * sizeof(float2), hipMemcpyDeviceToHost));
    return TW_OK;
}

tw_status tw_stage_span_scan(tw_engine* e, const float* fields, int npairs, int w, int h, int span, double threshold, int single_pair,
                             int* counts, int* xy, float* dxy)
{
    if (!e || !fields || !counts || !xy || !dxy || npairs < 1 || span < 1 || (single_pair != 0 && single_pair != 1) ||
        (single_pair && npairs != 1))
        return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.open(w, h));
    ScanStage sc;
    TW_TRY(open_scan_stage(s, sc, fields, npairs, span, true));
    TW_TRY(s.status);
    launch_scan_stage(s, sc, npairs, span, threshold, single_pair != 0);
    TW_TRY(s.finish());
    TW_TRY(s.read(counts, sc.d_cnt, sizeof(int) * (size_t)npairs));
    std::vector<ScanRec> hr(sc.nrec);
    TW_TRY(s.read(hr.data(), sc.d_rec, sc.nrec * sizeof(ScanRec)));
    for (size_t i = 0; i < sc.nrec; i++) {
        xy[2 * i] = hr[i].x;
        xy[2 * i + 1] = hr[i].y;
        dxy[2 * i] = hr[i].dx;
        dxy[2 * i + 1] = hr[i].dy;
    }
    return TW_OK;
}

tw_status tw_stage_hit_regions(tw_engine* e, const float* fields, int npairs, int w, int h, int span, double threshold, int gap,
                               const tw_rect* ignore, const int* n_ignore, int* n_regions, tw_region* regions, int* region_of)
{
    if (!e || !fields || !n_regions || !regions || !region_of || npairs < 1 || span < 1 || gap < 1 || gap > 8 ||
        (n_ignore && !ignore))
        return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    // the table a batch uploads: per pair a count and TW_MAX_IGNORE clipped rectangles
    std::vector<char> tab(region_table_bytes(npairs), 0);
    bool any_rect = false;
    for (int j = 0; n_ignore && j < npairs; j++) {
        std::vector<tw_rect> ign;
        TW_TRY(clip_ignore(e, ignore + (size_t)j * TW_MAX_IGNORE, n_ignore[j], w, h, &ign));
        ((int*)tab.data())[j] = (int)ign.size();
        std::copy(ign.begin(), ign.end(), (tw_rect*)(tab.data() + region_rects_off(npairs)) + (size_t)j * TW_MAX_IGNORE);
        any_rect = any_rect || !ign.empty();
    }
    TW_TRY(s.device());
    ScanStage sc;
    TW_TRY(open_scan_stage(s, sc, fields, npairs, span, false));
    const size_t nregs = (size_t)TW_MAX_REGIONS * npairs;
    char* d_tab = s.from_host<char>(tab.size(), tab.data(), tab.size());
    int* d_lab = (size_t)sc.gw * sc.gh > (size_t)RGN_LDS_POINTS ? s.alloc<int>(sc.nrec) : nullptr;
    // (0xff bytes: whatever the launch did not write reads back as -1 / 0xffffffff words)
    int* d_nreg = s.guarded<int>(npairs);
    RegionRec* d_regs = s.guarded<RegionRec>(nregs);
    int* d_regof = s.guarded<int>(sc.nrec);
    TW_TRY(s.status);
    const ScanArgs a = launch_scan_stage(s, sc, npairs, span, threshold, false);
    const RegionArgs ra = region_args(a, w, h, gap, any_rect ? (const int*)d_tab : nullptr,
                                      (const int4*)(d_tab + region_rects_off(npairs)), d_lab, d_nreg, d_regs, d_regof);
    {
        // (tw_prof_select(TW_K_SCAN): this launch alone, for tools/regions_prof.py — a batch's scope holds its scan as well)
        ProfScope pscope(e, s.st, TW_K_SCAN, 0);
        TW_TRY(launch_hit_regions(e, s.st, ra, npairs));
    }
    TW_TRY(s.finish());
    TW_TRY(s.read(n_regions, d_nreg, sizeof(int) * (size_t)npairs));
    TW_TRY(s.read(regions, d_regs, sizeof(RegionRec) * nregs));
    return s.read(region_of, d_regof, sc.nrec * sizeof(int));
}

tw_status tw_stage_warp_residual(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h,
                                 const float* flow2, int span, int tol, int* cells, int* n_changes, tw_change* changes)
{
    if (!e || !expect || !target || !flow2 || !cells || !n_changes || !changes || span < 1 || tol < 1 || tol > 254)
        return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    if (stride < w) return TW_E_BAD_PARAMETER;
    TW_TRY(s.device());
    Plan* pl = nullptr;
    TW_TRY(get_plan(e, w, h, &pl));
    const LevelPlan& L = pl->lv[0];  // (its layout is the stage's)
    const int gw = (w + span - 1) / span, gh = (h + span - 1) / span;
    const size_t G = (size_t)gw * gh;
    // the pair's two slots, as a batch stages a host pair: dense rows
    const size_t npx = staged_image_bytes(w, h);
    std::vector<uint8_t> img(2 * npx, 0);
    for (int y = 0; y < h; y++) {
        memcpy(img.data() + (size_t)y * w, expect + (size_t)y * stride, (size_t)w);
        memcpy(img.data() + npx + (size_t)y * w, target + (size_t)y * stride, (size_t)w);
    }
    uint8_t* d_img = s.from_host<uint8_t>(2 * npx, img.data(), img.size());
    const uint8_t* hp[2] = {d_img, d_img + npx};
    const uint8_t** d_ptrs = s.from_host<const uint8_t*>(2, hp, sizeof(hp));
    float* d_f = s.planes(2, flow2);
    // (0xff bytes: whatever the launches did not write reads back as -1 words)
    int4* d_cells = s.guarded<int4>(G);
    int* d_cnt = s.guarded<int>(1);
    ChangeRec* d_chg = s.guarded<ChangeRec>(G);
    TW_TRY(s.status);
    {
        // (tw_prof_select(TW_K_SCAN): these two launches alone, for measurements)
        ProfScope pscope(e, s.st, TW_K_SCAN, 0);
        launch_warp_residual(e, s.st, d_ptrs, (long long)w, d_f, L, span, tol, d_cells, 1);
        launch_change_scan(e, s.st, d_cells, span, gw, gh, d_cnt, d_chg, 1);
    }
    TW_TRY(s.finish());
    TW_TRY(s.read(cells, d_cells, G * sizeof(int4)));
    TW_TRY(s.read(n_changes, d_cnt, sizeof(int)));
    return s.read(changes, d_chg, G * sizeof(ChangeRec));
}

tw_status tw_stage_shift(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h, int radius,
                         int force_global, uint32_t* profiles, tw_shift* out)
{
    if (!e || !expect || !target || !out || radius < 1 || radius > 1024) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    if (stride < w) return TW_E_BAD_PARAMETER;
    TW_TRY(s.device());
    ShiftStage stage;
    TW_TRY(run_shift_stage(s, stage, expect, target, stride, radius, force_global,
                           [](hipStream_t, const uint8_t**, ShiftRec*) { return TW_OK; }));
    if (!still_ff(stage.hprof.data() + stage.P, stage.P * sizeof(unsigned))) {
        e->err = "tw_stage_shift: a launch wrote beyond the pair's profiles";
        return TW_E_DEVICE;
    }
    if (!still_ff(&stage.hrec[1], sizeof(ShiftRec))) {
        e->err = "tw_stage_shift: a launch wrote beyond the pair's record";
        return TW_E_DEVICE;
    }
    if (profiles) memcpy(profiles, stage.hprof.data(), stage.P * sizeof(unsigned));
    to_tw_shift(stage.hrec[0], out);
    return TW_OK;
}

tw_status tw_stage_shift_bands(tw_engine* e, const uint8_t* expect, const uint8_t* target, ptrdiff_t stride, int w, int h, int radius,
                               int band, int force_global, uint16_t* sig, tw_shift* global, tw_shift_band* bands, int* n_bands)
{
    if (!e || !expect || !target || !global || !bands || !n_bands || radius < 1 || radius > 1024) return TW_E_BAD_PARAMETER;
    if (band < 32 || band > 1024 || band % 16 != 0) return TW_E_BAD_PARAMETER;
    Stage s(e);
    TW_TRY(s.size(w, h));
    if (stride < w) return TW_E_BAD_PARAMETER;
    TW_TRY(s.device());
    const int nb = band_count(h, band), nblk0 = band_blocks(w);
    const size_t S = 2 * (size_t)h * nblk0;
    // the signatures and the band records are guarded as the profiles and the pair's record are
    unsigned short* d_sig = s.guarded<unsigned short>(2 * S);
    BandRec* d_bands = s.guarded<BandRec>(2 * (size_t)nb);
    ShiftStage stage;
    TW_TRY(run_shift_stage(s, stage, expect, target, stride, radius, force_global,
                           [&](hipStream_t st, const uint8_t** d_ptrs, ShiftRec* d_rec) {
                               return launch_band_estimate(e, st, d_ptrs, (long long)stride, w, h, radius, band, force_global != 0,
                                                           d_rec, d_sig, d_bands, nullptr, 1);
                           }));
    std::vector<unsigned short> hsig(2 * S);
    std::vector<BandRec> hb(2 * (size_t)nb);
    TW_TRY(s.read(hsig.data(), d_sig, 2 * S * sizeof(unsigned short)));
    TW_TRY(s.read(hb.data(), d_bands, 2 * (size_t)nb * sizeof(BandRec)));
    if (!still_ff(stage.hprof.data() + stage.P, stage.P * sizeof(unsigned)) ||
        !still_ff(hsig.data() + S, S * sizeof(unsigned short)) || !still_ff(&stage.hrec[1], sizeof(ShiftRec)) ||
        !still_ff(&hb[nb], (size_t)nb * sizeof(BandRec))) {
        e->err = "tw_stage_shift_bands: a launch wrote beyond the pair's share";
        return TW_E_DEVICE;
    }
    // the signatures' rows are nblk apart in each image's share of h * nblk0; behind them the share is zero
    const int dx = stage.hrec[0].dx, nblk = (std::min(w, w - dx) - std::max(0, -dx) + 63) / 64;
    for (int q = 0; q < 2; q++) {
        const unsigned short* sq = hsig.data() + (size_t)q * h * nblk0;
        for (size_t i = (size_t)h * nblk; i < (size_t)h * nblk0; i++)
            if (sq[i] != 0) {
                e->err = "tw_stage_shift_bands: the rest of an image's signatures is not zero";
                return TW_E_DEVICE;
            }
        if (sig) memcpy(sig + (size_t)q * h * nblk, sq, (size_t)h * nblk * sizeof(unsigned short));
    }
    to_tw_shift(stage.hrec[0], global);
    memcpy(bands, hb.data(), (size_t)nb * sizeof(BandRec));
    *n_bands = nb;
    return TW_OK;
}

tw_status tw_stage_overlay(tw_engine* e, const uint8_t* expect, const uint8_t* target, int width, int height, ptrdiff_t stride,
                           int misalign, const tw_rect* rects, int n_rects, const tw_overlay_hit* hits, int n_hits,
                           const tw_region* regions, int n_regions, int tol, uint8_t* out, ptrdiff_t pitch, int* path)
{
    if (!e || !expect || !target || !out) return TW_E_BAD_PARAMETER;
    e->err.clear();
    Stage s(e);
    TW_TRY(s.size(width, height));
    if (stride < width || misalign < 0 || misalign > 3 || n_hits < 0 || (n_hits > 0 && !hits) || n_regions < 0 ||
        n_regions > TW_MAX_REGIONS || (n_regions > 0 && !regions) || tol < 0 || tol > 255 || pitch < 3 * (ptrdiff_t)width) {
        e->err = "tw_stage_overlay: bad argument";
        return TW_E_BAD_PARAMETER;
    }
    std::vector<tw_rect> ign;
    TW_TRY(clip_ignore(e, rects, n_rects, width, height, &ign));
    TW_TRY(s.device());
    const size_t img = (size_t)stride * (size_t)(height - 1) + (size_t)width, obytes = (size_t)pitch * (size_t)height;
    uint8_t* d_E = s.alloc<uint8_t>(img + 4);
    uint8_t* d_T = s.alloc<uint8_t>(img + 4);
    s.fill(d_E + misalign, expect, img);
    s.fill(d_T + misalign, target, img);
    uint8_t* d_out = s.from_host<uint8_t>(obytes, out, obytes);
    ScanRec* d_hits = s.from_host<ScanRec>((size_t)std::max(n_hits, 1), hits, sizeof(ScanRec) * (size_t)n_hits);
    RegionRec* d_regs = s.from_host<RegionRec>((size_t)std::max(n_regions, 1), regions, sizeof(RegionRec) * (size_t)n_regions);
    TW_TRY(s.status);
    const OverlayJob oj{d_E + misalign, d_T + misalign, (long long)stride, d_out, (long long)pitch, width, height, tol, &ign,
                        d_regs, n_regions, d_hits, n_hits};
    const int vec = launch_overlay(e, s.st, oj);
    TW_TRY(s.finish());
    if (path) *path = vec;
    return s.read(out, d_out, obytes);
}

}  // extern "C"
