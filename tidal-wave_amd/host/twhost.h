// twhost.h — C++ host layer above the C ABI: the job queue, the per-GPU consumers and the result pump of
// tidal-wave (reference: src/message_queue.h, src/consumer.{h,cpp}, src/manager.{h,cpp}), re-stated on
// std::thread / std::mutex instead of libuv primitives.  Everything device-side goes through include/twflow.h.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/twflow.h"

namespace twhost {

// An image pair that is already decoded, in the caller's memory (8-bit gray, row stride in bytes).  Not part of
// the reference's Request: the throughput driver (tools/bench_queue.cpp, BASELINE config 4) uses it to feed the
// manager queue without touching the file system.  The buffers stay valid until the pair's response arrives;
// page-locked buffers (tw_host_alloc) are DMA-ed from directly.
struct RawPair {
    const uint8_t* expect = nullptr;
    const uint8_t* target = nullptr;
    int width = 0, height = 0;
    ptrdiff_t stride = 0;
};
// An ignore rectangle of a pair, in the expected image's coordinates (tw_rect of include/twflow.h)
using Rect = tw_rect;
// /root/reference/src/message_queue.h:13-48
struct Request {
    std::string expect_image;
    std::string target_image;
    double threshold;
    int span;
    RawPair raw;  // raw.expect != nullptr: the paths above are labels only
    // not in the reference: regions of the pair that may differ.  Inside them the engine replaces the target's pixels by
    // the expected image's before the flow and reports no vector from there (the tw_submit_*_ignore calls: the device
    // applies the mask, the host layer has no implementation of it); empty: the pair goes the way it always went
    std::vector<Rect> ignore;
};
struct Vector {
    int x, y;
    double dx, dy;
};
// A region of a pair's vectors (tw_region of include/twflow.h)
using Region = tw_region;
// A cell of a pair's span grid with a differing pixel (tw_change of include/twflow.h)
using Change = tw_change;
// A pair's estimated global translation (tw_shift of include/twflow.h): the two searches' answers, and whether the pair's flow
// started from them
struct Shift {
    int x = 0, y = 0;
    bool applied = false;
};
// One band of a pair's rows and its vertical shift (tw_shift_band of include/twflow.h): the band's first row and height, the
// band search's answer, and whether the band's rows of the pair's start field were (Shift::x, dy)
struct ShiftBand {
    int y = 0, rows = 0, dy = 0;
    bool applied = false;
};
struct Response {
    std::vector<Vector> vectors;
    // not in the reference (PairExtras::shift > 0 and ::shiftBands > 0 only): the pair's bands, top to bottom
    std::vector<ShiftBand> bands;
    bool hasBands = false;
    // not in the reference (PairExtras::shift > 0 only): the pair's integer translation, estimated and checked on the device
    Shift shift;
    bool hasShift = false;
    // not in the reference (PairExtras::residual > 0 only; empty otherwise): the cells with a pixel that differs by more than
    // the tolerance, each with the number of such pixels the pair's flow does not explain
    std::vector<Change> changes;
    bool hasChanges = false;
    // not in the reference (PairExtras::regions > 0 only; empty otherwise): the vectors grouped into regions on the device —
    // the kept records (at most TW_MAX_REGIONS), per vector the index of its region, and the pair's true number of regions
    std::vector<Region> regions;
    std::vector<int> regionOf;
    int regionCount = 0;
    bool hasRegions = false;
    std::string expect_image, target_image;
    float time = 0;
    double threshold = 0;
    int span = 0;
    std::string status, reason;
    int width = 0, height = 0;
    // not in the reference (PairExtras::overlayDir set, SUSPICIOUS pairs only; empty otherwise): the path of the pair's diff
    // image, a PNG rendered on the device (tw_ticket_overlay)
    std::string overlay;
    long long pushedNs = 0;  // host-internal: when the consumer handed the response to the pump (steady clock)
};
// How long responses sat between a consumer's push and the observer's callback since the last markEpoch() — the one
// pump thread of src/manager.cpp:80-90 is where N consumers' results are serialised
struct PumpStats {
    long delivered = 0;
    double meanUs = 0, maxUs = 0;
    double busyMs = 0;  // time the pump spent inside the observer's callbacks
};
struct Report {
    int requestCount = 0, dataCount = 0, errorCount = 0;
};

// The per-pair extras, none of them in the reference: what a consumer asks of its engine for every pair beyond the vectors.
// Parameter carries them in, Manager::start copies them whole into ConsumerShared, and a consumer keeps the copy that is in
// force on its engine.  Common to all: off (the defaults) means that the calls a consumer makes are exactly the ones it made
// before the extra existed; an extra that is asked for is never silently dropped — a library without its calls, or a value
// the engine refuses, leaves the consumer without an engine and every pair answers ERROR ("engine: <field>: ...").
struct PairExtras {
    // group every pair's vectors into regions (the engine option TW_OPT_REGIONS, collected with tw_wait_regions) — 0: off;
    // 1 .. 8: the gap, in grid steps, that still joins two vectors
    int regions = 0;
    // report the changes the flow does not explain (TW_OPT_RESIDUAL, tw_ticket_changes before each collecting wait) — 0: off;
    // 1 .. 254: the tolerance in gray levels.  residualMin (0: the status rule is untouched): a pair whose change records hold
    // at least that many unexplained pixels in total is SUSPICIOUS even without a vector — a flat repaint moves nothing
    int residual = 0;
    int residualMin = 0;
    // start every pair's flow from its global integer shift, found on the device (TW_OPT_SHIFT, tw_ticket_shift behind
    // tw_ticket_changes) — 0: off; 1 .. 1024: the search radius in pixels.  Response::status is unchanged by it
    int shift = 0;
    // with `shift` on, start every pair's flow from one vertical shift per band of this many rows (TW_OPT_SHIFT_BANDS, set
    // behind TW_OPT_SHIFT; tw_ticket_shift_bands behind tw_ticket_shift) — 0: off; 32 .. 1024, a multiple of 16: the band
    // height.  Ignored while `shift` is 0
    int shiftBands = 0;
    // a directory for diff images (empty: off).  With it a consumer asks tw_ticket_hits in front of each collecting wait —
    // behind tw_ticket_changes, so that the status pair_status will give is known — and for a pair that will be SUSPICIOUS
    // renders the picture on the device (tw_ticket_overlay at tolerance overlayTol, 0 .. 255) and writes it to
    // overlay_path(overlayDir, target_image); Response::overlay carries that path.  Other pairs get no call, no file and no
    // path.  The directory must exist and be writable when the consumers start: that, like a tolerance outside 0 .. 255, is
    // a refusal ("engine: overlay: ...").  A picture that fails later (a full disk) leaves its pair's answer without the
    // path; it is logged under TW_LOG and counted in ConsumerStats::overlayFailures.
    std::string overlayDir;
    int overlayTol = 16;
};

// struct Parameter of the reference (src/manager.h): per-instance options resolved by the broker
struct Parameter {
    double threshold = 5.0;
    int span = 10;
    int numThreads = 4;
    tw_params optParam;
    // not in the reference: consumers that share one GPU (0: TW_CONSUMERS_PER_DEVICE, default 1) and the engine
    // batch of a consumer (0: 32).  The consumer count is min(numThreads, devices * perDevice).
    int consumersPerDevice = 0;
    int batch = 0;
    // bracket the level-0 window-average and polynomial-expansion launches of every consumer's engine with events
    // (tw_prof_select): the queue driver's roofline figures come from them (tools/bench_queue.cpp)
    bool profileKernels = false;
    // not in the reference: megabytes of device memory each consumer may fill with resident expected images, keyed by the
    // file's identity (0: TW_RESIDENT_MB, else off — every pair then reads, decodes and uploads both files, as before)
    int residentMB = 0;
    // not in the reference: what a consumer asks of its engine for every pair, beyond the vectors
    PairExtras extras;
};
// Where the diff image of a pair goes: <dir>/<16 hex digits of the FNV-1a-64 hash of the target_image string>-<the target's
// base name without its extension>.png — two targets of one base name in different directories do not collide.
inline std::string overlay_path(const std::string& dir, const std::string& target_image)
{
    unsigned long long hsh = 14695981039346656037ull;
    for (unsigned char c : target_image) hsh = (hsh ^ c) * 1099511628211ull;
    const size_t slash = target_image.find_last_of("/\\");
    std::string base = slash == std::string::npos ? target_image : target_image.substr(slash + 1);
    const size_t dot = base.find_last_of('.');
    if (dot != std::string::npos && dot > 0) base.resize(dot);
    static const char hex[] = "0123456789abcdef";
    std::string name(16, '0');
    for (int i = 0; i < 16; i++) name[(size_t)i] = hex[(hsh >> (60 - 4 * i)) & 15];
    return dir + "/" + name + "-" + base + ".png";
}
// Response::status of an answered pair: the reference's rule (src/consumer.cpp:77), and PairExtras::residualMin's
inline const char* pair_status(size_t nvectors, const std::vector<Change>& changes, int residualMin)
{
    if (nvectors) return "SUSPICIOUS";
    if (residualMin <= 0) return "OK";
    long long unexplained = 0;
    for (const Change& c : changes) unexplained += c.n_unexplained;
    return unexplained >= residualMin ? "SUSPICIOUS" : "OK";
}

// What one consumer did, as seen by Manager::consumerStats() (a copy; the consumer thread owns the original).
struct ConsumerStats {
    int id = 0;
    int device = -1;          // id % deviceCount, -1 without a HIP device
    bool ready = false;       // the engine exists (or could not be created: engineError says why)
    std::string engineError;
    long pairs = 0;           // responses pushed since the last Manager::markEpoch()
    long batches = 0;         // engine batches submitted since then
    long overlayFailures = 0; // diff images of SUSPICIOUS pairs that could not be rendered or written since then (PairExtras::overlayDir)
    // event-bracketed level-0 launches since then: [0] window average + solve, [1] polynomial expansion
    double profMs[2] = {0, 0};
    int profLaunches[2] = {0, 0};
    // when the consumer worked since then (std::chrono::steady_clock, nanoseconds since its epoch): pop of its first
    // job, push of its last response, and the time it sat blocked on an EMPTY request queue in between — a driver
    // that knows its own clock derives each consumer's idle time from these (tools/bench_queue.cpp)
    long long firstJobNs = 0, lastResponseNs = 0;
    double waitMs = 0;
    // placement of the consumer thread (and, by inheritance / first touch, of its decode pool and of the page-locked
    // buffers its engine allocates): NUMA node of the GPU, -1 = not bound (TW_NUMA=0, no NUMA information, or none
    // of the node's CPUs is available to this process)
    std::string pciBusId;
    int numaNode = -1;
    std::vector<int> cpus;    // CPUs the consumer thread may run on after placement
};

// NUMA node and CPU list of a device from sysfs: /sys/bus/pci/devices/<bus id>/numa_node and
// /sys/devices/system/node/node<N>/cpulist (TW_SYSFS_ROOT replaces "/sys": tests).  false: unknown.
bool numa_cpus_of_device(int device, std::string* busid, int* node, std::vector<int>* cpus);
// Restrict the calling thread to `cpus` (those of them this process may use); false if none is usable.
bool bind_this_thread(const std::vector<int>& cpus);
std::vector<int> this_thread_cpus();

// Blocking MPMC queue, MessageQueue<T> of src/message_queue.h:50-118 (stop() wakes every waiter; as in the
// reference, items still queued at stop() are dropped — Appendix B#8 of SURVEY.md).
template <typename T>
class MessageQueue {
public:
    bool tryPop(T& out)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !q_.empty() || !running_; });
        if (q_.empty() || !running_) return false;
        out = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    // non-blocking: used by a consumer to fill a GPU batch with whatever is already queued
    bool tryPopNow(T& out)
    {
        std::lock_guard<std::mutex> lk(m_);
        if (q_.empty() || !running_) return false;
        out = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    void push(T v)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            q_.push_back(std::move(v));
        }
        cv_.notify_one();
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            running_ = false;
        }
        cv_.notify_all();
    }
    size_t size()
    {
        std::lock_guard<std::mutex> lk(m_);
        return q_.size();
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool running_ = true;
};

// A JPEG after its entropy decode: the quantised luma coefficients and what the inverse DCT needs (tw_submit_jpeg runs
// it on the device, jpeg_luma_to_gray here)
struct JpegLuma {
    int w = 0, h = 0;
    int bw = 0, bh = 0;         // luma blocks stored per row and per column: whole MCUs
    uint16_t quant[64] = {0};   // luma quantisation table, natural order
    std::vector<int16_t> coef;  // bw * bh blocks, row-major, 64 quantised coefficients each, natural order
};
// JPEG (baseline / progressive Huffman, 8-bit) up to and including every refusal (jpeg_gray.cpp); `luma` is untouched on
// failure
bool decode_jpeg_luma(const uint8_t* data, size_t n, JpegLuma& luma);
// the rest: dequantisation, libjpeg's integer IDCT (jidctint), level shift, range limit and the crop to w x h
void jpeg_luma_to_gray(const JpegLuma& luma, std::vector<uint8_t>& img);
// the two in sequence: JPEG -> luma plane
bool decode_jpeg_gray(const uint8_t* data, size_t n, std::vector<uint8_t>& img, int& w, int& h);
// 8-bit gray decode of a file: PGM (P5), PNG (zlib inflate + unfilter, libpng-1.5 gray conversion) and JPEG.
// Returns false if the file cannot be opened / decoded ("Can't open <path>", src/opticalflow.cpp:40,47).
bool load_gray(const std::string& path, std::vector<uint8_t>& img, int& w, int& h);
// load_gray, or — want_rows and an 8-bit non-interlaced non-palette PNG — the inflated but still filtered scanlines
// (ch 1-4: h rows of 1 + w * ch bytes for tw_submit_png8; ch 0: `img` is the gray image)
bool load_gray_or_png_rows(const std::string& path, bool want_rows, std::vector<uint8_t>& img, int& w, int& h, int& ch);
bool finish_png_rows_on_host(std::vector<uint8_t>& rows, int w, int h, int ch, std::vector<uint8_t>& gray);
// What an image's bytes are when they are not gray pixels: the IHDR kind (and PLTE body) of inflated, still filtered PNG
// rows that tw_submit_png finishes on the device.  color_type TW_PNG_PLAIN_GRAY: gray pixels.
struct PngKind {
    int color_type = TW_PNG_PLAIN_GRAY, bit_depth = 8;
    std::vector<uint8_t> plte;
    bool rows() const { return color_type != TW_PNG_PLAIN_GRAY; }
    // bytes of one filtered row of `w` pixels, filter type byte included
    size_t row_bytes(int w) const
    {
        const size_t samples = color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 1;
        return 1 + ((size_t)w * samples * (size_t)bit_depth + 7) / 8;
    }
};
// load_gray_or_png_rows for every kind tw_png_on_device admits (palette, 1- / 2- / 4-bit and 16-bit gray, 16-bit gray +
// alpha besides the 8-bit ones; all_kinds = false: the 8-bit ones only): `img` holds the rows and `kind` says what they
// are, or the gray image (kind.rows() false).  Every row's filter type is checked at the kind's row length.
bool load_gray_or_png_kind_rows(const std::string& path, bool want_rows, bool all_kinds, std::vector<uint8_t>& img, int& w,
                                int& h, PngKind& kind);
// The rest of the decode of such rows on the host (what the device does for tw_submit_png): false for a palette index
// without an entry, as cv::imread fails on it.
bool finish_png_kind_on_host(const uint8_t* rows, int w, int h, const PngKind& kind, std::vector<uint8_t>& gray);
// cv::resize(8-bit, INTER_LINEAR) — the "<= 5 px" reconcile of src/opticalflow.cpp:64-68.
void resize_u8_linear(const std::vector<uint8_t>& src, int sw, int sh, std::vector<uint8_t>& dst, int dw, int dh);

// Observer of src/observer.h:11-18
struct Observer {
    std::function<void(const Response&)> onNext;
    std::function<void(const std::string&)> onError;
    std::function<void(const Report&)> onCompleted;
};

// Consumer (src/consumer.{h,cpp}): one worker thread bound to one GPU; pulls requests, runs the engine, pushes
// responses.  Consumer i uses device i % deviceCount; with no HIP device every job answers ERROR (the engine
// has no CPU path).
// state shared between the Manager and its consumers
struct ConsumerShared {
    std::mutex m;
    std::condition_variable cv;
    std::vector<ConsumerStats> stats;  // [consumer id]
    std::atomic<int> epoch{0};
    std::atomic<long> inflight{0};  // pairs submitted to an engine and not yet collected, over all consumers
    bool profile = false;
    long long residentBytes = 0;  // the budget of a consumer's resident expected images (0: off)
    PairExtras extras;            // Parameter::extras
};

class Consumer {
public:
    Consumer(int id, MessageQueue<Request>& req, MessageQueue<Response>& res, const tw_params& p, int batch,
             int decode_threads, int n_consumers = 1, ConsumerShared* shared = nullptr);
    ~Consumer();
    void start();
    void join();

private:
    void run();
    int id_;
    MessageQueue<Request>& req_;
    MessageQueue<Response>& res_;
    tw_params params_;
    int batch_;
    int decode_threads_;  // images of a batch are decoded by this many threads
    int n_consumers_;     // consumers on the same request queue: a consumer leaves the others their share of a short queue
    ConsumerShared* shared_;
    std::thread th_;
};

// Manager (src/manager.{h,cpp}): owns the queues and the consumers; a pump thread hands responses to the
// observer (the addon forwards them to the JS thread).
class Manager {
public:
    explicit Manager(Observer obs) : obs_(std::move(obs)) {}
    ~Manager();
    void start(const Parameter& p);
    int request(const std::string& expect_image, const std::string& target_image);
    // the same with ignore rectangles (Request::ignore); a rectangle the engine refuses comes back as an ERROR response
    int request(const std::string& expect_image, const std::string& target_image, const std::vector<Rect>& ignore);
    // the same for an in-memory pair (see RawPair); the two names are only echoed in the response
    int requestRaw(const std::string& expect_name, const std::string& target_name, const RawPair& raw);
    int consumerCount() const { return (int)consumers_.size(); }
    // blocks until every consumer has bound its device and created its engine (or failed to)
    void waitReady();
    // snapshot of what every consumer did since the last markEpoch()
    std::vector<ConsumerStats> consumerStats();
    // every consumer zeroes its counters (and discards its pending kernel events) before the next job it takes;
    // call while the queue is empty and every response has arrived
    void markEpoch();
    PumpStats pumpStats();
    void stop();  // idempotent; completion is reported through onCompleted
    bool running() const { return running_; }

private:
    void work();
    Observer obs_;
    Parameter param_;
    MessageQueue<Request> requestQueue_;
    MessageQueue<Response> responseQueue_;
    std::vector<Consumer*> consumers_;
    std::thread pump_;
    std::atomic<bool> running_{false};
    std::atomic<bool> stopped_{false};
    Report report_;
    std::mutex report_m_;
    ConsumerShared shared_;
    PumpStats pump_stats_;
    double pump_sum_us_ = 0;
};

}  // namespace twhost
