// twhost.cpp — see twhost.h.  Host-side only: file decode, size reconcile, queueing.  All pixel arithmetic of
// the hot path happens in libtwflow.so (HIP); there is no CPU flow implementation here.
#include "twhost.h"
#include "resident_cache.h"
#include "tw_inflate.h"
#include "tw_png_write.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <sstream>

// additive within ABI 4: an engine library from before tw_submit_jpeg still loads, and JPEGs then stay on the host
#pragma weak tw_submit_jpeg
// likewise the resident images: without them every expected image is read, decoded and uploaded each time, as before
#pragma weak tw_image_keep
#pragma weak tw_image_release
#pragma weak tw_submit_image_png
#pragma weak tw_submit_image_jpeg
// and the ignore regions: a request that names rectangles answers ERROR on an engine library from before them
#pragma weak tw_submit_u8_ignore
#pragma weak tw_submit_png_ignore
#pragma weak tw_submit_jpeg_ignore
#pragma weak tw_submit_image_png_ignore
#pragma weak tw_submit_image_jpeg_ignore
#pragma weak tw_wait_regions
#pragma weak tw_ticket_changes
#pragma weak tw_ticket_shift
#pragma weak tw_ticket_shift_bands
#pragma weak tw_ticket_hits
#pragma weak tw_ticket_overlay

namespace twhost {

// TW_DEVICE_JPEG's default (profiles/jpeg_device.md)
constexpr bool kDeviceJpegDefault = true;

// ---------------------------------------------------------------------------------------------------
// progress prints of the reference (std::cout in src/manager.cpp:74, src/consumer.cpp:49,55,92), behind TW_LOG
// (the reference's own CLI had to dup2 stdout away to hide them).  TW_LOG=1: stdout like the
// reference, TW_LOG=2: stderr.
// ---------------------------------------------------------------------------------------------------
static FILE* log_stream()
{
    static FILE* f = [] {
        const char* ev = getenv("TW_LOG");
        const int v = ev ? atoi(ev) : 0;
        return v == 1 ? stdout : (v >= 2 ? stderr : (FILE*)nullptr);
    }();
    return f;
}
#define TW_LOGF(...)                      \
    do {                                  \
        if (FILE* lf_ = log_stream()) {   \
            fprintf(lf_, __VA_ARGS__);    \
            fflush(lf_);                  \
        }                                 \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// NUMA placement (SURVEY.md 8(e) "scaling risks": pin each worker + its staging buffers to the GPU's NUMA node)
// ---------------------------------------------------------------------------------------------------
static std::string sysfs_root()
{
    const char* ev = getenv("TW_SYSFS_ROOT");
    return ev && ev[0] ? std::string(ev) : std::string("/sys");
}

static bool read_first_line(const std::string& path, std::string& out)
{
    std::ifstream f(path);
    if (!f) return false;
    std::getline(f, out);
    return true;
}

// "0-3,8,10-11" -> {0,1,2,3,8,10,11}
static std::vector<int> parse_cpulist(const std::string& s)
{
    std::vector<int> v;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        if (tok.empty()) continue;
        const size_t dash = tok.find('-');
        const int a = atoi(tok.c_str());
        const int b = dash == std::string::npos ? a : atoi(tok.c_str() + dash + 1);
        for (int c = a; c <= b && c < CPU_SETSIZE; c++)
            if (c >= 0) v.push_back(c);
    }
    return v;
}

bool numa_cpus_of_device(int device, std::string* busid, int* node, std::vector<int>* cpus)
{
    char id[32];
    if (tw_device_pci_bus_id(device, id, (int)sizeof(id)) != TW_OK || !id[0]) return false;
    if (busid) *busid = id;
    std::string line;
    if (!read_first_line(sysfs_root() + "/bus/pci/devices/" + id + "/numa_node", line)) return false;
    const int n = atoi(line.c_str());
    if (node) *node = n;
    if (n < 0) return false;  // the platform reports no NUMA affinity for this device
    if (!read_first_line(sysfs_root() + "/devices/system/node/node" + std::to_string(n) + "/cpulist", line)) return false;
    std::vector<int> v = parse_cpulist(line);
    if (v.empty()) return false;
    if (cpus) *cpus = std::move(v);
    return true;
}

std::vector<int> this_thread_cpus()
{
    std::vector<int> v;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) != 0) return v;
    for (int c = 0; c < CPU_SETSIZE; c++)
        if (CPU_ISSET(c, &set)) v.push_back(c);
    return v;
}

bool bind_this_thread(const std::vector<int>& cpus)
{
    cpu_set_t allowed, want;
    CPU_ZERO(&allowed);
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
    int n = 0;
    for (int c : cpus)
        if (c >= 0 && c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) {
            CPU_SET(c, &want);
            n++;
        }
    if (n == 0) return false;  // e.g. a container whose CPU share lies on another node: stay where we are
    return sched_setaffinity(0, sizeof(want), &want) == 0;
}

// ---------------------------------------------------------------------------------------------------
// image files -> 8-bit gray  (cv::imread(path, IMREAD_GRAYSCALE), src/opticalflow.cpp:37,44)
// ---------------------------------------------------------------------------------------------------
static bool read_file(const std::string& path, std::vector<uint8_t>& buf)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n <= 0) {
        fclose(f);
        return false;
    }
    buf.resize((size_t)n);
    const size_t got = fread(buf.data(), 1, (size_t)n, f);
    fclose(f);
    return got == (size_t)n;
}

// OpenCV 2.4.9's own decoders (BMP, PxM) convert colour to gray with icvCvt_BGR2Gray_8u_C3C1R (highgui/utils.cpp):
// 14-bit coefficients, rounded — NOT libpng's formula.  No fixture of the reference is a BMP or a PNM: parity unpinned.
static inline uint8_t bgr_to_gray_cv(int b, int g, int r)
{
    return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14);
}

// PBM / PGM / PPM, binary and ASCII (P1-P6), maxval <= 255 (highgui/grfmt_pxm.cpp: values are scaled by 255 / maxval,
// bitmaps read 1 as black)
static bool decode_pnm(const std::vector<uint8_t>& d, std::vector<uint8_t>& img, int& w, int& h)
{
    const int kind = d[1] - '0';
    if (kind < 1 || kind > 6) return false;
    size_t p = 2;
    auto skip = [&] {
        for (;;) {
            while (p < d.size() && (d[p] == ' ' || d[p] == '\n' || d[p] == '\r' || d[p] == '\t')) p++;
            if (p < d.size() && d[p] == '#') {
                while (p < d.size() && d[p] != '\n') p++;
                continue;
            }
            return;
        }
    };
    auto number = [&](int& v) -> bool {
        skip();
        long long acc = 0;
        int nd = 0;
        while (p < d.size() && d[p] >= '0' && d[p] <= '9' && nd < 10) {
            acc = acc * 10 + (d[p] - '0');
            p++;
            nd++;
        }
        if (!nd || acc > 0x7fffffff) return false;
        v = (int)acc;
        return true;
    };
    const bool bitmap = kind == 1 || kind == 4, colour = kind == 3 || kind == 6, ascii = kind <= 3;
    int maxval = 1;
    if (!number(w) || !number(h) || (!bitmap && !number(maxval))) return false;
    if (w < 1 || h < 1 || w > 32768 || h > 32768 || maxval < 1 || maxval > 255) return false;
    if (!ascii) p++;  // a single whitespace byte ends the header of the binary kinds
    const size_t npx = (size_t)w * h;
    {
        // the payload must be able to hold the image the header announces BEFORE anything of that size is allocated
        // (a 20-byte file with a 32768 x 32768 header used to cost 1 GiB of zero-filled memory per decode
        // thread): binary kinds exactly; ASCII kinds at least one character per sample (P1) or a digit and a
        // separator per sample but the last (P2 / P3)
        const size_t rest = p < d.size() ? d.size() - p : 0;
        const size_t samples = npx * (colour ? 3 : 1);
        const size_t least = !ascii ? (bitmap ? (((size_t)w + 7) / 8) * (size_t)h : samples) : bitmap ? samples : 2 * samples - 1;
        if (rest < least) return false;
    }
    img.resize(npx);
    uint8_t scale[256];
    for (int i = 0; i <= maxval; i++) scale[i] = (uint8_t)(i * 255 / maxval);
    if (ascii) {
        for (size_t i = 0; i < npx; i++) {
            int v[3] = {0, 0, 0};
            for (int c = 0; c < (colour ? 3 : 1); c++) {
                if (bitmap) {  // digits need no separators in P1
                    skip();
                    if (p >= d.size() || (d[p] != '0' && d[p] != '1')) return false;
                    v[c] = d[p++] - '0';
                } else if (!number(v[c]) || v[c] > maxval) {
                    return false;
                }
            }
            img[i] = bitmap ? (v[0] ? 0 : 255) : colour ? bgr_to_gray_cv(scale[v[2]], scale[v[1]], scale[v[0]]) : scale[v[0]];
        }
        return true;
    }
    if (bitmap) {
        const size_t rb = ((size_t)w + 7) / 8;
        if (p + rb * h > d.size()) return false;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) img[(size_t)y * w + x] = (d[p + rb * y + (x >> 3)] >> (7 - (x & 7))) & 1 ? 0 : 255;
        return true;
    }
    const size_t need = npx * (colour ? 3 : 1);
    if (p + need > d.size()) return false;
    const uint8_t* q = &d[p];
    for (size_t i = 0; i < npx; i++) {
        if (colour) {
            if (q[3 * i] > maxval || q[3 * i + 1] > maxval || q[3 * i + 2] > maxval) return false;
            img[i] = bgr_to_gray_cv(scale[q[3 * i + 2]], scale[q[3 * i + 1]], scale[q[3 * i]]);
        } else {
            if (q[i] > maxval) return false;
            img[i] = scale[q[i]];
        }
    }
    return true;
}

// Windows / OS/2 bitmaps, uncompressed: 1 / 4 / 8 bits with a palette, 24 and 32 bits (highgui/grfmt_bmp.cpp reads RLE4 /
// RLE8 and 16-bit files as well: those answer "Can't open" here)
static bool decode_bmp(const std::vector<uint8_t>& d, std::vector<uint8_t>& img, int& w, int& h)
{
    auto u16 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    if (d.size() < 26) return false;
    const uint32_t off = u32(10), hs = u32(14);
    int bpp, comp = 0;
    bool topdown = false;
    size_t pal_entry = 4;
    if (hs == 12) {  // OS/2 core header: 16-bit sizes, 3-byte palette entries
        w = (int)u16(18);
        h = (int)u16(20);
        bpp = (int)u16(24);
        pal_entry = 3;
    } else if (hs >= 40 && d.size() >= 14 + 40) {
        w = (int)u32(18);
        int hh = (int)u32(22);
        topdown = hh < 0;
        h = topdown ? -hh : hh;
        bpp = (int)u16(28);
        comp = (int)u32(30);
    } else {
        return false;
    }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) return false;
    if (comp != 0 || !(bpp == 1 || bpp == 4 || bpp == 8 || bpp == 24 || bpp == 32)) return false;
    uint8_t pal[256];
    if (bpp <= 8) {
        const size_t po = 14 + (size_t)hs;
        uint32_t ncol = hs >= 40 ? u32(46) : 0;
        if (ncol == 0 || ncol > (1u << bpp)) ncol = 1u << bpp;
        if (po + pal_entry * ncol > d.size()) return false;
        memset(pal, 0, sizeof(pal));
        for (uint32_t i = 0; i < ncol; i++) pal[i] = bgr_to_gray_cv(d[po + pal_entry * i], d[po + pal_entry * i + 1], d[po + pal_entry * i + 2]);
    }
    const size_t stride = (((size_t)w * bpp + 31) / 32) * 4;
    if ((size_t)off + stride * h > d.size() || off < 14 + hs) return false;
    img.resize((size_t)w * h);
    for (int y = 0; y < h; y++) {
        const uint8_t* row = &d[(size_t)off + stride * (size_t)(topdown ? y : h - 1 - y)];
        uint8_t* out = &img[(size_t)y * w];
        for (int x = 0; x < w; x++) {
            if (bpp == 24) out[x] = bgr_to_gray_cv(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
            else if (bpp == 32) out[x] = bgr_to_gray_cv(row[4 * x], row[4 * x + 1], row[4 * x + 2]);
            else if (bpp == 8) out[x] = pal[row[x]];
            else if (bpp == 4) out[x] = pal[(row[x >> 1] >> ((x & 1) ? 0 : 4)) & 15];
            else out[x] = pal[(row[x >> 3] >> (7 - (x & 7))) & 1];
        }
    }
    return true;
}

static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

// libpng 1.5.12 (the copy OpenCV 2.4.9 bundles) png_set_rgb_to_gray(…, 0.299, 0.587): truncated 15-bit
// coefficients and a truncated sum; pinned by the reference's golden vectors (tests/golden/make_fixtures.py).
static inline uint8_t rgb_to_gray(int r, int g, int b)
{
    if (r == g && g == b) return (uint8_t)r;
    return (uint8_t)((9797 * r + 19234 * g + 3737 * b) >> 15);
}

// CRC-32 of PNG chunks (ISO 3309, reflected 0xEDB88320), slicing-by-8: ~1 % of a decode
static uint32_t png_crc32(const uint8_t* p, size_t n)
{
    static uint32_t T[8][256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int t = 1; t < 8; t++) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
    });
    uint32_t c = 0xFFFFFFFFu;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4);
        memcpy(&b, p + 4, 4);
        a ^= c;
        c = T[7][a & 0xFF] ^ T[6][(a >> 8) & 0xFF] ^ T[5][(a >> 16) & 0xFF] ^ T[4][a >> 24] ^ T[3][b & 0xFF] ^
            T[2][(b >> 8) & 0xFF] ^ T[1][(b >> 16) & 0xFF] ^ T[0][b >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// What is left of a PNG after its chunks are parsed and its IDAT stream is inflated: the filtered scanlines (one pass,
// or the seven Adam7 passes one after the other) and what is needed to finish them
struct PngStream {
    std::unique_ptr<uint8_t[]> raw;  // `total` bytes of filtered rows (+ 8 bytes of slack)
    size_t total = 0;
    int w = 0, h = 0, depth = 0, ctype = 0, interlace = 0, ch = 0;
    std::vector<uint8_t> plte, idat;  // idat: the concatenated IDAT chunks between png_parse and png_inflate
    // rows the device reconstructs (tw_submit_png): what tw_png_on_device admits — with all_kinds false
    // (TW_DEVICE_PNG_KINDS=0) only the 8-bit gray / gray + alpha / RGB / RGBA rows of tw_submit_png8.  A palette file
    // whose PLTE is not 1 to 256 whole entries stays with the host decoder, which answers for it as it always has.
    bool device_rows(bool all_kinds) const
    {
        if (!tw_png_on_device(ctype, depth, interlace)) return false;
        if (depth == 8 && ctype != 3) return true;
        if (!all_kinds) return false;
        return ctype != 3 || (plte.size() >= 3 && plte.size() <= 768 && plte.size() % 3 == 0);
    }
    size_t row_bytes() const { return 1 + ((size_t)w * (size_t)ch * (size_t)depth + 7) / 8; }  // filter type byte included
    PngKind kind() const
    {
        PngKind k;
        k.color_type = ctype;
        k.bit_depth = depth;
        if (ctype == 3) k.plte = plte;
        return k;
    }
};

// stage 1a of cv::imread on a PNG: the chunk walk (libpng's rules); the IDAT stream is gathered in ps.idat
static bool png_parse(const std::vector<uint8_t>& d, PngStream& ps)
{
    int w = 0, h = 0;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (d.size() < 33 || memcmp(d.data(), sig, 8) != 0) return false;
    size_t p = 8;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t>& idat = ps.idat;
    std::vector<uint8_t>& plte = ps.plte;
    bool have_ihdr = false, idat_done = false, first = true, have_iend = false;
    // Chunk rules the way libpng (cv::imread) enforces them — a file it refuses answers "Can't open" here as well
    // (ADVICE r3): IHDR first; the CRC of every CRITICAL chunk (IHDR, PLTE, IDAT; an upper-case first letter) must
    // hold — a mismatch there is png_error, in an ancillary chunk only a warning; IDAT chunks are consecutive; PLTE
    // comes before IDAT.  ADVICE r4 (parity unpinned — no fixture of the reference is such a file): IHDR is exactly 13
    // bytes with compression method 0 and filter method 0 (png_check_IHDR); a critical chunk libpng does not know is
    // png_chunk_error; IEND is a critical chunk too (its CRC must hold) and must be there — cv::imread calls
    // png_read_end inside its setjmp block, so a file that stops after its last IDAT fails to open.
    while (p + 12 <= d.size()) {
        const uint32_t len = be32(&d[p]);
        const char* type = (const char*)&d[p + 4];
        if (p + 12 + (size_t)len > d.size()) return false;
        const uint8_t* data = &d[p + 8];
        const bool critical = !(type[0] & 0x20);
        if (critical && png_crc32(&d[p + 4], 4 + (size_t)len) != be32(data + len)) return false;
        if (first && memcmp(type, "IHDR", 4) != 0) return false;
        first = false;
        const bool is_idat = !memcmp(type, "IDAT", 4);
        if (!is_idat && !idat.empty()) idat_done = true;
        if (!memcmp(type, "IHDR", 4)) {
            if (len != 13 || have_ihdr) return false;
            if (data[10] != 0 || data[11] != 0) return false;  // compression method, filter method
            w = (int)be32(data);
            h = (int)be32(data + 4);
            depth = data[8];
            ctype = data[9];
            interlace = data[12];
            have_ihdr = true;
        } else if (!memcmp(type, "PLTE", 4)) {
            if (!idat.empty()) return false;
            plte.assign(data, data + len);
        } else if (is_idat) {
            if (idat_done) return false;  // IDATs must be consecutive
            idat.insert(idat.end(), data, data + len);
        } else if (!memcmp(type, "IEND", 4)) {
            have_iend = true;
            break;
        } else if (critical) {
            return false;  // unknown critical chunk
        }
        p += 12 + (size_t)len;
    }
    if (!have_iend) return false;
    if (!have_ihdr || w < 1 || h < 1 || w > 32768 || h > 32768 || interlace > 1) return false;
    int ch;
    switch (ctype) {
        case 0: ch = 1; break;
        case 2: ch = 3; break;
        case 3: ch = 1; break;
        case 4: ch = 2; break;
        case 6: ch = 4; break;
        default: return false;
    }
    if (!(depth == 8 || depth == 16 || ((ctype == 0 || ctype == 3) && (depth == 1 || depth == 2 || depth == 4))))
        return false;
    const size_t bpp_bits = (size_t)ch * depth;
    // Adam7 (interlace 1): seven reduced images one after the other, each with its own filtered rows; a pass is
    // unfiltered and converted like a whole image and its pixels scattered to (x0 + i*dx, y0 + j*dy)
    static const int AX0[7] = {0, 4, 0, 2, 0, 1, 0}, AY0[7] = {0, 0, 4, 0, 2, 0, 1};
    static const int ADX[7] = {8, 8, 4, 4, 2, 2, 1}, ADY[7] = {8, 8, 8, 4, 4, 2, 2};
    const int npass = interlace ? 7 : 1;
    size_t total = 0;
    for (int ps = 0; ps < npass; ps++) {
        const int pw = interlace ? (w - AX0[ps] + ADX[ps] - 1) / ADX[ps] : w;
        const int ph = interlace ? (h - AY0[ps] + ADY[ps] - 1) / ADY[ps] : h;
        if (pw > 0 && ph > 0) total += (((size_t)pw * bpp_bits + 7) / 8 + 1) * (size_t)ph;
    }
    // DEFLATE expands by at most 1032 : 1: a stream too short for the image the header announces is refused before
    // `total` bytes (up to 8 GiB for 32768 x 32768 RGBA16) are allocated for it
    if (total / 1032 > idat.size()) return false;
    ps.total = total;
    ps.w = w;
    ps.h = h;
    ps.depth = depth;
    ps.ctype = ctype;
    ps.interlace = interlace;
    ps.ch = ch;
    return true;
}

// stage 1b: the inflate, into `dst` (ps.total bytes + 8 of slack: the caller's arena slot, or ps.raw)
static bool png_inflate(const PngStream& ps, uint8_t* dst)
{
    size_t outlen = 0;
    return tw_inflate_zlib(ps.idat.data(), ps.idat.size(), dst, ps.total, &outlen) && outlen == ps.total;
}

static bool png_parse_inflate(const std::vector<uint8_t>& d, PngStream& ps)
{
    if (!png_parse(d, ps)) return false;
    // (uninitialised: every byte is written by the inflate or the decode fails; + 8 bytes of slack for nothing — the
    // decoder never writes past `total`)
    ps.raw.reset(new (std::nothrow) uint8_t[ps.total + 8]);
    if (!ps.raw) return false;
    const bool ok = png_inflate(ps, ps.raw.get());
    std::vector<uint8_t>().swap(ps.idat);
    return ok;
}

// stage 2: scanline reconstruction (tw_inflate.cpp) + conversion to 8-bit gray with libpng 1.5's formula — on the host
// (every PNG kind; what tw_png_unfilter does on the device for the 8-bit non-interlaced kinds)
static bool png_finish_on_host(PngStream& st, std::vector<uint8_t>& img)
{
    uint8_t* const raw = st.raw.get();
    const int w = st.w, h = st.h, depth = st.depth, ctype = st.ctype, interlace = st.interlace, ch = st.ch;
    const std::vector<uint8_t>& plte = st.plte;
    const size_t bpp_bits = (size_t)ch * depth;
    const size_t fbpp = std::max<size_t>(1, bpp_bits / 8);
    static const int AX0[7] = {0, 4, 0, 2, 0, 1, 0}, AY0[7] = {0, 0, 4, 0, 2, 0, 1};
    static const int ADX[7] = {8, 8, 4, 4, 2, 2, 1}, ADY[7] = {8, 8, 8, 4, 4, 2, 2};
    const int npass = interlace ? 7 : 1;
    img.resize((size_t)w * h);
    size_t pass_off = 0;
    const int W = w, H = h;  // the loops below run over one pass: w/h are its dimensions
    for (int ps = 0; ps < npass; ps++) {
    const int x0 = interlace ? AX0[ps] : 0, y0 = interlace ? AY0[ps] : 0;
    const int dx = interlace ? ADX[ps] : 1, dy = interlace ? ADY[ps] : 1;
    const int w = interlace ? (W - x0 + dx - 1) / dx : W, h = interlace ? (H - y0 + dy - 1) / dy : H;
    if (w <= 0 || h <= 0) continue;
    const size_t rowbytes = ((size_t)w * bpp_bits + 7) / 8;
    std::vector<uint8_t> line((size_t)w);
    // unfilter the whole pass in place (tw_inflate.cpp: one loop per filter type, Paeth rows of 1-byte pixels two at a
    // time), then convert row by row
    if (!tw_png_unfilter(raw + pass_off, rowbytes, (size_t)h, fbpp)) return false;
    for (int y = 0; y < h; y++) {
        uint8_t* row = &raw[pass_off + (rowbytes + 1) * (size_t)y];
        uint8_t* cur = row + 1;
        uint8_t* out = line.data();
        if (depth == 8 && ctype == 0 && dx == 1) {
            memcpy(&img[(size_t)(y0 + y * dy) * W + x0], cur, (size_t)w);  // 8-bit gray, not interlaced: the row is the output
            continue;
        }
        auto sample8 = [&](size_t idx) -> int {  // idx-th sample of the row as 8 bits (16-bit: high byte)
            if (depth == 8) return cur[idx];
            if (depth == 16) return cur[idx * 2];
            const int per = 8 / depth;
            const int v2 = (cur[idx / per] >> ((per - 1 - (int)(idx % per)) * depth)) & ((1 << depth) - 1);
            return ctype == 3 ? v2 : v2 * 255 / ((1 << depth) - 1);
        };
        if (depth == 8 && ctype == 0) {
            memcpy(out, cur, (size_t)w);  // 8-bit gray: the row is the output
        } else if (depth == 8 && (ctype == 2 || ctype == 6)) {
            for (int x = 0; x < w; x++) out[x] = rgb_to_gray(cur[(size_t)x * ch], cur[(size_t)x * ch + 1], cur[(size_t)x * ch + 2]);
        } else
        for (int x = 0; x < w; x++) {
            if (ctype == 0 || ctype == 4) {
                out[x] = (uint8_t)sample8((size_t)x * ch);
            } else if (ctype == 3) {
                const size_t idx = (size_t)sample8((size_t)x) * 3;
                if (idx + 2 >= plte.size()) return false;
                out[x] = rgb_to_gray(plte[idx], plte[idx + 1], plte[idx + 2]);
            } else {
                out[x] = rgb_to_gray(sample8((size_t)x * ch), sample8((size_t)x * ch + 1), sample8((size_t)x * ch + 2));
            }
        }
        uint8_t* dst = &img[(size_t)(y0 + y * dy) * W + x0];
        for (int x = 0; x < w; x++) dst[(size_t)x * dx] = out[x];
    }
    pass_off += (rowbytes + 1) * (size_t)h;
    }
    return true;
}

static bool decode_png(const std::vector<uint8_t>& d, std::vector<uint8_t>& img, int& w, int& h)
{
    PngStream st;
    if (!png_parse_inflate(d, st)) return false;
    w = st.w;
    h = st.h;
    return png_finish_on_host(st, img);
}

// The rest of the decode of rows load_gray_or_png_rows() returned (size reconcile needs gray pixels on the host)
bool finish_png_rows_on_host(std::vector<uint8_t>& rows, int w, int h, int ch, std::vector<uint8_t>& gray)
{
    if (ch < 1 || ch > 4 || rows.size() != (size_t)h * ((size_t)w * ch + 1)) return false;
    PngStream st;
    st.total = rows.size();
    st.raw.reset(new (std::nothrow) uint8_t[st.total + 8]);
    if (!st.raw) return false;
    memcpy(st.raw.get(), rows.data(), st.total);
    st.w = w;
    st.h = h;
    st.depth = 8;
    st.interlace = 0;
    st.ch = ch;
    st.ctype = ch == 1 ? 0 : ch == 2 ? 4 : ch == 3 ? 2 : 6;
    return png_finish_on_host(st, gray);
}

bool finish_png_kind_on_host(const uint8_t* rows, int w, int h, const PngKind& kind, std::vector<uint8_t>& gray)
{
    const int ct = kind.color_type, d = kind.bit_depth;
    const bool depth_ok = d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
    if (!rows || w < 1 || h < 1 || !depth_ok || !(ct == 0 || (ct == 3 && d <= 8) || ((ct == 2 || ct == 4 || ct == 6) && d >= 8)))
        return false;
    PngStream st;
    st.total = kind.row_bytes(w) * (size_t)h;
    st.raw.reset(new (std::nothrow) uint8_t[st.total + 8]);
    if (!st.raw) return false;
    memcpy(st.raw.get(), rows, st.total);
    st.w = w;
    st.h = h;
    st.depth = d;
    st.interlace = 0;
    st.ctype = ct;
    st.ch = ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 1;
    st.plte = kind.plte;
    return png_finish_on_host(st, gray);
}

static bool decode_gray_or_png_kind_rows(const std::vector<uint8_t>& d, bool want_rows, bool all_kinds, std::vector<uint8_t>& img,
                                         int& w, int& h, PngKind& kind);
static bool decode_gray_or_png_rows(const std::vector<uint8_t>& d, bool want_rows, std::vector<uint8_t>& img, int& w, int& h, int& ch);

bool load_gray(const std::string& path, std::vector<uint8_t>& img, int& w, int& h)
{
    int ch = 0;
    return load_gray_or_png_rows(path, false, img, w, h, ch);
}

// cv::imread(path, GRAYSCALE) — or, with want_rows and an 8-bit non-interlaced gray / gray + alpha / RGB / RGBA PNG,
// only its first half: `img` then holds the inflated, still FILTERED scanlines (h rows of 1 + w * ch bytes) and ch is
// 1-4; the device finishes them (tw_submit_png8).  Every row's filter type is checked here (0-4, as libpng does).
// ch = 0: `img` is the gray image.
bool load_gray_or_png_rows(const std::string& path, bool want_rows, std::vector<uint8_t>& img, int& w, int& h, int& ch)
{
    std::vector<uint8_t> d;
    w = h = ch = 0;
    if (!read_file(path, d)) return false;
    return decode_gray_or_png_rows(d, want_rows, img, w, h, ch);
}

bool load_gray_or_png_kind_rows(const std::string& path, bool want_rows, bool all_kinds, std::vector<uint8_t>& img, int& w,
                                int& h, PngKind& kind)
{
    std::vector<uint8_t> d;
    w = h = 0;
    kind = PngKind();
    if (!read_file(path, d)) return false;
    return decode_gray_or_png_kind_rows(d, want_rows, all_kinds, img, w, h, kind);
}

// the same on the bytes of a file that has been read already (ch 1-4: the 8-bit kinds only, as its contract says)
static bool decode_gray_or_png_rows(const std::vector<uint8_t>& d, bool want_rows, std::vector<uint8_t>& img, int& w, int& h, int& ch)
{
    PngKind k;
    ch = 0;
    if (!decode_gray_or_png_kind_rows(d, want_rows, false, img, w, h, k)) return false;
    ch = k.color_type == 0 ? 1 : k.color_type == 4 ? 2 : k.color_type == 2 ? 3 : k.color_type == 6 ? 4 : 0;
    return true;
}

static bool decode_gray_or_png_kind_rows(const std::vector<uint8_t>& d, bool want_rows, bool all_kinds, std::vector<uint8_t>& img,
                                         int& w, int& h, PngKind& kind)
{
    w = h = 0;
    kind = PngKind();
    if (d.size() < 8) return false;
    bool ok = false;
    if (d[0] == 'P' && d[1] >= '1' && d[1] <= '6') ok = decode_pnm(d, img, w, h);
    else if (d[0] == 0x89 && d[1] == 'P' && want_rows) {
        PngStream st;
        ok = png_parse_inflate(d, st);
        if (ok) {
            w = st.w;
            h = st.h;
            if (st.device_rows(all_kinds)) {
                PngKind k = st.kind();
                const size_t rs = st.row_bytes();
                for (int y = 0; y < st.h && ok; y++) ok = st.raw[(size_t)y * rs] <= 4;
                if (ok) {
                    img.assign(st.raw.get(), st.raw.get() + st.total);
                    kind = std::move(k);
                }
            } else {
                ok = png_finish_on_host(st, img);
            }
        }
    } else if (d[0] == 0x89 && d[1] == 'P') ok = decode_png(d, img, w, h);
    else if (d[0] == 0xFF && d[1] == 0xD8) ok = decode_jpeg_gray(d.data(), d.size(), img, w, h);
    else if (d[0] == 'B' && d[1] == 'M') ok = decode_bmp(d, img, w, h);
    // (the other cv::imread formats — TIFF, JPEG-2000, Sun raster, ... — are not decoded: INTEGRATION.md)
    if (!ok) {
        // the decoders write w / h from the header before they can fail: a failed decode reports no size (ADVICE r3:
        // a 32768 x 32768 IHDR over a truncated IDAT used to size the page-locked arena)
        w = h = 0;
        kind = PngKind();
        std::vector<uint8_t>().swap(img);
    }
    return ok;
}

// cv::resize on CV_8UC1, INTER_LINEAR, 11-bit fixed point (imgproc/imgwarp.cpp: HResizeLinear<uchar,int,short>,
// VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>>).  No golden vector of the reference exercises
// this branch (its fixtures have equal sizes): parity unpinned.
void resize_u8_linear(const std::vector<uint8_t>& src, int sw, int sh, std::vector<uint8_t>& dst, int dw, int dh)
{
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    std::vector<int> xofs(dw), yofs(dh);
    std::vector<short> ia(2 * (size_t)dw), ib(2 * (size_t)dh);
    auto sat_short = [](double v) { long r = lrint(v); return (short)std::min<long>(32767, std::max<long>(-32768, r)); };
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        xofs[dx] = sx;
        ia[2 * dx] = sat_short((1.f - fx) * 2048);
        ia[2 * dx + 1] = sat_short(fx * 2048);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floor(fy);
        fy -= sy;
        yofs[dy] = sy;
        ib[2 * dy] = sat_short((1.f - fy) * 2048);
        ib[2 * dy + 1] = sat_short(fy * 2048);
    }
    dst.resize((size_t)dw * dh);
    std::vector<int> r0(dw), r1(dw);
    auto hrow = [&](int sy, std::vector<int>& out) {
        sy = std::min(std::max(sy, 0), sh - 1);
        const uint8_t* S = &src[(size_t)sy * sw];
        for (int dx = 0; dx < dw; dx++) {
            const int sx = xofs[dx];
            out[dx] = sx + 1 < sw ? S[sx] * ia[2 * dx] + S[sx + 1] * ia[2 * dx + 1] : S[sx] * 2048;
        }
    };
    for (int dy = 0; dy < dh; dy++) {
        hrow(yofs[dy], r0);
        hrow(yofs[dy] + 1, r1);
        const int b0 = ib[2 * dy], b1 = ib[2 * dy + 1];
        for (int dx = 0; dx < dw; dx++) {
            const int v = (((b0 * (r0[dx] >> 4)) >> 16) + ((b1 * (r1[dx] >> 4)) >> 16) + 2) >> 2;
            dst[(size_t)dy * dw + dx] = (uint8_t)std::min(255, std::max(0, v));
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Consumer
// ---------------------------------------------------------------------------------------------------
Consumer::Consumer(int id, MessageQueue<Request>& req, MessageQueue<Response>& res, const tw_params& p, int batch,
                   int decode_threads, int n_consumers, ConsumerShared* shared)
    : id_(id), req_(req), res_(res), params_(p), batch_(std::max(1, batch)), decode_threads_(std::max(1, decode_threads)),
      n_consumers_(std::max(1, n_consumers)), shared_(shared)
{
}
Consumer::~Consumer() { join(); }
void Consumer::start() { th_ = std::thread([this] { run(); }); }
void Consumer::join()
{
    if (th_.joinable()) th_.join();
}

namespace {
inline long long steady_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// cv::imread failed on `path` (src/opticalflow.cpp:40,47)
inline std::string cant_open(const std::string& path) { return "Can't open " + path; }
// a refused submit or wait: the engine's own words, else the status's
inline std::string engine_error(const tw_engine* eng, tw_status r)
{
    return std::string(tw_last_error(eng)[0] ? tw_last_error(eng) : tw_strerror(r));
}

// on(): an image's bytes are a JPEG's quantised luma coefficients, bw * bh blocks of 64 int16 (the device runs the inverse
// DCT: tw_submit_jpeg)
struct JpegHead {
    int bw = 0, bh = 0;
    uint16_t quant[64] = {0};
    bool on() const { return bw > 0; }
};
struct Staged {
    Request req;
    // One image of the pair: [0] the expected image, [1] the target
    struct Side {
        std::vector<uint8_t> bytes;  // the image where the host layer holds it itself (not in the arena, not the caller's)
        const uint8_t* p = nullptr;  // the image as handed to the engine (bytes, an arena slot or the caller's raw buffer)
        int w = 0, h = 0;            // the image's own size
        PngKind kind;                // rows(): filtered PNG rows of that kind (the device finishes them: tw_submit_png)
        JpegHead jpeg;
        std::string err;             // why it could not be opened
    } side[2];
    const std::string& path(int which) const { return which ? req.target_image : req.expect_image; }
    ptrdiff_t stride = 0;
    int w = 0, h = 0;                // the pair's size: the expected image's
    bool device_reconciles = false;  // the target goes up in its own size and the device resizes it (tw_submit_*_sized)
    std::string err;
    tw_ticket ticket = 0;
    bool submitted = false;
    bool done = false;  // response pushed
    // resident expected images (Parameter::residentMB): the identity of the expected file ("" : not looked at); hit: the
    // cache entry whose image stands in for the file (pinned until the pair is submitted); keep: the image this pair's
    // expected file becomes — kept by the pair that decoded it (kept), used by the pairs behind it that name the same file
    // (uses_keep) while that pair has not answered; leader: that pair when it sits in this very batch (index before the sort)
    std::string rkey;
    ResidentCache::Entry* hit = nullptr;
    std::shared_ptr<ResidentCache::Keep> keep;
    int leader = -1;
    bool follower = false, uses_keep = false;
    tw_image* kept = nullptr;
    bool no_expected_file() const { return hit || follower; }
};

// the rest of a JPEG's decode on the host (what the device does for tw_submit_jpeg): the side from coefficients to gray
void finish_jpeg_on_host(Staged::Side& sd)
{
    JpegLuma l;
    l.w = sd.w;
    l.h = sd.h;
    l.bw = sd.jpeg.bw;
    l.bh = sd.jpeg.bh;
    memcpy(l.quant, sd.jpeg.quant, sizeof(l.quant));
    l.coef.resize(sd.bytes.size() / 2);
    memcpy(l.coef.data(), sd.bytes.data(), l.coef.size() * 2);
    jpeg_luma_to_gray(l, sd.bytes);
    sd.jpeg = JpegHead();
}

// The environment switches of a consumer, read once when it starts
struct Switches {
    bool numa;  // TW_NUMA=0: the consumer thread stays where it is
    // PNG scanline reconstruction + gray conversion on the device (tw_submit_png8): the decode pool only inflates.
    // TW_DEVICE_PNG=0 keeps the whole decode on the host (A/B switch; same bytes either way).
    bool device_png;
    // The <= 5 px size reconcile of OpticalFlow::calculate on the device (tw_submit_*_sized): an unequal pair stays where it
    // was decoded — page-locked arena, filtered rows — like every other pair.  TW_DEVICE_RECONCILE=0 keeps the host path
    // (finish_png_rows_on_host + resize_u8_linear on copies outside the arena): A/B switch and fallback, same bytes.
    bool device_reconcile;
    // Palette, 1- / 2- / 4-bit gray, 16-bit gray and 16-bit gray + alpha files on the device as well (tw_submit_png: whatever
    // tw_png_on_device admits), so that one such file no longer takes its whole batch off the arena path.
    // TW_DEVICE_PNG_KINDS=0 finishes those kinds on the host as before: A/B switch and fallback, same bytes.  The device
    // side measured faster (profiles/png_kinds.md: 1.77 x on a palette corpus, 1.39 x with one palette pair in 32).
    bool png_kinds;
    // A JPEG's inverse DCT on the device (tw_submit_jpeg, where the engine exports it): the decode pool stops at the
    // coefficient plane.  TW_DEVICE_JPEG=0 keeps the whole decode on the host: A/B switch and fallback, same bytes
    // (profiles/jpeg_device.md has the measurement behind the default).
    bool device_jpeg;
    bool scan_fused_final;  // TW_SCAN_FUSED_FINAL=1: the engine option of that name (create_engine)
    long fair_slack;        // TW_FAIR_SLACK: pairs a consumer may hold beyond its fair share
    bool debug_takes;       // TW_DEBUG_TAKES: diagnostic: who takes what, when
    bool debug_batchtime;   // TW_DEBUG_BATCHTIME: diagnostic: where a batch's host time goes
    static bool flag(const char* name, bool otherwise)
    {
        const char* ev = getenv(name);
        return ev ? atoi(ev) != 0 : otherwise;
    }
    Switches()
        : numa(flag("TW_NUMA", true)), device_png(flag("TW_DEVICE_PNG", true)), device_reconcile(flag("TW_DEVICE_RECONCILE", true)),
          png_kinds(flag("TW_DEVICE_PNG_KINDS", true)), device_jpeg(flag("TW_DEVICE_JPEG", kDeviceJpegDefault)),
          scan_fused_final(flag("TW_SCAN_FUSED_FINAL", false)), fair_slack(getenv("TW_FAIR_SLACK") ? atol(getenv("TW_FAIR_SLACK")) : 0),
          debug_takes(getenv("TW_DEBUG_TAKES") != nullptr), debug_batchtime(getenv("TW_DEBUG_BATCHTIME") != nullptr)
    {
    }
};

// the two imreads of a pair are independent: the decode pool runs them as separate tasks (task = 2 * job + image), and
// each writes s.side[which] and nothing else
// (`file`: the bytes of the file when the caller has read it already, else null)
// (device_jpeg: a JPEG stops at its coefficient plane — Side::jpeg — and the device runs the inverse DCT)
void decode_one(Staged& s, int which, const Switches& sw, bool device_jpeg, const std::vector<uint8_t>* file)
{
    if (s.req.raw.expect) return;
    if (which == 0 && s.no_expected_file()) return;  // (a resident image stands in for the file)
    static const char* const kEmptyPath[2] = {"ExpectImagePath is empty.", "TargetImagePath is empty."};
    Staged::Side& sd = s.side[which];
    const std::string& path = s.path(which);
    if (path.empty()) { sd.err = kEmptyPath[which]; return; }
    if (device_jpeg && file && file->size() >= 8 && (*file)[0] == 0xFF && (*file)[1] == 0xD8) {
        JpegLuma l;
        if (!decode_jpeg_luma(file->data(), file->size(), l)) {
            sd.err = cant_open(path);
            return;
        }
        sd.w = l.w;
        sd.h = l.h;
        sd.jpeg.bw = l.bw;
        sd.jpeg.bh = l.bh;
        memcpy(sd.jpeg.quant, l.quant, sizeof(sd.jpeg.quant));
        sd.bytes.resize(l.coef.size() * 2);
        memcpy(sd.bytes.data(), l.coef.data(), sd.bytes.size());
        return;
    }
    const bool ok = file ? decode_gray_or_png_kind_rows(*file, sw.device_png, sw.png_kinds, sd.bytes, sd.w, sd.h, sd.kind)
                         : load_gray_or_png_kind_rows(path, sw.device_png, sw.png_kinds, sd.bytes, sd.w, sd.h, sd.kind);
    if (!ok) sd.err = cant_open(path);
}

// What OpticalFlow::calculate does with a pair of these two sizes (src/opticalflow.cpp:50-68)
enum class SizeRule {
    Same,
    DontMatch,          // more than 5 px apart: "Don't match image size"
    ReconcileOnDevice,  // within 5 px: the target goes up as it was decoded (tw_submit_*_sized)
    ReconcileOnHost     // TW_DEVICE_RECONCILE=0: the target's gray pixels are resized here
};
SizeRule size_rule(int w, int h, int tw, int th, bool device_reconcile)
{
    if (w == tw && h == th) return SizeRule::Same;
    if (abs(h - th) > 5 || abs(w - tw) > 5) return SizeRule::DontMatch;
    return device_reconcile ? SizeRule::ReconcileOnDevice : SizeRule::ReconcileOnHost;
}

// A pair behind the one that keeps its expected image, in the same batch: that one's size, and its failure to open the file
void inherit_from_leader(Staged& s, const std::vector<Staged>& jobs)
{
    if (!s.follower || s.leader < 0) return;
    const Staged::Side& le = jobs[(size_t)s.leader].side[0];
    if (!le.err.empty()) s.side[0].err = cant_open(s.req.expect_image);
    s.side[0].w = le.w;
    s.side[0].h = le.h;
}
// the reference checks and opens the expected image first (src/opticalflow.cpp:26-48): its error wins.  true: s.err is set
bool pair_refused(Staged& s)
{
    if (s.req.expect_image.empty()) s.err = "ExpectImagePath is empty.";
    else if (s.req.target_image.empty()) s.err = "TargetImagePath is empty.";
    else if (!s.side[0].err.empty()) s.err = s.side[0].err;
    else if (!s.side[1].err.empty()) s.err = s.side[1].err;
    return !s.err.empty();
}

// TW_DEVICE_RECONCILE=0: the reconcile resizes the TARGET's gray pixels here (src/opticalflow.cpp:64-68); a target that is
// still filtered PNG rows is finished on the host first (the expected image may stay as it is).  Both images are in
// Side::bytes.  false: s.err is set
bool reconcile_on_host(Staged& s)
{
    Staged::Side& t = s.side[1];
    if (t.kind.rows()) {
        std::vector<uint8_t> g;
        if (t.bytes.size() != t.kind.row_bytes(t.w) * (size_t)t.h || !finish_png_kind_on_host(t.bytes.data(), t.w, t.h, t.kind, g)) {
            s.err = cant_open(s.req.target_image);
            return false;
        }
        t.bytes.swap(g);
        t.kind = PngKind();
    }
    std::vector<uint8_t> r;
    resize_u8_linear(t.bytes, t.w, t.h, r, s.w, s.h);
    t.bytes.swap(r);
    t.w = s.w;
    t.h = s.h;
    return true;
}
void point_at_own_bytes(Staged& s)
{
    s.side[0].p = s.side[0].bytes.data();
    s.side[1].p = s.side[1].bytes.data();
    s.stride = s.w;
}

// OpticalFlow::calculate up to (not including) calculateInternal: src/opticalflow.cpp:20-68 — for a pair whose images
// decode_one left in Side::bytes (or the caller's raw buffers)
void prepare(Staged& s, bool device_reconcile)
{
    Staged::Side &e = s.side[0], &t = s.side[1];
    if (s.req.raw.expect) {  // in-memory pair: nothing to decode
        const RawPair& r = s.req.raw;
        if (!r.target || r.width < 1 || r.height < 1 || r.stride < r.width) { s.err = "bad raw image pair"; return; }
        e.p = r.expect;
        t.p = r.target;
        s.w = e.w = t.w = r.width;
        s.h = e.h = t.h = r.height;
        s.stride = r.stride;
        return;
    }
    s.w = e.w;
    s.h = e.h;
    if (pair_refused(s)) return;
    const SizeRule rule = size_rule(s.w, s.h, t.w, t.h, device_reconcile);
    if (rule == SizeRule::DontMatch) { s.err = "Don't match image size"; return; }
    // a JPEG beside half-decoded PNG rows (index.js pairs files by relative path: a corner): tw_submit_png takes rows and
    // gray images, so the JPEG is finished here; so is a JPEG target that the host is to resize
    if (e.jpeg.on() && t.kind.rows()) finish_jpeg_on_host(e);
    if (t.jpeg.on() && (e.kind.rows() || rule == SizeRule::ReconcileOnHost)) finish_jpeg_on_host(t);
    // the <= 5 px reconcile on the device (tw_submit_*_sized): the target stays as it was decoded, filtered rows included
    s.device_reconciles = rule == SizeRule::ReconcileOnDevice;
    if (rule == SizeRule::ReconcileOnHost && !reconcile_on_host(s)) return;
    point_at_own_bytes(s);
}

// Which entry point of the engine a staged pair goes through (`resident`: an image on the device stands in for the
// expected file, so only the target goes up, in whatever form it was decoded to)
enum class EntryPoint { ImageJpeg, ImagePng, Png, Jpeg, U8Sized, U8 };
EntryPoint entry_point(const Staged& s, bool resident)
{
    const Staged::Side &e = s.side[0], &t = s.side[1];
    if (resident) return t.jpeg.on() ? EntryPoint::ImageJpeg : EntryPoint::ImagePng;
    // half-decoded PNG(s): the device reconstructs the scanlines, and resizes a target within 5 px of the pair's size
    if (e.kind.rows() || t.kind.rows()) return EntryPoint::Png;
    // JPEG(s) that stopped at the coefficient plane: the device runs the inverse DCT (and the reconcile)
    if (e.jpeg.on() || t.jpeg.on()) return EntryPoint::Jpeg;
    return s.device_reconciles ? EntryPoint::U8Sized : EntryPoint::U8;
}
tw_png_rows rows_of(const Staged::Side& sd)
{
    tw_png_rows r;
    r.rows = sd.p;
    r.width = sd.w;
    r.height = sd.h;
    r.color_type = sd.kind.color_type;
    r.bit_depth = sd.kind.bit_depth;
    r.palette = sd.kind.plte.empty() ? nullptr : sd.kind.plte.data();
    r.palette_entries = (int)(sd.kind.plte.size() / 3);
    return r;
}
tw_jpeg_luma luma_of(const Staged::Side& sd)
{
    tw_jpeg_luma l;
    l.coef = sd.jpeg.on() ? (const int16_t*)sd.p : nullptr;
    l.gray = sd.jpeg.on() ? nullptr : sd.p;
    l.width = sd.w;
    l.height = sd.h;
    l.blocks_w = sd.jpeg.bw;
    l.blocks_h = sd.jpeg.bh;
    memcpy(l.quant, sd.jpeg.quant, sizeof(l.quant));
    return l;
}

// fn(0) .. fn(ntask - 1) on up to `threads` threads, the caller's among them
template <class Fn>
void parallel_for(size_t ntask, size_t threads, const Fn& fn)
{
    const size_t nt = std::min(ntask, threads);
    std::atomic<size_t> next{0};
    auto worker = [&] {
        for (size_t i = next++; i < ntask; i = next++) fn(i);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; t++) pool.emplace_back(worker);
    worker();
    for (std::thread& t : pool) t.join();
}

// page-locked (tw_host_alloc): the decoded pairs of the batch being filled / the two batches in flight
struct Arena {
    uint8_t* base = nullptr;
    size_t cap = 0;
};
// a file of the batch after Phase 1
struct Opened {
    std::vector<uint8_t> file;
    PngStream st;
    bool read_ok = false, rows_ok = false;
};
// What one turn of the consumer's loop works on
struct Batch {
    std::vector<Staged> jobs;
    std::vector<Opened> op;  // [2 * job + image]
    Arena* arena = nullptr;
    size_t slot = 0;  // bytes of an arena slot; image i of the batch sits at arena->base + slot * i
    long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;  // TW_DEBUG_BATCHTIME: taken, decoded, staged, flushed
    // (a resident image stands in for the expected file of that job: nothing to read, decode or copy)
    bool skipped(size_t i) const { return !(i & 1) && jobs[i >> 1].no_expected_file(); }
};

// What the calls of the per-pair extras write into, kept from pair to pair: tw_ticket_changes' and tw_ticket_shift_bands'
// records, tw_wait_regions' two arrays, tw_ticket_overlay's pixels (sized by the pair that gets a picture), and the counts
// and the shift record of the pair being collected
struct ExtrasScratch {
    std::vector<tw_change> change_recs;
    std::vector<tw_shift_band> band_recs;
    std::vector<int> region_of;
    std::vector<tw_region> region_recs;
    std::vector<uint8_t> overlay_px;
    int nchg = 0, nbands = 0, nreg = 0;
    tw_shift shift_rec;
    // for a pair of `cap` grid points, with `x` in force
    void reserve(int cap, const PairExtras& x)
    {
        nchg = nbands = nreg = 0;
        if (x.regions) {
            region_of.resize((size_t)cap);
            region_recs.resize(TW_MAX_REGIONS);
        }
        if (x.residual) change_recs.resize((size_t)cap);
        if (x.shiftBands && band_recs.empty()) band_recs.resize(64);
    }
};
// What ask_extras learnt: the first failing call's status and the engine's words for it
struct Asked {
    tw_status status = TW_OK;
    std::string message;
};
// What the collecting wait answered: the number of vectors (in ConsumerRun::hits) and the pair's time
struct Waited {
    tw_status status = TW_OK;
    int n = 0;
    float sec = 0;
};

// Consumer::run's state and its steps, in the order run() calls them
struct ConsumerRun {
    // the consumer's own (Consumer's members)
    const int id;
    MessageQueue<Request>& req;
    MessageQueue<Response>& res;
    const tw_params& params;
    const int batch_size, decode_threads, n_consumers;
    ConsumerShared* const shared;

    const Switches sw;
    ConsumerStats mine;  // this thread's own counters; published under the shared mutex
    int ndev = 0, dev = -1;
    tw_engine* eng = nullptr;
    std::string eng_err;
    bool device_jpeg = false;  // sw.device_jpeg, where the engine exports tw_submit_jpeg
    bool prof = false;
    int my_epoch = 0;
    // one scratch array for the hit records of a job, grown to the largest grid seen: a fresh zero-filled vector of
    // grid-capacity entries per job — 0.5 MB at 1080p / span 10 — cost 0.2 ms of every response, round 4
    std::unique_ptr<tw_vector[]> hits;
    size_t hits_cap = 0;
    // the extras in force on `eng` (ConsumerShared::extras once set_extras and check_overlay have passed; all off without an
    // engine), and what their calls write into
    PairExtras extras;
    ExtrasScratch scratch;
    // Resident expected images (Parameter::residentMB / TW_RESIDENT_MB; 0, the default: off, and no step below reaches the
    // cache): resident_cache.h
    std::unique_ptr<ResidentCache> cache;
    // Two batches are kept going: the one just submitted computes while the next one is popped, decoded and
    // uploaded (the engine itself holds up to three batches).  Responses leave in completion order, as in the
    // reference.
    Arena arena[3];
    int arena_idx = 0;
    // Batches in flight behind the one being prepared: `prev` was submitted last, `prev2` before it.  Round 4: with one
    // batch in flight the loop ran at the GPU's LATENCY for a batch (upload -> scanline reconstruction -> flow: ~22 ms for
    // 32 pairs) instead of at the host's own ~16 ms; the engine takes three batch contexts, so two stay outstanding while
    // the third is decoded.
    std::vector<Staged> prev, prev2;

    ConsumerRun(int id_, MessageQueue<Request>& req_, MessageQueue<Response>& res_, const tw_params& p, int batch, int decode_threads_,
                int n_consumers_, ConsumerShared* shared_)
        : id(id_), req(req_), res(res_), params(p), batch_size(batch), decode_threads(decode_threads_), n_consumers(n_consumers_),
          shared(shared_)
    {
    }

    void publish()
    {
        if (!shared) return;
        std::lock_guard<std::mutex> lk(shared->m);
        if ((size_t)id < shared->stats.size()) shared->stats[(size_t)id] = mine;
        shared->cv.notify_all();
    }
    // kernel events are read (a device synchronise) only when nothing of ours is in flight
    void read_prof(bool keep)
    {
        if (!prof) return;
        static const int kc[2] = {TW_K_BLUR_SOLVE, TW_K_POLYEXP};
        for (int i = 0; i < 2; i++) {
            double ms = 0;
            int n = 0;
            if (tw_prof_read(eng, kc[i], &ms, &n) == TW_OK && keep) {
                mine.profMs[i] += ms;
                mine.profLaunches[i] += n;
            }
        }
    }

    // device binding happens here, on the worker thread (the reference binds on the main thread:
    // src/consumer.cpp:22 via src/manager.cpp:56 — SURVEY.md Appendix B#6)
    void bind_device_and_numa()
    {
        ndev = tw_device_count();
        dev = ndev > 0 ? id % ndev : -1;
        mine.id = id;
        mine.device = dev;
        // NUMA placement BEFORE the engine exists: the thread — and with it the decode pool it spawns and, by first touch,
        // the page-locked staging / result buffers tw_engine_create and tw_submit_u8 allocate — moves to the CPUs of the
        // GPU's node, so that 8 consumers x ~16 GB/s of pinned H2D do not cross the socket link.  TW_NUMA=0 disables.
        std::vector<int> cpus;
        int node = -1;
        if (dev >= 0 && numa_cpus_of_device(dev, &mine.pciBusId, &node, &cpus) && sw.numa && bind_this_thread(cpus))
            mine.numaNode = node;
        mine.cpus = this_thread_cpus();
    }

    void create_engine()
    {
        device_jpeg = sw.device_jpeg && tw_submit_jpeg != nullptr;
        if (ndev > 0) {
            tw_status r = tw_engine_create(dev, &params, batch_size, &eng);
            if (r != TW_OK) eng_err = std::string("engine: ") + tw_strerror(r);
        } else {
            eng_err = "no HIP device available";
        }
        // Opt-in (TW_SCAN_FUSED_FINAL=1): the engine option that evaluates the last level-0 iteration at the span-grid points
        // only.  A consumer hands back vectors, never the flow field, so the option is invisible to the caller (bit-identical
        // vectors, tests/test_gpu_parity.py::test_scan_fused_final_iteration_option) and worth +3-5 % of GPU throughput; it
        // stays off by default because the reference's consumer computes the whole field (src/consumer.cpp:54).
        if (eng && sw.scan_fused_final) (void)tw_set_option(eng, TW_OPT_SCAN_FUSED_FINAL, 1);
    }

    // The first refusal of an extra: the consumer goes on without an engine (every pair answers `reason`) and with no extra in
    // force; no option call follows
    void drop_engine(const std::string& reason)
    {
        eng_err = reason;
        tw_engine_destroy(eng);
        eng = nullptr;
        extras = PairExtras();
    }
    // The extras that are engine options (PairExtras): each is set once, here, in this order; every batch of the engine then
    // carries it.  One that is off makes no call, and the bands are off while the shift is.
    void set_extras()
    {
        if (!eng || !shared) return;
        extras = shared->extras;
        if (!extras.shift) extras.shiftBands = 0;
        const struct {
            const char* label;  // in the error text
            int option;
            int PairExtras::*setting;
            bool linked;  // the library has the call that collects the extra
        } rows[] = {
            {"regions", TW_OPT_REGIONS, &PairExtras::regions, tw_wait_regions != nullptr},
            {"residual", TW_OPT_RESIDUAL, &PairExtras::residual, tw_ticket_changes != nullptr},
            {"shift", TW_OPT_SHIFT, &PairExtras::shift, tw_ticket_shift != nullptr},
            {"shiftBands", TW_OPT_SHIFT_BANDS, &PairExtras::shiftBands, tw_ticket_shift_bands != nullptr},
        };
        for (const auto& row : rows) {
            const int value = extras.*row.setting;
            if (!value) continue;
            const tw_status r = row.linked ? tw_set_option(eng, row.option, value) : TW_E_UNSUPPORTED;
            if (r != TW_OK) return drop_engine(std::string("engine: ") + row.label + ": " + tw_strerror(r));
        }
    }
    // Diff images have no option to set — the picture is rendered per ticket, on request.  What can be known to fail is refused
    // now: a library without the calls, a tolerance outside 0 .. 255, a directory that does not exist or cannot be written to.
    // (A picture that fails later — the disk fills up, the device refuses — is logged and the pair answered without the key.)
    std::string check_overlay() const
    {
        struct stat st;
        const std::string& dir = extras.overlayDir;
        if (dir.empty()) return std::string();
        if (!tw_ticket_hits || !tw_ticket_overlay) return tw_strerror(TW_E_UNSUPPORTED);
        if (extras.overlayTol < 0 || extras.overlayTol > 255) return tw_strerror(TW_E_BAD_PARAMETER);
        if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || access(dir.c_str(), W_OK | X_OK) != 0)
            return "not a writable directory: " + dir;
        return std::string();
    }
    // Profiling selection, the epoch, the resident cache — and the consumer says that it is ready
    void finish_start()
    {
        prof = eng && shared && shared->profile;
        if (prof) {
            (void)tw_prof_select(eng, TW_K_BLUR_SOLVE, 0);
            (void)tw_prof_select(eng, TW_K_POLYEXP, 0);
        }
        my_epoch = shared ? shared->epoch.load() : 0;
        const size_t budget = shared && shared->residentBytes > 0 ? (size_t)shared->residentBytes : 0;
        const bool resident_on = eng && budget > 0 && tw_image_keep && tw_image_release && tw_submit_image_png && tw_submit_image_jpeg;
        cache.reset(new ResidentCache(eng, resident_on ? budget : 0));
        mine.ready = true;
        mine.engineError = eng_err;
        publish();
    }

    // Fair share (round 5; the N = 8 ceiling run on the stub backend, tests/test_host_queue.py): a consumer keeps up to
    // three batches going, so near the END of a run — or for a run as short as BASELINE config 4's 2 048 pairs on 8 GPUs —
    // three consumers used to hold nine full batches while five idled (21.6 k instead of 32.7 k pairs/s).  What is left
    // (queued + in flight everywhere) is shared evenly: a consumer that already holds its share delivers its oldest batch
    // before it takes more, and never takes more than what brings it up to the share.
    long own_inflight() const
    {
        long k = 0;
        for (const Staged& s : prev) k += s.submitted && !s.done;
        for (const Staged& s : prev2) k += s.submitted && !s.done;
        return k;
    }
    long fair_share()
    {
        const long total = (long)req.size() + (shared ? shared->inflight.load() : own_inflight());
        return (total + (long)n_consumers - 1) / (long)n_consumers;
    }
    void deliver_down_to_share()
    {
        for (long own = own_inflight(); own > 0 && own >= fair_share() + sw.fair_slack; own = own_inflight()) {
            if (!prev2.empty()) collect_all(prev2);
            else collect_all(prev);
        }
    }

    // The next batch: one job (waiting for it if need be), then whatever is queued up to the take size.  false: the queue stopped
    bool take_batch(Batch& b)
    {
        Request first;
        if (!req.tryPopNow(first)) {
            collect_all(prev2);  // nothing queued: deliver what is outstanding before blocking
            collect_all(prev);
            read_prof(true);   // idle: nothing of ours is in flight, so the event read's synchronise costs nothing
            publish();
            const long long w0 = steady_ns();
            if (!req.tryPop(first)) return false;
            if (mine.firstJobNs) mine.waitMs += (double)(steady_ns() - w0) * 1e-6;  // blocked on an empty queue
        }
        if (shared && shared->epoch.load() != my_epoch) {
            // Manager::markEpoch(): counters restart here (the manager marks an epoch only while the queue is empty
            // and every response has arrived, so nothing of this consumer is in flight)
            my_epoch = shared->epoch.load();
            read_prof(false);
            mine.pairs = mine.batches = mine.overlayFailures = 0;
            mine.firstJobNs = mine.lastResponseNs = 0;
            mine.waitMs = 0;
            mine.profMs[0] = mine.profMs[1] = 0;
            mine.profLaunches[0] = mine.profLaunches[1] = 0;
        }
        if (!mine.firstJobNs) mine.firstJobNs = steady_ns();
        std::vector<Staged>& jobs = b.jobs;
        jobs.resize(1);
        jobs[0].req = std::move(first);
        // a consumer takes at most its share of what is queued, so that a short queue is spread over all GPUs
        // (a greedy grab of `batch` jobs starves the other consumers)
        // (its share of the queue alone, and — above — of everything that is left including what the engines still hold)
        // (round 6: the share of the QUEUE ALONE is no longer a limit of its own.  With it a burst of 2 048 jobs on 8 consumers
        // was handed out as 128, 127, 128, 127, ... and then 1/8 of whatever was left — 112, 98, 85, 49, 42, 25, 21, ... 2, 1,
        // 1, 1: three consumers ended 20 % short of their 256 and one of them worked the tail off in 30 batches of a few
        // pairs.  The fair share of EVERYTHING that is left already spreads a short queue: 10 jobs on 8 consumers are 2 each.)
        const long room = fair_share() + sw.fair_slack - own_inflight();
        const size_t take = std::max<size_t>(1, std::min<size_t>((size_t)batch_size, (size_t)std::max(1L, room)));
        if (sw.debug_takes)
            fprintf(stderr, "take t=%.3f ms consumer %d queue %zu inflight %ld own %ld share %ld -> take %zu\n", (double)(steady_ns() % 10000000000LL) * 1e-6,
                    id, req.size(), shared ? shared->inflight.load() : -1L, own_inflight(), fair_share(), take);
        Request more;
        while (jobs.size() < take && req.tryPopNow(more)) {
            jobs.emplace_back();
            jobs.back().req = std::move(more);
        }
        if (log_stream())
            for (const Staged& s : jobs)  // src/consumer.cpp:49
                TW_LOGF("consume: %s <-> %s\n", s.req.expect_image.c_str(), s.req.target_image.c_str());
        mine.batches++;
        b.t0 = b.t1 = b.t2 = b.t3 = steady_ns();
        return true;
    }

    // Phase 0 (resident expected images): stat every expected file; one that is cached, or that a pair in flight or
    // earlier in this batch is about to keep, is neither read nor decoded below
    void match_resident(Batch& b)
    {
        if (!cache->on()) return;
        std::vector<Staged>& jobs = b.jobs;
        for (size_t j = 0; j < jobs.size(); j++) {
            Staged& s = jobs[j];
            const std::string& path = s.req.expect_image;
            if (s.req.raw.expect || path.empty()) continue;
            s.rkey = file_identity(path);
            cache->note_identity(path, s.rkey);
            if (s.rkey.empty()) continue;  // (no such file: the path below answers "Can't open")
            if (ResidentCache::Entry* en = cache->lookup(s.rkey, path)) {
                s.hit = en;
                s.w = s.side[0].w = en->w;
                s.h = s.side[0].h = en->h;
                continue;
            }
            if ((s.keep = cache->find_pending(s.rkey))) {
                s.follower = true;
                s.w = s.side[0].w = s.keep->w;
                s.h = s.side[0].h = s.keep->h;
                continue;
            }
            for (size_t q = 0; q < j && !s.follower; q++)
                if (jobs[q].rkey == s.rkey && !jobs[q].no_expected_file()) {
                    s.keep = jobs[q].keep;
                    s.follower = true;
                    s.leader = (int)q;
                }
            if (!s.follower) s.keep = std::make_shared<ResidentCache::Keep>();
        }
    }

    // decode pool: once the flow runs on the GPU the two imreads of a pair are > 99 % of the wall time
    // (SURVEY §8 f1), so the pairs of a batch are decoded side by side
    // Phase 1 (pool): read every file.  A PNG the device can finish (tw_png_on_device: not interlaced, no 16-bit
    // colour) is only PARSED here; when every image of the batch is one, the arena is sized from the headers and the pool
    // inflates straight into it (round 4: the intermediate buffers — inflate output, its copy, the copy into the
    // arena, three 2 MB allocations per 1080p image — were a third of a batch's host time).
    void open_files(Batch& b)
    {
        b.op = std::vector<Opened>(2 * b.jobs.size());
        parallel_for(2 * b.jobs.size(), (size_t)decode_threads, [&](size_t i) {
            const Staged& s = b.jobs[i >> 1];
            const std::string& path = s.path((int)(i & 1));
            if (s.req.raw.expect || path.empty() || b.skipped(i)) return;
            Opened& o = b.op[i];
            o.read_ok = read_file(path, o.file);
            if (o.read_ok && sw.device_png && eng && o.file.size() >= 8 && o.file[0] == 0x89 && o.file[1] == 'P')
                o.rows_ok = png_parse(o.file, o.st) && o.st.device_rows(sw.png_kinds);
        });
        b.arena = &arena[arena_idx];  // (its last user was the batch three back: collected before this one is submitted)
        arena_idx = (arena_idx + 1) % 3;
    }

    static constexpr size_t kArenaSlotMax = (size_t)64 << 20;  // one 8192 x 8192 image
    static constexpr size_t kArenaMax = (size_t)4 << 30;       // per arena, three arenas per consumer
    // the arena is sized from PNG HEADERS, before anything is inflated.  Up to a 4K RGBA screenshot per
    // slot (kArenaFullBatchSlot) it is sized for a full batch at once (no regrowth while a batch fills up); a
    // larger slot gets only what the jobs actually present need, and an arena that an unusual batch blew up is
    // given back as soon as a batch needs less than a quarter of it — one 8192 x 8192 header pair no longer pins
    // 3 x 4 GiB per consumer for the life of the process (worst cases: INTEGRATION.md).
    static constexpr size_t kArenaFullBatchSlot = (size_t)40 << 20;
    static constexpr size_t kArenaShrinkAbove = (size_t)1 << 30;
    // the batch's arena holds two slots of `slot` bytes per job, or as much of that as the bounds allow (the only step
    // that calls tw_host_alloc / tw_host_free, on the consumer's own thread)
    void size_arena(Batch& b, size_t slot)
    {
        Arena& ar = *b.arena;
        const size_t need = std::min(kArenaMax, slot * 2 * b.jobs.size());
        if (!eng || !slot) return;
        const bool oversized = ar.base && ar.cap > kArenaShrinkAbove && need <= ar.cap / 4;
        if (need <= ar.cap && !oversized) return;
        if (ar.base) (void)tw_host_free(eng, ar.base);
        ar.base = nullptr;
        ar.cap = 0;
        void* hp = nullptr;
        // a full batch of this size (no regrowth), within the bound — for ordinary slots only
        const size_t full = slot <= kArenaFullBatchSlot ? slot * 2 * (size_t)batch_size : need;
        const size_t want = std::min(kArenaMax, std::max(need, full));
        if (tw_host_alloc(eng, want, &hp) == TW_OK) {
            ar.base = (uint8_t*)hp;
            ar.cap = want;
        }
    }

    // The fast path is open when every file of the batch is a PNG whose rows the device finishes and the arena has a slot
    // for each: b.slot is set and the arena sized from the headers.  false: decode_and_copy
    bool arena_from_headers(Batch& b)
    {
        bool fast = !b.op.empty();
        size_t fslot = 0;
        for (size_t i = 0; i < b.op.size(); i++) {
            if (b.skipped(i)) continue;
            const Opened& o = b.op[i];
            fast = fast && o.rows_ok;
            fslot = std::max(fslot, (o.st.total + 8 + 255) / 256 * 256);
        }
        if (!fast || fslot > kArenaSlotMax) return false;
        size_arena(b, fslot);
        b.slot = fslot;
        return b.arena->base && fslot * 2 * b.jobs.size() <= b.arena->cap;
    }
    // Phase 2 (pool): inflate into the arena slot; every row's filter type is checked as libpng does
    void inflate_into_arena(Batch& b)
    {
        parallel_for(2 * b.jobs.size(), (size_t)decode_threads, [&](size_t i) {
            if (b.skipped(i)) return;
            Opened& o = b.op[i];
            Staged& s = b.jobs[i >> 1];
            Staged::Side& sd = s.side[i & 1];
            uint8_t* dst = b.arena->base + b.slot * i;
            bool ok = png_inflate(o.st, dst);
            const size_t rs = o.st.row_bytes();  // the kind's row length
            for (int y = 0; y < o.st.h && ok; y++) ok = dst[(size_t)y * rs] <= 4;
            if (!ok) sd.err = cant_open(s.path((int)(i & 1)));
            sd.w = o.st.w;
            sd.h = o.st.h;
            sd.kind = o.st.kind();
            std::vector<uint8_t>().swap(o.file);
            std::vector<uint8_t>().swap(o.st.idat);
        });
        b.t1 = steady_ns();
    }
    // ... and the pairs are staged where they lie: only a pair that the HOST is to reconcile leaves the arena
    void stage_from_arena(Batch& b)
    {
        for (size_t j = 0; j < b.jobs.size(); j++) {
            Staged& s = b.jobs[j];
            Staged::Side &e = s.side[0], &t = s.side[1];
            // (a resident expected image: its size is the cache entry's, or that of the pair that keeps it)
            inherit_from_leader(s, b.jobs);
            if (pair_refused(s)) continue;
            s.w = e.w;
            s.h = e.h;
            uint8_t* da = b.arena->base + b.slot * (2 * j);
            uint8_t* db = da + b.slot;
            switch (size_rule(s.w, s.h, t.w, t.h, sw.device_reconcile)) {
                case SizeRule::DontMatch: s.err = "Don't match image size"; continue;
                case SizeRule::ReconcileOnHost:
                    // TW_DEVICE_RECONCILE=0: the reconcile on the host, on copies outside the arena
                    if (!s.no_expected_file()) e.bytes.assign(da, da + b.op[2 * j].st.total);
                    t.bytes.assign(db, db + b.op[2 * j + 1].st.total);
                    if (reconcile_on_host(s)) point_at_own_bytes(s);
                    continue;
                case SizeRule::ReconcileOnDevice:  // within 5 px: the pair stays in the arena, the device resizes the target
                    s.device_reconciles = true;
                    break;
                case SizeRule::Same: break;
            }
            e.p = da;
            t.p = db;
            s.stride = s.w;
        }
    }

    // The other path: every image is decoded into a buffer of its own, the pair is prepared there, and what fits is copied
    // into the arena
    void decode_and_copy(Batch& b)
    {
        std::vector<Staged>& jobs = b.jobs;
        parallel_for(2 * jobs.size(), (size_t)decode_threads, [&](size_t i) {
            decode_one(jobs[i >> 1], (int)(i & 1), sw, device_jpeg && eng, b.op[i].read_ok ? &b.op[i].file : nullptr);
            std::vector<uint8_t>().swap(b.op[i].file);
        });
        b.t1 = steady_ns();
        for (Staged& s : jobs) inherit_from_leader(s, jobs);
        parallel_for(jobs.size(), (size_t)decode_threads, [&](size_t j) { prepare(jobs[j], sw.device_reconcile); });
        // The arena is sized AFTER prepare(), over the pairs that decoded and reconciled (a header with
        // huge dimensions over a damaged stream must not size it), and it is bounded: a pair larger than
        // kArenaSlotMax, or one the bounded arena has no room for, keeps its pageable buffers (tw_submit_u8 stages
        // those itself — always correct, one memcpy slower).
        size_t slot = 0;
        for (const Staged& s : jobs) {
            if (!s.err.empty() || s.req.raw.expect) continue;
            // (an image is w * h gray bytes or, still filtered, h rows of its kind's PngKind::row_bytes(w))
            const size_t nb = (std::max(s.side[0].bytes.size(), s.side[1].bytes.size()) + 255) / 256 * 256;
            if (nb <= kArenaSlotMax) slot = std::max(slot, nb);
        }
        size_arena(b, slot);
        const Arena& ar = *b.arena;
        parallel_for(jobs.size(), (size_t)decode_threads, [&](size_t j) {
            Staged& s = jobs[j];
            Staged::Side &e = s.side[0], &t = s.side[1];
            if (!s.err.empty() || s.req.raw.expect || !ar.base || !slot) return;
            if (std::max(e.bytes.size(), t.bytes.size()) > slot || (2 * j + 2) * slot > ar.cap) return;  // stays pageable
            uint8_t* da = ar.base + slot * (2 * j);
            uint8_t* db = da + slot;
            if (!e.bytes.empty()) memcpy(da, e.bytes.data(), e.bytes.size());
            memcpy(db, t.bytes.data(), t.bytes.size());
            e.p = da;
            t.p = db;
            std::vector<uint8_t>().swap(e.bytes);
            std::vector<uint8_t>().swap(t.bytes);
        });
    }

    // one engine batch is homogeneous in size: group equal sizes so that a mixed queue makes few batches
    // (responses are delivered in completion order anyway, like the reference's)
    // (Staged::leader indexes the batch as it was before this: nothing reads it afterwards)
    void sort_by_size(Batch& b)
    {
        b.t2 = steady_ns();
        std::stable_sort(b.jobs.begin(), b.jobs.end(), [](const Staged& x, const Staged& y) {
            return x.w != y.w ? x.w < y.w : x.h < y.h;
        });
    }

    // A pair behind one that was to keep its expected image, and that one failed before it did (its target, the
    // sizes): this pair is decoded again on its own, expected file included, and goes the ordinary way
    void redecode_orphaned_follower(Staged& s)
    {
        s.follower = false;
        s.leader = -1;
        s.keep = std::make_shared<ResidentCache::Keep>();
        s.side[0] = s.side[1] = Staged::Side();
        s.device_reconciles = false;
        decode_one(s, 0, sw, false, nullptr);
        decode_one(s, 1, sw, false, nullptr);
        prepare(s, sw.device_reconcile);
    }
    // the image on the device that stands in for the pair's expected file, if any
    tw_image* resident_image_of(Staged& s)
    {
        if (s.hit) return s.hit->img;
        if (!s.follower) return nullptr;
        s.uses_keep = s.keep->img != nullptr;
        return s.uses_keep ? s.keep->img : cache->image_now(s.rkey, s.req.expect_image);
    }
    tw_status submit_to_engine(Staged& s)
    {
        const Staged::Side &e = s.side[0], &t = s.side[1];
        const tw_image* image = resident_image_of(s);
        const int span = s.req.span;
        const double thr = s.req.threshold;
        if (!s.req.ignore.empty()) return submit_to_engine_ignoring(s, image);
        switch (entry_point(s, image != nullptr)) {
            case EntryPoint::ImageJpeg: {
                const tw_jpeg_luma lb = luma_of(t);
                return tw_submit_image_jpeg(eng, image, &lb, span, thr, nullptr, nullptr, &s.ticket);
            }
            case EntryPoint::ImagePng: {
                const tw_png_rows rb = rows_of(t);
                return tw_submit_image_png(eng, image, &rb, span, thr, nullptr, nullptr, &s.ticket);
            }
            case EntryPoint::Png: {
                const tw_png_rows ra = rows_of(e), rb = rows_of(t);
                return tw_submit_png(eng, &ra, &rb, span, thr, nullptr, nullptr, &s.ticket);
            }
            case EntryPoint::Jpeg: {
                const tw_jpeg_luma la = luma_of(e), lb = luma_of(t);
                return tw_submit_jpeg(eng, &la, &lb, span, thr, nullptr, nullptr, &s.ticket);
            }
            case EntryPoint::U8Sized:
                return tw_submit_u8_sized(eng, e.p, s.w, s.h, s.stride, t.p, t.w, t.h, t.w, span, thr, nullptr, nullptr, &s.ticket);
            case EntryPoint::U8: break;
        }
        return tw_submit_u8(eng, e.p, t.p, s.w, s.h, s.stride, span, thr, &s.ticket);
    }
    // A pair with ignore rectangles: the _ignore form of the call it would take without them, the gray fallbacks included
    // (a file the host had to finish, a host-side reconcile, BMP, PNM and raw pairs all go to tw_submit_u8_ignore): the
    // device always applies the mask
    tw_status submit_to_engine_ignoring(Staged& s, const tw_image* image)
    {
        const Staged::Side &e = s.side[0], &t = s.side[1];
        const int span = s.req.span, n = (int)std::min<size_t>(s.req.ignore.size(), (size_t)TW_MAX_IGNORE + 1);
        const double thr = s.req.threshold;
        const tw_rect* rects = s.req.ignore.data();
        if (!tw_submit_u8_ignore || !tw_submit_png_ignore || !tw_submit_jpeg_ignore || !tw_submit_image_png_ignore ||
            !tw_submit_image_jpeg_ignore)
            return TW_E_UNSUPPORTED;  // (an engine library from before the ignore regions)
        switch (entry_point(s, image != nullptr)) {
            case EntryPoint::ImageJpeg: {
                const tw_jpeg_luma lb = luma_of(t);
                return tw_submit_image_jpeg_ignore(eng, image, &lb, span, thr, nullptr, nullptr, rects, n, &s.ticket);
            }
            case EntryPoint::ImagePng: {
                const tw_png_rows rb = rows_of(t);
                return tw_submit_image_png_ignore(eng, image, &rb, span, thr, nullptr, nullptr, rects, n, &s.ticket);
            }
            case EntryPoint::Png: {
                const tw_png_rows ra = rows_of(e), rb = rows_of(t);
                return tw_submit_png_ignore(eng, &ra, &rb, span, thr, nullptr, nullptr, rects, n, &s.ticket);
            }
            case EntryPoint::Jpeg: {
                const tw_jpeg_luma la = luma_of(e), lb = luma_of(t);
                return tw_submit_jpeg_ignore(eng, &la, &lb, span, thr, nullptr, nullptr, rects, n, &s.ticket);
            }
            case EntryPoint::U8Sized:
                return tw_submit_u8_ignore(eng, e.p, s.w, s.h, s.stride, t.p, t.w, t.h, t.w, span, thr, nullptr, nullptr, rects, n,
                                           &s.ticket);
            case EntryPoint::U8: break;
        }
        return tw_submit_u8_ignore(eng, e.p, s.w, s.h, s.stride, t.p, s.w, s.h, s.stride, span, thr, nullptr, nullptr, rects, n,
                                   &s.ticket);
    }
    // a miss: the image the batch sees stays on the device (one device-to-device copy behind its decode), and
    // enters the cache when the pair has answered OK
    void keep_expected(Staged& s)
    {
        if (!cache->on() || s.rkey.empty() || s.no_expected_file() || !s.keep) return;
        if (tw_image_keep(eng, s.ticket, TW_KEEP_EXPECT, &s.kept) == TW_OK) cache->open_pending(s.rkey, s.keep, s.kept, s.w, s.h);
        else s.kept = nullptr;
    }
    void submit_pair(Batch& b, size_t k)
    {
        Staged& s = b.jobs[k];
        if (s.err.empty() && !eng) s.err = eng_err;
        if (!s.err.empty()) return;
        if (s.follower && !s.keep->img && !cache->has(s.rkey)) {
            redecode_orphaned_follower(s);
            if (!s.err.empty()) return;
        }
        tw_status r = submit_to_engine(s);
        if (r == TW_E_BUSY) {
            // every batch context of the engine is owed to us (each size change opens one): collect what
            // is outstanding, then this job starts a fresh batch
            collect_all(prev2);
            collect_all(prev);
            for (size_t q = 0; q < k; q++) collect(b.jobs[q]);
            r = submit_to_engine(s);
        }
        if (r == TW_OK) {
            s.submitted = true;
            if (shared) shared->inflight++;
            keep_expected(s);
        } else s.err = engine_error(eng, r);
    }

    void unpin_and_flush(Batch& b)
    {
        for (Staged& s : b.jobs)  // (submitted or refused: the batch holds the image now, the cache entry may go)
            if (s.hit) {
                cache->unpin(s.hit);
                s.hit = nullptr;
            }
        cache->sweep();
        if (eng) (void)tw_flush(eng);  // a partly filled batch starts now, not when its first result is asked for
        b.t3 = steady_ns();
    }

    void deliver_refused_and_rotate(Batch& b)
    {
        const size_t njobs = b.jobs.size();
        for (Staged& s : b.jobs)
            if (!s.submitted) collect(s);  // errors do not wait for the GPU
        collect_all(prev2);  // the batch before the previous one: its results have had two batches' time to arrive
        prev2 = std::move(prev);
        prev = std::move(b.jobs);
        if (sw.debug_batchtime)
            fprintf(stderr, "twhost: consumer %d batch of %zu: decode %.2f ms, prepare + arena %.2f, submit + flush %.2f, "
                            "previous batch's results %.2f\n", id, njobs, (b.t1 - b.t0) * 1e-6, (b.t2 - b.t1) * 1e-6,
                    (b.t3 - b.t2) * 1e-6, (steady_ns() - b.t3) * 1e-6);
    }

    // Before the wait, the extras that are read from the ticket — the changes, then the shift, then its bands — up to the first
    // that fails.  Each call leaves the ticket to the wait, which answers a pair's own error as it always did.
    Asked ask_extras(const Staged& s, int cap)
    {
        Asked a;
        ExtrasScratch& x = scratch;
        if (extras.residual) a.status = tw_ticket_changes(eng, s.ticket, x.change_recs.data(), cap, &x.nchg);
        if (extras.shift && a.status == TW_OK) a.status = tw_ticket_shift(eng, s.ticket, &x.shift_rec);
        if (extras.shiftBands && a.status == TW_OK) {
            // (a pair's own height decides the number of its bands: asked again when the array was too short)
            a.status = tw_ticket_shift_bands(eng, s.ticket, x.band_recs.data(), (int)x.band_recs.size(), &x.nbands);
            if (a.status == TW_OK && x.nbands > (int)x.band_recs.size()) {
                x.band_recs.resize((size_t)x.nbands);
                a.status = tw_ticket_shift_bands(eng, s.ticket, x.band_recs.data(), x.nbands, &x.nbands);
            }
        }
        if (a.status != TW_OK) a.message = engine_error(eng, a.status);
        return a;
    }
    // The diff image: the count the wait will report, with the changes so far, is the status the pair will get, and a pair that
    // will be SUSPICIOUS gets its picture.  Returns the file's path, empty where there is none; a picture that fails is said
    // aloud (TW_LOG) and counted, and the pair keeps its answer.  A pair's own error is left to the wait.
    std::string draw_overlay(const Staged& s, int cap)
    {
        int nh = 0;
        if (tw_ticket_hits(eng, s.ticket, &nh) != TW_OK) return std::string();
        ExtrasScratch& x = scratch;
        std::vector<Change> so_far;
        if (extras.residual) so_far.assign(x.change_recs.begin(), x.change_recs.begin() + std::max(0, std::min(x.nchg, cap)));
        if (strcmp(pair_status((size_t)std::max(nh, 0), so_far, extras.residualMin), "SUSPICIOUS")) return std::string();
        const ptrdiff_t pitch = 3 * (ptrdiff_t)s.w;
        x.overlay_px.resize((size_t)pitch * (size_t)s.h);
        const tw_overlay_out oo = {x.overlay_px.data(), pitch, TW_OVERLAY_RGB8};
        const std::string path = overlay_path(extras.overlayDir, s.req.target_image);
        const tw_status ro = tw_ticket_overlay(eng, s.ticket, extras.overlayTol, &oo);
        if (ro == TW_OK && png_write_rgb8(path, x.overlay_px.data(), s.w, s.h, pitch)) return path;
        mine.overlayFailures++;
        TW_LOGF("overlay: %s: %s\n", path.c_str(), ro == TW_OK ? "cannot write the file" : engine_error(eng, ro).c_str());
        return std::string();
    }
    // The collecting wait — with the regions on, the one that returns them — and what hangs on its answer: the count of pairs
    // in flight and the resident image this pair kept
    Waited wait_pair(Staged& s, int cap)
    {
        Waited w;
        ExtrasScratch& x = scratch;
        w.status = extras.regions ? tw_wait_regions(eng, s.ticket, hits.get(), cap, &w.n, x.region_of.data(), x.region_recs.data(),
                                                    TW_MAX_REGIONS, &x.nreg, &w.sec)
                                  : tw_wait(eng, s.ticket, hits.get(), cap, &w.n, &w.sec);
        if (shared) shared->inflight--;
        if (s.kept) {
            cache->settle(s.rkey, s.req.expect_image, s.keep, s.kept, s.w, s.h, w.status);
            s.kept = nullptr;
        }
        return w;
    }
    // Why a waited-for pair answers ERROR, or empty: a shared expected image that turned out bad, a bad palette index that the
    // engine names, the wait's own error, an extra's error — in this order
    std::string pair_error(const Staged& s, tw_status waited, const Asked& asked)
    {
        if (s.uses_keep && s.keep->expect_bad) return cant_open(s.req.expect_image);
        if (waited == TW_E_BAD_IMAGE_FORMAT && (s.side[0].kind.rows() || s.side[1].kind.rows())) {
            // a palette index without a PLTE entry, found by the device: cv::imread fails on that file, and the
            // ticket's message names it (the expected image first, as the reference opens it first)
            const bool target = strstr(tw_last_error(eng), "target") != nullptr;
            return cant_open(s.path(target));
        }
        if (waited != TW_OK) return engine_error(eng, waited);
        return asked.message;
    }
    void fill_response(Response& out, const Staged& s, const Waited& w, int cap, const std::string& overlay_file)
    {
        const ExtrasScratch& x = scratch;
        const tw_vector* const v = hits.get();
        out.vectors.resize((size_t)std::min(w.n, cap));
        for (size_t i = 0; i < out.vectors.size(); i++) out.vectors[i] = {v[i].x, v[i].y, v[i].dx, v[i].dy};
        if (extras.residual) {
            out.hasChanges = true;
            out.changes.assign(x.change_recs.begin(), x.change_recs.begin() + std::max(0, std::min(x.nchg, cap)));
        }
        if (extras.shift) {
            out.hasShift = true;
            out.shift = Shift{x.shift_rec.dx, x.shift_rec.dy, x.shift_rec.applied != 0};
        }
        if (extras.shiftBands) {
            out.hasBands = true;
            for (int b = 0; b < x.nbands; b++) {
                ShiftBand sb;
                sb.y = x.band_recs[b].y, sb.rows = x.band_recs[b].rows, sb.dy = x.band_recs[b].dy, sb.applied = x.band_recs[b].applied != 0;
                out.bands.push_back(sb);
            }
        }
        if (extras.regions) {
            out.hasRegions = true;
            out.regionCount = x.nreg;
            out.regionOf.assign(x.region_of.begin(), x.region_of.begin() + (long)out.vectors.size());
            out.regions.assign(x.region_recs.begin(), x.region_recs.begin() + std::max(0, std::min(x.nreg, (int)TW_MAX_REGIONS)));
        }
        // (the shift leaves the status alone: a moved page has vectors above the threshold and is SUSPICIOUS as ever)
        out.status = pair_status(out.vectors.size(), out.changes, extras.residualMin);  // src/consumer.cpp:77
        out.time = w.sec;
        out.expect_image = s.req.expect_image;
        out.target_image = s.req.target_image;
        out.span = s.req.span;
        out.threshold = s.req.threshold;
        out.height = s.h;
        out.width = s.w;
        out.overlay = overlay_file;
    }

    // wait for one job and hand its response to the pump
    void collect(Staged& s)
    {
        if (s.done) return;
        s.done = true;
        Response out;
        if (s.submitted) {
            const int cap = std::max(1, tw_grid_capacity(s.w, s.h, s.req.span));
            if ((size_t)cap > hits_cap) {
                hits.reset(new tw_vector[(size_t)cap]);
                hits_cap = (size_t)cap;
            }
            scratch.reserve(cap, extras);
            const Asked asked = ask_extras(s, cap);
            const std::string overlay_file =
                !extras.overlayDir.empty() && asked.status == TW_OK ? draw_overlay(s, cap) : std::string();
            const Waited w = wait_pair(s, cap);
            s.err = pair_error(s, w.status, asked);
            if (s.err.empty()) fill_response(out, s, w, cap, overlay_file);
        }
        if (!s.err.empty()) {
            out = Response();
            out.status = "ERROR";  // src/consumer.cpp:85-88
            out.reason = s.err;
        }
        TW_LOGF("finish optical flow: %g\n", (double)out.time);  // src/consumer.cpp:55
        mine.pairs++;
        mine.lastResponseNs = steady_ns();
        publish();  // before the response leaves: whoever has seen N responses sees N pairs in the stats
        out.pushedNs = mine.lastResponseNs;
        res.push(std::move(out));
    }
    void collect_all(std::vector<Staged>& v)
    {
        for (Staged& s : v) collect(s);
        v.clear();
    }

    void shut_down()
    {
        collect_all(prev2);
        collect_all(prev);
        read_prof(true);
        publish();
        cache.reset();  // Manager::stop: every resident image goes back, while the engine exists
        for (Arena& ar : arena)
            if (eng && ar.base) (void)tw_host_free(eng, ar.base);
        if (eng) tw_engine_destroy(eng);
        TW_LOGF("finish consumer%d\n", id);  // src/consumer.cpp:92
    }
};
}  // namespace

void Consumer::run()
{
    ConsumerRun c(id_, req_, res_, params_, batch_, decode_threads_, n_consumers_, shared_);
    c.bind_device_and_numa();
    c.create_engine();
    c.set_extras();
    const std::string overlay_err = c.check_overlay();
    if (!overlay_err.empty()) c.drop_engine("engine: overlay: " + overlay_err);
    c.finish_start();
    for (;;) {
        c.deliver_down_to_share();
        Batch b;
        if (!c.take_batch(b)) break;
        c.match_resident(b);
        c.open_files(b);
        if (c.arena_from_headers(b)) {
            c.inflate_into_arena(b);
            c.stage_from_arena(b);
        } else {
            c.decode_and_copy(b);
        }
        c.sort_by_size(b);
        for (size_t k = 0; k < b.jobs.size(); k++) c.submit_pair(b, k);
        c.unpin_and_flush(b);
        c.deliver_refused_and_rotate(b);
    }
    c.shut_down();
}


// ---------------------------------------------------------------------------------------------------
// Manager
// ---------------------------------------------------------------------------------------------------
Manager::~Manager()
{
    stop();
    if (pump_.joinable()) pump_.join();
    for (Consumer* c : consumers_) delete c;
}

void Manager::start(const Parameter& p)
{
    param_ = p;
    running_ = true;
    const int ndev = tw_device_count();
    // numThreads consumers as in src/manager.cpp:55-59, at most `perDevice` of them per GPU (default 1: more
    // consumers than GPUs only time-share a device, the surplus is folded into the per-consumer batch instead;
    // TW_CONSUMERS_PER_DEVICE / Parameter::consumersPerDevice raise it — consumer i runs on device i % ndev)
    int per_dev = p.consumersPerDevice;
    if (per_dev <= 0)
        if (const char* ev = getenv("TW_CONSUMERS_PER_DEVICE")) per_dev = atoi(ev);
    if (per_dev <= 0) per_dev = 1;
    const int n = std::max(1, ndev > 0 ? std::min(p.numThreads, ndev * per_dev) : 1);
    // (a batch also bounds how many images decode side by side: 32 pairs = 64 decode tasks for the pool)
    const int batch = p.batch > 0 ? std::min(256, p.batch) : 32;
    // decode threads per consumer: TW_DECODE_THREADS, else the host cores shared between the consumers
    int dec = 0;
    if (const char* ev = getenv("TW_DECODE_THREADS")) dec = atoi(ev);
    if (dec <= 0) dec = std::max(1, std::min(16, (int)std::thread::hardware_concurrency() / n));
    shared_.profile = p.profileKernels;
    // the budget of every consumer's cache of resident expected images: Parameter::residentMB, else TW_RESIDENT_MB; 0 = off
    long long res_mb = p.residentMB;
    if (res_mb <= 0)
        if (const char* ev = getenv("TW_RESIDENT_MB")) res_mb = atoll(ev);
    shared_.residentBytes = res_mb > 0 ? res_mb << 20 : 0;
    shared_.extras = p.extras;
    shared_.stats.assign((size_t)n, ConsumerStats());
    for (int i = 0; i < n; i++) {
        consumers_.push_back(new Consumer(i, requestQueue_, responseQueue_, p.optParam, batch, dec, n, &shared_));
        consumers_.back()->start();
    }
    pump_ = std::thread([this] { work(); });
}

void Manager::waitReady()
{
    std::unique_lock<std::mutex> lk(shared_.m);
    shared_.cv.wait(lk, [&] {
        for (const ConsumerStats& s : shared_.stats)
            if (!s.ready) return false;
        return true;
    });
}

std::vector<ConsumerStats> Manager::consumerStats()
{
    std::lock_guard<std::mutex> lk(shared_.m);
    return shared_.stats;
}

void Manager::markEpoch()
{
    shared_.epoch++;
    std::lock_guard<std::mutex> lk(report_m_);
    pump_stats_ = PumpStats();
    pump_sum_us_ = 0;
}

PumpStats Manager::pumpStats()
{
    std::lock_guard<std::mutex> lk(report_m_);
    PumpStats p = pump_stats_;
    p.meanUs = p.delivered ? pump_sum_us_ / (double)p.delivered : 0;
    return p;
}

int Manager::request(const std::string& expect_image, const std::string& target_image)
{
    Request r;
    r.expect_image = expect_image;
    r.target_image = target_image;
    r.span = param_.span;
    r.threshold = param_.threshold;
    TW_LOGF("request: %s <-> %s\n", expect_image.c_str(), target_image.c_str());  // src/manager.cpp:74
    {
        std::lock_guard<std::mutex> lk(report_m_);
        report_.requestCount++;
    }
    requestQueue_.push(std::move(r));
    return 0;
}

int Manager::request(const std::string& expect_image, const std::string& target_image, const std::vector<Rect>& ignore)
{
    Request r;
    r.expect_image = expect_image;
    r.target_image = target_image;
    r.span = param_.span;
    r.threshold = param_.threshold;
    r.ignore = ignore;
    TW_LOGF("request: %s <-> %s (%zu ignore regions)\n", expect_image.c_str(), target_image.c_str(), ignore.size());
    {
        std::lock_guard<std::mutex> lk(report_m_);
        report_.requestCount++;
    }
    requestQueue_.push(std::move(r));
    return 0;
}

int Manager::requestRaw(const std::string& expect_name, const std::string& target_name, const RawPair& raw)
{
    Request r;
    r.expect_image = expect_name;
    r.target_image = target_name;
    r.span = param_.span;
    r.threshold = param_.threshold;
    r.raw = raw;
    {
        std::lock_guard<std::mutex> lk(report_m_);
        report_.requestCount++;
    }
    requestQueue_.push(std::move(r));
    return 0;
}

void Manager::stop()
{
    bool expected = false;
    if (!stopped_.compare_exchange_strong(expected, true)) return;
    running_ = false;
    responseQueue_.stop();
}

void Manager::work()
{
    Response res;
    while (responseQueue_.tryPop(res)) {  // src/manager.cpp:80-90 + notify() :102-116
        const long long t_pop = steady_ns();
        const bool is_err = res.status == "ERROR";
        {
            std::lock_guard<std::mutex> lk(report_m_);
            if (is_err) report_.errorCount++;
            else report_.dataCount++;
            if (res.pushedNs) {
                const double us = (double)(t_pop - res.pushedNs) * 1e-3;
                pump_stats_.delivered++;
                pump_sum_us_ += us;
                if (us > pump_stats_.maxUs) pump_stats_.maxUs = us;
            }
        }
        if (is_err) {
            if (obs_.onError) obs_.onError(res.reason);
        } else {
            if (obs_.onNext) obs_.onNext(res);
        }
        const double cb_ms = (double)(steady_ns() - t_pop) * 1e-6;
        std::lock_guard<std::mutex> lk(report_m_);
        pump_stats_.busyMs += cb_ms;
    }
    requestQueue_.stop();  // src/manager.cpp:93-97
    for (Consumer* c : consumers_) c->join();
    Report rep;
    {
        std::lock_guard<std::mutex> lk(report_m_);
        rep = report_;
    }
    if (obs_.onCompleted) obs_.onCompleted(rep);
}

}  // namespace twhost
