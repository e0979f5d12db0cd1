// tw_png_write.h — a PNG writer for the diff images of tw_ticket_overlay (PairExtras::overlayDir): colour type 2, depth 8, no
// interlace, every row with filter type 0, the zlib stream made of STORED deflate blocks.  No compression on purpose: stored
// blocks open in every viewer, the file is written for suspicious pairs only, and its cost is a CRC and an Adler-32 over the
// pixels.  Header-only, so that every program that links the fixed list of host sources keeps building.
#ifndef TW_PNG_WRITE_H
#define TW_PNG_WRITE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace twhost {

// CRC-32 of ISO/IEC 15948 annex D (the reflected polynomial 0xEDB88320), continued from `crc` (0 to start)
inline uint32_t png_crc32(uint32_t crc, const uint8_t* p, size_t n)
{
    static const struct Table {
        uint32_t t[256];
        Table()
        {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
                t[i] = c;
            }
        }
    } table;
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table.t[(crc ^ p[i]) & 255u] ^ (crc >> 8);
    return ~crc;
}

// Adler-32 of RFC 1950, continued from `adler` (1 to start); the sums are reduced every 5552 bytes, the most that cannot
// overflow 32 bits
inline uint32_t png_adler32(uint32_t adler, const uint8_t* p, size_t n)
{
    uint32_t a = adler & 0xffffu, b = adler >> 16;
    while (n > 0) {
        const size_t k = n < 5552 ? n : 5552;
        for (size_t i = 0; i < k; i++) {
            a += p[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
        p += k;
        n -= k;
    }
    return b << 16 | a;
}

inline void png_put32(std::vector<uint8_t>& v, uint32_t x)
{
    v.push_back((uint8_t)(x >> 24));
    v.push_back((uint8_t)(x >> 16));
    v.push_back((uint8_t)(x >> 8));
    v.push_back((uint8_t)x);
}

// one chunk: length, type, data, CRC over type and data
inline void png_put_chunk(std::vector<uint8_t>& out, const char type[4], const uint8_t* data, size_t n)
{
    png_put32(out, (uint32_t)n);
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    if (n) out.insert(out.end(), data, data + n);
    png_put32(out, png_crc32(0, out.data() + at, n + 4));
}

// The file's bytes for `height` rows of 3 * width RGB bytes, `pitch` bytes apart (bytes of the pitch behind a row are not
// read).  False for a size PNG cannot hold or this writer does not take: a side below 1, or a zlib stream beyond 2^31 - 1 bytes
// (one IDAT chunk).
inline bool png_encode_rgb8(const uint8_t* rgb, int width, int height, ptrdiff_t pitch, std::vector<uint8_t>& out)
{
    out.clear();
    if (!rgb || width < 1 || height < 1 || pitch < 3 * (ptrdiff_t)width) return false;
    const size_t row = 1 + 3 * (size_t)width, raw = row * (size_t)height;
    const size_t blocks = (raw + 65534) / 65535;  // (raw >= 4)
    const size_t zbytes = 2 + raw + 5 * blocks + 4;
    if (zbytes > 0x7fffffffu) return false;
    // the filtered rows: a 0 in front of each
    std::vector<uint8_t> stream(raw);
    for (int y = 0; y < height; y++) {
        stream[(size_t)y * row] = 0;
        memcpy(&stream[(size_t)y * row + 1], rgb + (ptrdiff_t)y * pitch, row - 1);
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    out.reserve(8 + 25 + 12 + zbytes + 12);
    out.insert(out.end(), sig, sig + 8);
    std::vector<uint8_t> ihdr;
    png_put32(ihdr, (uint32_t)width);
    png_put32(ihdr, (uint32_t)height);
    const uint8_t kind[5] = {8, 2, 0, 0, 0};  // depth, colour type, compression, filter, interlace
    ihdr.insert(ihdr.end(), kind, kind + 5);
    png_put_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    std::vector<uint8_t> z;
    z.reserve(zbytes);
    z.push_back(0x78);  // deflate, 32 KB window
    z.push_back(0x01);  // no dictionary, fastest; (0x78 << 8 | 0x01) % 31 == 0
    for (size_t o = 0; o < raw; o += 65535) {
        const size_t k = raw - o < 65535 ? raw - o : 65535;
        z.push_back(o + k == raw ? 1 : 0);  // BFINAL, BTYPE 00 = stored; the block starts at a byte boundary
        z.push_back((uint8_t)(k & 255));
        z.push_back((uint8_t)(k >> 8));
        z.push_back((uint8_t)(~k & 255));
        z.push_back((uint8_t)((~k >> 8) & 255));
        z.insert(z.end(), stream.begin() + (ptrdiff_t)o, stream.begin() + (ptrdiff_t)(o + k));
    }
    png_put32(z, png_adler32(1, stream.data(), raw));
    png_put_chunk(out, "IDAT", z.data(), z.size());
    png_put_chunk(out, "IEND", nullptr, 0);
    return true;
}

// ... written to `path` (replaced if it exists).  False when the size is refused or the file cannot be written whole.
inline bool png_write_rgb8(const std::string& path, const uint8_t* rgb, int width, int height, ptrdiff_t pitch)
{
    std::vector<uint8_t> bytes;
    if (!png_encode_rgb8(rgb, width, height, pitch, bytes)) return false;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return (fclose(f) == 0) && ok;
}

}  // namespace twhost
#endif
