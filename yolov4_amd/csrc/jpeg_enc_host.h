// Host stage of the JPEG encoder: geometry and quality-scaled tables for a new image, and the file itself from quantised
// coefficients: SOI, JFIF APP0, DQT, SOF0, DHT, SOS, the Huffman-coded interleaved scan with the standard (ITU-T T.81 Annex K)
// tables, EOI -- segment for segment what libjpeg-turbo writes by default (no optimised tables, restart markers, progression
// or EXIF).  Plain C++17, no HIP: jpeg_enc.hip exports it through the C ABI, and a stand-alone CPU program can include it too.
// Every write is checked against out_cap; a coefficient is never read at a dummy block.  No threads, no global state.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/yolov4_amd.h"

namespace y4jpegenc {

// zigzag position -> natural (row-major) position in the 8x8 block
static constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 tables K.1 / K.2 (natural order) and K.3 - K.6 (code counts per length, symbols in code order)
static const uint8_t kBaseQt[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kAcVals[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,
     66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,
     52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100,
     101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
     149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
     195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232,
     233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161,
     177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,
     41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,
     100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146,
     147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185,
     186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231,
     232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// the geometry y4_jpeg_parse_host gives for (width, height, ncomp, hs[0], vs[0]); false when the record differs from it
static inline bool info_ok(const y4_jpeg_info& f) {
    if (f.width < 1 || f.width > 65535 || f.height < 1 || f.height > 65535) return false;
    if (f.ncomp != 1 && f.ncomp != 3) return false;
    const int hv = f.hs[0] * 16 + f.vs[0];
    if (f.ncomp == 1 ? hv != 0x11 : (hv != 0x11 && hv != 0x21 && hv != 0x22)) return false;
    const int mx = (f.width + 8 * f.hs[0] - 1) / (8 * f.hs[0]), my = (f.height + 8 * f.vs[0] - 1) / (8 * f.vs[0]);
    if (f.mcus_x != mx || f.mcus_y != my) return false;
    long long count = 0;
    for (int c = 0; c < 3; ++c) {
        const int hs = c < f.ncomp ? (c == 0 ? f.hs[0] : 1) : 0, vs = c < f.ncomp ? (c == 0 ? f.vs[0] : 1) : 0;
        if (f.hs[c] != hs || f.vs[c] != vs || f.blocks_w[c] != mx * hs || f.blocks_h[c] != my * vs) return false;
        count += 64ll * f.blocks_w[c] * f.blocks_h[c];
    }
    return f.coef_count == count;
}

// blocks of component c that hold samples: ceil(ceil(extent * factor_c / factor_max) / 8); the rest of the padded grid is dummy
static inline int real_blocks_w(const y4_jpeg_info& f, int c) { return ((f.width * f.hs[c] + f.hs[0] - 1) / f.hs[0] + 7) / 8; }
static inline int real_blocks_h(const y4_jpeg_info& f, int c) { return ((f.height * f.vs[c] + f.vs[0] - 1) / f.vs[0] + 7) / 8; }

// a table is usable when every divisor is 1..255 (8-bit DQT) and, for colour, both chroma components share one
static inline bool qt_ok(const uint16_t* qt, int ncomp) {
    for (int i = 0; i < 64 * ncomp; ++i)
        if (qt[i] < 1 || qt[i] > 255) return false;
    return ncomp == 1 || memcmp(qt + 64, qt + 128, 64 * sizeof(uint16_t)) == 0;
}

inline int setup(int width, int height, int ncomp, int hs, int vs, int quality, y4_jpeg_info* info, uint16_t* qt /* [3][64] */) {
    if (!info || !qt) return Y4_ERR_NULL;
    if (quality < 1 || quality > 100) return Y4_ERR_SHAPE;
    y4_jpeg_info f;
    memset(&f, 0, sizeof(f));
    f.width = width;
    f.height = height;
    f.ncomp = ncomp;
    if (width < 1 || width > 65535 || height < 1 || height > 65535 || (ncomp != 1 && ncomp != 3)) return Y4_ERR_SHAPE;
    const int hv = hs * 16 + vs;
    if (ncomp == 1 ? hv != 0x11 : (hv != 0x11 && hv != 0x21 && hv != 0x22)) return Y4_ERR_SHAPE;
    f.mcus_x = (width + 8 * hs - 1) / (8 * hs);
    f.mcus_y = (height + 8 * vs - 1) / (8 * vs);
    for (int c = 0; c < ncomp; ++c) {
        f.hs[c] = c == 0 ? hs : 1;
        f.vs[c] = c == 0 ? vs : 1;
        f.blocks_w[c] = f.mcus_x * f.hs[c];
        f.blocks_h[c] = f.mcus_y * f.vs[c];
        f.coef_count += 64ll * f.blocks_w[c] * f.blocks_h[c];
    }
    f.orientation = 1;
    *info = f;
    // jpeg_set_quality: scale 5000 / q below 50, else 200 - 2 q; entries (base * scale + 50) / 100 clamped to 1..255
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) {
            int v = (kBaseQt[c ? 1 : 0][i] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            qt[c * 64 + i] = c < ncomp ? (uint16_t)v : (uint16_t)0;
        }
    return Y4_OK;
}

// A bound on the file size.  Scan: a DC coefficient costs at most a 9-bit code + 11 value bits, an AC coefficient at most a
// 16-bit code + 10 value bits, ZRL and EOB codes stand for coefficients that cost nothing themselves (11 bits per 16 zeros,
// 4 bits for the tail): at most 26 bits per coefficient, 64 * 26 / 8 = 208 bytes per block; every byte may be FF and take a
// stuffed 00: 416 bytes per block, dummy blocks included.  Markers: 2 + 18 + 2 * 69 + 19 + (33 + 183) * 2 + 14 + 2 = 625 bytes
// and one byte of padding, rounded up to 1024.
inline size_t bound(const y4_jpeg_info* info) {
    if (!info || !info_ok(*info)) return 0;
    return (size_t)1024 + (size_t)416 * (size_t)(info->coef_count / 64);
}

struct Code {
    uint32_t cl[256];       // (code << 5) | length; 0: the symbol has no code
};

static inline void build_code(Code& t, const uint8_t* bits, const uint8_t* vals) {
    memset(&t, 0, sizeof(t));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) t.cl[vals[k]] = (code << 5) | (unsigned)l;
        code <<= 1;
    }
}

// MSB-first bit writer with FF 00 stuffing; `full` once a byte did not fit.  Bits gather in a 64-bit accumulator and leave
// four bytes at a time: one store when none of them is FF and the buffer has room to spare, byte by byte otherwise.
struct Bits {
    uint8_t* out;
    size_t cap, pos;
    uint64_t acc = 0;       // the low nbits bits are pending
    int nbits = 0;          // < 32 between calls
    bool full = false;
    Bits(uint8_t* o, size_t c, size_t p) : out(o), cap(c), pos(p) {}
    void byte(unsigned b) {
        if (pos < cap) out[pos++] = (uint8_t)b;
        else full = true;
    }
    void stuffed(unsigned b) {
        byte(b);
        if (b == 0xFF) byte(0);
    }
    void put(unsigned v, int n) {           // v < 2^n, n <= 27: 31 pending bits + n fit the accumulator
        acc = (acc << n) | (uint64_t)v;
        nbits += n;
        if (nbits >= 32) {
            nbits -= 32;
            const uint32_t w = (uint32_t)(acc >> nbits);
            const bool has_ff = ((~w - 0x01010101u) & w & 0x80808080u) != 0;    // a zero byte in ~w
            if (!has_ff && cap - pos >= 4) {          // (pos <= cap always)
                out[pos] = (uint8_t)(w >> 24);
                out[pos + 1] = (uint8_t)(w >> 16);
                out[pos + 2] = (uint8_t)(w >> 8);
                out[pos + 3] = (uint8_t)w;
                pos += 4;
            } else {
                stuffed(w >> 24);
                stuffed((w >> 16) & 255u);
                stuffed((w >> 8) & 255u);
                stuffed(w & 255u);
            }
        }
    }
    void flush() {                          // whole bytes, then the final byte padded with one-bits
        while (nbits >= 8) {
            nbits -= 8;
            stuffed((unsigned)(acc >> nbits) & 255u);
        }
        if (nbits) {
            stuffed((((unsigned)acc << (8 - nbits)) | (0xFFu >> nbits)) & 255u);
            nbits = 0;
        }
    }
};

static inline int category(int a) {         // bits needed for |value|
    return a ? 32 - __builtin_clz((unsigned)a) : 0;
}

// Magnitudes: samples are -128..127 after the level shift and the FDCT's output is 8 times the orthonormal DCT, divided by
// 8 * table entry >= 8.  DC lies in [-1024, 1016], a difference of two in [-2040, 2040]: 11 bits.  The largest AC response is
// that of the (4,4) basis, 1/4 * (sum |cos| = 4 sqrt 2)^2 / 2 * (127 + 128) = 1020, and the integer transform is within 1 of it:
// 10 bits.  These are the largest categories the standard tables code, so what the device stage makes always fits, at
// quality 100 too; coefficients from elsewhere that do not fit return Y4_ERR_FORMAT.
inline int encode(const int16_t* coef, const y4_jpeg_info* info, const uint16_t* qt /* [3][64] */, uint8_t* out, size_t out_cap,
                  size_t* out_bytes) {
    if (!coef || !info || !qt || !out || !out_bytes) return Y4_ERR_NULL;
    *out_bytes = 0;
    const y4_jpeg_info& f = *info;
    if (!info_ok(f) || !qt_ok(qt, f.ncomp)) return Y4_ERR_SHAPE;
    Bits w(out, out_cap, 0);
    auto bytes = [&](const uint8_t* p, size_t n) {
        for (size_t i = 0; i < n; ++i) w.byte(p[i]);
    };
    auto be16 = [&](unsigned v) {
        w.byte(v >> 8);
        w.byte(v & 255u);
    };
    const int ntab = f.ncomp == 1 ? 1 : 2;
    static const uint8_t soi_app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    bytes(soi_app0, sizeof(soi_app0));
    for (int t = 0; t < ntab; ++t) {
        be16(0xFFDB);
        be16(67);
        w.byte((unsigned)t);
        for (int i = 0; i < 64; ++i) w.byte(qt[t * 64 + kNatural[i]]);
    }
    be16(0xFFC0);
    be16(8 + 3 * f.ncomp);
    w.byte(8);
    be16((unsigned)f.height);
    be16((unsigned)f.width);
    w.byte((unsigned)f.ncomp);
    for (int c = 0; c < f.ncomp; ++c) {
        w.byte((unsigned)(c + 1));
        w.byte((unsigned)(f.hs[c] * 16 + f.vs[c]));
        w.byte(c ? 1u : 0u);
    }
    Code dc[2], ac[2];
    for (int t = 0; t < ntab; ++t) {
        build_code(dc[t], kDcBits[t], kDcVals);
        build_code(ac[t], kAcBits[t], kAcVals[t]);
        be16(0xFFC4);
        be16(2 + 1 + 16 + 12);
        w.byte((unsigned)t);
        bytes(kDcBits[t], 16);
        bytes(kDcVals, 12);
        be16(0xFFC4);
        be16(2 + 1 + 16 + 162);
        w.byte(0x10u | (unsigned)t);
        bytes(kAcBits[t], 16);
        bytes(kAcVals[t], 162);
    }
    be16(0xFFDA);
    be16(6 + 2 * f.ncomp);
    w.byte((unsigned)f.ncomp);
    for (int c = 0; c < f.ncomp; ++c) {
        w.byte((unsigned)(c + 1));
        w.byte(c ? 0x11u : 0x00u);
    }
    w.byte(0);
    w.byte(63);
    w.byte(0);
    if (w.full) return Y4_ERR_WORKSPACE;

    long long comp_off[3] = {0, 0, 0};
    int rw[3] = {0, 0, 0}, rh[3] = {0, 0, 0};
    for (int c = 0; c < f.ncomp; ++c) {
        if (c) comp_off[c] = comp_off[c - 1] + 64ll * f.blocks_w[c - 1] * f.blocks_h[c - 1];
        rw[c] = real_blocks_w(f, c);
        rh[c] = real_blocks_h(f, c);
    }
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < f.mcus_y; ++my) {
        for (int mx = 0; mx < f.mcus_x; ++mx) {
            for (int c = 0; c < f.ncomp; ++c) {
                const Code& hd = dc[c ? 1 : 0];
                const Code& ha = ac[c ? 1 : 0];
                for (int by = 0; by < f.vs[c]; ++by) {
                    for (int bx = 0; bx < f.hs[c]; ++bx) {
                        const int row = my * f.vs[c] + by, col = mx * f.hs[c] + bx;
                        // a dummy block repeats the DC just coded (difference 0) with no AC; the first block of an MCU is real
                        const bool real = row < rh[c] && col < rw[c];
                        const int16_t* blk = coef + comp_off[c] + 64 * ((long long)row * f.blocks_w[c] + col);
                        const int diff = real ? (int)blk[0] - pred[c] : 0;
                        if (real) pred[c] = blk[0];
                        int a = diff < 0 ? -diff : diff;
                        int s = category(a);
                        if (s > 11) return Y4_ERR_FORMAT;
                        const uint32_t cd = hd.cl[s];
                        w.put(((cd >> 5) << s) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), (int)(cd & 31u) + s);
                        int last = 0;                   // zigzag position of the last coefficient coded
                        if (real) {
                            // the block in zigzag order and the set of its non-zero positions: the scan then visits those
                            // only, with no branch on a coefficient's value
                            int16_t z[64];
                            uint64_t nonzero = 0;
#pragma GCC unroll 64
                            for (int k = 1; k < 64; ++k) {              // unrolled: kNatural[k] and the shift are constants
                                const int16_t v = blk[kNatural[k]];
                                z[k] = v;
                                nonzero |= (uint64_t)(v != 0) << k;
                            }
                            while (nonzero) {
                                const int k = __builtin_ctzll(nonzero);
                                nonzero &= nonzero - 1;
                                int run = k - last - 1;
                                last = k;
                                while (run > 15) {
                                    w.put(ha.cl[0xF0] >> 5, (int)(ha.cl[0xF0] & 31u));
                                    run -= 16;
                                }
                                const int v = z[k];
                                a = v < 0 ? -v : v;
                                s = category(a);
                                if (s > 10) return Y4_ERR_FORMAT;
                                const uint32_t ca = ha.cl[(run << 4) | s];
                                w.put(((ca >> 5) << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(ca & 31u) + s);
                            }
                        }
                        if (last != 63) w.put(ha.cl[0] >> 5, (int)(ha.cl[0] & 31u));
                        if (w.full) return Y4_ERR_WORKSPACE;
                    }
                }
            }
        }
    }
    w.flush();
    be16(0xFFD9);
    if (w.full) return Y4_ERR_WORKSPACE;
    *out_bytes = w.pos;
    return Y4_OK;
}

}  // namespace y4jpegenc
