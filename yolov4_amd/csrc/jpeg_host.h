// Host stage of the JPEG decoder: marker parsing and Huffman entropy decoding of baseline / extended sequential JPEG
// (ITU-T T.81: SOF0 / SOF1, 8-bit, one interleaved scan, 1 component or 3 YCbCr components at 4:4:4, 4:2:2 h2v1, 4:2:0 h2v2).
// Plain C++17, no HIP: jpeg.hip exports it through the C ABI, and a stand-alone CPU program can include it too.
// The input is untrusted: every read is checked against nbytes and every write against coef_cap; an error returns before
// anything is written past a cap.  No threads, no global state: callers run it from a thread pool.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/yolov4_amd.h"

namespace y4jpeg {

// zigzag position -> natural (row-major) position in the 8x8 block
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;

struct Huff {
    bool defined = false;
    uint16_t look[1 << kLookBits];      // (length << 8) | symbol for codes of at most kLookBits bits; 0: longer code
    int32_t maxcode[18];                // largest code of each length, -1 when the length has none
    int32_t valoff[17];                 // symbol index = code + valoff[length]
    uint8_t vals[256];
};

struct Header {
    int width = 0, height = 0, ncomp = 0;
    int comp_id[3] = {0, 0, 0}, hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool have_sof = false, jfif = false;
    int adobe_transform = -1;
    uint16_t qt[4][64];
    bool qt_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart_interval = 0;
    int orientation = 1;
    size_t scan_start = 0;              // first entropy-coded byte
};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// EXIF orientation from an APP1 payload (after the length field); 1 when absent or unreadable
static inline int exif_orientation(const uint8_t* s, size_t n) {
    if (n < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 0;
    const uint8_t* t = s + 6;           // TIFF header
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 1;
    auto u16 = [&](size_t o) -> unsigned { return le ? (unsigned)(t[o] | (t[o + 1] << 8)) : (unsigned)((t[o] << 8) | t[o + 1]); };
    auto u32 = [&](size_t o) -> uint32_t {
        return le ? ((uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
                  : (((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]);
    };
    if (u16(2) != 42) return 1;
    const uint32_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 1;
    const unsigned count = u16(ifd);
    for (unsigned i = 0; i < count; ++i) {
        const size_t e = (size_t)ifd + 2 + 12 * (size_t)i;
        if (e > tn || tn - e < 12) return 1;
        if (u16(e) == 0x0112) {
            if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;
            const unsigned v = u16(e + 8);
            return (v >= 1 && v <= 8) ? (int)v : 1;
        }
    }
    return 1;
}

static inline int build_huff(Huff& h, const uint8_t* counts, const uint8_t* syms, int nsyms) {
    memset(h.look, 0, sizeof(h.look));
    memcpy(h.vals, syms, (size_t)nsyms);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        h.valoff[l] = k - code;
        if (c) {
            if (code + c > (1 << l)) return Y4_ERR_FORMAT;          // more codes than the length can hold
            for (int i = 0; i < c; ++i, ++code, ++k) {
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l), span = 1 << (kLookBits - l);
                    for (int j = 0; j < span; ++j) h.look[first + j] = (uint16_t)((l << 8) | syms[k]);
                }
            }
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.maxcode[0] = -1;
    h.valoff[0] = 0;
    h.defined = true;
    return Y4_OK;
}

// Walks the markers up to and including SOS.  Everything the two entry points need lands in `h`.
static inline int read_headers(const uint8_t* d, size_t n, Header& h) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return Y4_ERR_FORMAT;
    size_t pos = 2;
    for (;;) {
        if (pos >= n || d[pos] != 0xFF) return Y4_ERR_FORMAT;
        while (pos < n && d[pos] == 0xFF) ++pos;                    // fill bytes
        if (pos >= n) return Y4_ERR_FORMAT;
        const int m = d[pos++];
        if (m == 0x00 || m == 0xD9) return Y4_ERR_FORMAT;           // stuffed zero outside a scan, EOI before SOS
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
        if (n - pos < 2) return Y4_ERR_FORMAT;
        const size_t len = (size_t)be16(d + pos);
        if (len < 2 || len > n - pos) return Y4_ERR_FORMAT;
        const uint8_t* s = d + pos + 2;
        const size_t sn = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (h.have_sof || sn < 6) return Y4_ERR_FORMAT;
            const int prec = s[0], nf = s[5];
            h.height = be16(s + 1);
            h.width = be16(s + 3);
            if (prec != 8) return Y4_ERR_UNSUPPORTED;
            if (nf != 1 && nf != 3) return nf == 0 ? Y4_ERR_FORMAT : Y4_ERR_UNSUPPORTED;
            if (sn < 6 + 3 * (size_t)nf) return Y4_ERR_FORMAT;
            if (h.width == 0 || h.height == 0) return Y4_ERR_FORMAT;
            h.ncomp = nf;
            for (int c = 0; c < nf; ++c) {
                h.comp_id[c] = s[6 + 3 * c];
                h.hs[c] = s[7 + 3 * c] >> 4;
                h.vs[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
                if (h.hs[c] < 1 || h.hs[c] > 4 || h.vs[c] < 1 || h.vs[c] > 4 || h.tq[c] > 3) return Y4_ERR_FORMAT;
            }
            if (nf == 1) {
                h.hs[0] = h.vs[0] = 1;                              // one component: the scan is not interleaved, blocks in raster order
            } else {
                if (h.hs[1] != 1 || h.vs[1] != 1 || h.hs[2] != 1 || h.vs[2] != 1) return Y4_ERR_UNSUPPORTED;
                const int hv = h.hs[0] * 16 + h.vs[0];
                if (hv != 0x11 && hv != 0x21 && hv != 0x22) return Y4_ERR_UNSUPPORTED;
            }
            h.have_sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4) {
            return Y4_ERR_UNSUPPORTED;                              // progressive, lossless, differential, arithmetic (SOFn, JPG, DAC)
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < sn) {
                if (sn - o < 17) return Y4_ERR_FORMAT;
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return Y4_ERR_FORMAT;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
                if (total > 256 || sn - o - 17 < (size_t)total) return Y4_ERR_FORMAT;
                const int rc = build_huff(tc ? h.ac[th] : h.dc[th], s + o + 1, s + o + 17, total);
                if (rc != Y4_OK) return rc;
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < sn) {
                const int pq = s[o] >> 4, t = s[o] & 15;
                if (pq > 1 || t > 3) return Y4_ERR_FORMAT;
                const size_t need = pq ? 128 : 64;
                if (sn - o - 1 < need) return Y4_ERR_FORMAT;
                for (int i = 0; i < 64; ++i)
                    h.qt[t][kNatural[i]] = pq ? (uint16_t)be16(s + o + 1 + 2 * i) : (uint16_t)s[o + 1 + i];
                h.qt_defined[t] = true;
                o += 1 + need;
            }
        } else if (m == 0xDD) {
            if (sn < 2) return Y4_ERR_FORMAT;
            h.restart_interval = be16(s);
        } else if (m == 0xE0) {
            if (sn >= 5 && memcmp(s, "JFIF\0", 5) == 0) h.jfif = true;
        } else if (m == 0xE1) {
            const int o = exif_orientation(s, sn);
            if (o) h.orientation = o;
        } else if (m == 0xEE) {
            if (sn >= 12 && memcmp(s, "Adobe", 5) == 0) h.adobe_transform = s[11];
        } else if (m == 0xDA) {
            if (!h.have_sof) return Y4_ERR_FORMAT;
            if (sn < 1) return Y4_ERR_FORMAT;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sn < 1 + 2 * (size_t)ns + 3) return Y4_ERR_FORMAT;
            if (ns != h.ncomp) return Y4_ERR_UNSUPPORTED;           // the first of several scans
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.comp_id[c]) return Y4_ERR_UNSUPPORTED;   // components out of frame order
                h.td[c] = s[2 + 2 * c] >> 4;
                h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return Y4_ERR_FORMAT;
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return Y4_ERR_FORMAT;
            if (h.ncomp == 3) {
                // colour space as libjpeg guesses it: an Adobe marker decides; else JFIF or any ids but "RGB" mean YCbCr
                if (h.adobe_transform == 0) return Y4_ERR_UNSUPPORTED;
                if (h.adobe_transform < 0 && !h.jfif && h.comp_id[0] == 'R' && h.comp_id[1] == 'G' && h.comp_id[2] == 'B')
                    return Y4_ERR_UNSUPPORTED;
            }
            for (int c = 0; c < h.ncomp; ++c)
                if (!h.qt_defined[h.tq[c]] || !h.dc[h.td[c]].defined || !h.ac[h.ta[c]].defined) return Y4_ERR_FORMAT;
            h.scan_start = pos + len;
            return Y4_OK;
        }
        pos += len;
    }
}

static inline void fill_info(const Header& h, y4_jpeg_info* info) {
    memset(info, 0, sizeof(*info));
    info->width = h.width;
    info->height = h.height;
    info->ncomp = h.ncomp;
    const int hmax = h.hs[0], vmax = h.vs[0];                       // chroma is 1x1 in every supported layout
    info->mcus_x = (h.width + 8 * hmax - 1) / (8 * hmax);
    info->mcus_y = (h.height + 8 * vmax - 1) / (8 * vmax);
    long long count = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        info->hs[c] = h.hs[c];
        info->vs[c] = h.vs[c];
        info->blocks_w[c] = info->mcus_x * h.hs[c];
        info->blocks_h[c] = info->mcus_y * h.vs[c];
        count += 64ll * info->blocks_w[c] * info->blocks_h[c];
    }
    info->restart_interval = h.restart_interval;
    info->orientation = h.orientation;
    info->coef_count = count;
}

inline int parse(const uint8_t* d, size_t n, y4_jpeg_info* info) {
    if (!d || !info) return Y4_ERR_NULL;
    Header h;
    const int rc = read_headers(d, n, h);
    if (rc != Y4_OK) return rc;
    fill_info(h, info);
    return Y4_OK;
}

// MSB-first bit reader over the entropy-coded segment.  FF 00 is a data byte FF; any other FF xx (a marker) or the end of
// the data stops the supply: zero bits are fed from there on and counted, and consuming one of them is an error.
struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint64_t acc = 0;
    int nbits = 0, fake = 0;
    Bits(const uint8_t* d_, size_t n_, size_t pos_) : d(d_), n(n_), pos(pos_) {}
    void fill() {
        while (nbits <= 56) {
            unsigned b = 0;
            if (fake || pos >= n) {
                fake += 8;
            } else if (d[pos] != 0xFF) {
                b = d[pos++];
            } else if (pos + 1 < n && d[pos + 1] == 0x00) {
                b = 0xFF;
                pos += 2;
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)((acc >> (nbits - k)) & ((1u << k) - 1u)); }
    bool skip(int k) {
        nbits -= k;
        return nbits >= fake;
    }
    void reset() { acc = 0; nbits = 0; fake = 0; }
};

// one Huffman symbol; -1 for a code that is not in the table or that runs into the end of the data
static inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned e = h.look[b.peek(kLookBits)];
    if (e) return b.skip((int)(e >> 8)) ? (int)(e & 255u) : -1;
    int l = kLookBits + 1;
    while (l <= 16 && (int32_t)b.peek(l) > h.maxcode[l]) ++l;
    if (l > 16) return -1;
    const int idx = (int)b.peek(l) + h.valoff[l];
    if (idx < 0 || idx > 255 || !b.skip(l)) return -1;
    return h.vals[idx];
}

// s extra bits -> the signed value of category s (T.81 F.2.2.1 EXTEND)
static inline bool receive_extend(Bits& b, int s, int& v) {
    const int raw = (int)b.peek(s);
    if (!b.skip(s)) return false;
    v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
    return true;
}

inline int entropy(const uint8_t* d, size_t n, const y4_jpeg_info* info, int16_t* coef, long long coef_cap,
                   uint16_t* qt_out /* [3][64] */) {
    if (!d || !info || !coef || !qt_out) return Y4_ERR_NULL;
    Header h;
    int rc = read_headers(d, n, h);
    if (rc != Y4_OK) return rc;
    y4_jpeg_info now;
    fill_info(h, &now);
    if (now.width != info->width || now.height != info->height || now.ncomp != info->ncomp ||
        now.coef_count != info->coef_count || now.hs[0] != info->hs[0] || now.vs[0] != info->vs[0])
        return Y4_ERR_SHAPE;                                        // the record belongs to another file
    if (coef_cap < now.coef_count) return Y4_ERR_WORKSPACE;
    memset(coef, 0, sizeof(int16_t) * (size_t)now.coef_count);
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt_out[c * 64 + i] = c < h.ncomp ? h.qt[h.tq[c]][i] : (uint16_t)0;

    long long comp_off[3] = {0, 0, 0};
    for (int c = 1; c < h.ncomp; ++c) comp_off[c] = comp_off[c - 1] + 64ll * now.blocks_w[c - 1] * now.blocks_h[c - 1];
    Bits bits(d, n, h.scan_start);
    int pred[3] = {0, 0, 0};
    const int ri = h.restart_interval;
    int next_rst = 0;
    long long done = 0;
    for (int my = 0; my < now.mcus_y; ++my) {
        for (int mx = 0; mx < now.mcus_x; ++mx, ++done) {
            if (ri && done && done % ri == 0) {
                // byte-align; the reader never passes a marker, so it has to stand on one now
                bits.reset();
                size_t p = bits.pos;
                while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + next_rst) return Y4_ERR_FORMAT;
                bits.pos = p + 2;
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const Huff& hd = h.dc[h.td[c]];
                const Huff& ha = h.ac[h.ta[c]];
                for (int by = 0; by < h.vs[c]; ++by) {
                    for (int bx = 0; bx < h.hs[c]; ++bx) {
                        const long long row = (long long)my * h.vs[c] + by, col = (long long)mx * h.hs[c] + bx;
                        const long long at = comp_off[c] + 64 * (row * now.blocks_w[c] + col);
                        if (at < 0 || at + 64 > now.coef_count) return Y4_ERR_FORMAT;   // (cannot happen: the grid is ours)
                        int16_t* blk = coef + at;
                        bits.fill();
                        int s = decode_symbol(bits, hd);
                        if (s < 0 || s > 15) return Y4_ERR_FORMAT;
                        int v = 0;
                        if (s && !receive_extend(bits, s, v)) return Y4_ERR_FORMAT;
                        pred[c] += v;
                        if (pred[c] < -32768 || pred[c] > 32767) return Y4_ERR_FORMAT;
                        blk[0] = (int16_t)pred[c];
                        int k = 1;
                        while (k < 64) {
                            bits.fill();
                            const int rs = decode_symbol(bits, ha);
                            if (rs < 0) return Y4_ERR_FORMAT;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;                 // EOB
                                k += 16;
                                if (k > 64) return Y4_ERR_FORMAT;   // a zero run past coefficient 63
                                continue;
                            }
                            k += r;
                            if (k > 63) return Y4_ERR_FORMAT;
                            if (!receive_extend(bits, s, v)) return Y4_ERR_FORMAT;
                            blk[kNatural[k]] = (int16_t)v;          // |v| < 2^15: fits
                            ++k;
                        }
                    }
                }
            }
        }
    }
    return Y4_OK;
}

}  // namespace y4jpeg
