// JPEG encoding: the host stage (jpeg_enc_host.h: tables, markers, Huffman) behind the C ABI, and the device stage as ONE
// launch per BATCH: colour conversion, edge replication, chroma downsampling, level shift, libjpeg "islow" integer FDCT and
// quantisation of every real 8x8 block of every image, into the coefficient layout y4_jpeg_entropy_host writes.  The
// arithmetic is libjpeg-turbo's default compression path bit for bit; include/yolov4_amd.h states it.
// The mirror image of jpeg.hip's IDCT kernel: 8 lanes per block, lane r owns row r on the way in and out and column r between,
// two transposes through padded LDS, one 16-byte store per lane (a block is 128 contiguous bytes).  It is a gather: a lane
// computes its eight samples from the (clamped) pixels they depend on, so replication costs nothing and nothing is staged.
// Integer byte work: no MFMA.
#include "common.h"
#include "jpeg_enc_host.h"

namespace {

constexpr int kBlocksPerGroup = 32;     // 8x8 blocks per 256-thread workgroup: 8 lanes per block, 8 blocks per wave64
constexpr int kLdsBlock = 72;           // dwords per block in LDS: 8 rows of pitch 9 (rows and columns both conflict-free)

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of jfdctint's jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2): the row pass scales up by 4, the column pass
// removes it again.  |in| <= 128 gives |row out| < 2^13 and every product below 2^31.
template <bool kFirst>
__device__ __forceinline__ void fdct_islow_1d(const int (&d)[8], int (&o)[8]) {
    constexpr int n = kFirst ? 11 : 15;
    const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    o[0] = kFirst ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    o[4] = kFirst ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    o[2] = descale(z + t13 * 6270, n);
    o[6] = descale(z - t12 * 15137, n);
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = descale(t4 + z1 + z3, n);
    o[5] = descale(t5 + z2 + z4, n);
    o[3] = descale(t6 + z2 + z3, n);
    o[1] = descale(t7 + z1 + z4, n);
}

// the weights of one component: value = (kr R + kg G + kb B + add) >> 16
struct Ycc {
    int kr, kg, kb, add;
};

__device__ __forceinline__ Ycc ycc_of(int comp) {
    if (comp == 0) return Ycc{19595, 38470, 7471, 32768};
    if (comp == 1) return Ycc{-11059, -21709, 32768, (128 << 16) + 32767};
    return Ycc{32768, -27439, -5329, (128 << 16) + 32767};
}

// component value of the pixel whose three bytes are the low 24 bits of p (memory order); first / last: the byte that is R / B
__device__ __forceinline__ int convert(unsigned p, const Ycc k, bool swap_rb) {
    const int a = p & 255u, g = (p >> 8) & 255u, c = (p >> 16) & 255u;
    const int r = swap_rb ? a : c, b = swap_rb ? c : a;
    return (k.kr * r + k.kg * g + k.kb * b + k.add) >> 16;
}

__device__ __forceinline__ unsigned pixel(const unsigned char* row, int x) {
    const unsigned char* p = row + 3ll * x;
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// grid (ceil(max blocks of a job / 32), n_jobs)
__global__ void __launch_bounds__(256)
jpeg_fdct_kernel(const y4_jpeg_enc_job* __restrict__ jobs) {
    __shared__ int lds[kBlocksPerGroup * kLdsBlock];
    const y4_jpeg_enc_job& job = jobs[blockIdx.y];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int g = blockIdx.x * kBlocksPerGroup + lb;
    const int W = job.info.width, H = job.info.height, ncomp = job.info.ncomp;
    const int hs = job.info.hs[0], vs = job.info.vs[0];
    const int nb0 = job.info.blocks_w[0] * job.info.blocks_h[0];
    const int nb1 = job.info.blocks_w[1] * job.info.blocks_h[1];
    const int nb2 = job.info.blocks_w[2] * job.info.blocks_h[2];
    const int comp = g < nb0 ? 0 : (g < nb0 + nb1 ? 1 : 2);
    const int gl = g - (comp == 0 ? 0 : (comp == 1 ? nb0 : nb0 + nb1));
    const int bw = comp == 0 ? job.info.blocks_w[0] : job.info.blocks_w[1];
    const int by = gl / (bw > 0 ? bw : 1), bx = gl - by * bw;       // (bw is 0 only past the last block of a gray image)
    // sampling of this component against the pixel grid: 1 or 2 in each direction
    const int fx = comp == 0 ? 1 : hs, fy = comp == 0 ? 1 : vs;
    const int cw = (W + fx - 1) / fx, ch = (H + fy - 1) / fy;           // real samples of the component
    // dummy blocks (beyond the blocks that hold samples, inside the last MCU column / row) are never written
    const bool real = g < nb0 + nb1 + nb2 && bx < (cw + 7) / 8 && by < (ch + 7) / 8;
    int* mine = lds + lb * kLdsBlock;

    int v[8], o[8];
    if (real) {
        const unsigned char* px = (const unsigned char*)job.pixels;
        const int sx0 = bx * 8;
        int sy = by * 8 + r;
        sy = sy < ch ? sy : ch - 1;                                     // the last (downsampled) row, replicated down
        if (ncomp == 1) {
            const unsigned char* row = px + (long long)sy * job.pitch;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int x = sx0 + j < W ? sx0 + j : W - 1;
                v[j] = row[x];
            }
        } else {
            const Ycc k = ycc_of(comp);
            const bool swap = job.swap_rb != 0;
            if (fx == 1) {
                const unsigned char* row = px + (long long)sy * job.pitch;
                if (sx0 + 8 <= W && (((unsigned long long)px | (unsigned long long)job.pitch) & 3ull) == 0) {
                    // 24 bytes at a multiple of 24 from an aligned row: six dwords
                    const unsigned* q = reinterpret_cast<const unsigned*>(row + 24ll * bx);
                    const unsigned a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5];
                    v[0] = convert(a0, k, swap);
                    v[1] = convert((a0 >> 24) | (a1 << 8), k, swap);
                    v[2] = convert((a1 >> 16) | (a2 << 16), k, swap);
                    v[3] = convert(a2 >> 8, k, swap);
                    v[4] = convert(a3, k, swap);
                    v[5] = convert((a3 >> 24) | (a4 << 8), k, swap);
                    v[6] = convert((a4 >> 16) | (a5 << 16), k, swap);
                    v[7] = convert(a5 >> 8, k, swap);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int x = sx0 + j < W ? sx0 + j : W - 1;
                        v[j] = convert(pixel(row, x), k, swap);
                    }
                }
            } else {
                // rows 2 sy and 2 sy + 1 (h2v2) or row sy (h2v1), the odd one replicated from the last pixel row
                const int y0 = fy == 2 ? 2 * sy : sy;
                const int y1 = fy == 2 ? (y0 + 1 < H ? y0 + 1 : H - 1) : y0;
                const unsigned char* row0 = px + (long long)y0 * job.pitch;
                const unsigned char* row1 = px + (long long)y1 * job.pitch;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int sx = sx0 + j;
                    const int x0 = 2 * sx < W ? 2 * sx : W - 1, x1 = 2 * sx + 1 < W ? 2 * sx + 1 : W - 1;
                    const int top = convert(pixel(row0, x0), k, swap) + convert(pixel(row0, x1), k, swap);
                    if (fy == 2) {
                        const int bottom = convert(pixel(row1, x0), k, swap) + convert(pixel(row1, x1), k, swap);
                        v[j] = (top + bottom + 1 + (sx & 1)) >> 2;      // bias 1, 2, 1, 2, ...
                    } else {
                        v[j] = (top + (sx & 1)) >> 1;                   // bias 0, 1, 0, 1, ...
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] -= 128;
        fdct_islow_1d<true>(v, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) mine[r * 9 + j] = o[j];
    }
    __syncthreads();
    if (real) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = mine[k * 9 + r];
        fdct_islow_1d<false>(v, o);
    }
    __syncthreads();
    if (real) {
#pragma unroll
        for (int k = 0; k < 8; ++k) mine[k * 9 + r] = o[k];
    }
    __syncthreads();
    if (real) {
        const uint4 q4 = *reinterpret_cast<const uint4*>(&job.qt[comp][r * 8]);
        const unsigned qw[4] = {q4.x, q4.y, q4.z, q4.w};
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned h[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = mine[r * 9 + 2 * j + e];
                // exact by construction: an integer divide.  divisor = 8 * table entry (1..255, checked on the host)
                const unsigned d = 8u * (e ? qw[j] >> 16 : qw[j] & 0xffffu);
                const unsigned a = (unsigned)(c < 0 ? -c : c) + (d >> 1);
                const int m = a >= d ? (int)(a / d) : 0;
                h[e] = (unsigned)(c < 0 ? -m : m) & 0xffffu;
            }
            w[j] = h[0] | (h[1] << 16);
        }
        *reinterpret_cast<uint4*>(job.coef + ((long long)g * 64 + r * 8)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

extern "C" int y4_jpeg_encode_setup(int width, int height, int ncomp, int hs, int vs, int quality, y4_jpeg_info* info_host,
                                    unsigned short* qt_host) {
    return y4jpegenc::setup(width, height, ncomp, hs, vs, quality, info_host, qt_host);
}

extern "C" size_t y4_jpeg_encode_bound(const y4_jpeg_info* info_host) { return y4jpegenc::bound(info_host); }

extern "C" int y4_jpeg_encode_host(const short* coef_host, const y4_jpeg_info* info_host, const unsigned short* qt_host,
                                   void* out_host, size_t out_cap, size_t* out_bytes) {
    return y4jpegenc::encode(coef_host, info_host, qt_host, (uint8_t*)out_host, out_cap, out_bytes);
}

extern "C" int y4_jpeg_encode_u8(const y4_jpeg_enc_job* jobs_dev, const y4_jpeg_enc_job* jobs_host, int n_jobs, void* stream) {
    if (!jobs_dev || !jobs_host) return Y4_ERR_NULL;
    if (n_jobs < 1 || n_jobs > 65535) return Y4_ERR_SHAPE;
    if ((unsigned long long)jobs_dev & 15ull) return Y4_ERR_SHAPE;
    long long max_blocks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const y4_jpeg_enc_job& j = jobs_host[i];
        if (!j.pixels || !j.coef) return Y4_ERR_NULL;
        if (!y4jpegenc::info_ok(j.info) || !y4jpegenc::qt_ok(&j.qt[0][0], j.info.ncomp)) return Y4_ERR_SHAPE;
        if ((unsigned long long)j.coef & 15ull) return Y4_ERR_SHAPE;
        if (j.pitch < (long long)(j.info.ncomp == 3 ? 3 : 1) * j.info.width) return Y4_ERR_SHAPE;
        const long long blocks = j.info.coef_count / 64;
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
    }
    // 65535 x 65535 at 4:4:4 is 2.0e8 blocks: the grid's x fits an int, the kernel's block index too
    const dim3 grid((unsigned)((max_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)n_jobs);
    hipLaunchKernelGGL(jpeg_fdct_kernel, grid, dim3(256), 0, y4_stream(stream), jobs_dev);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
