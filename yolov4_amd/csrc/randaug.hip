// RandAugment on the device (reference: darknet/main_amp.py:221-227 -- torchvision's RandAugment between the flip and the
// collate): fourteen Pillow operations on the uint8 RGB S x S crops, between the resized-crop gather (rcrop_gather_body.inc) and its
// normalisation.  include/yolov4_amd.h states the arithmetic; the host (yolov4_amd/darknet/data.py) draws the operations and
// turns every magnitude into the integers and the one float of a y4_randaug_op.  Compiled with -ffp-contract=off: the blends
// and the 3 x 3 filter are Pillow's unfused fp32, the AutoContrast table its unfused fp64.
//
// Launches for n_ops >= 1: the coefficient tables (resample.hip); the gather into uint8 batch 0 (which also zeroes the
// statistics of every round); then per round r
//   statistics  per sample 3 x 256 counts and the sum of L: LDS atomics per block of kStatPix pixels, then one global integer
//               atomic per occupied bin -- integer sums, so the result does not depend on the order.  Launched only when the
//               host sees a Contrast, AutoContrast or Equalize in round r; blocks of other samples leave at once.
//   apply       one thread per pixel, blocks of 2048 consecutive pixels of one sample (256 at a time), so the operation is
//               block-uniform.  A block of a table operation builds its 3 x 256 table in LDS first, thread t owning bin t
//               (first / last occupied bin by wave ballots, Equalize's running sum by a wave scan, one barrier to combine the
//               four waves).  The 3 x 3 filter reads each row's nine bytes as three aligned words.  Rounds before the last
//               go from one uint8 batch to the other; the last one writes (float(u8) - mean) / std to the destination and,
//               like the gather, runs a second set of blocks for the pixels inside paste rectangles, which evaluate the
//               PARTNER's operation on the partner's batch.
// Otherwise byte loads and stores, as in the gather: three per pixel each way, 192 contiguous bytes per wave instruction.
#include "rcrop_gather.h"

namespace {

constexpr int kMaxOps = 8;
constexpr int kMaxSideRA = 4096;    // 16.16 coordinates stay below 2^15; 255 * 4096^2 < 2^32 for the sum of L
constexpr int kStatWords = 772;     // 3 x 256 counts, the sum of L, padding to 16 bytes
constexpr int kStatPix = 4096;      // pixels per block of the statistics launch
constexpr int kApplyThreads = 256;
constexpr int kApplyPix = 2048;     // pixels per block of an apply launch: a table is built once per 2048 pixels

__host__ __device__ inline bool ra_needs_stats(int op) {
    return op == Y4_RA_CONTRAST || op == Y4_RA_AUTOCONTRAST || op == Y4_RA_EQUALIZE;
}
size_t ra_batch_bytes(int n, int S) { return ((size_t)n * S * S * 3 + 255) & ~(size_t)255; }

// the gather of rcrop_gather_body.inc into the uint8 batch [n][S][S][3], output channel order, flip applied, no paste
__global__ void __launch_bounds__(kTileX)
randaug_gather_u8_kernel(const y4_rcrop_job* __restrict__ jobs, int n, int S, const int* __restrict__ ws,
                         unsigned char* __restrict__ u8, unsigned* __restrict__ stats, int stat_words) {
    if (blockIdx.x == 0 && blockIdx.y == 0)                   // this sample's statistics of every round
        for (int i = threadIdx.x; i < stat_words; i += kTileX) stats[(long long)blockIdx.z * stat_words + i] = 0u;
#define RC_GATHER_U8 1
#include "rcrop_gather_body.inc"
#undef RC_GATHER_U8
}

__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__global__ void __launch_bounds__(256)
randaug_stats_kernel(const y4_randaug_op* __restrict__ ops, int n_ops, int round, int S, const unsigned char* __restrict__ in,
                     unsigned* __restrict__ stats) {
    const int b = blockIdx.y;
    if (!ra_needs_stats(ops[(long long)b * n_ops + round].op)) return;    // block-uniform
    __shared__ unsigned h[769];
    for (int i = threadIdx.x; i < 769; i += 256) h[i] = 0u;
    __syncthreads();
    const int P = S * S;
    const int p0 = blockIdx.x * kStatPix, p1 = min(p0 + kStatPix, P);
    const unsigned char* __restrict__ px = in + 3ll * P * b;
    unsigned sum = 0u;
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        const int r = px[3ll * p], g = px[3ll * p + 1], bl = px[3ll * p + 2];
        atomicAdd(&h[r], 1u);
        atomicAdd(&h[256 + g], 1u);
        atomicAdd(&h[512 + bl], 1u);
        sum += (unsigned)ra_luma(r, g, bl);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += (unsigned)__shfl_xor((int)sum, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&h[768], sum);
    __syncthreads();
    unsigned* __restrict__ out = stats + ((long long)b * n_ops + round) * kStatWords;
    for (int i = threadIdx.x; i < 769; i += 256)
        if (h[i]) atomicAdd(&out[i], h[i]);
}

__device__ __forceinline__ int ra_clip_f(float t) { return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t); }

// ImagingBlend(deg, px, a): fp32, unfused
__device__ __forceinline__ int ra_blend(int deg, int px, float a, bool interpolate) {
    const float t = (float)deg + a * (float)(px - deg);
    return interpolate ? (int)t : ra_clip_f(t);
}

// Nine consecutive bytes from p (the three channels of three neighbouring pixels) by three ALIGNED 4-byte loads: bytes 0-3 in
// d0, 4-7 in d1, byte 8 in the low byte of d2.  The words hold up to three bytes on either side of the nine; the uint8 batches
// start on a 16-byte boundary and are a multiple of 256 bytes long, so those lie inside the batch.
struct ra_row9 {
    unsigned d0, d1, d2;
    __device__ __forceinline__ float f(int k) const {         // byte k as fp32 (k is a constant after unrolling)
        return (float)(((k < 4 ? d0 : (k < 8 ? d1 : d2)) >> (8 * (k & 3))) & 255u);
    }
};
__device__ __forceinline__ ra_row9 ra_load9(const unsigned char* p) {
    const uintptr_t addr = (uintptr_t)p;
    const unsigned* __restrict__ w = (const unsigned*)(addr & ~(uintptr_t)3);
    const unsigned r = (unsigned)(addr & 3u);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
    return ra_row9{__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r), w2 >> (8u * r)};
}

// FINAL = false: batch `in` -> batch `out8`, every sample its own operation of this round.
// FINAL = true: blockIdx.z = 0: sample b's pixels outside its paste rectangle, from its own operation; 1 (launched only when
// the batch has a paste): the pixels inside it, from the partner's operation, batch and statistics; fp32 out.
// A block owns kApplyPix consecutive pixels of one sample, 256 at a time.
template <bool FINAL>
__global__ void __launch_bounds__(kApplyThreads)
randaug_apply_kernel(const y4_rcrop_job* __restrict__ jobs, const y4_randaug_op* __restrict__ ops, int n, int n_ops, int round,
                     int S, const unsigned char* __restrict__ in, const unsigned* __restrict__ stats,
                     unsigned char* __restrict__ out8, rc_norm nm, float* __restrict__ dst, long long dsb, long long dsc,
                     long long dsh, long long dsw) {
    const int P = S * S, t = threadIdx.x;
    const int pass = FINAL ? (int)blockIdx.z : 0;
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * kApplyPix, p1 = min(p0 + kApplyPix, P);
    int j = b, px0 = 0, px1 = 0, py0 = 0, py1 = 0;            // the paste rectangle; empty without a partner
    if (FINAL) {
        const y4_rcrop_job self = jobs[b];
        if (self.paste_from >= 0) { px0 = self.paste_x0; px1 = self.paste_x1; py0 = self.paste_y0; py1 = self.paste_y1; }
        if (pass) {                                           // block-uniform: no row of this block crosses the rectangle
            if (px0 >= px1 || (p1 - 1) / S < py0 || p0 / S >= py1) return;
            j = self.paste_from;
        }
    }
    const y4_randaug_op op = ops[(long long)j * n_ops + round];
    const unsigned* __restrict__ st = stats + ((long long)j * n_ops + round) * kStatWords;

    __shared__ int s_h[3][256];
    __shared__ int s_wsum[3][4], s_wlo[3][4], s_whi[3][4];
    __shared__ unsigned char s_lut[3][256];
    int mean = 0;
    if (op.op == Y4_RA_CONTRAST) mean = (int)((double)st[768] / (double)P + 0.5);
    if (op.op == Y4_RA_AUTOCONTRAST || op.op == Y4_RA_EQUALIZE) {         // block-uniform; thread t owns bin t
        const int lane = t & 63, wv = t >> 6;
        int hc[3], inc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hc[c] = (int)st[c * 256 + t];
            s_h[c][t] = hc[c];
            int x = hc[c];                                    // inclusive running sum inside the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(x, off, 64);
                if (lane >= off) x += v;
            }
            inc[c] = x;
            const unsigned long long m = __ballot(hc[c] > 0); // the wave's occupied bins
            if (lane == 63) s_wsum[c][wv] = x;
            if (lane == 0) {
                s_wlo[c][wv] = m ? wv * 64 + __ffsll(m) - 1 : 256;
                s_whi[c][wv] = m ? wv * 64 + 63 - __clzll((long long)m) : -1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int lo = 256, hi = -1, before = 0;                // first / last occupied bin; pixels in the waves before this one
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                lo = min(lo, s_wlo[c][w]);
                hi = max(hi, s_whi[c][w]);
                if (w < wv) before += s_wsum[c][w];
            }
            int v = t;
            if (hi > lo) {                                    // (P >= 1 pixels occupy a bin: hi >= 0)
                if (op.op == Y4_RA_AUTOCONTRAST) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double offset = (double)(-lo) * scale;
                    v = (int)((double)t * scale + offset);
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                } else {
                    const int step = (P - s_h[c][hi]) / 255;
                    if (step != 0) {
                        v = (step / 2 + (before + inc[c] - hc[c])) / step;
                        v = v > 255 ? 255 : v;
                    }
                }
            }
            s_lut[c][t] = (unsigned char)v;
        }
        __syncthreads();
    }

    const unsigned char* __restrict__ img = in + 3ll * P * j;
    const bool interpolate = op.factor >= 0.0f && op.factor <= 1.0f;
    const int dy = kApplyThreads / S, dx = kApplyThreads - dy * S;        // 256 pixels further on
    int ys = (p0 + t) / S, xs = (p0 + t) - ys * S;
    for (int p = p0 + t; p < p1; p += kApplyThreads) {
        const int x = xs, y = ys;
        xs += dx;
        ys += dy;
        if (xs >= S) { xs -= S; ++ys; }
        if (FINAL) {
            const bool inside = x >= px0 && x < px1 && y >= py0 && y < py1;
            if (inside != (pass == 1)) continue;
        }
        int v[3];
        if (op.op >= Y4_RA_SHEAR_X && op.op <= Y4_RA_ROTATE) {
            const long long sx = ((long long)op.a[2] + (long long)op.a[1] * y + (long long)op.a[0] * x) >> 16;
            const long long sy = ((long long)op.a[5] + (long long)op.a[4] * y + (long long)op.a[3] * x) >> 16;
            v[0] = v[1] = v[2] = 0;
            if (sx >= 0 && sx < S && sy >= 0 && sy < S) {
                const unsigned char* __restrict__ q = img + 3ll * (sy * S + sx);
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
            }
        } else if (op.op == Y4_RA_SHARPNESS && x >= 1 && x < S - 1 && y >= 1 && y < S - 1) {
            // ImageFilter.SMOOTH inside the frame, then the blend; on the frame the smoothed pixel is the pixel (below)
            const unsigned char* __restrict__ q = img + 3ll * (p - 1);    // the left neighbour's first channel
            const ra_row9 dn = ra_load9(q + 3ll * S), mid = ra_load9(q), up = ra_load9(q - 3ll * S);
            const float k = 1.0f / 13.0f, ctr = 5.0f / 13.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ss = 0.5f;
                ss += (dn.f(c) * k + dn.f(3 + c) * k) + dn.f(6 + c) * k;
                ss += (mid.f(c) * k + mid.f(3 + c) * ctr) + mid.f(6 + c) * k;
                ss += (up.f(c) * k + up.f(3 + c) * k) + up.f(6 + c) * k;
                v[c] = ra_blend(ra_clip_f(ss), (int)mid.f(3 + c), op.factor, interpolate);
            }
        } else {
            const unsigned char* __restrict__ q = img + 3ll * p;
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
            switch (op.op) {
                case Y4_RA_BRIGHTNESS:
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = ra_blend(0, v[c], op.factor, interpolate);
                    break;
                case Y4_RA_COLOR: {
                    const int L = ra_luma(v[0], v[1], v[2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = ra_blend(L, v[c], op.factor, interpolate);
                    break;
                }
                case Y4_RA_CONTRAST:
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = ra_blend(mean, v[c], op.factor, interpolate);
                    break;
                case Y4_RA_POSTERIZE: {
                    const int mask = ~((1 << (8 - op.bits)) - 1) & 255;
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] &= mask;
                    break;
                }
                case Y4_RA_SOLARIZE:
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = v[c] < op.threshold ? v[c] : 255 - v[c];
                    break;
                case Y4_RA_AUTOCONTRAST:
                case Y4_RA_EQUALIZE:
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = s_lut[c][v[c]];
                    break;
                default: break;                               // Y4_RA_IDENTITY; Y4_RA_SHARPNESS on the frame
            }
        }
        if (FINAL) {
            float* __restrict__ o = dst + (long long)b * dsb + (long long)y * dsh + (long long)x * dsw;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(long long)c * dsc] = __fdiv_rn((float)v[c] - nm.mean[c], nm.std[c]);
        } else {
            unsigned char* __restrict__ o = out8 + 3ll * P * b + 3ll * p;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (unsigned char)v[c];
        }
    }
}

}  // namespace

extern "C" size_t y4_randaug_workspace(int n, int S, int n_ops) {
    if (n < 1 || n > 65535 || S < 1 || S > kMaxSideRA || n_ops < 1 || n_ops > kMaxOps) return 0;
    return 2 * ra_batch_bytes(n, S) + (size_t)n * n_ops * kStatWords * 4;
}

extern "C" int y4_rcrop_randaug_u8_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S,
                                       const float* mean3_host, const float* std3_host, float* dst, long long dst_sb,
                                       long long dst_sc, long long dst_sh, long long dst_sw, void* workspace, size_t ws_bytes,
                                       const y4_randaug_op* ops_dev, const y4_randaug_op* ops_host, int n_ops,
                                       void* workspace2, size_t ws2_bytes, void* stream) {
    if (!mean3_host || !std3_host || !dst) return Y4_ERR_NULL;
    int rc = y4::rcrop_check(jobs_dev, jobs_host, n, S, workspace, ws_bytes);
    if (rc != Y4_OK) return rc;
    rc_norm nm;
    rc = y4::rcrop_norm(mean3_host, std3_host, &nm);
    if (rc != Y4_OK) return rc;
    if (n_ops < 0 || n_ops > kMaxOps) return Y4_ERR_SHAPE;
    bool stats_in[kMaxOps] = {};
    if (n_ops > 0) {
        if (!ops_dev || !ops_host || !workspace2) return Y4_ERR_NULL;
        if (S > kMaxSideRA || ((uintptr_t)workspace2 & 15)) return Y4_ERR_SHAPE;
        for (long long i = 0; i < (long long)n * n_ops; ++i) {
            const y4_randaug_op& o = ops_host[i];
            if (o.op < Y4_RA_IDENTITY || o.op > Y4_RA_EQUALIZE || !isfinite(o.factor)) return Y4_ERR_SHAPE;
            if (o.op == Y4_RA_POSTERIZE && (o.bits < 0 || o.bits > 8)) return Y4_ERR_SHAPE;
            stats_in[i % n_ops] = stats_in[i % n_ops] || ra_needs_stats(o.op);
        }
        if (ws2_bytes < y4_randaug_workspace(n, S, n_ops)) return Y4_ERR_WORKSPACE;
    }
    hipStream_t st = y4_stream(stream);
    y4::rcrop_launch_coeffs(jobs_dev, n, S, workspace, st);
    Y4_CHECK_LAUNCH();
    if (n_ops == 0) {
        y4::rcrop_launch_gather_f32(jobs_dev, jobs_host, n, S, workspace, nm, dst, dst_sb, dst_sc, dst_sh, dst_sw, st);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    unsigned char* batch[2] = {(unsigned char*)workspace2, (unsigned char*)workspace2 + ra_batch_bytes(n, S)};
    unsigned* stats = (unsigned*)((unsigned char*)workspace2 + 2 * ra_batch_bytes(n, S));
    hipLaunchKernelGGL(randaug_gather_u8_kernel, dim3((S + kTileX - 1) / kTileX, (S + kTileY - 1) / kTileY, n), dim3(kTileX), 0,
                       st, jobs_dev, n, S, (const int*)workspace, batch[0], stats, n_ops * kStatWords);
    Y4_CHECK_LAUNCH();
    bool pastes = false;
    for (int i = 0; i < n; ++i) pastes = pastes || jobs_host[i].paste_from >= 0;
    const int P = S * S;
    for (int r = 0; r < n_ops; ++r) {
        const unsigned char* in = batch[r & 1];
        if (stats_in[r]) {
            hipLaunchKernelGGL(randaug_stats_kernel, dim3((P + kStatPix - 1) / kStatPix, n), dim3(256), 0, st, ops_dev, n_ops, r,
                               S, in, stats);
            Y4_CHECK_LAUNCH();
        }
        const int blocks = (P + kApplyPix - 1) / kApplyPix;
        if (r + 1 < n_ops)
            hipLaunchKernelGGL(randaug_apply_kernel<false>, dim3(blocks, n), dim3(kApplyThreads), 0, st, jobs_dev, ops_dev, n,
                               n_ops, r, S, in, (const unsigned*)stats, batch[(r + 1) & 1], nm, dst, dst_sb, dst_sc, dst_sh,
                               dst_sw);
        else
            hipLaunchKernelGGL(randaug_apply_kernel<true>, dim3(blocks, n, pastes ? 2 : 1), dim3(kApplyThreads), 0, st,
                               jobs_dev, ops_dev, n, n_ops, r, S, in, (const unsigned*)stats, (unsigned char*)nullptr, nm, dst,
                               dst_sb, dst_sc, dst_sh, dst_sw);
        Y4_CHECK_LAUNCH();
    }
    return Y4_OK;
}
