// Training input pipeline: crop-and-pad with a mean fill, horizontal flip, float bilinear resize to SxS, HSV jitter and the
// 4-image mosaic of the reference (yolo/data/transform.py:81-152 crop_and_pad, :155-170 left_right_flip, :173-187
// image_resize, :211-245 color_dithering, :287-329 blend_mosaic), fused into ONE gather per batch: every output pixel
// finds its tile, its position in that tile's resized image, the four taps in the (never materialised) crop image and
// the source bytes or the mean behind each tap.  The random draws are made on the host (AugParams / MosaicParams in
// yolo/data/transform.py); the kernels are deterministic functions of the descriptor table.
// The arithmetic restates OpenCV's float paths (imgproc resize.cpp, generic linear: fp32 coordinates and weights, horizontal
// pass first; color_hsv: RGB2HSV_f / HSV2RGB_f with hrange 360); see include/yolov4_amd.h for the exact statement.
// Byte-gather work: no LDS, no MFMA; one thread per output pixel, three coalesced channel-plane stores.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kSumBlocks = 32;      // blocks per source in the sums launch (grid.x); rows are dealt round-robin

// Exact integer sums of every source's three channels (memory order): uint8 addends, 64-bit accumulators, integer atomics,
// so the totals do not depend on the grid or on the order the blocks arrive in.  h, w <= 65535: a total is < 2^40.
__global__ void __launch_bounds__(256)
augment_sums_kernel(const y4_aug_src* __restrict__ table, unsigned long long* __restrict__ sums) {
    const y4_aug_src s = table[blockIdx.y];
    const unsigned char* __restrict__ src = (const unsigned char*)s.src;
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int y = blockIdx.x; y < s.h; y += gridDim.x) {
        const unsigned char* row = src + (long long)y * s.pitch;
        for (int x = threadIdx.x; x < s.w; x += 256) {
            a0 += row[3 * x];
            a1 += row[3 * x + 1];
            a2 += row[3 * x + 2];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down(a0, off);
        a1 += __shfl_down(a1, off);
        a2 += __shfl_down(a2, off);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* o = sums + 3ll * blockIdx.y;
        if (a0) atomicAdd(o, a0);
        if (a1) atomicAdd(o + 1, a1);
        if (a2) atomicAdd(o + 2, a2);
    }
}

// OpenCV's coordinate of output index r in a source of n samples: fp32 position, floor, fp32 fraction
__device__ __forceinline__ void lin_coord(int r, double scale, int& s, float& f) {
    f = (float)((r + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

__global__ void __launch_bounds__(256)
augment_mosaic_kernel(const y4_aug_src* __restrict__ table, const y4_aug_sample* __restrict__ samples,
                      const unsigned long long* __restrict__ sums, float* __restrict__ dst, long long dsb, long long dsc,
                      long long dsh, long long dsw, int S) {
    const int ox = blockIdx.x * 256 + threadIdx.x;
    const int oy = blockIdx.y;
    const int b = blockIdx.z;
    if (ox >= S) return;
    const y4_aug_sample sm = samples[b];
    int q = 0, tx0 = 0, ty0 = 0;
    if (sm.n_src == 4) {
        const int right = ox >= sm.cut_x, low = oy >= sm.cut_y;
        q = low * 2 + right;
        tx0 = right ? sm.cut_x : 0;
        ty0 = low ? sm.cut_y : 0;
    }
    const int t = sm.first + q;
    const y4_aug_src s = table[t];
    const int rx = ox - tx0 + s.win_x, ry = oy - ty0 + s.win_y;        // position in the tile's resized S x S image

    // --- the four taps in the crop image (crop_h x crop_w)
    const double scale_x = 1.0 / ((double)S / (double)s.crop_w), scale_y = 1.0 / ((double)S / (double)s.crop_h);
    int sx, sy;
    float fx, fy;
    lin_coord(rx, scale_x, sx, fx);
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= s.crop_w - 1) { fx = 0.f; sx = s.crop_w - 1; }
    const int sx1 = sx + 1 < s.crop_w ? sx + 1 : s.crop_w - 1;
    lin_coord(ry, scale_y, sy, fy);
    const int y0 = sy < 0 ? 0 : (sy > s.crop_h - 1 ? s.crop_h - 1 : sy);
    const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > s.crop_h - 1 ? s.crop_h - 1 : sy + 1);
    const float wx0 = 1.f - fx, wx1 = fx, wy0 = 1.f - fy, wy1 = fy;

    // --- crop image -> source: undo the flip, add the crop origin
    const int ux0 = (s.flip ? s.crop_w - 1 - sx : sx) + s.crop_left;
    const int ux1 = (s.flip ? s.crop_w - 1 - sx1 : sx1) + s.crop_left;
    const int uy0 = y0 + s.crop_top, uy1 = y1 + s.crop_top;
    const bool inx0 = ux0 >= 0 && ux0 < s.w, inx1 = ux1 >= 0 && ux1 < s.w;
    const bool iny0 = uy0 >= 0 && uy0 < s.h, iny1 = uy1 >= 0 && uy1 < s.h;
    const bool in00 = iny0 && inx0, in01 = iny0 && inx1, in10 = iny1 && inx0, in11 = iny1 && inx1;
    const unsigned char* __restrict__ src = (const unsigned char*)s.src;
    const unsigned char* p00 = src + (long long)uy0 * s.pitch + 3ll * ux0;
    const unsigned char* p01 = src + (long long)uy0 * s.pitch + 3ll * ux1;
    const unsigned char* p10 = src + (long long)uy1 * s.pitch + 3ll * ux0;
    const unsigned char* p11 = src + (long long)uy1 * s.pitch + 3ll * ux1;
    const bool pad = !(in00 && in01 && in10 && in11);
    const double npix = (double)s.h * (double)s.w;

    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {                       // c: output channel; k: channel in source memory
        const int k = s.swap_rb ? 2 - c : c;
        float m = 0.f;
        if (pad) m = (float)((double)sums[3ll * t + k] / npix);
        const float t00 = in00 ? (float)p00[k] : m, t01 = in01 ? (float)p01[k] : m;
        const float t10 = in10 ? (float)p10[k] : m, t11 = in11 ? (float)p11[k] : m;
        const float h0 = t00 * wx0 + t01 * wx1, h1 = t10 * wx0 + t11 * wx1;
        rgb[c] = h0 * wy0 + h1 * wy1;
    }

    if (s.color && (s.dsat != 1.f || s.dexp != 1.f || s.dhue != 0.f)) {
        const float r = rgb[0], g = rgb[1], bl = rgb[2];
        float v = fmaxf(r, fmaxf(g, bl));
        const float d = v - fminf(r, fminf(g, bl));
        float sat = __fdiv_rn(d, fabsf(v) + FLT_EPSILON);
        const float kk = __fdiv_rn(60.f, d + FLT_EPSILON);
        float h = v == r ? (g - bl) * kk : (v == g ? (bl - r) * kk + 120.f : (r - g) * kk + 240.f);
        if (h < 0.f) h += 360.f;
        h += 179.f * s.dhue;
        sat *= s.dsat;
        v *= s.dexp;
        if (sat == 0.f) {
            rgb[0] = rgb[1] = rgb[2] = v;
        } else {
            h = __fdiv_rn(h, 60.f);
            while (h < 0.f) h += 6.f;                   // |dhue| <= 4 (checked by the host): a handful of laps at most
            while (h >= 6.f) h -= 6.f;
            int sec = (int)floorf(h);
            float f = h - (float)sec;
            if (sec >= 6) { sec = 0; f = 0.f; }         // -tiny + 6 rounds to 6: hue 6 is hue 0
            const float c0 = v, c1 = v * (1.f - sat), c2 = v * (1.f - sat * f), c3 = v * (1.f - sat * (1.f - f));
            // sector:   0   1   2   3   4   5
            //   r      c0  c2  c1  c1  c3  c0
            //   g      c3  c0  c0  c2  c1  c1
            //   b      c1  c1  c3  c0  c0  c2
            rgb[0] = (sec == 0 || sec == 5) ? c0 : (sec == 1 ? c2 : (sec == 4 ? c3 : c1));
            rgb[1] = (sec == 1 || sec == 2) ? c0 : (sec == 0 ? c3 : (sec == 3 ? c2 : c1));
            rgb[2] = (sec == 3 || sec == 4) ? c0 : (sec == 2 ? c3 : (sec == 5 ? c2 : c1));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = fminf(fmaxf(rgb[c], 0.f), 255.f);
    }

    float* o = dst + (long long)b * dsb + (long long)oy * dsh + (long long)ox * dsw;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * dsc] = __fdiv_rn(rgb[c], 255.f);
}

constexpr int kMaxExtent = 1 << 24;    // |crop offsets| and crop sizes: keeps every index sum inside int

bool src_ok(const y4_aug_src& s) {
    if (s.h < 1 || s.w < 1 || s.h > 65535 || s.w > 65535 || s.pitch < 3ll * s.w) return false;
    return true;
}

}  // namespace

extern "C" int y4_augment_means_u8(const y4_aug_src* table_dev, const y4_aug_src* table_host, int n_src,
                                   unsigned long long* sums_dev, void* stream) {
    if (!table_dev || !table_host || !sums_dev) return Y4_ERR_NULL;
    if (n_src < 1 || n_src > 65535) return Y4_ERR_SHAPE;
    for (int i = 0; i < n_src; ++i) {
        if (!table_host[i].src) return Y4_ERR_NULL;
        if (!src_ok(table_host[i])) return Y4_ERR_SHAPE;
    }
    if (hipMemsetAsync(sums_dev, 0, sizeof(unsigned long long) * 3 * (size_t)n_src, y4_stream(stream)) != hipSuccess)
        return Y4_ERR_LAUNCH;
    hipLaunchKernelGGL(augment_sums_kernel, dim3(kSumBlocks, n_src), dim3(256), 0, y4_stream(stream), table_dev, sums_dev);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_augment_mosaic_u8_f32(const y4_aug_src* table_dev, const y4_aug_src* table_host, int n_table,
                                        const y4_aug_sample* samples_dev, const y4_aug_sample* samples_host, int B,
                                        const unsigned long long* sums_dev, float* dst, long long dst_sb, long long dst_sc,
                                        long long dst_sh, long long dst_sw, int S, void* stream) {
    if (!table_dev || !table_host || !samples_dev || !samples_host || !sums_dev || !dst) return Y4_ERR_NULL;
    if (B < 1 || B > 65535 || S < 1 || S > 65535 || n_table < 1) return Y4_ERR_SHAPE;
    for (int b = 0; b < B; ++b) {
        const y4_aug_sample& sm = samples_host[b];
        if (sm.n_src != 1 && sm.n_src != 4) return Y4_ERR_SHAPE;
        if (sm.first < 0 || sm.first > n_table - sm.n_src) return Y4_ERR_SHAPE;
        if (sm.cut_x < 0 || sm.cut_x > S || sm.cut_y < 0 || sm.cut_y > S) return Y4_ERR_SHAPE;
        for (int q = 0; q < sm.n_src; ++q) {
            const y4_aug_src& s = table_host[sm.first + q];
            if (!s.src) return Y4_ERR_NULL;
            if (!src_ok(s)) return Y4_ERR_SHAPE;
            if (s.crop_w < 1 || s.crop_h < 1 || s.crop_w > kMaxExtent || s.crop_h > kMaxExtent) return Y4_ERR_SHAPE;
            if (s.crop_left < -kMaxExtent || s.crop_left > kMaxExtent || s.crop_top < -kMaxExtent || s.crop_top > kMaxExtent)
                return Y4_ERR_SHAPE;
            if (!(fabsf(s.dhue) <= 4.f) || !isfinite(s.dsat) || !isfinite(s.dexp)) return Y4_ERR_SHAPE;
            // the window the tile shows of its resized image has to lie inside that image
            const int ext_x = sm.n_src == 1 ? S : ((q & 1) ? S - sm.cut_x : sm.cut_x);
            const int ext_y = sm.n_src == 1 ? S : ((q & 2) ? S - sm.cut_y : sm.cut_y);
            if (s.win_x < 0 || s.win_y < 0 || s.win_x > S - ext_x || s.win_y > S - ext_y) return Y4_ERR_SHAPE;
        }
    }
    dim3 grid((S + 255) / 256, S, B);
    hipLaunchKernelGGL(augment_mosaic_kernel, grid, dim3(256), 0, y4_stream(stream), table_dev, samples_dev, sums_dev, dst,
                       dst_sb, dst_sc, dst_sh, dst_sw, S);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
