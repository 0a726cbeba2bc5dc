// Eval input pipeline: resize-to-SxS + BGR->RGB + /255 + HWC->CHW in one pass.
// Restates the arithmetic of cv2.resize(..., INTER_LINEAR) on 8-bit images (OpenCV imgproc resize.cpp:
// 11-bit fixed-point coefficients, horizontal pass in int32, vertical pass ((b*(S>>4))>>16, +2, >>2), and the
// exact-2x-downscale special case that OpenCV routes to the 2x2 box average), which is what the reference
// calls at yolo/data/transform.py:173-174; channel flip :437; /255 and permute(2,0,1) :461.
// HBM-bound byte work: one thread per output pixel, 3 channels, source rows stay in L2.
#include "common.h"

namespace {

__device__ __forceinline__ int sat_short(float v) {
    int r = __float2int_rn(v);                      // cvRound: round half to even
    return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}

__global__ void __launch_bounds__(256)
preprocess_kernel(const unsigned char* __restrict__ src, int sh, int sw, long long pitch, int swap_rb,
                  float* __restrict__ dst, long long dsc, long long dsh, long long dsw, int S,
                  double scale_x, double scale_y, int area2x) {
    const int dx = blockIdx.x * 256 + threadIdx.x;
    const int dy = blockIdx.y;
    if (dx >= S) return;
    int v[3];
    if (area2x) {
        const unsigned char* r0 = src + (long long)(2 * dy) * pitch + (long long)(2 * dx) * 3;
        const unsigned char* r1 = r0 + pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2;
    } else {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
        const int a0 = sat_short((1.f - fx) * 2048.f), a1 = sat_short(fx * 2048.f);
        const int sx1 = sx + 1 < sw ? sx + 1 : sw - 1;
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = sat_short((1.f - fy) * 2048.f), b1 = sat_short(fy * 2048.f);
        const int y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        const unsigned char* r0 = src + (long long)y0 * pitch;
        const unsigned char* r1 = src + (long long)y1 * pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
            const int h1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
            int r = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
            v[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int co = swap_rb ? 2 - c : c;
        dst[co * dsc + (long long)dy * dsh + (long long)dx * dsw] = __fdiv_rn((float)v[c], 255.f);
    }
}

// Letterbox for a whole batch in one launch: image b of the descriptor table is resized to (nh, nw) with the arithmetic of
// preprocess_kernel above and placed at (top, left) of its Hc x Wc canvas; everything around it is the fill value, written by
// the same lanes.  HBM-bound (12 B out per pixel): a lane owns four consecutive ox of one row, so a planar row goes out as one
// 16-B store per channel where its address allows it; NHWC slots, unaligned bases and the ragged end of a row take scalar
// stores.  The y coefficients are the lane's, shared by its four pixels.  The two scales are constants of the image: one lane of
// the block forms them (four fp64 divisions) and hands them to the others through LDS.
__global__ void __launch_bounds__(256)
letterbox_batch_kernel(const y4_letterbox_src* __restrict__ table, float* __restrict__ dst, long long dsb, long long dsc,
                       long long dsh, long long dsw, int Hc, int Wc, int W4, float fillv) {
    __shared__ double scales[2];
    const y4_letterbox_src r = table[blockIdx.y];
    if (threadIdx.x == 0) {
        // OpenCV: inv_scale = dsize/ssize (double); scale = 1./inv_scale
        scales[0] = 1.0 / ((double)r.nw / (double)r.w);
        scales[1] = 1.0 / ((double)r.nh / (double)r.h);
    }
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Hc * W4) return;
    const int oy = q / W4, ox0 = (q - oy * W4) * 4;
    const int sh = r.h, sw = r.w;
    const long long pitch = r.pitch;
    const unsigned char* __restrict__ src = static_cast<const unsigned char*>(r.src);
    float v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = fillv;
    const int ry = oy - r.top;
    if (ry >= 0 && ry < r.nh) {
        const bool area2x = sw == 2 * r.nw && sh == 2 * r.nh;
        const double scale_x = scales[0], scale_y = scales[1];
        float fy = (float)((ry + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = sat_short((1.f - fy) * 2048.f), b1 = sat_short(fy * 2048.f);
        const int y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        const unsigned char* r0 = src + (long long)(area2x ? 2 * ry : y0) * pitch;
        const unsigned char* r1 = src + (long long)(area2x ? 2 * ry + 1 : y1) * pitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int rx = ox0 + k - r.left;
            if (rx < 0 || rx >= r.nw) continue;                 // left + nw <= Wc: a pixel inside the image is inside the canvas
            if (area2x) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[k][c] = __fdiv_rn((float)((r0[6 * rx + c] + r0[6 * rx + 3 + c] + r1[6 * rx + c] + r1[6 * rx + 3 + c] + 2) >> 2), 255.f);
            } else {
                float fx = (float)((rx + 0.5) * scale_x - 0.5);
                int sx = (int)floorf(fx);
                fx -= (float)sx;
                if (sx < 0) { fx = 0.f; sx = 0; }
                if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
                const int a0 = sat_short((1.f - fx) * 2048.f), a1 = sat_short(fx * 2048.f);
                const int sx1 = sx + 1 < sw ? sx + 1 : sw - 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
                    const int h1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
                    int t = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    t = t < 0 ? 0 : (t > 255 ? 255 : t);
                    v[k][c] = __fdiv_rn((float)t, 255.f);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int co = r.swap_rb ? 2 - c : c;
        float* p = dst + (long long)blockIdx.y * dsb + co * dsc + (long long)oy * dsh + (long long)ox0 * dsw;
        if (dsw == 1 && ox0 + 3 < Wc && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<f32x4*>(p) = f32x4{v[0][c], v[1][c], v[2][c], v[3][c]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ox0 + k < Wc) p[k * dsw] = v[k][c];
        }
    }
}

}  // namespace

extern "C" int y4_letterbox_batch_u8_f32(const y4_letterbox_src* table_dev, const y4_letterbox_src* table_host, int B,
                                         float* dst, long long dst_sb, long long dst_sc, long long dst_sh, long long dst_sw,
                                         int Hc, int Wc, int fill, void* stream) {
    if (!table_dev || !table_host || !dst) return Y4_ERR_NULL;
    if (B < 1 || B > 65535 || Hc < 1 || Hc > 65535 || Wc < 1 || Wc > 65535 || fill < 0 || fill > 255) return Y4_ERR_SHAPE;
    for (int b = 0; b < B; ++b) {
        const y4_letterbox_src& s = table_host[b];
        if (!s.src) return Y4_ERR_NULL;
        if (s.h < 1 || s.h > 65535 || s.w < 1 || s.w > 65535 || s.pitch < (long long)s.w * 3) return Y4_ERR_SHAPE;
        if (s.nh < 1 || s.nw < 1 || s.top < 0 || s.left < 0 || s.nh > Hc || s.nw > Wc || s.top > Hc - s.nh || s.left > Wc - s.nw)
            return Y4_ERR_SHAPE;
    }
    const int W4 = (Wc + 3) / 4;                           // Hc * W4 <= 65535 * 16384 < 2^31
    dim3 grid((Hc * W4 + 255) / 256, B);
    hipLaunchKernelGGL(letterbox_batch_kernel, grid, dim3(256), 0, (hipStream_t)stream, table_dev, dst, dst_sb, dst_sc,
                       dst_sh, dst_sw, Hc, Wc, W4, (float)fill / 255.0f);
    return hipGetLastError() == hipSuccess ? Y4_OK : Y4_ERR_LAUNCH;
}

extern "C" int y4_preprocess_u8_f32(const void* src, int src_h, int src_w, long long src_pitch_bytes, int swap_rb,
                                    float* dst, long long dst_sc, long long dst_sh, long long dst_sw, int S,
                                    void* stream) {
    if (!src || !dst) return Y4_ERR_NULL;
    if (src_h < 1 || src_w < 1 || S < 1 || S > 65535 || src_pitch_bytes < (long long)src_w * 3) return Y4_ERR_SHAPE;
    // OpenCV: inv_scale = dsize/ssize (double); scale = 1./inv_scale
    const double scale_x = 1.0 / ((double)S / (double)src_w), scale_y = 1.0 / ((double)S / (double)src_h);
    const int area2x = (src_w == 2 * S && src_h == 2 * S) ? 1 : 0;
    dim3 grid((S + 255) / 256, S);
    hipLaunchKernelGGL(preprocess_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src, src_h,
                       src_w, src_pitch_bytes, swap_rb, dst, dst_sc, dst_sh, dst_sw, S, scale_x, scale_y, area2x);
    return hipGetLastError() == hipSuccess ? Y4_OK : Y4_ERR_LAUNCH;
}
