// Test-time augmentation: one kernel makes a rescaled / mirrored view of an fp32 input batch, one copies a
// view's eval prediction into its rows of the merged prediction with the boxes mapped back to the base canvas.  Both are
// compared bit for bit with a NumPy float32 restatement (tests/fusion_cases.py): every step below is one fp32 operation in
// the documented order, and this file is built with -ffp-contract=off.  Semantics: include/yolov4_amd.h.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPx = 4;                 // view: consecutive x of one row per lane (one 16-B store on a planar row)
constexpr int kEpt = 4;                // merge: elements per thread and loop trip, kThreads apart (coalesced dwords)

// HBM-bound: 4 B out per element, and at a down-scale r about 1 / r^2 * 4 B in (the four taps of neighbouring lanes share
// their lines).  A lane owns kPx consecutive x of one (b, c, y) row; the y taps and weight are the lane's, shared by its
// pixels.  Pixels right of cw or below ch (the padding up to the stride multiple) are the fill value, written by the same
// lanes.  With flip the lane's pixels read mirrored sources: xs = Wv - 1 - x.
__global__ void __launch_bounds__(kThreads)
tta_view_kernel(const float* __restrict__ in, int H, int W, long long isb, long long isc, long long isy, long long isx,
                float* __restrict__ out, int Hv, int Wv, long long osb, long long osc, long long osy, long long osx, int ch,
                int cw, float ry, float rx, int flip, float fill, int W4) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= Hv * W4) return;
    const int y = q / W4, x0 = (q - y * W4) * kPx;
    const float* __restrict__ src = in + (long long)blockIdx.z * isb + (long long)blockIdx.y * isc;
    float v[kPx];
#pragma unroll
    for (int k = 0; k < kPx; ++k) v[k] = fill;
    if (y < ch) {
        float sy = ((float)y + 0.5f) * ry - 0.5f;
        sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));
        const float fy0 = floorf(sy);
        const float fy = sy - fy0;
        const int y0 = (int)fy0, y1 = min(y0 + 1, H - 1);
        const float* __restrict__ r0 = src + (long long)y0 * isy;
        const float* __restrict__ r1 = src + (long long)y1 * isy;
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const int x = x0 + k;
            const int xs = flip ? Wv - 1 - x : x;
            if (x >= Wv || xs >= cw) continue;              // (xs >= 0: x < Wv)
            float sx = ((float)xs + 0.5f) * rx - 0.5f;
            sx = fminf(fmaxf(sx, 0.f), (float)(W - 1));
            const float fx0 = floorf(sx);
            const float fx = sx - fx0;
            const int xa = (int)fx0, xb = min(xa + 1, W - 1);
            const float a = r0[xa * isx], b = r0[xb * isx], c = r1[xa * isx], d = r1[xb * isx];
            const float top = a + (b - a) * fx;
            const float bot = c + (d - c) * fx;
            v[k] = top + (bot - top) * fy;
        }
    }
    float* p = out + (long long)blockIdx.z * osb + (long long)blockIdx.y * osc + (long long)y * osy + (long long)x0 * osx;
    if (osx == 1 && x0 + kPx - 1 < Wv && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < kPx; ++k)
            if (x0 + k < Wv) p[k * osx] = v[k];
    }
}

// One view's prediction [B, N, n_ch] into rows [row_off, row_off + N) of out [B, n_total, n_ch].  A row of 85 floats is not
// 16-byte aligned and neither are the two slabs against each other, so the kernel indexes flat over the image's slab
// (blockIdx.y), one coalesced dword per lane, and picks the box columns by e % n_ch.  IDENT: a plain copy.
template <bool IDENT>
__global__ void __launch_bounds__(kThreads)
tta_merge_kernel(const float* __restrict__ pred, unsigned slab, unsigned n_ch, float* __restrict__ out, long long out_img,
                 long long out_off, float view_w, int flip, float inv_sx, float inv_sy) {
    const float* __restrict__ src = pred + (long long)blockIdx.y * slab;
    float* __restrict__ dst = out + (long long)blockIdx.y * out_img + out_off;
    for (unsigned base = blockIdx.x * (kThreads * kEpt); base < slab; base += gridDim.x * (kThreads * kEpt)) {
#pragma unroll
        for (int k = 0; k < kEpt; ++k) {
            const unsigned e = base + k * kThreads + threadIdx.x;
            if (e >= slab) continue;
            float v = src[e];
            if (!IDENT) {
                const unsigned c = e % n_ch;
                if (c == 0) v = (flip ? view_w - v : v) * inv_sx;
                else if (c == 1) v = v * inv_sy;
                else if (c == 2) v = v * inv_sx;
                else if (c == 3) v = v * inv_sy;
            }
            dst[e] = v;
        }
    }
}

}  // namespace

extern "C" int y4_tta_view_f32(const float* in, int B, int C, int H, int W, long long in_sb, long long in_sc, long long in_sy,
                               long long in_sx, float* out, int Hv, int Wv, long long out_sb, long long out_sc,
                               long long out_sy, long long out_sx, int ch, int cw, float ry, float rx, int flip, float fill,
                               void* stream) {
    if (!in || !out) return Y4_ERR_NULL;
    if (B < 1 || B > 65535 || C < 1 || C > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || Hv < 1 || Hv > 65535 ||
        Wv < 1 || Wv > 65535 || ch < 1 || cw < 1 || ch > Hv || cw > Wv || (flip != 0 && flip != 1) || !(ry > 0.f) ||
        !(rx > 0.f)) return Y4_ERR_SHAPE;
    const int W4 = (Wv + kPx - 1) / kPx;                   // Hv * W4 <= 65535 * 16384 < 2^31
    dim3 grid((Hv * W4 + kThreads - 1) / kThreads, C, B);
    hipLaunchKernelGGL(tta_view_kernel, grid, dim3(kThreads), 0, y4_stream(stream), in, H, W, in_sb, in_sc, in_sy, in_sx, out,
                       Hv, Wv, out_sb, out_sc, out_sy, out_sx, ch, cw, ry, rx, flip, fill, W4);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_tta_merge_f32(const float* pred, int B, long long N, int n_ch, float* out, long long n_total,
                                long long row_off, float view_w, int flip, float inv_sx, float inv_sy, void* stream) {
    if (!pred || !out) return Y4_ERR_NULL;
    if (B < 1 || B > 65535 || N < 1 || n_ch < 5 || n_total < 1 || row_off < 0 || row_off > n_total || N > n_total - row_off ||
        N * n_ch >= (1ll << 31) || (flip != 0 && flip != 1)) return Y4_ERR_SHAPE;
    const unsigned slab = (unsigned)(N * n_ch);
    const bool ident = flip == 0 && inv_sx == 1.f && inv_sy == 1.f;
    long long blocks = ((long long)slab + kThreads * kEpt - 1) / (kThreads * kEpt);
    if (blocks > 4096) blocks = 4096;
    auto kern = ident ? tta_merge_kernel<true> : tta_merge_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, B), dim3(kThreads), 0, y4_stream(stream), pred, slab, (unsigned)n_ch, out,
                       n_total * n_ch, row_off * n_ch, view_w, flip, inv_sx, inv_sy);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
