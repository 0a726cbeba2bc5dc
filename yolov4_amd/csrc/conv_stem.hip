// The stem convolution (Cin = 3) for gfx950: forward on VALU (conv mode 0) or on the bf16 matrix cores, the filter gradient
// with its two-stage fold, and their C entries.  (stem_fused.hip holds the variants that recompute the conv inside the
// BatchNorm passes; it borrows y4::stem_wgrad_fold from here.)
#include "common.h"

namespace {

// Cin = 3, k = 3, stride 1, pad 1 (yolo/model/yolov4.py:30).  One thread per output pixel, all
// Cout (<= 32) channels in registers, filter taps come in through the scalar path (uniform
// addresses); the 128-B pixel rows are transposed through LDS so stores are lane-contiguous.
struct StemGeom {
    const float* x; const float* w; float* y; const float* scale; const float* shift;
    float* stats;                 // optional [blocks][2][Cout] column sums of the (raw) output
    long long sxb, sxc, sxh, sxw, ldy;
    int B, H, W, Cout, act;
    long long M;
};

__global__ __launch_bounds__(256) void conv_stem_fwd_kernel(const StemGeom g) {
    __shared__ float tile[4][64][33];
    __shared__ __attribute__((aligned(16))) float wl[27 * 32];          // filter, [tap*3+c][n] (n contiguous)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 27 * 32; i += 256) {
        const int n = i & 31, kk = i >> 5;
        wl[i] = n < g.Cout ? g.w[n * 27 + kk] : 0.f;
    }
    __syncthreads();
    const long long pix0 = (long long)blockIdx.x * 256 + wave * 64;
    const long long pix = pix0 + lane;
    float acc[32];
#pragma unroll
    for (int n = 0; n < 32; ++n) acc[n] = 0.f;
    if (pix < g.M) {
        const int b = (int)(pix / ((long long)g.H * g.W));
        const int rem = (int)(pix - (long long)b * g.H * g.W);
        const int h = rem / g.W, w = rem - h * g.W;
        const float* xb = g.x + b * g.sxb;
        float xv[27];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int hi = h + r - 1, wi = w + q - 1;
                const bool ok = (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
#pragma unroll
                for (int c = 0; c < 3; ++c) xv[(r * 3 + q) * 3 + c] = ok ? xb[c * g.sxc + hi * g.sxh + wi * g.sxw] : 0.f;
            }
        // taps one at a time (sched_barrier keeps the 216 LDS broadcasts from being hoisted into 864 registers)
#pragma unroll
        for (int kk = 0; kk < 27; ++kk) {
            const f32x4* wp = reinterpret_cast<const f32x4*>(wl + kk * 32);
            const float v = xv[kk];
#pragma unroll
            for (int n4 = 0; n4 < 8; ++n4) {
                const f32x4 wv = wp[n4];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[n4 * 4 + e] = fmaf(v, wv[e], acc[n4 * 4 + e]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int n = 0; n < 32; ++n) {
        float v = acc[n];
        if (n < g.Cout) {
            v = v * (g.scale ? g.scale[n] : 1.f) + (g.shift ? g.shift[n] : 0.f);
            v = y4_act(v, g.act);
        }
        tile[wave][lane][n] = v;
    }
    __syncthreads();
    // 64 pixels x 32 ch: lane -> (pixel = it*2 + lane/32, ch = lane%32): 128-B contiguous per half wave
    const int ch = lane & 31;
    if (ch < g.Cout) {
#pragma unroll 4
        for (int it = 0; it < 32; ++it) {
            const int pl = it * 2 + (lane >> 5);
            const long long p = pix0 + pl;
            if (p < g.M) g.y[p * g.ldy + ch] = tile[wave][pl][ch];
        }
    }
    if (g.stats) {                                   // uniform branch: column sums of this block's 256 pixels
        __shared__ float sred[8][32][2];
        const int grp = tid >> 5;                    // 8 groups of 32 pixels
        float cs = 0.f, css = 0.f;
        for (int i = 0; i < 32; ++i) { const float v = tile[grp >> 1][(grp & 1) * 32 + i][ch]; cs += v; css += v * v; }
        sred[grp][ch][0] = cs; sred[grp][ch][1] = css;
        __syncthreads();
        if (tid < 64) {
            const int c = tid & 31, which = tid >> 5;
            float t = 0.f;
            for (int k = 0; k < 8; ++k) t += sred[k][c][which];
            if (c < g.Cout) g.stats[((long long)blockIdx.x * 2 + which) * g.Cout + c] = t;
        }
    }
}

// Stem forward on the matrix cores (bf16x3 mode): the 27-value patch of a pixel is the A row (K = 27 -> 32,
// ordered k = r*9 + c*3 + q so that the three q of one (r, c) are neighbours in memory), gathered straight from
// the strided input into the MFMA A layout (lane = pixel, 2 x 8 k values), split in registers; the filter is
// 24 VGPRs of B fragments per wave.  12 MFMAs per 32 pixels x 32 channels; the C layout (lane = channel) gives
// 128-byte contiguous stores.  Persistent blocks walk groups of 256 pixels and leave one BN-statistics row
// per group (same contract as the VALU kernel above).
__global__ __launch_bounds__(256) void conv_stem_fwd_bf16x3_kernel(const StemGeom g, const int ngroups, const float inv_hw,
                                                                   const float inv_w) {
    __shared__ float sred[4][32][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const int HW = g.H * g.W;
    bf16x8 fb[2][3];
    int koff[16];          // element offset of k relative to the pixel, per lane
    int ktap[16];          // r*3+q (bit index into the 9-bit validity mask), 9 = padding k
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int k = (i >> 3) * 16 + fh * 8 + (i & 7);
        const int r = k / 9, c = (k - r * 9) / 3, q = k - r * 9 - c * 3;
        const bool kv = k < 27;
        koff[i] = kv ? (int)(c * g.sxc + (r - 1) * g.sxh + (q - 1) * g.sxw) * 4 : 0;
        ktap[i] = kv ? r * 3 + q : 9;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        f32x4 w0, w1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = ks * 16 + fh * 8 + i;
            const int r = k / 9, c = (k - r * 9) / 3, q = k - r * 9 - c * 3;
            const float v = (k < 27 && fr < g.Cout) ? g.w[fr * 27 + (r * 3 + q) * 3 + c] : 0.f;
            if (i < 4) w0[i] = v; else w1[i - 4] = v;
        }
        u32x2 a1, a2, a3, b1, b2, b3;
        split3x4(w0, a1, a2, a3);
        split3x4(w1, b1, b2, b3);
        const u32x4 q1 = {a1[0], a1[1], b1[0], b1[1]}, q2 = {a2[0], a2[1], b2[0], b2[1]}, q3 = {a3[0], a3[1], b3[0], b3[1]};
        fb[ks][0] = __builtin_bit_cast(bf16x8, q1); fb[ks][1] = __builtin_bit_cast(bf16x8, q2); fb[ks][2] = __builtin_bit_cast(bf16x8, q3);
    }
    const float sc = (g.scale && fr < g.Cout) ? g.scale[fr] : 1.f;
    const float sh = (g.shift && fr < g.Cout) ? g.shift[fr] : 0.f;
    const __amdgpu_buffer_rsrc_t rsrc = y4_make_rsrc(g.x, 0xfffffff0u);      // extent checked on the host
    float xv0[16], xv1[16];
    auto load = [&](float (&xv)[16], long long tile) {
        const long long p = tile * 32 + fr;
        unsigned base = 0xffffffffu;
        unsigned m9 = 0;
        if (p < g.M) {
            int b = (int)((float)p * inv_hw);
            int rem = (int)(p - (long long)b * HW);
            if (rem < 0) { --b; rem += HW; } else if (rem >= HW) { ++b; rem -= HW; }
            int h = (int)((float)rem * inv_w);
            int w = rem - h * g.W;
            if (w < 0) { --h; w += g.W; } else if (w >= g.W) { ++h; w -= g.W; }
            base = (unsigned)(b * g.sxb + h * g.sxh + w * g.sxw) * 4u;
            const unsigned hm = (h > 0 ? 1u : 0u) | 2u | (h + 1 < g.H ? 4u : 0u);
            const unsigned wm = (w > 0 ? 1u : 0u) | 2u | (w + 1 < g.W ? 4u : 0u);
            m9 = ((hm & 1u) ? wm : 0u) | ((hm & 2u) ? wm << 3 : 0u) | ((hm & 4u) ? wm << 6 : 0u);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool ok = (m9 >> ktap[i]) & 1u;
            xv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, ok ? (int)(base + (unsigned)koff[i]) : -1, 0, 0));
        }
    };
    float cs = 0.f, css = 0.f;
    auto compute = [&](float (&xv)[16], long long tile) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f32x4 v0 = {xv[ks * 8 + 0], xv[ks * 8 + 1], xv[ks * 8 + 2], xv[ks * 8 + 3]};
            const f32x4 v1 = {xv[ks * 8 + 4], xv[ks * 8 + 5], xv[ks * 8 + 6], xv[ks * 8 + 7]};
            u32x2 a1, a2, a3, b1, b2, b3;
            split3x4(v0, a1, a2, a3);
            split3x4(v1, b1, b2, b3);
            const u32x4 q1 = {a1[0], a1[1], b1[0], b1[1]}, q2 = {a2[0], a2[1], b2[0], b2[1]}, q3 = {a3[0], a3[1], b3[0], b3[1]};
            const bf16x8 f1 = __builtin_bit_cast(bf16x8, q1), f2 = __builtin_bit_cast(bf16x8, q2), f3 = __builtin_bit_cast(bf16x8, q3);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f3, fb[ks][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f2, fb[ks][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, fb[ks][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f2, fb[ks][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, fb[ks][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, fb[ks][0], acc, 0, 0, 0);
        }
        const long long mbase = tile * 32 + 4 * fh;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float raw = acc[e];
            cs += raw; css += raw * raw;                  // pixels past M contribute exact zeros
            const long long m = mbase + (e & 3) + 8 * (e >> 2);
            if (fr < g.Cout && m < g.M) g.y[m * g.ldy + fr] = y4_act(raw * sc + sh, g.act);
        }
    };
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long t0 = (long long)grp * 8 + wave * 2;
        load(xv0, t0);
        load(xv1, t0 + 1);
        cs = 0.f; css = 0.f;
        compute(xv0, t0);
        compute(xv1, t0 + 1);
        if (g.stats) {
            cs += __shfl_xor(cs, 32, 64);
            css += __shfl_xor(css, 32, 64);
            if (fh == 0) { sred[wave][fr][0] = cs; sred[wave][fr][1] = css; }
            __syncthreads();
            if (tid < 64) {
                const int c = tid & 31, which = tid >> 5;
                const float t = (sred[0][c][which] + sred[1][c][which]) + (sred[2][c][which] + sred[3][c][which]);
                if (c < g.Cout) g.stats[((long long)grp * 2 + which) * g.Cout + c] = t;
            }
            __syncthreads();
        }
    }
}

// wgrad of the stem: D[n][j] (32 x 27->32) = sum_p dy[p][n] * x[p + tap(j)][c(j)], operands
// straight from global memory into the MFMA (a dy pixel row IS the 32-float A fragment).
struct StemWgradGeom {
    const float* x; const float* dy; float* slabs;
    long long sxb, sxc, sxh, sxw, lddy;
    int B, H, W, Cout;
    long long M, pix_per_wave;
};

__global__ __launch_bounds__(256) void conv_stem_wgrad_kernel(const StemWgradGeom g) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long long wave_id = (long long)blockIdx.x * 4 + (tid >> 6);
    const long long p_begin = wave_id * g.pix_per_wave;
    long long p_end = p_begin + g.pix_per_wave;
    if (p_end > g.M) p_end = g.M;
    const int fr = lane & 31, fh = lane >> 5;
    const bool jok = fr < 27;
    const int tap = jok ? fr / 3 : 0, c = jok ? fr - tap * 3 : 0;
    const int r = tap / 3 - 1, q = tap - (tap / 3) * 3 - 1;
    const bool nok = fr < g.Cout;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    // running (b, h, w) of this lane's pixel p = p_begin + fh + 2*iter: no divisions in the loop
    long long p = p_begin + fh;
    int b = 0, h = 0, w = 0;
    if (p < g.M) {
        b = (int)(p / ((long long)g.H * g.W));
        const int rem = (int)(p - (long long)b * g.H * g.W);
        h = rem / g.W; w = rem - h * g.W;
    }
    // 8 pixel pairs per trip: 16 independent buffer loads (out-of-range / halo lanes read zeros through the
    // descriptor's bounds check) are in flight before the 8 MFMAs consume them -- the loop is latency-bound otherwise
    const long long dy_first = p_begin < g.M ? p_begin : 0;
    const __amdgpu_buffer_rsrc_t dy_rsrc = y4_make_rsrc(g.dy + dy_first * g.lddy, (unsigned)(g.pix_per_wave * g.lddy * 4));
    const __amdgpu_buffer_rsrc_t x_rsrc = y4_make_rsrc(g.x, 0xfffffff0u);                     // extent checked on the host
    const unsigned dy_step = (unsigned)g.lddy * 8u;                                            // 2 pixels
    unsigned dy_off = ((unsigned)fh * (unsigned)g.lddy + (unsigned)fr) * 4u;
    const long long coff = c * g.sxc;
    for (long long pc = p_begin; pc < p_end; pc += 16) {
        float a[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool pok = p < p_end;
            const int hi = h + r, wi = w + q;
            const bool xok = pok && jok && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
            const unsigned xo = (unsigned)(b * g.sxb + coff + hi * g.sxh + wi * g.sxw) * 4u;
            a[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dy_rsrc, (pok && nok) ? (int)dy_off : -1, 0, 0));
            bv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rsrc, xok ? (int)xo : -1, 0, 0));
            dy_off += dy_step;
            p += 2;
            w += 2;
            if (w >= g.W) { w -= g.W; if (++h == g.H) { h = 0; ++b; } }  // W >= 2
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bv[u], acc, 0, 0, 0);
    }
    float* out = g.slabs + wave_id * 1024;     // [32 n][32 j]
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int n = (e & 3) + 8 * (e >> 2) + 4 * fh;
        out[n * 32 + fr] = acc[e];
    }
}

// Two coalesced stages over the per-wave slabs [nslabs][32 n][32 j]: 64 blocks each fold nslabs/64 slabs for all
// 1024 entries (thread <-> 4 consecutive entries, fp64), then one block folds the 64 partial rows in a fixed order.
__global__ __launch_bounds__(256) void stem_wgrad_reduce1_kernel(const float* __restrict__ slabs, double* __restrict__ part,
                                                                 int nslabs) {
    const int per = (nslabs + gridDim.x - 1) / gridDim.x;
    const int k0 = blockIdx.x * per;
    const int k1 = min(nslabs, k0 + per);
    double s[4] = {0, 0, 0, 0};
    for (int k = k0; k < k1; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slabs + (long long)k * 1024 + threadIdx.x * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[(long long)blockIdx.x * 1024 + threadIdx.x * 4 + e] = s[e];
}
__global__ __launch_bounds__(256) void stem_wgrad_reduce2_kernel(const double* __restrict__ part, float* __restrict__ dw,
                                                                 int nparts, int Cout) {
    for (int i = threadIdx.x; i < Cout * 27; i += 256) {
        const int n = i / 27, j = i - n * 27;
        double s = 0.0;
        for (int k = 0; k < nparts; ++k) s += part[(long long)k * 1024 + n * 32 + j];
        dw[i] = (float)s;
    }
}

constexpr int STEM_WAVES = 4096;

}  // namespace

namespace y4 {
// the two fold launches of y4_conv2d_stem_wgrad_f32 over another producer's slabs (stem_fused.hip)
int stem_wgrad_fold(const float* slabs, int nslabs, double* part, float* dw, int Cout, hipStream_t st) {
    hipLaunchKernelGGL(stem_wgrad_reduce1_kernel, dim3(64), dim3(256), 0, st, slabs, part, nslabs);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(stem_wgrad_reduce2_kernel, dim3(1), dim3(256), 0, st, part, dw, 64, Cout);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
}  // namespace y4

extern "C" {

int y4_conv2d_stem_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw,
                           const float* w, float* y, int ldy, int B, int H, int W, int Cout,
                           const float* scale, const float* shift, int act,
                           float* bnstats_partials, void* stream) {
    if (!x || !w || !y) return Y4_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 32 || ldy < Cout) return Y4_ERR_SHAPE;
    StemGeom g{};
    g.x = x; g.w = w; g.y = y; g.scale = scale; g.shift = shift; g.stats = bnstats_partials;
    g.sxb = sxb; g.sxc = sxc; g.sxh = sxh; g.sxw = sxw; g.ldy = ldy;
    g.B = B; g.H = H; g.W = W; g.Cout = Cout; g.act = act;
    g.M = (long long)B * H * W;
    const long long blocks = (g.M + 255) / 256;
    if (blocks >= (1ll << 31)) return Y4_ERR_SHAPE;
    // matrix-core variant: bf16x3 arithmetic, 32-bit byte offsets into x (non-negative strides)
    const int mode = y4_get_conv_mode();
    const bool mfma_ok = (mode >= 1 && mode <= 3) && sxb >= 0 && sxc >= 0 && sxh >= 0 && sxw >= 0 &&
                         ((long long)(B - 1) * sxb + 2 * sxc + (long long)(H - 1) * sxh + (long long)(W - 1) * sxw + 1) * 4 < 0xfffffff0ll &&
                         (long long)H * W < (1 << 24);
    if (mfma_ok) {
        const int grid = (int)(blocks < 2048 ? blocks : 2048);
        hipLaunchKernelGGL(conv_stem_fwd_bf16x3_kernel, dim3(grid), dim3(256), 0, y4_stream(stream), g, (int)blocks,
                           1.0f / (float)((long long)H * W), 1.0f / (float)W);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    hipLaunchKernelGGL(conv_stem_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, y4_stream(stream), g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_conv2d_stem_wgrad_workspace(int, int, int, int) {
    return (size_t)STEM_WAVES * 1024 * sizeof(float) + 64 * 1024 * sizeof(double);
}

int y4_conv2d_stem_wgrad_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw,
                             const float* dy, int lddy, float* dw, int B, int H, int W, int Cout,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !dy || !dw || !workspace) return Y4_ERR_NULL;
    if (B <= 0 || H <= 0 || W < 2 || Cout <= 0 || Cout > 32 || lddy < Cout) return Y4_ERR_SHAPE;
    if (workspace_bytes < y4_conv2d_stem_wgrad_workspace(B, H, W, Cout)) return Y4_ERR_WORKSPACE;
    StemWgradGeom g{};
    g.x = x; g.dy = dy; g.slabs = static_cast<float*>(workspace);
    g.sxb = sxb; g.sxc = sxc; g.sxh = sxh; g.sxw = sxw; g.lddy = lddy;
    g.B = B; g.H = H; g.W = W; g.Cout = Cout;
    g.M = (long long)B * H * W;
    long long ppw = (g.M + STEM_WAVES - 1) / STEM_WAVES;
    ppw = (ppw + 15) & ~15ll;                     // 16-pixel trips (8 MFMA pixel pairs) never straddle waves
    if ((long long)ppw * lddy * 4 >= 0xfffffff0ll || sxb < 0 || sxc < 0 || sxh < 0 || sxw < 0 ||
        ((long long)(B - 1) * sxb + 2 * sxc + (long long)(H - 1) * sxh + (long long)(W - 1) * sxw + 1) * 4 >= 0xfffffff0ll)
        return Y4_ERR_SHAPE;
    g.pix_per_wave = ppw;
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(conv_stem_wgrad_kernel, dim3(STEM_WAVES / 4), dim3(256), 0, st, g);
    Y4_CHECK_LAUNCH();
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + (size_t)STEM_WAVES * 1024 * sizeof(float));
    return y4::stem_wgrad_fold(static_cast<const float*>(workspace), STEM_WAVES, part, dw, Cout, st);
}

}  // extern "C"
