// Kernels that only YOLOv4-tiny needs (yolo/model/yolov4_tiny.py): nn.MaxPool2d(2, 2) in both directions and the
// 3 -> Cout 3x3 stride-2 stem conv (forward and filter gradient).  Everything here is memory-bound glue around the
// implicit-GEMM convs: 16-byte accesses per lane over channels, grid-stride loops under a grid cap, two-stage fixed-order
// reductions and no float atomics, so every result is reproducible run to run.
#include "common.h"

namespace {

constexpr int TN_THREADS = 256;
constexpr int TN_GRID_CAP = 2048;          // 256 CUs x 8 blocks: more only shortens the grid-stride loops

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

inline int grid_for(long long total, int cap = TN_GRID_CAP) {
    long long b = (total + TN_THREADS - 1) / TN_THREADS;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}
inline bool vec_ok(const void* p, long long ld, int C) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0 && (C & 3) == 0 && ld >= C && C > 0;
}

// ---------------------------------------------------------------- max pool 2x2, stride 2 (floor)
// one thread per output pixel and four channels; the window is scanned row-major with aten's rule
// (v > best || isnan(v)): the first maximum wins a tie, a NaN wins and the LAST NaN keeps the code
__global__ __launch_bounds__(TN_THREADS) void pool2_fwd_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ y,
                                                               long long ldy, signed char* __restrict__ idx, int B, int H, int W,
                                                               int Ho, int Wo, int C4) {
    const long long total = (long long)B * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const long long pix = i / C4;
        const int wo = (int)(pix % Wo), ho = (int)((pix / Wo) % Ho);
        const long long b = pix / ((long long)Wo * Ho);
        const float* x0 = x + ((b * H + 2 * ho) * W + 2 * wo) * ldx + c;
        f32x4 best = ld4(x0);
        int bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int code = 1; code < 4; ++code) {
            const f32x4 v = ld4(x0 + ((code >> 1) * (long long)W + (code & 1)) * ldx);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = code; }
        }
        st4(y + pix * ldy + c, best);
        if (idx) {
            char4 o;
            o.x = (signed char)bi[0]; o.y = (signed char)bi[1]; o.z = (signed char)bi[2]; o.w = (signed char)bi[3];
            *reinterpret_cast<char4*>(idx + pix * (long long)(C4 * 4) + c) = o;
        }
    }
}

// one thread per 2x2 input block (ceil(H/2) x ceil(W/2) of them) and four channels: it writes the block's up to four dx
// pixels, so every dx element is written exactly once -- dy where the code points, 0 elsewhere and in a dropped odd row / column
__global__ __launch_bounds__(TN_THREADS) void pool2_bwd_kernel(const float* __restrict__ dy, long long lddy,
                                                               const signed char* __restrict__ idx, float* __restrict__ dx,
                                                               long long lddx, int B, int H, int W, int Ho, int Wo, int C4) {
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const long long total = (long long)B * Hc * Wc * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const long long blk = i / C4;
        const int wc = (int)(blk % Wc), hc = (int)((blk / Wc) % Hc);
        const long long b = blk / ((long long)Wc * Hc);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        int code[4] = {-1, -1, -1, -1};
        if (hc < Ho && wc < Wo) {
            const long long pix = (b * Ho + hc) * Wo + wc;
            g = ld4(dy + pix * lddy + c);
            const char4 k = *reinterpret_cast<const char4*>(idx + pix * (long long)(C4 * 4) + c);
            code[0] = k.x; code[1] = k.y; code[2] = k.z; code[3] = k.w;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int h = 2 * hc + (p >> 1), w = 2 * wc + (p & 1);
            if (h >= H || w >= W) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = code[e] == p ? g[e] : 0.f;
            st4(dx + ((b * H + h) * W + w) * lddx + c, o);
        }
    }
}

// ---------------------------------------------------------------- gradient fan-in of the half-channel route
// x is read whole (gradient g_full, C channels) and as its upper half (gradient g_hi, C / 2 channels):
// dx[:, c] = g_full[:, c] + (c >= C / 2 ? g_hi[:, c - C / 2] : 0), either operand absent (NULL) standing for zeros
__global__ __launch_bounds__(TN_THREADS) void fork_half_bwd_kernel(const float* __restrict__ gf, long long ldf,
                                                                   const float* __restrict__ gh, long long ldh,
                                                                   float* __restrict__ dx, long long ldx, long long M, int C4) {
    const long long total = M * C4;
    const int half = C4 / 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / C4;
        const int c4 = (int)(i - m * C4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gf) v = ld4(gf + m * ldf + c4 * 4);
        if (gh && c4 >= half) {
            const f32x4 u = ld4(gh + m * ldh + (c4 - half) * 4);
            v = gf ? v + u : u;
        }
        st4(dx + m * ldx + c4 * 4, v);
    }
}

// ---------------------------------------------------------------- stem 3 -> Cout, 3x3, stride 2, pad 1
// forward: one thread per output pixel and four output channels (the channel group runs fastest: a wave stores whole pixel
// rows back to back).  The filter sits transposed in LDS, [27][Cout], one 16-byte read per tap.  Each output is ONE fma chain
// over the in-bounds taps in (r, q, c) order and then the direct kernel's epilogue expression: the bits of
// y4_conv2d_generic_fwd_f32 (conv_generic.hip)
__global__ __launch_bounds__(TN_THREADS) void stem_s2_fwd_kernel(const float* __restrict__ x, long long sxb, long long sxc,
                                                                 long long sxh, long long sxw, const float* __restrict__ w,
                                                                 float* __restrict__ y, long long ldy, int B, int H, int W,
                                                                 int Cout, int Ho, int Wo, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int act) {
    __shared__ __attribute__((aligned(16))) float ws[27 * 64];
    for (int i = threadIdx.x; i < Cout * 27; i += TN_THREADS) ws[(i % 27) * Cout + i / 27] = w[i];
    __syncthreads();
    const int G = Cout / 4;
    const long long total = (long long)B * Ho * Wo * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int n0 = (int)(i % G) * 4;
        const long long m = i / G;
        const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
        const long long b = m / ((long long)Wo * Ho);
        const float* xb = x + b * sxb;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = ho * 2 - 1 + r;
            if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int wi = wo * 2 - 1 + q;
                if ((unsigned)wi >= (unsigned)W) continue;
                const float* xp = xb + hi * sxh + wi * sxw;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float xv = xp[c * sxc];
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + ((r * 3 + q) * 3 + c) * Cout + n0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv, wv[e], acc[e]);
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = n0 + e;
            float v = acc[e] * (scale ? scale[n] : 1.0f) + (shift ? shift[n] : 0.0f);
            o[e] = y4_act(v, act);
        }
        st4(y + m * ldy + n0, o);
    }
}

// filter gradient, stage 1.  Block `blk` owns the pixels [blk T, (blk + 1) T).  Thread t = (pixel lane pl = t / G, channel
// group g = t % G), G = Cout / 4, P = 256 / G lanes: it walks the pixels pl, pl + P, ... of the tile with 27 x 4 accumulators in
// registers (one fp32 fma chain each, at most ceil(T / P) long), dy read as whole 16-byte groups, the 27 x values once per
// pixel.  The P lanes of a channel group are then summed in lane order through LDS, nine taps at a time, into the block's slab
// slabs[blk][27][Cout].
constexpr int WG_MAX_BLOCKS = 1024;
constexpr int WG_MIN_PIX_PER_LANE = 4;

__global__ __launch_bounds__(TN_THREADS) void stem_s2_wgrad_kernel(const float* __restrict__ x, long long sxb, long long sxc,
                                                                   long long sxh, long long sxw, const float* __restrict__ dy,
                                                                   long long lddy, float* __restrict__ slabs, int B, int H, int W,
                                                                   int Cout, int Ho, int Wo, long long T) {
    __shared__ f32x4 red[9][TN_THREADS];
    const int G = Cout / 4, P = TN_THREADS / G;
    const int g = threadIdx.x % G, pl = threadIdx.x / G;
    const long long M = (long long)B * Ho * Wo;
    const long long m0 = blockIdx.x * T;
    const long long m1 = m0 + T < M ? m0 + T : M;
    f32x4 acc[27];
#pragma unroll
    for (int j = 0; j < 27; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pl < P) {
        for (long long m = m0 + pl; m < m1; m += P) {
            const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
            const long long b = m / ((long long)Wo * Ho);
            const f32x4 d = ld4(dy + m * lddy + g * 4);
            const float* xb = x + b * sxb;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int hi = ho * 2 - 1 + r;
                if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int wi = wo * 2 - 1 + q;
                    if ((unsigned)wi >= (unsigned)W) continue;
                    const float* xp = xb + hi * sxh + wi * sxw;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float xv = xp[c * sxc];
                        const int j = (r * 3 + q) * 3 + c;
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(d[e], xv, acc[j][e]);
                    }
                }
            }
        }
    }
    float* slab = slabs + (long long)blockIdx.x * 27 * Cout;
#pragma unroll
    for (int round = 0; round < 3; ++round) {
#pragma unroll
        for (int j = 0; j < 9; ++j) red[j][threadIdx.x] = acc[round * 9 + j];
        __syncthreads();
        for (int o = threadIdx.x; o < 9 * G; o += TN_THREADS) {
            const int j = o / G, gg = o % G;
            f32x4 s = red[j][gg];
            for (int p = 1; p < P; ++p) s += red[j][p * G + gg];
            st4(slab + (round * 9 + j) * Cout + gg * 4, s);
        }
        __syncthreads();
    }
}

// stage 2: dw[n][j] = sum over the slabs in fp64, fixed order: 16 elements x 16 lanes per block, lane l takes the slabs
// l, l + 16, ..., the 16 lane sums are added in lane order
__global__ __launch_bounds__(TN_THREADS) void stem_s2_wgrad_fold_kernel(const float* __restrict__ slabs, int nslabs, int Cout,
                                                                        float* __restrict__ dw) {
    __shared__ double part[16][16];
    const int ne = 27 * Cout;
    const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;                    // slab element: j * Cout + n
    double s = 0.0;
    if (e < ne)
        for (int k = lane; k < nslabs; k += 16) s += (double)slabs[(long long)k * ne + e];
    part[lane][el] = s;
    __syncthreads();
    if (lane == 0 && e < ne) {
        double t = part[0][el];
        for (int l = 1; l < 16; ++l) t += part[l][el];
        dw[(e % Cout) * 27 + e / Cout] = (float)t;
    }
}

inline bool stem_s2_ok(int B, int H, int W, int Cout) { return B > 0 && H > 0 && W > 0 && Cout > 0 && Cout <= 64 && (Cout & 3) == 0; }

inline int wgrad_blocks(long long M, int Cout) {
    const int P = TN_THREADS / (Cout / 4);
    long long nb = (M + (long long)P * WG_MIN_PIX_PER_LANE - 1) / ((long long)P * WG_MIN_PIX_PER_LANE);
    if (nb > WG_MAX_BLOCKS) nb = WG_MAX_BLOCKS;
    return (int)(nb < 1 ? 1 : nb);
}

}  // namespace

extern "C" {

int y4_maxpool2x2_s2_fwd_f32(const float* x, int ldx, float* y, int ldy, signed char* idx, int B, int H, int W, int C,
                             void* stream) {
    if (!x || !y) return Y4_ERR_NULL;
    if (!vec_ok(x, ldx, C) || !vec_ok(y, ldy, C) || B <= 0 || H <= 0 || W <= 0) return Y4_ERR_SHAPE;
    if (idx && (reinterpret_cast<uintptr_t>(idx) & 3)) return Y4_ERR_SHAPE;
    const int Ho = H / 2, Wo = W / 2;
    if (Ho == 0 || Wo == 0) return Y4_OK;                  // no output element
    hipLaunchKernelGGL(pool2_fwd_kernel, dim3(grid_for((long long)B * Ho * Wo * (C / 4))), dim3(TN_THREADS), 0, y4_stream(stream),
                       x, (long long)ldx, y, (long long)ldy, idx, B, H, W, Ho, Wo, C / 4);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_maxpool2x2_s2_bwd_f32(const float* dy, int lddy, const signed char* idx, float* dx, int lddx, int B, int H, int W, int C,
                             void* stream) {
    if (!dx) return Y4_ERR_NULL;
    const int Ho = H / 2, Wo = W / 2;
    const bool any = Ho > 0 && Wo > 0;                     // (no output element: dy and idx are empty, dx is all zeros)
    if (any && (!dy || !idx)) return Y4_ERR_NULL;
    if (!vec_ok(dx, lddx, C) || B <= 0 || H <= 0 || W <= 0) return Y4_ERR_SHAPE;
    if (any && (!vec_ok(dy, lddy, C) || (reinterpret_cast<uintptr_t>(idx) & 3))) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(pool2_bwd_kernel, dim3(grid_for((long long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4))), dim3(TN_THREADS),
                       0, y4_stream(stream), dy, (long long)lddy, idx, dx, (long long)lddx, B, H, W, Ho, Wo, C / 4);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_fork_half_bwd_f32(const float* g_full, int ldf, const float* g_hi, int ldh, float* dx, int ldx, long long M, int C,
                         void* stream) {
    if (!dx || (!g_full && !g_hi)) return Y4_ERR_NULL;
    if (M <= 0 || C <= 0 || (C & 7) || !vec_ok(dx, ldx, C) || (g_full && !vec_ok(g_full, ldf, C)) ||
        (g_hi && !vec_ok(g_hi, ldh, C / 2)))
        return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(fork_half_bwd_kernel, dim3(grid_for(M * (C / 4))), dim3(TN_THREADS), 0, y4_stream(stream), g_full,
                       (long long)ldf, g_hi, (long long)ldh, dx, (long long)ldx, M, C / 4);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_conv2d_stem_s2_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                              float* y, int ldy, int B, int H, int W, int Cout, const float* scale, const float* shift, int act,
                              void* stream) {
    if (!x || !w || !y) return Y4_ERR_NULL;
    if (!stem_s2_ok(B, H, W, Cout) || ldy < Cout || (ldy & 3) || (reinterpret_cast<uintptr_t>(y) & 15) || act < 0 || act > 3 ||
        sxb < 0 || sxc < 0 || sxh < 0 || sxw < 0)
        return Y4_ERR_SHAPE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(stem_s2_fwd_kernel, dim3(grid_for((long long)B * Ho * Wo * (Cout / 4))), dim3(TN_THREADS), 0,
                       y4_stream(stream), x, sxb, sxc, sxh, sxw, w, y, (long long)ldy, B, H, W, Cout, Ho, Wo, scale, shift, act);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_conv2d_stem_s2_wgrad_workspace(int B, int H, int W, int Cout) {
    if (!stem_s2_ok(B, H, W, Cout)) return 0;
    const long long M = (long long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return (size_t)wgrad_blocks(M, Cout) * 27 * (size_t)Cout * sizeof(float);
}

int y4_conv2d_stem_s2_wgrad_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* dy,
                                int lddy, float* dw, int B, int H, int W, int Cout, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!x || !dy || !dw || !workspace) return Y4_ERR_NULL;
    if (!stem_s2_ok(B, H, W, Cout) || lddy < Cout || (lddy & 3) || (reinterpret_cast<uintptr_t>(dy) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15) || sxb < 0 || sxc < 0 || sxh < 0 || sxw < 0)
        return Y4_ERR_SHAPE;
    if (workspace_bytes < y4_conv2d_stem_s2_wgrad_workspace(B, H, W, Cout)) return Y4_ERR_WORKSPACE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long M = (long long)B * Ho * Wo;
    const int nb = wgrad_blocks(M, Cout);
    const long long T = (M + nb - 1) / nb;
    float* slabs = static_cast<float*>(workspace);
    hipLaunchKernelGGL(stem_s2_wgrad_kernel, dim3(nb), dim3(TN_THREADS), 0, y4_stream(stream), x, sxb, sxc, sxh, sxw, dy,
                       (long long)lddy, slabs, B, H, W, Cout, Ho, Wo, T);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(stem_s2_wgrad_fold_kernel, dim3((27 * Cout + 15) / 16), dim3(TN_THREADS), 0, y4_stream(stream), slabs, nb,
                       Cout, dw);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

}  // extern "C"
