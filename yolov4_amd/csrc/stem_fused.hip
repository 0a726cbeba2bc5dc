// The 3 -> Cout (<= 32) 3x3 stem in training mode WITHOUT its pre-BatchNorm tensor: y0 = conv(x) is 27 multiply-adds per
// value out of an input that sits in L1 / L2, while y0 and its gradient dy0 are the two largest tensors of the step
// (B H W Cout floats each).  Every pass that needs y0 re-forms it in registers with the body of conv_stem_fwd_bf16x3_kernel
// (conv_stem.hip) -- the same gather, the same three-piece split, the same 12 MFMAs in the same order, hence the same
// bits in every pass -- and differs only in what it does with the accumulator tile (lane = channel, 16 pixels per lane):
//   forward   1. statistics   column sums of y0 and y0^2, one row per 256-pixel group (the rows and the order of additions
//                             of conv_stem_fwd_bf16x3_kernel: bit-identical partials), then y4_bn_finalize_partials_f32
//             2. write        z = act(y0 a + b), a = invstd gamma, b = beta - mean a, max|z| into the out_amax word
//   backward  3. reduce       g = dz act'(gamma xhat + beta): sum g, sum g xhat per block, then the BatchNorm fold + finalize
//             4. apply+wgrad  dy0 = gamma invstd (g - k1 - xhat k2) stays in registers and is the A operand of
//                             v_mfma_f32_32x32x2_f32 (K pair = the two pixels the lane halves hold in register e); the B
//                             operand is gathered from x; per-wave [32][32] slabs, folded as y4_conv2d_stem_wgrad_f32 does
// No floating-point atomics, no cross-block synchronisation: every reduction is two-stage and fixed-order.
// Addressing: x through one 32-bit window (checked by y4_stem_fused_ok); z and dz through a window re-based per 256-pixel
// group, so their size is not limited.
#include "conv_geom.h"

namespace {

struct StemFusedGeom {
    const float* x; const float* w;
    long long sxb, sxc, sxh, sxw;
    int B, H, W, Cout;
    long long M;
    int ngroups;
    float inv_hw, inv_w;
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    float* stats;                                  // 1: [ngroups][2][Cout]
    float* z; long long ldz; unsigned* out_amax;   // 2
    const float* dz; long long lddz;               // 3, 4
    float* part;                                   // 3: [gridDim][2][Cout]
    const double* acc; double invM;                // 4: sum g, sum g xhat (fp64, from the finalize)
    float* slabs;                                  // 4: [gridDim * 4][32 n][32 j]
};

// The conv body.  Lane (fr, fh) of a wave gathers for pixel fr of a 32-pixel tile the 16 patch values k = 16 ks + 8 fh + i
// (k = r*9 + c*3 + q; k >= 27 and halo taps read zeros through the buffer bounds check), and receives channel fr of the
// pixels 4 fh + (e & 3) + 8 (e >> 2), e = 0 .. 15, of the tile.
struct StemBody {
    bf16x8 fb[2][3];
    int koff[16];          // byte offset of k relative to the pixel, per lane
    int ktap[16];          // r*3+q (bit index into the 9-bit validity mask), 9 = padding k
    __amdgpu_buffer_rsrc_t rsrc;

    __device__ __forceinline__ void init(const StemFusedGeom& g, int fr, int fh) {
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
        rsrc = y4_make_rsrc(g.x, 0xfffffff0u);      // extent checked on the host
    }

    // (b, h, w) of pixel p < M without an integer division (H W < 2^24: the float quotient is off by one at most)
    static __device__ __forceinline__ void coords(const StemFusedGeom& g, long long p, int& b, int& h, int& w) {
        const int HW = g.H * g.W;
        b = (int)((float)p * g.inv_hw);
        int rem = (int)(p - (long long)b * HW);
        if (rem < 0) { --b; rem += HW; } else if (rem >= HW) { ++b; rem -= HW; }
        h = (int)((float)rem * g.inv_w);
        w = rem - h * g.W;
        if (w < 0) { --h; w += g.W; } else if (w >= g.W) { ++h; w -= g.W; }
    }

    __device__ __forceinline__ void load(const StemFusedGeom& g, float (&xv)[16], long long tile, int fr) const {
        const long long p = tile * 32 + fr;
        unsigned base = 0xffffffffu;
        unsigned m9 = 0;
        if (p < g.M) {
            int b, h, w;
            coords(g, p, b, h, w);
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
    }

    __device__ __forceinline__ f32x16 mma(const float (&xv)[16]) const {
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
        return acc;
    }
};

// row of register e inside a 32-pixel tile, for lane half fh
__device__ __forceinline__ int acc_row(int e, int fh) { return 4 * fh + (e & 3) + 8 * (e >> 2); }

// A [rows][ld] fp32 tensor seen through a window over the (<= 256) rows of one group: lane offsets are 32-bit, rows past
// the tensor's end and channels >= Cout fall outside and read zeros / are not written.
struct GroupWindow {
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ GroupWindow(const float* t, long long ld, int Cout, long long p0, long long M) {
        const long long rows = M - p0 < 256 ? M - p0 : 256;
        rs = y4_make_rsrc(t + p0 * ld, (unsigned)(((rows - 1) * ld + Cout) * 4));
    }
};
// byte offset of (row, channel fr) in the window; channels >= Cout: out of every window
__device__ __forceinline__ int win_off(int row, long long ld, int fr, bool cok) {
    return cok ? (int)(((unsigned)row * (unsigned)ld + (unsigned)fr) * 4u) : -1;
}

// ---------------------------------------------------------------------------------------------- 1. statistics
// The partial rows must come out as conv_stem_fwd_bf16x3_kernel leaves them, bit for bit: the running statistics and the
// values normalised later depend on them.  That kernel adds the ROUNDED square to its sum (its compiled form does not
// contract the pair into an fma), one chain over the 32 values of a lane in register order, both tiles.
__device__ __forceinline__ float square_rounded(float v) {
#pragma clang fp contract(off)
    return v * v;
}

__global__ __launch_bounds__(256) void stem_bn_stats_kernel(const StemFusedGeom g) {
    __shared__ float sred[4][32][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    StemBody body;
    body.init(g, fr, fh);
    float xv0[16], xv1[16];
    for (int grp = blockIdx.x; grp < g.ngroups; grp += gridDim.x) {
        const long long t0 = (long long)grp * 8 + wave * 2;
        body.load(g, xv0, t0, fr);
        body.load(g, xv1, t0 + 1, fr);
        float cs = 0.f, css = 0.f;
        {
            const f32x16 acc = body.mma(xv0);
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float raw = acc[e]; cs += raw; css += square_rounded(raw); }   // pixels past M: exact zeros
        }
        {
            const f32x16 acc = body.mma(xv1);
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float raw = acc[e]; cs += raw; css += square_rounded(raw); }
        }
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

// ---------------------------------------------------------------------------------------------- 2. write
template <int ACT>
__global__ __launch_bounds__(256, 3) void stem_bn_act_write_kernel(const StemFusedGeom g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const bool cok = fr < g.Cout;
    StemBody body;
    body.init(g, fr, fh);
    // as bn_act_fwd_kernel (pointwise.hip) forms them: the same z for the same y0, mean and invstd
    const float a = cok ? g.invstd[fr] * g.gamma[fr] : 0.f;
    const float b = cok ? g.beta[fr] - g.mean[fr] * a : 0.f;
    unsigned amax = 0u;
    float xv0[16], xv1[16];
    for (int grp = blockIdx.x; grp < g.ngroups; grp += gridDim.x) {
        const long long p0 = (long long)grp * 256;
        const long long t0 = (long long)grp * 8 + wave * 2;
        const GroupWindow zw(g.z, g.ldz, g.Cout, p0, g.M);
        const int rows = (int)(g.M - p0 < 256 ? g.M - p0 : 256);
        body.load(g, xv0, t0, fr);
        body.load(g, xv1, t0 + 1, fr);
        auto emit = [&](const f32x16 acc, int row0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = row0 + acc_row(e, fh);
                const float o = y4_act_t<ACT>(acc[e] * a + b);
                // (the whole offset in the vector operand: see st_off in pointwise.hip)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), zw.rs, win_off(row, g.ldz, fr, cok), 0, 0);
                if (cok && row < rows) amax_track1(amax, o);
            }
        };
        emit(body.mma(xv0), wave * 64);
        emit(body.mma(xv1), wave * 64 + 32);
    }
    if (g.out_amax) amax_commit(amax, g.out_amax);
}

// per-lane BatchNorm constants of channel fr (zeros for the idle lanes fr >= Cout: their g and dy0 come out as zeros)
struct BnLane {
    float mu, is, ga, be;
    __device__ __forceinline__ BnLane(const StemFusedGeom& g, int fr, bool cok) {
        mu = cok ? g.mean[fr] : 0.f; is = cok ? g.invstd[fr] : 0.f; ga = cok ? g.gamma[fr] : 0.f; be = cok ? g.beta[fr] : 0.f;
    }
};

__device__ __forceinline__ void load_dz(const GroupWindow& dw, const StemFusedGeom& g, float (&d)[16], int row0, int fr, int fh, bool cok) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
        d[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dw.rs, win_off(row0 + acc_row(e, fh), g.lddz, fr, cok), 0, 0));
}

// ---------------------------------------------------------------------------------------------- 3. reduce
template <int ACT>
__global__ __launch_bounds__(256, 3) void stem_bn_bwd_reduce_kernel(const StemFusedGeom g) {
    __shared__ float sred[4][32][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const bool cok = fr < g.Cout;
    StemBody body;
    body.init(g, fr, fh);
    const BnLane bn(g, fr, cok);
    float S = 0.f, SX = 0.f;                       // the block's sums: group sums (32 values per lane) added group by group
    float xv0[16], xv1[16], d0[16], d1[16];
    for (int grp = blockIdx.x; grp < g.ngroups; grp += gridDim.x) {
        const long long p0 = (long long)grp * 256;
        const long long t0 = (long long)grp * 8 + wave * 2;
        const GroupWindow dw(g.dz, g.lddz, g.Cout, p0, g.M);
        body.load(g, xv0, t0, fr);
        body.load(g, xv1, t0 + 1, fr);
        load_dz(dw, g, d0, wave * 64, fr, fh, cok);
        load_dz(dw, g, d1, wave * 64 + 32, fr, fh, cok);
        float s = 0.f, sx = 0.f;
        auto add = [&](const f32x16 acc, const float (&d)[16]) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {                    // pixels past M: dz reads zero, so g is zero
                const float xh = (acc[e] - bn.mu) * bn.is;
                const float gq = d[e] * y4_act_grad_t<ACT>(bn.ga * xh + bn.be);
                s += gq;
                sx += gq * xh;
            }
        };
        add(body.mma(xv0), d0);
        add(body.mma(xv1), d1);
        S += s; SX += sx;
    }
    S += __shfl_xor(S, 32, 64);
    SX += __shfl_xor(SX, 32, 64);
    if (fh == 0) { sred[wave][fr][0] = S; sred[wave][fr][1] = SX; }
    __syncthreads();
    if (tid < 64) {
        const int c = tid & 31, which = tid >> 5;
        const float t = (sred[0][c][which] + sred[1][c][which]) + (sred[2][c][which] + sred[3][c][which]);
        if (c < g.Cout) g.part[((long long)blockIdx.x * 2 + which) * g.Cout + c] = t;
    }
}

// ---------------------------------------------------------------------------------------------- 4. apply + wgrad
// D[n][j] (32 x 27 -> 32) += sum_p dy0[p][n] x[p + tap(j)][c(j)], j = tap*3 + c as the KRSC filter rows.  MFMA e of a tile
// contracts over the pixel pair {row(e, 0), row(e, 1)}: lane (fr, fh) holds A = dy0[row(e, fh)][n = fr] in its own
// accumulator-derived register and loads B = x[row(e, fh) + tap(fr)][c(fr)].
template <int ACT>
__global__ __launch_bounds__(256, 2) void stem_bn_bwd_apply_wgrad_kernel(const StemFusedGeom g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const bool cok = fr < g.Cout;
    StemBody body;
    body.init(g, fr, fh);
    const BnLane bn(g, fr, cok);
    const float k1 = cok ? (float)(g.acc[fr] * g.invM) : 0.f;
    const float k2 = cok ? (float)(g.acc[g.Cout + fr] * g.invM) : 0.f;
    const float gi = bn.ga * bn.is;
    const bool jok = fr < 27;
    const int tap = jok ? fr / 3 : 0, cj = jok ? fr - tap * 3 : 0;
    const int rj = tap / 3 - 1, qj = tap - (tap / 3) * 3 - 1;
    const unsigned joff = (unsigned)(cj * g.sxc + rj * g.sxh + qj * g.sxw);      // element offset of the lane's tap
    f32x16 wacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) wacc[e] = 0.f;
    // B operand of a tile: the lane's 16 pixels are rows 4 fh + {0..3, 8..11, 16..19, 24..27}; (b, h, w) of the first by
    // reciprocal, the others by stepping (W >= 5: a step of at most 5 pixels wraps at most one image row)
    auto load_b = [&](float (&bv)[16], long long tile) {
        long long p = tile * 32 + 4 * fh;
        int b = 0, h = 0, w = 0;
        if (p < g.M) StemBody::coords(g, p, b, h, w);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int hi = h + rj, wi = w + qj;
            const bool ok = jok && p < g.M && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
            const unsigned xo = ((unsigned)(b * g.sxb + h * g.sxh + w * g.sxw) + joff) * 4u;
            bv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(body.rsrc, ok ? (int)xo : -1, 0, 0));
            const int d = (e & 3) == 3 ? 5 : 1;
            p += d;
            w += d;
            if (w >= g.W) { w -= g.W; if (++h == g.H) { h = 0; ++b; } }
        }
    };
    float xv0[16], xv1[16], d[16], bv[16];
    for (int grp = blockIdx.x; grp < g.ngroups; grp += gridDim.x) {
        const long long p0 = (long long)grp * 256;
        const long long t0 = (long long)grp * 8 + wave * 2;
        const GroupWindow dw(g.dz, g.lddz, g.Cout, p0, g.M);
        const int rows = (int)(g.M - p0 < 256 ? g.M - p0 : 256);
        body.load(g, xv0, t0, fr);
        body.load(g, xv1, t0 + 1, fr);
        load_dz(dw, g, d, wave * 64, fr, fh, cok);
        load_b(bv, t0);
        auto fold = [&](const f32x16 acc, int row0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float xh = (acc[e] - bn.mu) * bn.is;
                const float gq = d[e] * y4_act_grad_t<ACT>(bn.ga * xh + bn.be);
                float dy = gi * (gq - k1 - xh * k2);
                if (row0 + acc_row(e, fh) >= rows) dy = 0.f;          // pixels past M (their B operand is zero as well)
                wacc = __builtin_amdgcn_mfma_f32_32x32x2f32(dy, bv[e], wacc, 0, 0, 0);
            }
        };
        // (one tile's dz and B registers at a time: two waves per SIMD instead of one)
        fold(body.mma(xv0), wave * 64);
        load_dz(dw, g, d, wave * 64 + 32, fr, fh, cok);
        load_b(bv, t0 + 1);
        fold(body.mma(xv1), wave * 64 + 32);
    }
    float* out = g.slabs + ((long long)blockIdx.x * 4 + wave) * 1024;     // [32 n][32 j]
#pragma unroll
    for (int e = 0; e < 16; ++e) out[acc_row(e, fh) * 32 + fr] = wacc[e];
}

constexpr int STATS_GRID = 2048;       // persistent blocks of the passes that stream z / dz
constexpr int WGRAD_GRID = 1024;       // 4096 slabs at most, as y4_conv2d_stem_wgrad_f32

bool fill_geom(StemFusedGeom& g, const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
               int B, int H, int W, int Cout) {
    if (!y4_stem_fused_ok(sxb, sxc, sxh, sxw, B, H, W, Cout)) return false;
    g.x = x; g.w = w; g.sxb = sxb; g.sxc = sxc; g.sxh = sxh; g.sxw = sxw;
    g.B = B; g.H = H; g.W = W; g.Cout = Cout;
    g.M = (long long)B * H * W;
    g.ngroups = (int)((g.M + 255) / 256);
    g.inv_hw = 1.0f / (float)((long long)H * W);
    g.inv_w = 1.0f / (float)W;
    return true;
}
// a 256-row group of a tensor with this pitch fits a 32-bit window
bool pitch_ok(int ld, int Cout) { return ld >= Cout && ld < (1 << 21); }
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
size_t stats_bytes(long long M, int Cout) { return align256((size_t)((M + 255) / 256) * 2 * Cout * sizeof(float)); }

#define Y4_STEM_ACT_SWITCH(ACTV, CALL)                                         \
    switch (ACTV) {                                                            \
        case Y4_ACT_MISH: { constexpr int A_ = Y4_ACT_MISH; CALL; } break;     \
        case Y4_ACT_LEAKY: { constexpr int A_ = Y4_ACT_LEAKY; CALL; } break;   \
        case Y4_ACT_RELU: { constexpr int A_ = Y4_ACT_RELU; CALL; } break;     \
        default: { constexpr int A_ = Y4_ACT_LINEAR; CALL; } break;            \
    }

}  // namespace

extern "C" {

int y4_stem_fused_ok(long long sxb, long long sxc, long long sxh, long long sxw, int B, int H, int W, int Cout) {
    const int mode = y4_get_conv_mode();
    if (mode < 1 || mode > 3) return 0;                                  // the fp32 mode keeps its VALU stem
    if (B <= 0 || H <= 0 || W < 5 || Cout <= 0 || Cout > 32 || (Cout & 3)) return 0;
    if (sxb < 0 || sxc < 0 || sxh < 0 || sxw < 0) return 0;
    if ((long long)H * W >= (1 << 24)) return 0;
    if (((long long)B * H * W + 255) / 256 >= (1ll << 31)) return 0;
    // x: one window, 32-bit byte offsets
    return ((long long)(B - 1) * sxb + 2 * sxc + (long long)(H - 1) * sxh + (long long)(W - 1) * sxw + 1) * 4 < 0xfffffff0ll;
}

size_t y4_stem_bn_act_fwd_workspace(int B, int H, int W, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
    return stats_bytes((long long)B * H * W, Cout) + y4_bn_finalize_workspace(Cout);
}

int y4_stem_bn_act_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                           int B, int H, int W, int Cout, const float* gamma, const float* beta, int act,
                           float* mean, float* invstd, float* running_mean, float* running_var, long long* num_batches_tracked,
                           float momentum, float eps, float* z, int ldz, unsigned* out_amax,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !gamma || !beta || !mean || !invstd || !z || !workspace) return Y4_ERR_NULL;
    StemFusedGeom g{};
    if (!fill_geom(g, x, sxb, sxc, sxh, sxw, w, B, H, W, Cout) || !pitch_ok(ldz, Cout)) return Y4_ERR_SHAPE;
    if (workspace_bytes < y4_stem_bn_act_fwd_workspace(B, H, W, Cout)) return Y4_ERR_WORKSPACE;
    hipStream_t st = y4_stream(stream);
    g.stats = static_cast<float*>(workspace);
    void* fin = static_cast<char*>(workspace) + stats_bytes(g.M, Cout);
    const int grid = g.ngroups < STATS_GRID ? g.ngroups : STATS_GRID;
    hipLaunchKernelGGL(stem_bn_stats_kernel, dim3(grid), dim3(256), 0, st, g);
    Y4_CHECK_LAUNCH();
    const int rc = y4_bn_finalize_partials_f32(g.stats, g.ngroups, g.M, Cout, mean, invstd, running_mean, running_var,
                                               num_batches_tracked, momentum, eps, fin, y4_bn_finalize_workspace(Cout), stream);
    if (rc != Y4_OK) return rc;
    g.mean = mean; g.invstd = invstd; g.gamma = gamma; g.beta = beta;
    g.z = z; g.ldz = ldz; g.out_amax = out_amax;
    Y4_STEM_ACT_SWITCH(act, hipLaunchKernelGGL(stem_bn_act_write_kernel<A_>, dim3(grid), dim3(256), 0, st, g));
    Y4_CHECK_LAUNCH();
    y4::note_kernel("stem_bn_act_write_kernel<%d>", act);
    return Y4_OK;
}

// [finalize words: acc[2C] | bacc][reduce rows][slabs][64 x 1024 doubles]
size_t y4_stem_bn_act_bwd_workspace(int B, int H, int W, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
    return align256(y4_bn_finalize_workspace(Cout)) + align256((size_t)STATS_GRID * 2 * Cout * sizeof(float)) +
           (size_t)WGRAD_GRID * 4 * 1024 * sizeof(float) + 64 * 1024 * sizeof(double);
}

int y4_stem_bn_act_bwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                           const float* dz, int lddz, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, int act, int B, int H, int W, int Cout,
                           float* dgamma, float* dbeta, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !dz || !mean || !invstd || !gamma || !beta || !dgamma || !dbeta || !dw || !workspace) return Y4_ERR_NULL;
    StemFusedGeom g{};
    if (!fill_geom(g, x, sxb, sxc, sxh, sxw, w, B, H, W, Cout) || !pitch_ok(lddz, Cout)) return Y4_ERR_SHAPE;
    if (workspace_bytes < y4_stem_bn_act_bwd_workspace(B, H, W, Cout)) return Y4_ERR_WORKSPACE;
    hipStream_t st = y4_stream(stream);
    char* ws = static_cast<char*>(workspace);
    void* fin = ws;
    g.part = reinterpret_cast<float*>(ws + align256(y4_bn_finalize_workspace(Cout)));
    g.slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(g.part) + align256((size_t)STATS_GRID * 2 * Cout * sizeof(float)));
    double* wpart = reinterpret_cast<double*>(g.slabs + (size_t)WGRAD_GRID * 4 * 1024);
    g.mean = mean; g.invstd = invstd; g.gamma = gamma; g.beta = beta;
    g.dz = dz; g.lddz = lddz;
    g.acc = static_cast<const double*>(fin); g.invM = 1.0 / (double)g.M;
    const int rgrid = g.ngroups < STATS_GRID ? g.ngroups : STATS_GRID;
    Y4_STEM_ACT_SWITCH(act, hipLaunchKernelGGL(stem_bn_bwd_reduce_kernel<A_>, dim3(rgrid), dim3(256), 0, st, g));
    Y4_CHECK_LAUNCH();
    int rc = y4::bn_bwd_fold_finalize(g.part, rgrid, g.M, Cout, fin, dgamma, dbeta, gamma, invstd, st);
    if (rc != Y4_OK) return rc;
    const int wgrid = g.ngroups < WGRAD_GRID ? g.ngroups : WGRAD_GRID;
    Y4_STEM_ACT_SWITCH(act, hipLaunchKernelGGL(stem_bn_bwd_apply_wgrad_kernel<A_>, dim3(wgrid), dim3(256), 0, st, g));
    Y4_CHECK_LAUNCH();
    rc = y4::stem_wgrad_fold(g.slabs, wgrid * 4, wpart, dw, Cout, st);
    if (rc != Y4_OK) return rc;
    y4::note_kernel("stem_bn_bwd_apply_wgrad_kernel<%d>", act);
    return Y4_OK;
}

}  // extern "C"
