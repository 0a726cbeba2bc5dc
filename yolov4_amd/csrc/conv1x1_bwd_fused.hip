// Backward of a 1x1 stride-1 conv + training-mode BatchNorm + activation on a large map, f16x2 arithmetic, in ONE sweep:
// the BatchNorm backward apply (dy from dz and y), the input gradient dx = dy W and the filter gradient dW = dy^T x.
// These layers (Cout 32 / 64, Cin 64 / 128 on the 304^2 and 152^2 maps) are HBM-bound; run as three kernels they write dy once
// and read it twice (7 tensor passes), here dy exists only in registers and LDS (4 passes: dz, y, x in, dx out).
//
// Structure: conv_wgrad_f16x2<., ., 32> (conv_f16x2.hip) with the whole dW tile in one block's accumulators and split-K over
// contiguous pixel ranges, one block per range:
//   * per 32-pixel chunk, threads own 4-pixel x 4-channel blocks: a "dy" thread loads its block of dz and of y, evaluates
//     dy = gamma invstd (g - k1 - xhat k2), g = dz act'(gamma xhat + beta) -- the expression of bn_act_bwd_apply_kernel
//     (pointwise.hip), k1 / k2 from the same fp64 sums -- and splits it under the scale of the BOUND of max|dy| the reduce /
//     finalize kernels derived (word [5], as the plane layers); an "x" thread loads and splits its block of x.  Both images go
//     to LDS transposed, [channel][32 pixels] rows of two fp16 planes, two stages, one barrier per chunk.  The waves swap
//     roles from chunk to chunk so that the activation derivative's VALU work lands on all four SIMDs.
//   * dW[n][j] += sum_p dy[p][n] x[p][j]: 32x32x16 MFMAs over the staged rows, accumulators live across the block's chunks,
//     one fp32 slab per block (two where the dW tile has only two 32 x 32 tiles: wave pairs then halve the chunk's pixels),
//     y4::slab_reduce in fixed order afterwards.
//   * dx[p][c] = sum_n dy[p][n] W[n][c] from the SAME staged dy rows: read back through ds_read_b64_tr_b16 (pixels become the
//     MFMA column, 8 consecutive channels the k axis), against the transposed split filter [Cin][Cout] resident in LDS, with
//     16x16x32 MFMAs in the order D[c][p] = W^T dy^T -- a lane then holds four consecutive channels of one pixel and stores
//     16 B.  Accumulators zeroed and stored per chunk, + the skip operand; stores and skip loads go through a buffer window
//     re-based at the block's first pixel that ends at row M.
// Three MFMAs per product, two accumulator sets, as everywhere in the f16x2 mode.  No atomics, no block waits on another:
// results are bit-identical from run to run.
#include "common.h"
#include "conv_geom.h"
#include "f16x2.h"

namespace {

using namespace y4x2;

struct FusedGeom {
    const float* dz; const float* y; const float* x; const float* res;
    float* dx; float* slabs;
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    const double* acc;                    // (sum g, sum g xhat)[2 Cout] in fp64: the finalize kernel's words
    unsigned* bounds;                     // words [0..4] from the reduce / finalize kernels; [5] receives the bound of max|dy|
    const unsigned char* wt_planes;       // transposed split filter [Cin][Cout / 32][64 B hi | 64 B lo]
    const unsigned* wt_amax; const unsigned* x_amax;
    long long lddz, ldy, ldx, lddx, ldr;  // pixel pitches (elements)
    int M, chunks_per_split;              // chunks of 32 pixels; every block has at least one
    double invM;
};

typedef __fp16 trh4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// rows [p0, M) of a tensor with pitch ld as a 32-bit window: rows past M read zeros and are not written
__device__ __forceinline__ __amdgpu_buffer_rsrc_t px_window(const float* t, long long ld, long long p0, long long M) {
    const unsigned long long left = (unsigned long long)(M - p0) * (unsigned long long)ld * 4ull;
    return y4_make_rsrc(t + p0 * ld, (unsigned)(left < 0xfffffff0ull ? left : 0xfffffff0ull));
}

template <int CO, int CI, int ACT, bool RES>
__global__ __launch_bounds__(256, 2) void conv1x1_bn_act_bwd_fused_f16x2(const FusedGeom g) {
    static_assert((CO == 32 || CO == 64) && (CI == 64 || CI == 128), "supported channel counts");
    constexpr int NAW = CO / 32;                           // waves forming dy per chunk (64 blocks of 4 px x 4 ch each)
    constexpr int ROT = CO == 64 ? 2 : 1;                  // role rotation per chunk (keeps a thread's dy channel group fixed)
    constexpr int NXW = 2;                                 // waves staging x per chunk
    constexpr int XB = (CI / 32) / NXW;                    // x blocks per thread of such a wave (64 blocks per 32 channels)
    constexpr int STAGE = 2 * (CO + CI) * ROWB;            // bytes per LDS stage: 2 planes of dy rows and of x rows
    constexpr int B_OFF = 2 * CO * ROWB;                   // x rows inside a stage
    constexpr int W_OFF = 2 * STAGE;                       // filter planes [2][CI] rows of CO fp16, behind the stages
    constexpr int RW = CO * 2;                             // bytes per filter row: 64 or 128, unpadded, 16-B chunks XOR-swizzled
    constexpr int WI = CO / 32;                            // dW: 32-row tiles along n; 2 waves along j
    constexpr int KSP = 2 / WI;                            // ... and wave pairs halving the chunk's pixels where WI == 1
    constexpr int MJ = CI / 64;                            // dW: 32-column tiles per wave
    constexpr int NCT = CI / 32;                           // dgrad: 16-channel tiles of dx per wave (2 pixel tiles x 2 halves of Cin)
    constexpr int KS = CO / 32;                            // dgrad: 32-deep k steps
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int split = blockIdx.x;
    const int chunk0 = split * g.chunks_per_split;
    int nchunks = (g.M + 31) / 32 - chunk0;
    if (nchunks > g.chunks_per_split) nchunks = g.chunks_per_split;
    const long long p_first = (long long)chunk0 * 32;

    // ---- the filter, once per block: chunk c of row r at c ^ wswz(r) (conflict-free ds_read_b128 down 16 rows)
    auto wswz = [](int row) { return RW == 64 ? (row >> 2) & 3 : (row >> 1) & 7; };
    {
        constexpr int CPR = CO / 8;                        // 16-B chunks per row and plane
        for (int i = tid; i < 2 * CI * CPR; i += 256) {
            const int pl = i / (CI * CPR);
            const int rem = i - pl * (CI * CPR);
            const int row = rem / CPR, ch = rem - row * CPR;
            const u32x4 v = *reinterpret_cast<const u32x4*>(g.wt_planes + (size_t)row * (CO * 4) + (ch >> 2) * 128 + pl * 64 + (ch & 3) * 16);
            *reinterpret_cast<u32x4*>(smem_b + W_OFF + (pl * CI + row) * RW + ((ch ^ wswz(row)) << 4)) = v;
        }
    }

    // ---- scales: dy under the bound of the reduce pass, formed exactly as bn_act_bwd_apply_kernel forms word [5]
    const float bnd = __uint_as_float(g.bounds[2]) *
                      (__uint_as_float(g.bounds[0]) + __uint_as_float(g.bounds[3]) + __uint_as_float(g.bounds[1]) * __uint_as_float(g.bounds[4])) * 1.0001f;
    const unsigned bb = __float_as_uint(bnd);
    if (blockIdx.x == 0 && tid == 0) g.bounds[5] = bb;
    const unsigned se_dy = f16x2_scale_exp(bb);            // a poisoned word (NaN / Inf): scale 1
    const float ps = __uint_as_float(se_dy << 23), un_dy = __uint_as_float((254u - se_dy) << 23);
    const float s_x = f16x2_scale(g.x_amax);

    const __amdgpu_buffer_rsrc_t dz_rs = px_window(g.dz, g.lddz, p_first, g.M), y_rs = px_window(g.y, g.ldy, p_first, g.M),
                                 x_rs = px_window(g.x, g.ldx, p_first, g.M), dx_rs = px_window(g.dx, g.lddx, p_first, g.M),
                                 r_rs = px_window(RES ? g.res : g.dx, RES ? g.ldr : g.lddx, p_first, g.M);
    const unsigned OOB = 0xffffffffu;
    const unsigned dz_pix = (unsigned)g.lddz * 4u, y_pix = (unsigned)g.ldy * 4u, x_pix = (unsigned)g.ldx * 4u;

    // ---- staging roles.  pg: the thread's group of 4 pixels in the chunk.  As a dy thread it owns channels cga*4 .. +3 of dy
    // for the whole kernel (wave w & (NAW - 1) takes the w-th 64 blocks): the per-channel constants stay in registers
    const int pg = lane & 7;
    const int cga = (wave & (NAW - 1)) * 8 + (lane >> 3);
    f32x4 mu, is, ga, be, k1, k2, gi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = cga * 4 + e;
        mu[e] = g.mean[c]; is[e] = g.invstd[c]; ga[e] = g.gamma[c]; be[e] = g.beta[c];
        k1[e] = (float)(g.acc[c] * g.invM);
        k2[e] = (float)(g.acc[CO + c] * g.invM);
        gi[e] = ga[e] * is[e];
    }
    // role of this wave in chunk c: rot < NAW: dy; NAW <= rot < NAW + NXW: x, blocks (rot - NAW) * 64 * XB + u * 64 + lane
    auto rot_of = [&](int c) { return (wave + ROT * c) & 3; };
    // LDS byte offset of the 8-B piece (4 pixels) in row 4 cg of a plane (rows 4 cg + e: + e ROWB; same swizzle)
    auto piece = [&](int cg) { return cg * 4 * ROWB + (((pg >> 1) ^ (cg & 3)) << 4) + ((pg & 1) << 3); };

    f32x4 r[8];                                            // dy role: dz of 4 pixels, y of 4 pixels; x role: XB x 4 pixels
    int ld_chunk = 0;
    auto load_chunk = [&]() {
        const int c = ld_chunk++;
        const int rot = rot_of(c);
        const int pbase = (chunk0 + c) * 32 + pg * 4;
        if (rot < NAW) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = pbase + i < g.M;
                const unsigned pin = (unsigned)(pg * 4 + i);
                r[i] = y4_buf_load4(dz_rs, ok ? pin * dz_pix + (unsigned)cga * 16u : OOB, (unsigned)c * 32u * dz_pix);
                r[4 + i] = y4_buf_load4(y_rs, ok ? pin * y_pix + (unsigned)cga * 16u : OOB, (unsigned)c * 32u * y_pix);
            }
        } else if (rot < NAW + NXW) {
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                const int cg = ((rot - NAW) * XB + u) * 8 + (lane >> 3);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = pbase + i < g.M;
                    r[u * 4 + i] = y4_buf_load4(x_rs, ok ? (unsigned)(pg * 4 + i) * x_pix + (unsigned)cg * 16u : OOB, (unsigned)c * 32u * x_pix);
                }
            }
        }
    };
    // split 4 pixels x 4 channels and write the 4 channel rows (2 planes each) transposed
    auto split_store = [&](const f32x4 (&v)[4], const float s, unsigned char* base, int rows, int off) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x4 col = {v[0][e], v[1][e], v[2][e], v[3][e]};      // channel e of the 4 pixels
            u32x2 hi, lo;
            split2x4(col, s, hi, lo);
            *reinterpret_cast<u32x2*>(base + off + e * ROWB) = hi;
            *reinterpret_cast<u32x2*>(base + rows * ROWB + off + e * ROWB) = lo;
        }
    };
    auto store_chunk = [&](int c) {
        unsigned char* st = smem_b + (c & 1) * STAGE;
        const int rot = rot_of(c);
        if (rot < NAW) {
            f32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (r[4 + i][e] - mu[e]) * is[e];
                    const float gg = r[i][e] * y4_act_grad_t<ACT>(ga[e] * xh + be[e]);
                    o[i][e] = gi[e] * (gg - k1[e] - xh * k2[e]);
                }
            const int pbase = (chunk0 + c) * 32 + pg * 4;
            if (pbase + 3 >= g.M) {                        // rows past M: dy = 0 (its x row is zero too, but 0 * Inf is not)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (pbase + i >= g.M) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            split_store(o, ps, st, CO, piece(cga));
        } else if (rot < NAW + NXW) {
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                const int cg = ((rot - NAW) * XB + u) * 8 + (lane >> 3);
                const f32x4 v[4] = {r[u * 4], r[u * 4 + 1], r[u * 4 + 2], r[u * 4 + 3]};
                split_store(v, s_x, st + B_OFF, CI, piece(cg));
            }
        }
    };

    // ---- dW: wave (wi, wj, wk): rows 32 wi .. of dy^T, columns (CI / 2) wj .. of x, k steps of 16 pixels [wk WI, wk WI + WI)
    const int wj = wave & 1, wi = (wave >> 1) % WI, wk = (wave >> 1) / WI;
    const int fr = lane & 31, fq = lane >> 5;
    const int fsw = (fr >> 2) & 3;
    f32x16 wacc0[MJ], wacc1[MJ];
#pragma unroll
    for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
        for (int e = 0; e < 16; ++e) { wacc0[jj][e] = 0.f; wacc1[jj][e] = 0.f; }
    const int a_row = (wi * 32 + fr) * ROWB, b_row = B_OFF + (wj * (CI / 2) + fr) * ROWB;
    auto wgrad = [&](const unsigned char* base) {
#pragma unroll
        for (int kk = 0; kk < WI; ++kk) {
            const int ks = wk * WI + kk;
            const int co = ((2 * ks + fq) ^ fsw) << 4;
            f16x8 fa[2], fb[MJ][2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) fa[pl] = *reinterpret_cast<const f16x8*>(base + pl * CO * ROWB + a_row + co);
#pragma unroll
            for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fb[jj][pl] = *reinterpret_cast<const f16x8*>(base + pl * CI * ROWB + b_row + jj * 32 * ROWB + co);
#pragma unroll
            for (int jj = 0; jj < MJ; ++jj) {
                wacc1[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1], fb[jj][0], wacc1[jj], 0, 0, 0);
                wacc1[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0], fb[jj][1], wacc1[jj], 0, 0, 0);
                wacc0[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0], fb[jj][0], wacc0[jj], 0, 0, 0);
            }
        }
    };

    // ---- dgrad: wave (pt, ch): pixels 16 pt .. of the chunk, channels (CI / 2) ch .. of dx in NCT tiles of 16.
    // B operand (k = 8 consecutive dy channels, column = pixel) through the transpose read: lane 4 q + p of a 16-lane group
    // addresses row (k base + q), pixels 4 p .. 4 p + 3 of the tile, and receives rows k base .. + 3 of pixel (lane & 15);
    // every lane of the wave takes part (no branch around this code).
    const int pt = wave & 1, chh = wave >> 1;
    const int fr16 = lane & 15, fq4 = lane >> 4;
    int tr_off[KS][2];                                      // per k step and half (rows + 0 .. 3 / + 4 .. 7) inside a plane
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = ks * 32 + fq4 * 8 + h * 4 + (fr16 >> 2);
            const int pgd = pt * 4 + (fr16 & 3);
            tr_off[ks][h] = n * ROWB + (((pgd >> 1) ^ ((n >> 2) & 3)) << 4) + ((pgd & 1) << 3);
        }
    int wa_off[NCT][KS];                                    // filter fragment: row = dx channel, 8 dy channels at k base
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c = (chh * NCT + t) * 16 + fr16;
            wa_off[t][ks] = W_OFF + c * RW + (((ks * 4 + fq4) ^ wswz(c)) << 4);
        }
    const float un_g = un_dy * f16x2_unscale(g.wt_amax), un_g1 = un_g * (1.0f / 2048.0f);
    const unsigned dx_pix = (unsigned)g.lddx * 4u, r_pix = (unsigned)(RES ? g.ldr : g.lddx) * 4u;
    const unsigned col_b = (unsigned)(chh * NCT * 16 + fq4 * 4) * 4u;       // byte column of the lane's 4 channels in tile 0
    f32x4 rr[RES ? NCT : 1];
    auto res_load = [&](int c) {
        if constexpr (RES) {
            const unsigned off = (unsigned)(c * 32 + pt * 16 + fr16) * r_pix + col_b;
#pragma unroll
            for (int t = 0; t < NCT; ++t) rr[t] = y4_buf_load4(r_rs, off + (unsigned)t * 64u, 0u);
        }
    };
    auto dgrad = [&](const unsigned char* base, int c) {
        typedef __attribute__((address_space(3))) trh4* lp;
        f16x8 fb[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const trh4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp)(base + pl * CO * ROWB + tr_off[ks][0]));
                const trh4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp)(base + pl * CO * ROWB + tr_off[ks][1]));
#pragma unroll
                for (int e = 0; e < 4; ++e) { fb[ks][pl][e] = (_Float16)a[e]; fb[ks][pl][4 + e] = (_Float16)b[e]; }
            }
        const unsigned off = (unsigned)(c * 32 + pt * 16 + fr16) * dx_pix + col_b;
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const f16x8 wh = *reinterpret_cast<const f16x8*>(smem_b + wa_off[t][ks]);
                const f16x8 wl = *reinterpret_cast<const f16x8*>(smem_b + wa_off[t][ks] + CI * RW);
                d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, fb[ks][0], d1, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fb[ks][1], d1, 0, 0, 0);
                d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fb[ks][0], d0, 0, 0, 0);
            }
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = d0[e] * un_g + d1[e] * un_g1;
            if constexpr (RES) v += rr[t];
            // (the whole offset in the vector register, no scalar offset on stores: see st_off in pointwise.hip)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), dx_rs, (int)(off + (unsigned)t * 64u), 0, 0);
        }
    };

    load_chunk();
    store_chunk(0);
    if (nchunks > 1) load_chunk();
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) store_chunk(ch + 1);
        if (ch + 2 < nchunks) load_chunk();
        res_load(ch);
        const unsigned char* base = smem_b + (ch & 1) * STAGE;
        wgrad(base);
        dgrad(base, ch);
        __syncthreads();
    }

    const float un_w = un_dy * f16x2_unscale(g.x_amax), un_w1 = un_w * (1.0f / 2048.0f);
    float* out = g.slabs + (long long)(split * KSP + wk) * CO * CI;
#pragma unroll
    for (int jj = 0; jj < MJ; ++jj) {
        const int jcol = wj * (CI / 2) + jj * 32 + fr;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * fq;
            out[n * CI + jcol] = wacc0[jj][e] * un_w + wacc1[jj][e] * un_w1;
        }
    }
}

int plan_splits(long long M, int* cps) {
    const long long nc = (M + 31) / 32;
    long long per = (nc + 511) / 512;                      // two resident blocks on each of 256 CUs
    if (per < 1) per = 1;
    *cps = (int)per;
    return (int)((nc + per - 1) / per);                    // every block gets a chunk
}

template <int CO, int CI, int ACT, bool RES>
int launch_fused(const FusedGeom& g, int splits, hipStream_t st) {
    const size_t smem = 2ull * 2 * (CO + CI) * ROWB + 2ull * CI * CO * 2;
    auto kern = conv1x1_bn_act_bwd_fused_f16x2<CO, CI, ACT, RES>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    y4::note_kernel("conv1x1_bn_act_bwd_fused_f16x2<%d, %d, %d, %s>", CO, CI, ACT, RES ? "true" : "false");
    hipLaunchKernelGGL(kern, dim3(splits), dim3(256), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
template <int CO, int CI>
int launch_fused_act(const FusedGeom& g, int act, int splits, hipStream_t st) {
#define Y4_FUSED(A_) (g.res ? launch_fused<CO, CI, A_, true>(g, splits, st) : launch_fused<CO, CI, A_, false>(g, splits, st))
    switch (act) {
        case Y4_ACT_MISH: return Y4_FUSED(Y4_ACT_MISH);
        case Y4_ACT_LEAKY: return Y4_FUSED(Y4_ACT_LEAKY);
        case Y4_ACT_RELU: return Y4_FUSED(Y4_ACT_RELU);
        default: return Y4_FUSED(Y4_ACT_LINEAR);
    }
#undef Y4_FUSED
}

bool shape_ok(long long M, int Cin, int Cout) {
    return M > 0 && M < (1ll << 31) - 64 && (Cout == 32 || Cout == 64) && (Cin == 64 || Cin == 128) && !(Cout == 32 && Cin == 128);
}
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

// [BatchNorm workspace][transposed filter planes (when the call splits the filter itself)][64 B: x maximum][dW slabs]
size_t y4_conv1x1_bn_act_bwd_fused_workspace(long long M, int Cin, int Cout) {
    if (!shape_ok(M, Cin, Cout)) return 0;
    int cps = 0;
    const int splits = plan_splits(M, &cps);
    return align256(y4_bn_workspace(M, Cout)) + align256(y4_conv2d_dgrad_workspace(Cin, Cout, 1)) + 256 +
           (size_t)splits * (Cout == 32 ? 2 : 1) * Cout * Cin * sizeof(float);
}

int y4_conv1x1_bn_act_bwd_fused_f32(const float* dz, int lddz, const float* y, int ldy,
                                    const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                                    float* dgamma, float* dbeta, long long M, int Cin, int Cout,
                                    const float* x, int ldx, const unsigned* x_amax,
                                    const float* w, const void* w_prepared,
                                    float* dx, int lddx, const float* res, int ldr, float* dw,
                                    void* workspace, size_t workspace_bytes, unsigned* bounds, int frozen_stats, void* stream) {
    if (!dz || !y || !mean || !invstd || !gamma || !beta || !dgamma || !dbeta || !x || !dx || !dw || !workspace || !bounds ||
        (!w && !w_prepared))
        return Y4_ERR_NULL;
    if (y4_get_conv_mode() != 3 || frozen_stats || !shape_ok(M, Cin, Cout) || act < 0 || act > 3) return Y4_ERR_SHAPE;
    auto vec_ok = [](const void* p, long long ld, int C) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0 && ld >= C; };
    if (!vec_ok(dz, lddz, Cout) || !vec_ok(y, ldy, Cout) || !vec_ok(x, ldx, Cin) || !vec_ok(dx, lddx, Cin) ||
        (res && !vec_ok(res, ldr, Cin)) || (reinterpret_cast<uintptr_t>(dw) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
        (w && (reinterpret_cast<uintptr_t>(w) & 15)) || (w_prepared && (reinterpret_cast<uintptr_t>(w_prepared) & 15)))
        return Y4_ERR_SHAPE;
    int cps = 0;
    const int splits = plan_splits(M, &cps);
    {
        // a block addresses its pixel range (+ one chunk) through 32-bit windows
        long long ldmax = lddz > ldy ? lddz : ldy;
        if (ldx > ldmax) ldmax = ldx;
        if (lddx > ldmax) ldmax = lddx;
        if (res && ldr > ldmax) ldmax = ldr;
        if (((unsigned long long)cps + 1ull) * 32ull * (unsigned long long)ldmax * 4ull >= 0xfffffff0ull) return Y4_ERR_SHAPE;
    }
    if (workspace_bytes < y4_conv1x1_bn_act_bwd_fused_workspace(M, Cin, Cout)) return Y4_ERR_WORKSPACE;
    hipStream_t st = y4_stream(stream);
    char* ws = static_cast<char*>(workspace);
    char* wsf = ws + align256(y4_bn_workspace(M, Cout));
    unsigned* hdr = reinterpret_cast<unsigned*>(wsf + align256(y4_conv2d_dgrad_workspace(Cin, Cout, 1)));
    float* slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(hdr) + 256);

    int rc = y4::bn_bwd_reduce_finalize_bounds(dz, lddz, y, ldy, mean, invstd, gamma, beta, act, M, Cout, ws, dgamma, dbeta, bounds, st);
    if (rc != Y4_OK) return rc;
    // the transposed split filter: laid out as y4_conv2d_dgrad_f32's workspace (planes, then the maximum word)
    const size_t wtotal = (size_t)Cin * Cout;
    const char* prep = static_cast<const char*>(w_prepared);
    if (!prep) {
        unsigned* fh = reinterpret_cast<unsigned*>(wsf + wtotal * 6);
        rc = y4::f16x2_filter_planes_transposed(w, reinterpret_cast<unsigned short*>(wsf), Cout, Cin, 1, Cout, fh, fh + 16, st, false);
        if (rc != Y4_OK) return rc;
        prep = wsf;
    }
    if (!x_amax) {
        rc = y4::amax_launch(x, ldx, M, Cin, hdr, st);
        if (rc != Y4_OK) return rc;
        x_amax = hdr;
    }
    FusedGeom g{};
    g.dz = dz; g.y = y; g.x = x; g.res = res; g.dx = dx; g.slabs = slabs;
    g.mean = mean; g.invstd = invstd; g.gamma = gamma; g.beta = beta;
    g.acc = reinterpret_cast<const double*>(ws);
    g.bounds = bounds;
    g.wt_planes = reinterpret_cast<const unsigned char*>(prep);
    g.wt_amax = reinterpret_cast<const unsigned*>(prep + wtotal * 6);
    g.x_amax = x_amax;
    g.lddz = lddz; g.ldy = ldy; g.ldx = ldx; g.lddx = lddx; g.ldr = ldr;
    g.M = (int)M; g.chunks_per_split = cps;
    g.invM = 1.0 / (double)M;
    if (Cout == 64 && Cin == 64) rc = launch_fused_act<64, 64>(g, act, splits, st);
    else if (Cout == 64) rc = launch_fused_act<64, 128>(g, act, splits, st);
    else rc = launch_fused_act<32, 64>(g, act, splits, st);
    if (rc != Y4_OK) return rc;
    return y4::slab_reduce(slabs, dw, (long long)Cout * Cin, splits * (Cout == 32 ? 2 : 1), st);
}

}  // extern "C"
