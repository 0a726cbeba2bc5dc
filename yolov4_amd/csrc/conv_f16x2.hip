// Implicit-GEMM convolution on the fp16 matrix cores with a two-piece operand split ("f16x2"), gfx950 only.
//
// Arithmetic.  The reference computes in fp32.  Every fp32 operand x of a tensor T is first scaled by a
// power of two s_T (exact) chosen from max|T| so that max|s_T x| lies in [2^14, 2^15), then split into two fp16 pieces
//     hi = RN16(s x),    lo = RN16((s x - hi) * 2^11)          (s x - hi is exact in fp32)
// so that s x = hi + 2^-11 lo + e with |e| <= 2^-22 |s x| (11 + 11 significant bits, round to nearest both times).
// A product is three fp16 MFMAs with exact products and fp32 accumulation,
//     acc0 += a_hi b_hi          acc1 += a_hi b_lo + a_lo b_hi          c = (acc0 + 2^-11 acc1) / (s_A s_B),
// dropping a_lo b_lo 2^-22: relative error per product ~2^-22 (random sign), i.e. 2.4e-7 of the rms of the sum for any
// K -- below the rounding of an fp32 fma chain of the same length (1.2e-6 at K = 4608) and of the accumulation inside
// the MFMA itself.  The second accumulator keeps the low pieces at full fp16 precision down to |x| = 2^-29 max|T|
// (hi normal), below which precision degrades gradually to an absolute floor of 2^-50 max|T|.  Half the MFMAs of the
// 3-piece bf16 split (3 instead of 6), 2 staged planes instead of 3, 3.5 VALU per staged element instead of 5.5.
//
// Structure (forward / dgrad "gather" kernel and wgrad): 128x128 (or 64x128, 128x64, 128x32) tile, 4 waves, wave tile
// of 32x32x16 or 16x16x32 MFMA tiles, LDS rows of 32 k-values = 64 B unpadded with an XOR swizzle of the 16-B chunks
// chosen per MFMA shape so that every ds_read_b128 lane group is conflict-free, TWO LDS stages and one barrier per
// K-tile: [barrier] split + write tile t+1 into the other stage, issue the global loads of tile t+2, MFMAs of tile t.
#include <stdlib.h>
#include "common.h"
#include <cstdlib>
#include "conv_geom.h"
#include "f16x2.h"

namespace {

using y4::ConvGeom;
using y4::WgradGeom;

using namespace y4x2;                                    // scale, split and LDS row image: f16x2.h

// ==================================================================================== forward / dgrad
// TRANSPOSED = false: source pixel = (hd*stride - pad + r, wd*stride - pad + q)      [forward]
// TRANSPOSED = true : source pixel = ((hd + pad - r)/stride, (wd + pad - q)/stride)   [dgrad]
// LDS map of conv_gather_f16x2: [two staging buffers | re-used by the vector epilogue: 4 wave patches of
// [WTM][WTN + 4] floats][row_m: BM ints]
template <int BM, int BN, int WM, int WN, int MS>
__host__ __device__ constexpr int gather_rowm_off() {       // byte offset of row_m[]: behind the stages AND the patches
    constexpr int patches = (MS == 16 && (BN / WN == 64 || BN / WN == 32)) ? 4 * (BM / WM) * (BN / WN + 4) * 4 : 0;
    constexpr int stages = 2 * 2 * (BM + BN) * ROWB;
    return patches > stages ? patches : stages;
}

template <int BM, int BN, int WM, int WN, bool TRANSPOSED, int MS>
__global__ __launch_bounds__(256, 2) void conv_gather_f16x2(const ConvGeom g) {
    constexpr int BK = 32;
    constexpr int PA = BM / 32;                            // fp32 row chunks of the A tile per thread
    constexpr int NB = (BN * 8 + 255) / 256;               // 16-B chunks of the B tile per thread (both planes)
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / MS, TN = WTN / MS;
    constexpr int ACCN = MS == 32 ? 16 : 4;
    constexpr int STAGE = 2 * (BM + BN) * ROWB;            // bytes per LDS stage (2 planes of A and B)
    static_assert(WM * WN == 4, "4 waves");
    typedef float accv __attribute__((ext_vector_type(ACCN)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    int* row_m = reinterpret_cast<int*>(smem_b + gather_rowm_off<BM, BN, WM, WN, MS>());

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    int r0 = 0, q0 = 0, tstep = 1;
    int ph = 0, pw = 0, mt_local, nt;
    const bool classed = TRANSPOSED && g.stride == 2;
    if (!classed) {
        const int lt = y4_xcd_remap(blockIdx.x, g.mtiles * g.ntiles);
        mt_local = lt / g.ntiles;
        nt = lt - mt_local * g.ntiles;
    } else {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        int c = 0;
        while (c < 3 && slot >= g.cls_slot0[c + 1]) ++c;
        const int per = g.cls_slot0[c + 1] - g.cls_slot0[c];
        const int t = xcd * per + (slot - g.cls_slot0[c]);
        const int tiles_c = (g.cls_tile0[c + 1] - g.cls_tile0[c]) * g.ntiles;
        if (t >= tiles_c) return;                          // padding slot (whole block, before any barrier)
        mt_local = t / g.ntiles;
        nt = t - mt_local * g.ntiles;
        ph = (3 - c) >> 1; pw = (3 - c) & 1;
        r0 = (ph + g.pad) & 1; q0 = (pw + g.pad) & 1; tstep = 2;
    }
    const int n0 = nt * BN;
    const int nr = (g.k - r0 + tstep - 1) / tstep, nq = (g.k - q0 + tstep - 1) / tstep;
    const int lrow = tid >> 3, kc = tid & 7;

    const int pix_per_img = classed ? g.cls_h[ph] * g.cls_w[pw] : g.Hd * g.Wd;
    const int b_first = (int)(((long long)mt_local * BM) / pix_per_img);
    const unsigned long long img_bytes = (unsigned long long)g.Hs * g.Ws * (unsigned long long)g.lds_ * 4ull;
    const unsigned long long src_skip = (unsigned long long)b_first * img_bytes;
    const unsigned long long src_left = g.src_total_bytes > src_skip ? g.src_total_bytes - src_skip : 0ull;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.src) + src_skip, (unsigned)(src_left < 0xfffffff0ull ? src_left : 0xfffffff0ull));
    const __amdgpu_buffer_rsrc_t wt_rsrc = y4_make_rsrc(g.wt_planes, g.wt_bytes);     // 2 planes of N*K fp16
    const unsigned OOB = 0xffffffffu;
    const float sa = f16x2_scale(g.src_amax);
    unsigned a_base[PA];
    int a_h[PA], a_w[PA];
    bool a_ok[PA];
    int a_lds[PA];
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int row = p * 32 + lrow;
        const int i = mt_local * BM + row;
        int b, hd, wd;
        if (!classed) {
            a_ok[p] = i < g.M && row < BM;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (g.Hd * g.Wd);
            const int rem = ii - b * (g.Hd * g.Wd);
            hd = rem / g.Wd; wd = rem - hd * g.Wd;
        } else {
            const int hc = g.cls_h[ph], wc = g.cls_w[pw];
            a_ok[p] = i < g.B * hc * wc && row < BM;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (hc * wc);
            const int rem = ii - b * (hc * wc);
            const int hh = rem / wc;
            hd = 2 * hh + ph; wd = 2 * (rem - hh * wc) + pw;
        }
        const int ach = kc;                                // 16-B chunk inside the K-tile row
        if (ach == 0 && row < BM) row_m[row] = a_ok[p] ? (b * g.Hd + hd) * g.Wd + wd : -1;
        a_base[p] = (unsigned)(b - b_first) * (unsigned)(g.Hs * g.Ws) * pix_bytes + ach * 16u;
        if (!TRANSPOSED) { a_h[p] = hd * g.stride - g.pad; a_w[p] = wd * g.stride - g.pad; }
        else { a_h[p] = hd + g.pad; a_w[p] = wd + g.pad; }
        a_lds[p] = row * ROWB + (((kc >> 1) ^ lds_swz<MS>(row)) << 4) + ((kc & 1) << 3);
    }
    unsigned b_off[NB];
    int b_lds[NB];
    // filter planes are interleaved per 32-deep K-tile: row n = [tile 0: 64 B hi | 64 B lo][tile 1: ...] -- the 8 lanes
    // of a row read one whole 128-B line (half lines per instruction cost the texture addresser twice the cycles)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int slot = tid + 256 * i;
        const int row = slot >> 3, ch = slot & 3, bpl = (slot >> 2) & 1;
        const bool ok = row < BN && (n0 + row) < g.N;
        b_off[i] = ok ? (unsigned)(n0 + row) * (unsigned)g.K * 4u + (unsigned)(slot & 7) * 16u : OOB;
        b_lds[i] = row < BN ? bpl * BN * ROWB + row * ROWB + ((ch ^ lds_swz<MS>(row)) << 4) : -1;
    }

    f32x4 ra[PA];
    u32x4 rb[NB];
    const int CC = g.Cs / BK;
    int r = r0, q = q0, cc = 0;
    unsigned a_off[PA];
    auto tap_setup = [&]() {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            int hi, wi;
            bool ok = a_ok[p];
            if (!TRANSPOSED) {
                hi = a_h[p] + r; wi = a_w[p] + q;
                ok = ok && (unsigned)hi < (unsigned)g.Hs && (unsigned)wi < (unsigned)g.Ws;
            } else {
                const int th = a_h[p] - r, tw = a_w[p] - q;
                hi = th; wi = tw;
                if (g.stride == 2) { hi = th >> 1; wi = tw >> 1; }
                ok = ok && th >= 0 && tw >= 0 && hi < g.Hs && wi < g.Ws;
            }
            a_off[p] = ok ? a_base[p] + (unsigned)(hi * g.Ws + wi) * pix_bytes : OOB;
        }
    };
    tap_setup();
    auto load_tile = [&]() {
#pragma unroll
        for (int p = 0; p < PA; ++p) ra[p] = y4_buf_load4(src_rsrc, a_off[p], (unsigned)(cc * BK) * 4u);
        const unsigned koff = (unsigned)((r * g.k + q) * CC + cc) * (BK * 4u);
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = __builtin_amdgcn_raw_buffer_load_b128(wt_rsrc, (int)b_off[i], (int)koff, 0);
        if (++cc == CC) { cc = 0; q += tstep; if (q >= g.k) { q = q0; r += tstep; } tap_setup(); }
    };
    int st_cc = 0;
    auto store_tile = [&](int buf) {
        unsigned char* as = smem_b + buf * STAGE;
        unsigned char* bs = as + 2 * BM * ROWB;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = ra[p];
            if (TRANSPOSED && g.Cs_valid != g.Cs) {        // pad channels of dy (255 -> 256) may hold anything
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (st_cc * BK + kc * 4 + e >= g.Cs_valid) v[e] = 0.f;
            }
            u32x2 hi, lo;
            split2x4(v, sa, hi, lo);
            *reinterpret_cast<u32x2*>(as + a_lds[p]) = hi;
            *reinterpret_cast<u32x2*>(as + BM * ROWB + a_lds[p]) = lo;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (b_lds[i] >= 0) {
                *reinterpret_cast<u32x4*>(bs + b_lds[i]) = rb[i];
            }
        if (++st_cc == CC) st_cc = 0;
    };

    accv acc0[TM][TN], acc1[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < ACCN; ++e) { acc0[i][j][e] = 0.f; acc1[i][j][e] = 0.f; }

    // fragment addressing: lane -> (row inside an MS-row tile, 16-B chunk of the 32-deep K-tile)
    const int fr = lane & (MS - 1);                        // row of the MFMA tile
    const int fq = lane / MS;                              // 32x32x16: k half (0/1); 16x16x32: k quarter (0..3)
    const int fsw = lds_swz<MS>(fr);
    const int a_row = (wm * WTM + fr) * ROWB, b_row = 2 * BM * ROWB + (wn * WTN + fr) * ROWB;

    auto compute = [&](int buf) {
        const unsigned char* base = smem_b + buf * STAGE;
        if constexpr (MS == 32) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int co = ((2 * ks + fq) ^ fsw) << 4;
                f16x8 fa[TM][2], fb[TN][2];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        fa[i][pl] = *reinterpret_cast<const f16x8*>(base + pl * BM * ROWB + a_row + i * 32 * ROWB + co);
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        fb[j][pl] = *reinterpret_cast<const f16x8*>(base + pl * BN * ROWB + b_row + j * 32 * ROWB + co);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][1], fb[j][0], acc1[i][j], 0, 0, 0);
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][0], fb[j][1], acc1[i][j], 0, 0, 0);
                        acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][0], fb[j][0], acc0[i][j], 0, 0, 0);
                    }
            }
        } else {
            const int co = (fq ^ fsw) << 4;
            f16x8 fb[TN][2];
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fb[j][pl] = *reinterpret_cast<const f16x8*>(base + pl * BN * ROWB + b_row + j * 16 * ROWB + co);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                f16x8 fa[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fa[pl] = *reinterpret_cast<const f16x8*>(base + pl * BM * ROWB + a_row + i * 16 * ROWB + co);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[1], fb[j][0], acc1[i][j], 0, 0, 0);
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0], fb[j][1], acc1[i][j], 0, 0, 0);
                    acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0], fb[j][0], acc0[i][j], 0, 0, 0);
                }
            }
        }
    };

    const int KT = nr * nq * CC;
    load_tile();
    store_tile(0);
    if (KT > 1) load_tile();
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        if (kt + 1 < KT) store_tile((kt + 1) & 1);         // split + write the prefetched tile into the other stage
        if (kt + 2 < KT) load_tile();                      // its successor's loads fly under this tile's MFMAs
        compute(kt & 1);
        __syncthreads();
    }

    // ---- epilogue: c = (acc0 + 2^-11 acc1) / (s_A s_B); element (row, col) of a tile:
    //   32x32: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5);   16x16: col = lane & 15, row = 4 (lane >> 4) + e
    const float un = f16x2_unscale(g.src_amax) * f16x2_unscale(g.wt_amax);
    const float un1 = un * (1.0f / 2048.0f);
    unsigned out_max = 0u;
    // Vector form (16x16 shape, whole float4 columns, no BatchNorm-backward fold): in the MFMA layout a lane owns single
    // floats of 4 rows, i.e. 64 scalar stores per lane, each wave instruction touching 4 rows x 64 B.  Instead every wave
    // passes its WTM x WTN sub-tile through its own LDS patch ([row][WTN + 4] floats, no barrier: nobody else reads it) and
    // writes float4 rows: 16 stores per lane, each instruction 4 rows x 256 contiguous bytes; the skip operand is read the
    // same way.
    bool vec = false;
    if constexpr (MS == 16 && (WTN == 64 || WTN == 32)) {
        vec = (g.N & 3) == 0 && (g.ldd & 3) == 0 && (reinterpret_cast<uintptr_t>(g.dst) & 15) == 0 &&
              (!g.res || ((g.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(g.res) & 15) == 0)) &&
              (!g.scale || (reinterpret_cast<uintptr_t>(g.scale) & 15) == 0) && (!g.shift || (reinterpret_cast<uintptr_t>(g.shift) & 15) == 0);
    }
    // both accumulators are combined once, ahead of the branch: acc1 is dead in either epilogue form (with it alive
    // across the branch the 128x128 forward instance spilled 12 registers)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < ACCN; ++e) acc0[i][j][e] = acc0[i][j][e] * un + acc1[i][j][e] * un1;   // also the BN statistics' input
    if (vec) {
        constexpr int EP = WTN + 4;                        // patch row pitch in floats (272 B: 16-B aligned rows)
        float* patch = reinterpret_cast<float*>(smem_b) + wave * (WTM * EP);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < ACCN; ++e) patch[(i * MS + 4 * fq + e) * EP + j * MS + fr] = acc0[i][j][e];
        // (wave-local: the LDS writes above are ordered before the reads below by the wave's own lgkmcnt wait)
        constexpr int LPR = WTN / 4, RPI = 64 / LPR;       // lanes per patch row, rows per wave instruction
        const int c4 = (lane % LPR) * 4;
        const int nv = n0 + wn * WTN + c4;
        const bool nok4 = nv < g.N;                         // N % 4 == 0: the four columns are valid together
        f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
        if (g.scale && nok4) sc4 = *reinterpret_cast<const f32x4*>(g.scale + nv);
        if (g.shift && nok4) sh4 = *reinterpret_cast<const f32x4*>(g.shift + nv);
#pragma unroll
        for (int it = 0; it < WTM / RPI; it += 4) {
            int mrow[4];
            f32x4 rr4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = (it + u) * RPI + lane / LPR;
                mrow[u] = row_m[wm * WTM + row];
                rr4[u] = (g.res && nok4 && mrow[u] >= 0) ? *reinterpret_cast<const f32x4*>(g.res + (long long)mrow[u] * g.ldr + nv)
                                                        : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = (it + u) * RPI + lane / LPR;
                f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * EP + c4);
                if (nok4 && mrow[u] >= 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float t = v[q] * sc4[q] + sh4[q];
                        t = y4_act(t, g.act);
                        t += rr4[u][q];
                        v[q] = t;
                        const unsigned vb = __float_as_uint(t) & 0x7fffffffu;
                        if (vb < 0x7f800000u && vb > out_max) out_max = vb;
                    }
                    *reinterpret_cast<f32x4*>(g.dst + (long long)mrow[u] * g.ldd + nv) = v;
                }
            }
        }
    } else
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * MS + fr;
        const bool nok = n < g.N;
        const float sc = (g.scale && nok) ? g.scale[n] : 1.0f;
        const float sh = (g.shift && nok) ? g.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // the skip / fan-in operand of this tile column is fetched as one batch BEFORE the stores (the compiler may
            // not move a load across a store that might alias it: one exposed round trip per element otherwise)
            int mm[ACCN];
            float rr[ACCN];
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const int rl = MS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * fq : 4 * fq + e;
                mm[e] = row_m[wm * WTM + i * MS + rl];
                rr[e] = (g.res && nok && mm[e] >= 0) ? g.res[(long long)mm[e] * g.ldr + n] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const float raw = acc0[i][j][e];
                const int m = mm[e];
                if (nok && m >= 0) {
                    float v = raw * sc + sh;
                    v = y4_act(v, g.act);
                    v += rr[e];
                    g.dst[(long long)m * g.ldd + n] = v;
                    const unsigned vb = __float_as_uint(v) & 0x7fffffffu;
                    if (vb < 0x7f800000u && vb > out_max) out_max = vb;
                }
            }
        }
    }
    if (!TRANSPOSED && g.dst_amax) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)out_max, off, 64);
            out_max = o > out_max ? o : out_max;
        }
        if (lane == 0 && out_max > __hip_atomic_load(g.dst_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g.dst_amax, out_max);
    }
    float* const colsums = TRANSPOSED ? nullptr : g.stats;       // forward only: BatchNorm statistics
    if (colsums) {
        __syncthreads();                                   // `red` lies inside wave 0's epilogue patch
        float* red = reinterpret_cast<float*>(smem_b);     // [WM][BN][2]
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < ACCN; ++e) {
                    const float v = acc0[i][j][e];
                    cs += v;
                    css += v * v;
                }
            if constexpr (MS == 16) {
                cs += __shfl_xor(cs, 16, 64);
                css += __shfl_xor(css, 16, 64);
            }
            cs += __shfl_xor(cs, 32, 64);
            css += __shfl_xor(css, 32, 64);
            if (fq == 0) {
                const int c = wn * WTN + j * MS + fr;
                red[(wm * BN + c) * 2 + 0] = cs;
                red[(wm * BN + c) * 2 + 1] = css;
            }
        }
        __syncthreads();
        for (int c = tid; c < BN; c += 256) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) { cs += red[(w * BN + c) * 2]; css += red[(w * BN + c) * 2 + 1]; }
            const int n = n0 + c;
            if (n < g.N) {
                colsums[((long long)mt_local * 2 + 0) * g.N + n] = cs;
                colsums[((long long)mt_local * 2 + 1) * g.N + n] = css;
            }
        }
    }
}

// ==================================================================================== wgrad
// D[n][j] = sum_p dy[p][n] * xg[p][j]; both operands transposed into LDS as [n or j][32 pixels] rows while being
// split: each thread owns one 4-pixel x 4-channel block of each operand per 32-pixel chunk (4 coalesced 16-B loads,
// a 4x4 register transpose folded into the fp16 packing, 8 ds_write_b64).
// (Measured and dropped: an 8-wave "ping-pong" form -- one block per CU, two 4-wave groups taking alternate chunks, one
// staging while the other runs its MFMAs -- was 1.5x SLOWER (64.8 vs 42.4 ms per step over all wgrad launches): the
// kernel is bound by the VALU work of the operand split, and a ping-pong lets only half the waves do VALU at a time.)
template <int TN_, int TJ_, int MS>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f16x2(const WgradGeom g) {
    constexpr int WTN = TN_ / 2, WTJ = TJ_ / 2;
    constexpr int MI = WTN / MS, MJ = WTJ / MS;
    constexpr int ACCN = MS == 32 ? 16 : 4;
    constexpr int NBLK_A = 8 * (TN_ / 4), NBLK_B = 8 * (TJ_ / 4);     // 4x4 blocks per chunk (<= 256)
    constexpr int STAGE = 2 * (TN_ + TJ_) * ROWB;
    typedef float accv __attribute__((ext_vector_type(ACCN)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int tiles = g.ntn * g.ntj;
    int bid = y4_xcd_remap(blockIdx.x, tiles * g.splits);
    const int split = bid / tiles;
    bid -= split * tiles;
    const int tn = bid / g.ntj, tj = bid - tn * g.ntj;
    const int n0 = tn * TN_, j0 = tj * TJ_;

    const int pg = tid & 7, cg = tid >> 3;               // pixel group (4 px), channel group (4 ch)
    const bool a_act = tid < NBLK_A, b_act = tid < NBLK_B;
    const int Cout4 = (g.Cout + 3) & ~3;
    const bool an_ok = a_act && (n0 + cg * 4) < Cout4;
    const int j = j0 + cg * 4;
    const bool bj_ok = b_act && j < g.J;
    int jr = 0, jq = 0, jc = 0;
    if (bj_ok) { const int tap = j / g.Cin; jc = j - tap * g.Cin; jr = tap / g.k; jq = tap - jr * g.k; }

    const int chunk0 = split * g.chunks_per_split;
    int nchunks = (g.M + 31) / 32 - chunk0;
    if (nchunks > g.chunks_per_split) nchunks = g.chunks_per_split;

    const long long p_first = (long long)chunk0 * 32;
    const int b_first = (int)(p_first / ((long long)g.Ho * g.Wo));
    const unsigned long long x_skip = (unsigned long long)b_first * g.H * g.W * (unsigned long long)g.ldx * 4ull;
    const unsigned long long dy_skip = (unsigned long long)p_first * (unsigned long long)g.lddy * 4ull;
    const unsigned long long x_left = g.x_total_bytes > x_skip ? g.x_total_bytes - x_skip : 0ull;
    const unsigned long long dy_left = g.dy_total_bytes > dy_skip ? g.dy_total_bytes - dy_skip : 0ull;
    const __amdgpu_buffer_rsrc_t x_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.x) + x_skip, (unsigned)(x_left < 0xfffffff0ull ? x_left : 0xfffffff0ull));
    const __amdgpu_buffer_rsrc_t dy_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.dy) + dy_skip, (unsigned)(dy_left < 0xfffffff0ull ? dy_left : 0xfffffff0ull));
    const unsigned OOB = 0xffffffffu;
    const float s_dy = f16x2_scale(g.dy_amax), s_x = f16x2_scale(g.x_amax);
    // raster position (image - b_first, row, column) of this thread's FIRST pixel of the chunk; its three neighbours are
    // derived from it (one running state per thread instead of four)
    int pb_b, pb_h, pb_w;
    {
        const int pix = chunk0 * 32 + pg * 4;
        const int pp = pix < g.M ? pix : (int)p_first;
        const int bb = pp / (g.Ho * g.Wo);
        pb_b = bb - b_first;
        const int rem = pp - bb * (g.Ho * g.Wo);
        pb_h = rem / g.Wo;
        pb_w = rem - pb_h * g.Wo;
    }
    const unsigned a_off0 = an_ok ? (unsigned)(pg * 4) * (unsigned)g.lddy * 4u + (unsigned)(n0 + cg * 4) * 4u : OOB;
    const unsigned dy_pix_bytes = (unsigned)g.lddy * 4u;
    const unsigned chunk_bytes = 32u * dy_pix_bytes;
    const unsigned x_pix_bytes = (unsigned)g.ldx * 4u;
    // LDS byte offset of this thread's 8-B piece (4 pixels) inside row (cg*4 + e)
    int w_lds[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = cg * 4 + e;
        w_lds[e] = row * ROWB + (((pg >> 1) ^ lds_swz<MS>(row)) << 4) + ((pg & 1) << 3);
    }

    f32x4 ra[4], rb[4];
    int ld_chunk = 0;
    auto load_chunk = [&]() {
        const int pbase = (chunk0 + ld_chunk) * 32 + pg * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = an_ok && pbase + i < g.M;
            ra[i] = y4_buf_load4(dy_rsrc, ok ? a_off0 + (unsigned)i * dy_pix_bytes : OOB, (unsigned)ld_chunk * chunk_bytes);
        }
        {
            int qb = pb_b, qh = pb_h, qw = pb_w;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hi = qh * g.stride - g.pad + jr, wi = qw * g.stride - g.pad + jq;
                const bool ok = bj_ok && pbase + i < g.M && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
                const unsigned off = (unsigned)((qb * g.H + hi) * g.W + wi) * x_pix_bytes + (unsigned)jc * 4u;
                rb[i] = y4_buf_load4(x_rsrc, ok ? off : OOB, 0u);
                if (++qw == g.Wo) { qw = 0; if (++qh == g.Ho) { qh = 0; ++qb; } }
            }
            pb_w += 32;
            while (pb_w >= g.Wo) { pb_w -= g.Wo; if (++pb_h == g.Ho) { pb_h = 0; ++pb_b; } }
        }
        ++ld_chunk;
    };
    // split 4 pixels x 4 channels and write the 4 channel rows (2 planes each) transposed
    auto split_store = [&](const f32x4 (&v)[4], const float s, unsigned char* base, int rows) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x4 col = {v[0][e], v[1][e], v[2][e], v[3][e]};      // channel e of the 4 pixels
            u32x2 hi, lo;
            split2x4(col, s, hi, lo);
            *reinterpret_cast<u32x2*>(base + w_lds[e]) = hi;
            *reinterpret_cast<u32x2*>(base + rows * ROWB + w_lds[e]) = lo;
        }
    };
    auto store_chunk = [&](int buf) {
        unsigned char* as = smem_b + buf * STAGE;
        if (a_act) split_store(ra, s_dy, as, TN_);
        if (b_act) split_store(rb, s_x, as + 2 * TN_ * ROWB, TJ_);
    };

    accv acc0[MI][MJ], acc1[MI][MJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
            for (int e = 0; e < ACCN; ++e) { acc0[i][jj][e] = 0.f; acc1[i][jj][e] = 0.f; }

    const int fr = lane & (MS - 1), fq = lane / MS;
    const int fsw = lds_swz<MS>(fr);
    const int a_row = (wm * WTN + fr) * ROWB, b_row = 2 * TN_ * ROWB + (wn * WTJ + fr) * ROWB;
    auto compute = [&](int buf) {
        const unsigned char* base = smem_b + buf * STAGE;
        if constexpr (MS == 32) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int co = ((2 * ks + fq) ^ fsw) << 4;
                f16x8 fa[MI][2], fb[MJ][2];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        fa[i][pl] = *reinterpret_cast<const f16x8*>(base + pl * TN_ * ROWB + a_row + i * 32 * ROWB + co);
#pragma unroll
                for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        fb[jj][pl] = *reinterpret_cast<const f16x8*>(base + pl * TJ_ * ROWB + b_row + jj * 32 * ROWB + co);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int jj = 0; jj < MJ; ++jj) {
                        acc1[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][1], fb[jj][0], acc1[i][jj], 0, 0, 0);
                        acc1[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][0], fb[jj][1], acc1[i][jj], 0, 0, 0);
                        acc0[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][0], fb[jj][0], acc0[i][jj], 0, 0, 0);
                    }
            }
        } else {
            const int co = (fq ^ fsw) << 4;
            f16x8 fb[MJ][2];
#pragma unroll
            for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fb[jj][pl] = *reinterpret_cast<const f16x8*>(base + pl * TJ_ * ROWB + b_row + jj * 16 * ROWB + co);
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                f16x8 fa[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fa[pl] = *reinterpret_cast<const f16x8*>(base + pl * TN_ * ROWB + a_row + i * 16 * ROWB + co);
#pragma unroll
                for (int jj = 0; jj < MJ; ++jj) {
                    acc1[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[1], fb[jj][0], acc1[i][jj], 0, 0, 0);
                    acc1[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0], fb[jj][1], acc1[i][jj], 0, 0, 0);
                    acc0[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0], fb[jj][0], acc0[i][jj], 0, 0, 0);
                }
            }
        }
    };

    if (nchunks > 0) {
        load_chunk();
        store_chunk(0);
        if (nchunks > 1) load_chunk();
        __syncthreads();
        for (int ch = 0; ch < nchunks; ++ch) {
            if (ch + 1 < nchunks) store_chunk((ch + 1) & 1);
            if (ch + 2 < nchunks) load_chunk();
            compute(ch & 1);
            __syncthreads();
        }
    }
    const float un = f16x2_unscale(g.dy_amax) * f16x2_unscale(g.x_amax);
    const float un1 = un * (1.0f / 2048.0f);
    float* out = g.out + (long long)split * g.Cout * g.J;
#pragma unroll
    for (int jj = 0; jj < MJ; ++jj) {
        const int jcol = j0 + wn * WTJ + jj * MS + fr;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int nb = n0 + wm * WTN + i * MS;
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const int n = nb + (MS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * fq : 4 * fq + e);
                if (n < g.Cout && jcol < g.J) out[(long long)n * g.J + jcol] = acc0[i][jj][e] * un + acc1[i][jj][e] * un1;
            }
        }
    }
}

// ==================================================================================== 3x3 stride-1 "halo" kernel
// The gather kernel fetches and splits every input pixel once per filter tap (9x) and per N-tile.  For 3x3 / stride 1 /
// pad 1 layers on maps up to 76 px wide this kernel stages, per 32-channel chunk, the PATCH of input pixels that the 128
// output pixels of its M-tile touch -- once -- and runs the nine taps out of it:
//   * M-tiles never cross an image: 128 consecutive output pixels (h, w) of one image (the last tile of an image is
//     partial).  In the zero-padded image (H+2) x (W+2), output pixel (h, w) and tap (r, q) read padded position
//     (h + r, w + q) [dgrad: (h + 2 - r, w + 2 - q)], i.e. flat padded index base(h, w) + r Wp + q: the tap offset is
//     the same for every row of the tile, and the halo zeros are part of the patch (written at staging time by the
//     buffer loads' out-of-range zero fill) -- no masks in the MFMA loop.
//   * patch = padded flat positions [base(first pixel), base(last pixel) + 2 Wp + 2]: <= 290 rows of 32 channels for
//     W <= 76 (2 fp16 planes x 64 B: 37 KB), single stage, restaged every 9 taps; filter tiles double buffered per
//     tap with register prefetch as in the gather kernel.  71 KB of LDS: two blocks per CU.
//   * per 9 taps a thread issues <= 10 activation loads and splits <= 40 values instead of 36 loads / 144 values.
constexpr int HALO_ROWS = 304;                             // patch capacity (rows of 32 channels)

template <int BN, bool TRANSPOSED, int MS>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_f16x2(const ConvGeom g, const int tiles_per_img) {
    constexpr int BM = 128, WM = 2, WN = 2;
    constexpr int NB = (BN * 8 + 255) / 256;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / MS, TN = WTN / MS;
    constexpr int ACCN = MS == 32 ? 16 : 4;
    constexpr int PP = (HALO_ROWS + 31) / 32;              // patch rows per thread
    constexpr int PATCH = 2 * HALO_ROWS * ROWB;            // bytes: 2 planes
    constexpr int BSTAGE = 2 * BN * ROWB;                  // bytes per filter stage: 2 planes
    typedef float accv __attribute__((ext_vector_type(ACCN)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    unsigned char* const bsm = smem_b + PATCH;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lt = y4_xcd_remap(blockIdx.x, g.mtiles * g.ntiles);
    const int mt = lt / g.ntiles, nt = lt - mt * g.ntiles;
    const int b = mt / tiles_per_img, t = mt - b * tiles_per_img;
    const int n0 = nt * BN;
    const int H = g.Hs, W = g.Ws, Wp = W + 2, HW = H * W;
    const int i0 = t * BM;                                 // first output pixel of the tile inside image b
    const int cnt = (HW - i0) < BM ? (HW - i0) : BM;       // valid rows of this tile
    const int h0 = i0 / W, w0 = i0 - h0 * W;
    const int p_lo = h0 * Wp + w0;                         // padded flat position of (first pixel, tap (0, 0))
    const int il_last = i0 + cnt - 1;
    const int h1 = il_last / W, w1 = il_last - h1 * W;
    const int prow_n = (h1 + 2) * Wp + (w1 + 2) - p_lo + 1;   // patch rows in use (<= HALO_ROWS, checked on the host)

    const unsigned long long img_bytes = (unsigned long long)HW * (unsigned long long)g.lds_ * 4ull;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.src) + (unsigned long long)b * img_bytes, (unsigned)img_bytes);
    const __amdgpu_buffer_rsrc_t wt_rsrc = y4_make_rsrc(g.wt_planes, g.wt_bytes);
    const unsigned OOB = 0xffffffffu;
    const float sa = f16x2_scale(g.src_amax);
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
    const int lrow = tid >> 3, kc = tid & 7;

    // ---- patch rows of this thread: source offset (or OOB for halo / unused rows) and LDS position, fixed for the kernel
    unsigned a_off[PP];
    int a_lds[PP];
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        const int j = p * 32 + lrow;
        const int ach = kc;
        const int pf = p_lo + j;
        const int hp = pf / Wp, wp = pf - hp * Wp;
        const bool ok = j < prow_n && hp >= 1 && hp <= H && wp >= 1 && wp <= W;
        a_off[p] = ok ? (unsigned)((hp - 1) * W + (wp - 1)) * pix_bytes + ach * 16u : OOB;
        a_lds[p] = j < HALO_ROWS ? j * ROWB + (((kc >> 1) ^ lds_swz<MS>(j)) << 4) + ((kc & 1) << 3) : -1;
    }
    // ---- filter chunks of this thread
    unsigned b_off[NB];
    int b_lds[NB];
    // filter planes are interleaved per 32-deep K-tile: row n = [tile 0: 64 B hi | 64 B lo][tile 1: ...] -- the 8 lanes
    // of a row read one whole 128-B line (half lines per instruction cost the texture addresser twice the cycles)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int slot = tid + 256 * i;
        const int row = slot >> 3, ch = slot & 3, bpl = (slot >> 2) & 1;
        const bool ok = row < BN && (n0 + row) < g.N;
        b_off[i] = ok ? (unsigned)(n0 + row) * (unsigned)g.K * 4u + (unsigned)(slot & 7) * 16u : OOB;
        b_lds[i] = row < BN ? bpl * BN * ROWB + row * ROWB + ((ch ^ lds_swz<MS>(row)) << 4) : -1;
    }
    const int CC = g.Cs / 32;
    const int S = 9 * CC;                                  // steps: s = cc * 9 + tap
    u32x4 rb[NB];
    int ld_s = 0;
    auto load_b = [&]() {
        const int cc = ld_s / 9, tap = ld_s - cc * 9;
        const unsigned koff = (unsigned)(tap * CC + cc) * 128u;
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = __builtin_amdgcn_raw_buffer_load_b128(wt_rsrc, (int)b_off[i], (int)koff, 0);
        ++ld_s;
    };
    auto store_b = [&](int buf) {
        unsigned char* bs = bsm + buf * BSTAGE;
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (b_lds[i] >= 0) {
                *reinterpret_cast<u32x4*>(bs + b_lds[i]) = rb[i];
            }
    };
    auto stage_patch = [&](int cc) {
        f32x4 ra[PP];
#pragma unroll
        for (int p = 0; p < PP; ++p) ra[p] = y4_buf_load4(src_rsrc, a_off[p], (unsigned)cc * 128u);
#pragma unroll
        for (int p = 0; p < PP; ++p) {
            if (a_lds[p] < 0) continue;
            f32x4 v = ra[p];
            if (TRANSPOSED && g.Cs_valid != g.Cs) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (cc * 32 + kc * 4 + e >= g.Cs_valid) v[e] = 0.f;
            }
            u32x2 hi, lo;
            split2x4(v, sa, hi, lo);
            *reinterpret_cast<u32x2*>(smem_b + a_lds[p]) = hi;
            *reinterpret_cast<u32x2*>(smem_b + HALO_ROWS * ROWB + a_lds[p]) = lo;
        }
    };

    accv acc0[TM][TN], acc1[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < ACCN; ++e) { acc0[i][j][e] = 0.f; acc1[i][j][e] = 0.f; }

    const int fr = lane & (MS - 1), fq = lane / MS;
    const int fswb = lds_swz<MS>(fr);
    const int b_row = (wn * WTN + fr) * ROWB;
    // patch row (relative to p_lo) of tap (0, 0) for the output pixel of each of this lane's A fragment rows
    int a_rel[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int il = wm * WTM + i * MS + fr;
        if (il >= cnt) il = cnt - 1;                       // rows past the image end: computed, never stored
        const int pix = i0 + il;
        const int h = pix / W, w = pix - h * W;
        a_rel[i] = h * Wp + w - p_lo;
    }

    auto compute = [&](int buf, int tap) {
        const unsigned char* bs = bsm + buf * BSTAGE;
        const int r = tap / 3, q = tap - r * 3;
        const int toff = TRANSPOSED ? (2 - r) * Wp + (2 - q) : r * Wp + q;
        constexpr int KSN = MS == 32 ? 2 : 1;
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
            const int cb = MS == 32 ? 2 * ks + fq : fq;    // logical 16-B chunk of the 32-deep K-tile
            const int cob = (cb ^ fswb) << 4;
            f16x8 fb[TN][2];
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    fb[j][pl] = *reinterpret_cast<const f16x8*>(bs + pl * BN * ROWB + b_row + j * MS * ROWB + cob);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = a_rel[i] + toff;
                const int ao = row * ROWB + ((cb ^ lds_swz<MS>(row)) << 4);
                const f16x8 fa0 = *reinterpret_cast<const f16x8*>(smem_b + ao);
                const f16x8 fa1 = *reinterpret_cast<const f16x8*>(smem_b + HALO_ROWS * ROWB + ao);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if constexpr (MS == 32) {
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb[j][0], acc1[i][j], 0, 0, 0);
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb[j][1], acc1[i][j], 0, 0, 0);
                        acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb[j][0], acc0[i][j], 0, 0, 0);
                    } else {
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1, fb[j][0], acc1[i][j], 0, 0, 0);
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb[j][1], acc1[i][j], 0, 0, 0);
                        acc0[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb[j][0], acc0[i][j], 0, 0, 0);
                    }
                }
            }
        }
    };

    load_b();
    store_b(0);
    if (S > 1) load_b();
    for (int s = 0; s < S; ++s) {
        const int cc = s / 9, tap = s - cc * 9;
        if (tap == 0) {
            stage_patch(cc);                               // every wave left the previous patch at the last barrier
            __syncthreads();
        }
        if (s + 1 < S) store_b((s + 1) & 1);
        if (s + 2 < S) load_b();
        compute(s & 1, tap);
        __syncthreads();
    }

    // ---- epilogue (as the gather kernel; output pixel m = b HW + i0 + row, rows >= cnt are not part of the image)
    const float un = f16x2_unscale(g.src_amax) * f16x2_unscale(g.wt_amax);
    const float un1 = un * (1.0f / 2048.0f);
    const long long mbase = (long long)b * HW + i0;
    unsigned out_max = 0u;
    // vector form of the epilogue: see conv_gather_f16x2 (the staging buffers, 70 KB, hold the four wave patches)
    bool vec = false;
    if constexpr (MS == 16 && WTN == 64) {
        vec = (g.N & 3) == 0 && (g.ldd & 3) == 0 && (reinterpret_cast<uintptr_t>(g.dst) & 15) == 0 &&
              (!g.res || ((g.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(g.res) & 15) == 0)) &&
              (!g.scale || (reinterpret_cast<uintptr_t>(g.scale) & 15) == 0) && (!g.shift || (reinterpret_cast<uintptr_t>(g.shift) & 15) == 0);
    }
    // combined once ahead of the branch (see the gather kernel); rows past the image end become exact zeros (BN statistics)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const int rl = wm * WTM + i * MS + (MS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * fq : 4 * fq + e);
                acc0[i][j][e] = rl < cnt ? acc0[i][j][e] * un + acc1[i][j][e] * un1 : 0.f;
            }
    if (vec) {
        constexpr int EP = WTN + 4;
        static_assert(4 * WTM * EP * 4 <= 2 * HALO_ROWS * ROWB + 2 * 2 * BN * ROWB, "wave patches must fit the staging buffers");
        float* patch = reinterpret_cast<float*>(smem_b) + wave * (WTM * EP);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < ACCN; ++e) patch[(i * MS + 4 * fq + e) * EP + j * MS + fr] = acc0[i][j][e];
        const int c4 = (lane & 15) * 4;
        const int nv = n0 + wn * WTN + c4;
        const bool nok4 = nv < g.N;
        f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
        if (g.scale && nok4) sc4 = *reinterpret_cast<const f32x4*>(g.scale + nv);
        if (g.shift && nok4) sh4 = *reinterpret_cast<const f32x4*>(g.shift + nv);
#pragma unroll
        for (int it = 0; it < WTM / 4; it += 4) {
            f32x4 rr4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rl = wm * WTM + (it + u) * 4 + (lane >> 4);
                rr4[u] = (g.res && nok4 && rl < cnt) ? *reinterpret_cast<const f32x4*>(g.res + (mbase + rl) * g.ldr + nv)
                                                    : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = (it + u) * 4 + (lane >> 4);
                const int rl = wm * WTM + row;
                f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * EP + c4);
                if (nok4 && rl < cnt) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float t = v[q] * sc4[q] + sh4[q];
                        t = y4_act(t, g.act);
                        t += rr4[u][q];
                        v[q] = t;
                        const unsigned vb = __float_as_uint(t) & 0x7fffffffu;
                        if (vb < 0x7f800000u && vb > out_max) out_max = vb;
                    }
                    *reinterpret_cast<f32x4*>(g.dst + (mbase + rl) * g.ldd + nv) = v;
                }
            }
        }
    } else
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * MS + fr;
        const bool nok = n < g.N;
        const float sc = (g.scale && nok) ? g.scale[n] : 1.0f;
        const float sh = (g.shift && nok) ? g.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float rr[ACCN];
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const int rl = wm * WTM + i * MS + (MS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * fq : 4 * fq + e);
                rr[e] = (g.res && nok && rl < cnt) ? g.res[(mbase + rl) * g.ldr + n] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < ACCN; ++e) {
                const int rl = wm * WTM + i * MS + (MS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * fq : 4 * fq + e);
                const bool rok = rl < cnt;
                const float raw = acc0[i][j][e];
                if (nok && rok) {
                    float v = raw * sc + sh;
                    v = y4_act(v, g.act);
                    v += rr[e];
                    g.dst[(mbase + rl) * g.ldd + n] = v;
                    const unsigned vb = __float_as_uint(v) & 0x7fffffffu;
                    if (vb < 0x7f800000u && vb > out_max) out_max = vb;
                }
            }
        }
    }
    if (!TRANSPOSED && g.dst_amax) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)out_max, off, 64);
            out_max = o > out_max ? o : out_max;
        }
        if (lane == 0 && out_max > __hip_atomic_load(g.dst_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g.dst_amax, out_max);
    }
    float* const colsums = TRANSPOSED ? nullptr : g.stats;       // forward only: BatchNorm statistics
    if (colsums) {
        __syncthreads();                                   // `red` lies inside wave 0's epilogue patch
        float* red = reinterpret_cast<float*>(smem_b);     // [WM][BN][2]
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < ACCN; ++e) {
                    const float v = acc0[i][j][e];
                    cs += v;
                    css += v * v;
                }
            if constexpr (MS == 16) {
                cs += __shfl_xor(cs, 16, 64);
                css += __shfl_xor(css, 16, 64);
            }
            cs += __shfl_xor(cs, 32, 64);
            css += __shfl_xor(css, 32, 64);
            if (fq == 0) {
                const int c = wn * WTN + j * MS + fr;
                red[(wm * BN + c) * 2 + 0] = cs;
                red[(wm * BN + c) * 2 + 1] = css;
            }
        }
        __syncthreads();
        for (int c = tid; c < BN; c += 256) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) { cs += red[(w * BN + c) * 2]; css += red[(w * BN + c) * 2 + 1]; }
            const int n = n0 + c;
            if (n < g.N) {
                colsums[((long long)mt * 2 + 0) * g.N + n] = cs;
                colsums[((long long)mt * 2 + 1) * g.N + n] = css;
            }
        }
    }
}

// rows of the patch of the worst tile of an H x W image (tiles start at multiples of 128 pixels)
int halo_patch_rows(int H, int W) {
    const int HW = H * W, Wp = W + 2;
    int worst = 0;
    for (int i0 = 0; i0 < HW; i0 += 128) {
        const int i1 = (i0 + 127 < HW ? i0 + 127 : HW - 1);
        const int h0 = i0 / W, w0 = i0 % W, h1 = i1 / W, w1 = i1 % W;
        const int n = (h1 + 2) * Wp + (w1 + 2) - (h0 * Wp + w0) + 1;
        if (n > worst) worst = n;
    }
    return worst;
}

bool halo_ok(const ConvGeom& g) {
    static const bool off = getenv("Y4_NO_HALO") != nullptr;
    if (off || g.k != 3 || g.stride != 1 || g.pad != 1 || !g.wt_planes) return false;
    if (g.N <= 64 || g.Cs % 32 != 0 || g.Hd != g.Hs || g.Wd != g.Ws) return false;
    if ((unsigned long long)g.Hs * g.Ws * (unsigned long long)g.lds_ * 4ull >= 0xfffffff0ull) return false;
    return halo_patch_rows(g.Hs, g.Ws) <= HALO_ROWS;
}

template <bool TR, int MS>
int launch_halo_f16x2(const ConvGeom& g0, hipStream_t st, int* nparts) {
    constexpr int BN = 128;
    ConvGeom g = g0;
    const int tiles_per_img = (g.Hs * g.Ws + 127) / 128;
    g.mtiles = g.B * tiles_per_img;
    g.ntiles = (g.N + BN - 1) / BN;
    if ((unsigned long long)g.N * g.K * 4ull >= 0xfffffff0ull) return Y4_ERR_SHAPE;
    g.wt_bytes = (unsigned)((unsigned long long)g.N * g.K * 2ull * 2ull);
    if (nparts) *nparts = g.mtiles;
    const size_t smem = 2ull * HALO_ROWS * ROWB + 2ull * 2 * BN * ROWB;
    auto kern = conv3x3_halo_f16x2<BN, TR, MS>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    y4::note_kernel("conv3x3_halo_f16x2<%d, %s, %d>", BN, TR ? "true" : "false", MS);
    hipLaunchKernelGGL(kern, dim3(g.mtiles * g.ntiles), dim3(256), smem, st, g, tiles_per_img);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

// ==================================================================================== streaming 1x1 (small K, small N)
// The 1x1 layers on the 304^2 / 152^2 / 76^2 maps with K, N <= 128 are HBM-bound; the whole filter (2 fp16 planes)
// stays in LDS for the life of a persistent block and every wave streams its own 32 pixel rows from global memory
// straight into the MFMA A-operand layout (lane = pixel, 8 consecutive channels = 32 contiguous bytes), splits them
// in registers and never meets a barrier; the next tile's loads fly under this tile's MFMAs / stores.
// RESB: the launch has a skip operand: its loads are batched ahead of the stores.
// PLAIN: no scale / shift / activation / BatchNorm statistics (a dgrad launch): 16 fewer live registers, which the
//        K = N = 128 form with a skip operand needs to stay out of scratch.
template <int KS, int NT, int NW = 4, bool RESB = false, bool PLAIN = false>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void conv1x1_stream_f16x2(const ConvGeom g) {
    constexpr int NTHR = NW * 64, TROWS = NW * 32;
    constexpr int K = KS * 16;
    constexpr int PITCH = K * 2 + 16;                    // LDS row pitch: conflict-free ds_read_b128 for K = 32/64/128
    constexpr int N32 = NT * 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    {
        constexpr int CPR = K / 8;                       // 16-B chunks per filter row
        const unsigned char* wp = reinterpret_cast<const unsigned char*>(g.wt_planes);
        for (int i = tid; i < 2 * N32 * CPR; i += NTHR) {
            const int pl = i / (N32 * CPR);
            const int rem = i - pl * (N32 * CPR);
            const int row = rem / CPR, ch = rem - row * CPR;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < g.N) v = *reinterpret_cast<const u32x4*>(wp + (size_t)row * (K * 4) + (ch >> 2) * 128 + pl * 64 + (ch & 3) * 16);
            *reinterpret_cast<u32x4*>(smem_b + (pl * N32 + row) * PITCH + ch * 16) = v;
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t src_rsrc = y4_make_rsrc(g.src, (unsigned)g.src_total_bytes);   // < 4 GiB (host)
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
    const int mtiles = g.mtiles;
    const float sa = f16x2_scale(g.src_amax);
    const float un = f16x2_unscale(g.src_amax) * f16x2_unscale(g.wt_amax);
    const float un1 = un * (1.0f / 2048.0f);
    constexpr int KH = KS == 8 ? 4 : KS;
    f32x4 ra0[KH][2], ra1[KH][2];
    auto load = [&](f32x4 (&ra)[KH][2], int tile, int ks0) {
        const int m = tile * TROWS + wave * 32 + fr;
        const unsigned off = m < g.M ? (unsigned)m * pix_bytes + (unsigned)fh * 32u : 0xffffffffu;
#pragma unroll
        for (int ks = 0; ks < KH; ++ks) {
            // (nt loads here: 452.8 vs 457 img/s, measured -- the wgrad of the same layer re-reads x from the Infinity Cache)
            ra[ks][0] = y4_buf_load4(src_rsrc, off, (unsigned)(ks0 + ks) * 64u);
            ra[ks][1] = y4_buf_load4(src_rsrc, off, (unsigned)(ks0 + ks) * 64u + 16u);
        }
    };
    float cs[PLAIN ? 1 : NT], css[PLAIN ? 1 : NT];
    float sc[PLAIN ? 1 : NT], sh[PLAIN ? 1 : NT];
    if constexpr (!PLAIN) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            cs[j] = 0.f; css[j] = 0.f;
            const int n = j * 32 + fr;
            sc[j] = (g.scale && n < g.N) ? g.scale[n] : 1.0f;
            sh[j] = (g.shift && n < g.N) ? g.shift[n] : 0.0f;
        }
    }
    const unsigned char* b_frag = smem_b + fr * PITCH + fh * 16;
    f32x16 acc0[NT], acc1[NT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc0[j][e] = 0.f; acc1[j][e] = 0.f; }
    };
    auto mma = [&](f32x4 (&ra)[KH][2], int ks0) {
        if constexpr (KS == 8) asm volatile("" ::: "memory");      // re-read the filter fragments per tile (no spills)
#pragma unroll
        for (int ks = 0; ks < KH; ++ks) {
            f16x8 fah, fal;
            {
                u32x2 h0, l0, h1, l1;
                split2x4(ra[ks][0], sa, h0, l0);
                split2x4(ra[ks][1], sa, h1, l1);
                const u32x4 qh = {h0[0], h0[1], h1[0], h1[1]}, ql = {l0[0], l0[1], l1[0], l1[1]};
                fah = __builtin_bit_cast(f16x8, qh);
                fal = __builtin_bit_cast(f16x8, ql);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const f16x8 fbh = *reinterpret_cast<const f16x8*>(b_frag + (j * 32) * PITCH + (ks0 + ks) * 32);
                const f16x8 fbl = *reinterpret_cast<const f16x8*>(b_frag + (N32 + j * 32) * PITCH + (ks0 + ks) * 32);
                acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal, fbh, acc1[j], 0, 0, 0);
                acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, fbl, acc1[j], 0, 0, 0);
                acc0[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, fbh, acc0[j], 0, 0, 0);
            }
        }
    };
    unsigned out_max = 0u;
    // Branch-free epilogue: raw buffer stores / skip-operand loads on a window re-based at the tile's first row whose extent
    // ends at row M (rows past M fall out of range: the hardware drops them), the lane's row and column in the vector offset,
    // the accumulator register's row ((e & 3) + 8 (e >> 2)) times the pitch in the SCALAR offset, the column tile as the
    // immediate: no address arithmetic and no exec-mask branch per element (the per-element `if (valid)` form ran the
    // launches with a skip operand at 1.9-2.9 TB/s against 4.3-5.3 without one).
    const unsigned drow_bytes = (unsigned)g.ldd * 4u, rrow_bytes = (unsigned)g.ldr * 4u;
    // (launches without a skip operand keep the per-element form: they run at 4.1-5.3 TB/s with it, the N = 128 forms have no
    // registers left for the offset vectors, and the flat form measured 5 % slower on 64 -> 64 @304.  ONE lambda with two bodies: a second, unused closure would still take the
    // address of the accumulators and push them into scratch)
    auto epilogue = [&](int tile) {
        if constexpr (RESB) {
            const long long row0 = (long long)tile * TROWS;
            const unsigned long long rows_left = (unsigned long long)(g.M - row0);
            const unsigned long long dby = rows_left * drow_bytes, rby = rows_left * rrow_bytes;
            const __amdgpu_buffer_rsrc_t drs = y4_make_rsrc(reinterpret_cast<char*>(g.dst) + row0 * (long long)drow_bytes,
                                                            (unsigned)(dby < 0xfffffff0ull ? dby : 0xfffffff0ull));
            const bool has_res = RESB || g.res != nullptr;
            const __amdgpu_buffer_rsrc_t rrs = y4_make_rsrc(has_res ? reinterpret_cast<const char*>(g.res) + row0 * (long long)rrow_bytes : nullptr,
                                                            has_res ? (unsigned)(rby < 0xfffffff0ull ? rby : 0xfffffff0ull) : 0u);
            const int lrow = wave * 32 + 4 * fh;
            const bool rows_in = row0 + TROWS <= g.M;              // uniform: the whole tile lies inside the tensor
    #pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = j * 32 + fr;
                const bool nok = n < g.N;
                // rows 8 g + (e & 3) of the lane's 32-row tile, g = e >> 2: the 8 g part in four vector offsets, the (e & 3) part
                // in the scalar offset (three scalars instead of sixteen: the kernel is short of SGPRs too)
                unsigned dvo4[4], rvo4[4];
    #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    dvo4[q] = nok ? (unsigned)(lrow + 8 * q) * drow_bytes + (unsigned)n * 4u : 0xffffffffu;
                    rvo4[q] = nok ? (unsigned)(lrow + 8 * q) * rrow_bytes + (unsigned)n * 4u : 0xffffffffu;
                }
                // the skip operand arrives in batches ahead of the stores: all 16 cells of a column where the launch is known to
                // have one (RESB), 4 otherwise (registers: the K = 64 / N = 128 form has none to spare)
                constexpr int RB = RESB ? 16 : 4;
    #pragma unroll
                for (int eb = 0; eb < 16; eb += RB) {
                    float rr[RB];
                    if (has_res) {
    #pragma unroll
                        for (int ee = 0; ee < RB; ++ee) {
                            const int e = eb + ee;
                            rr[ee] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrs, (int)(rvo4[e >> 2]), (int)((e & 3) * rrow_bytes), 0));
                        }
                    }
    #pragma unroll
                    for (int ee = 0; ee < RB; ++ee) {
                        const int e = eb + ee;
                        const float raw = acc0[j][e] * un + acc1[j][e] * un1;
                        if constexpr (!PLAIN) { cs[j] += raw; css[j] += raw * raw; }      // rows past M are exact zeros
                        float v = raw;
                        if constexpr (!PLAIN) {
                            v = raw * sc[j] + sh[j];
                            v = y4_act(v, g.act);
                        }
                        if (has_res) v += rr[ee];
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), drs, (int)(dvo4[e >> 2]), (int)((e & 3) * drow_bytes), 0);
                        if (g.dst_amax) {
                            const bool ok = nok && (rows_in || row0 + lrow + (e & 3) + 8 * (e >> 2) < g.M);
                            const unsigned vb = __float_as_uint(v) & 0x7fffffffu;
                            if (ok && vb < 0x7f800000u && vb > out_max) out_max = vb;
                        }
                    }
                }
            }
        } else {
            const int mbase = tile * TROWS + wave * 32 + 4 * fh;
    #pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = j * 32 + fr;
                const bool nok = n < g.N;
                // RESB: the skip operand is fetched in batches ahead of the stores (16 cells of a column at NT <= 2, 8 at NT = 4,
                // where registers are short), as in the gather kernel: a load may not be moved across a store that might alias it
                constexpr int RB = RESB ? (NT <= 2 ? 16 : 8) : 16;
    #pragma unroll
                for (int eb = 0; eb < 16; eb += RB) {
                    float rr[RESB ? RB : 1];
                    if constexpr (RESB) {
    #pragma unroll
                        for (int e = 0; e < RB; ++e) {
                            const int m = mbase + ((eb + e) & 3) + 8 * ((eb + e) >> 2);
                            rr[e] = (g.res && nok && m < g.M) ? g.res[(long long)m * g.ldr + n] : 0.f;
                        }
                    }
    #pragma unroll
                    for (int ee = 0; ee < RB; ++ee) {
                        const int e = eb + ee;
                        const float raw = acc0[j][e] * un + acc1[j][e] * un1;
                        if constexpr (!PLAIN) { cs[j] += raw; css[j] += raw * raw; }      // rows past M are exact zeros
                        const int m = mbase + (e & 3) + 8 * (e >> 2);
                        if (nok && m < g.M) {
                            float v = raw;
                            if constexpr (!PLAIN) {
                                v = raw * sc[j] + sh[j];
                                v = y4_act(v, g.act);
                            }
                            if constexpr (RESB) v += rr[ee];
                            else if (g.res) v += g.res[(long long)m * g.ldr + n];
                            g.dst[(long long)m * g.ldd + n] = v;
                            const unsigned vb = __float_as_uint(v) & 0x7fffffffu;
                            if (vb < 0x7f800000u && vb > out_max) out_max = vb;
                        }
                    }
                }
            }
        }
    };
    int tile = blockIdx.x;
    if (tile < mtiles) load(ra0, tile, 0);
    if constexpr (KS == 8) {
        while (tile < mtiles) {
            load(ra1, tile, KH);
            zero_acc();
            mma(ra0, 0);
            const int tn = tile + gridDim.x;
            if (tn < mtiles) load(ra0, tn, 0);
            mma(ra1, KH);
            epilogue(tile);
            tile = tn;
        }
    } else {
        while (tile < mtiles) {
            const int t1 = tile + gridDim.x;
            if (t1 < mtiles) load(ra1, t1, 0);
            zero_acc(); mma(ra0, 0); epilogue(tile);
            if (t1 >= mtiles) break;
            const int t2 = t1 + gridDim.x;
            if (t2 < mtiles) load(ra0, t2, 0);
            zero_acc(); mma(ra1, 0); epilogue(t1);
            tile = t2;
        }
    }
    if (g.dst_amax) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)out_max, off, 64);
            out_max = o > out_max ? o : out_max;
        }
        if (lane == 0 && out_max > __hip_atomic_load(g.dst_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g.dst_amax, out_max);
    }
    if (!PLAIN && g.stats) {                              // one partial row per block: [gridDim][2][N]
        __syncthreads();                                  // every wave is done with the filter planes
        float* red = reinterpret_cast<float*>(smem_b);    // [NW][N32][2]
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float a = cs[j], b = css[j];
            a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 32, 64);
            if (fh == 0) { red[(wave * N32 + j * 32 + fr) * 2] = a; red[(wave * N32 + j * 32 + fr) * 2 + 1] = b; }
        }
        __syncthreads();
        for (int c = tid; c < N32; c += NTHR) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) { a += red[(w * N32 + c) * 2]; b += red[(w * N32 + c) * 2 + 1]; }
            if (c < g.N) {
                g.stats[((long long)blockIdx.x * 2 + 0) * g.N + c] = a;
                g.stats[((long long)blockIdx.x * 2 + 1) * g.N + c] = b;
            }
        }
    }
}

template <int KS, int NT, int NW, bool RESB, bool PLAIN = false>
int launch_stream1x1_f16x2_impl(const ConvGeom& g0, hipStream_t st, int* nparts);
template <int KS, int NT, int NW = 4>
int launch_stream1x1_f16x2(const ConvGeom& g0, hipStream_t st, int* nparts) {
    if constexpr (KS == 8 && NT == 4) {                    // K = N = 128 with a skip operand: in registers only as PLAIN
        if (g0.res && !g0.scale && !g0.shift && !g0.stats && g0.act == Y4_ACT_LINEAR)
            return launch_stream1x1_f16x2_impl<KS, NT, NW, true, true>(g0, st, nparts);
    } else if constexpr (NT <= 2) {                        // (the other NT = 4 forms spill 20-88 registers with the batch)
        if (g0.res) return launch_stream1x1_f16x2_impl<KS, NT, NW, true>(g0, st, nparts);
    }
    return launch_stream1x1_f16x2_impl<KS, NT, NW, false>(g0, st, nparts);
}
template <int KS, int NT, int NW, bool RESB, bool PLAIN>
int launch_stream1x1_f16x2_impl(const ConvGeom& g0, hipStream_t st, int* nparts) {
    ConvGeom g = g0;
    g.mtiles = (g.M + NW * 32 - 1) / (NW * 32);
    g.ntiles = 1;
    g.src_total_bytes = (unsigned long long)g.M * (unsigned long long)g.lds_ * 4ull;
    size_t smem = (size_t)2 * NT * 32 * (KS * 32 + 16);
    const size_t red = (size_t)NW * NT * 32 * 2 * sizeof(float);
    if (smem < red) smem = red;
    auto kern = conv1x1_stream_f16x2<KS, NT, NW, RESB, PLAIN>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    const int resident = NW == 8 ? 256 : 512;             // blocks per CU: 1 (8 waves) or 2
    const int grid = g.mtiles < resident ? g.mtiles : resident;
    if (nparts) *nparts = grid;
    y4::note_kernel("conv1x1_stream_f16x2<%d, %d, %d, %s, %s>", KS, NT, NW, RESB ? "true" : "false", PLAIN ? "true" : "false");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

// eligibility: 1x1 stride 1, K in {32,64,128}, N <= 128, 32-bit addressable source, every source channel valid, and
// enough rows to be worth a persistent launch
bool stream1x1_f16x2_ok(const ConvGeom& g) {
    if (g.k != 1 || g.stride != 1 || !g.wt_planes) return false;
    if (g.Cs != 32 && g.Cs != 64 && g.Cs != 128) return false;
    if (g.Cs_valid != g.Cs || g.N > 128) return false;
    if ((unsigned long long)g.M * (unsigned long long)g.lds_ * 4ull >= 0xfffffff0ull) return false;
    return g.M >= 128 * 1024;
}

int dispatch_stream1x1_f16x2(const ConvGeom& g, hipStream_t st, int* nparts) {
    const int nt = (g.N + 31) / 32;
    switch (g.Cs / 16 * 10 + nt) {
        case 21: return launch_stream1x1_f16x2<2, 1>(g, st, nparts);
        case 22: return launch_stream1x1_f16x2<2, 2>(g, st, nparts);
        case 23: case 24: return launch_stream1x1_f16x2<2, 4>(g, st, nparts);
        case 41: return launch_stream1x1_f16x2<4, 1>(g, st, nparts);
        case 42: return launch_stream1x1_f16x2<4, 2>(g, st, nparts);
        case 43: case 44: return launch_stream1x1_f16x2<4, 4>(g, st, nparts);
        case 81: return launch_stream1x1_f16x2<8, 1>(g, st, nparts);
        case 82: return launch_stream1x1_f16x2<8, 2>(g, st, nparts);
        case 83: case 84: return launch_stream1x1_f16x2<8, 4, 8>(g, st, nparts);
        default: return Y4_ERR_SHAPE;
    }
}

// ==================================================================================== filter planes, amax
// max |finite element| over the first C channels of an NHWC tensor with pitch: bit pattern, folded with atomicMax
// (order independent -> deterministic) into a word the caller has zeroed (or that already holds a lower bound)
// one atomic per BLOCK (waves folded through LDS), and only when it would raise the word
__device__ __forceinline__ void amax_block_commit(unsigned m, unsigned* out) {
    __shared__ unsigned wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
        const unsigned v = a > b ? a : b;
        if (v > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, v);
    }
}
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long ld, long long M, int C,
                                                   unsigned* __restrict__ out) {
    unsigned m = 0u;
    const int C4 = (C + 3) >> 2;
    const long long total = M * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C4;
        const int c = (int)(i - row * C4) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * ld + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned b = __float_as_uint(v[e]) & 0x7fffffffu;
            if (c + e < C && b < 0x7f800000u && b > m) m = b;
        }
    }
    amax_block_commit(m, out);
}
__global__ __launch_bounds__(256) void amax_strided_kernel(const float* __restrict__ x, long long ld, long long M, int C,
                                                           unsigned* __restrict__ out) {
    unsigned m = 0u;
    const long long total = M * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C;
        const unsigned b = __float_as_uint(x[row * ld + (i - row * C)]) & 0x7fffffffu;
        if (b < 0x7f800000u && b > m) m = b;
    }
    amax_block_commit(m, out);
}
__global__ void amax_merge_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { const unsigned v = *src; if (v) atomicMax(dst, v); }
}

// ---- filter maximum without atomics: stage 1 leaves one maximum per block, stage 2 lives in the split kernels' prologue
constexpr int AMAX_PART_MAX = 1024;
__global__ __launch_bounds__(256) void amax_partials_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ part) {
    __shared__ unsigned wmax[4];
    unsigned m = 0u;
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned b = __float_as_uint(v[e]) & 0x7fffffffu;
            if (b < 0x7f800000u && b > m) m = b;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
        const unsigned b = __float_as_uint(x[(n4 << 2) + threadIdx.x]) & 0x7fffffffu;
        if (b < 0x7f800000u && b > m) m = b;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
        part[blockIdx.x] = a > b ? a : b;
    }
}
// every block folds the <= 1024 block maxima (4 KiB out of L2); block 0 publishes the result for the conv kernel
__device__ __forceinline__ unsigned amax_fold_partials(const unsigned* __restrict__ part, int nparts, unsigned* __restrict__ out) {
    __shared__ unsigned wmax[4];
    unsigned m = 0u;
    for (int i = threadIdx.x; i < nparts; i += 256) { const unsigned v = part[i]; m = v > m ? v : m; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    const unsigned a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
    const unsigned v = a > b ? a : b;
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = v;
    return v;
}
__global__ __launch_bounds__(256) void f16x2_split_filter_folded_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes,
                                                                        long long n, const unsigned* __restrict__ part, int nparts,
                                                                        unsigned* __restrict__ amax_out) {
    const unsigned amax = amax_fold_partials(part, nparts, amax_out);
    const float s = __uint_as_float(f16x2_scale_exp(amax) << 23);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        unsigned short hi, lo;
        split2(w[i], s, hi, lo);
        const long long o = (i >> 5) * 64 + (i & 31);
        planes[o] = hi;
        planes[o + 32] = lo;
    }
}
// forward planes AND the transposed (dgrad) planes of one filter in one launch: a training forward prepares both, the
// backward pass of the same layer then starts without its own maximum + split launches (the filter cannot change between the
// two: autograd saved it).  Same element arithmetic as the two kernels below / above, one shared maximum.
__global__ __launch_bounds__(256) void f16x2_split_filter_dual_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes,
                                                                      unsigned short* __restrict__ planes_t, int Cout, int Cin, int kk,
                                                                      int Cout_pad, const unsigned* __restrict__ part, int nparts,
                                                                      unsigned* __restrict__ amax_out, unsigned* __restrict__ amax_out_t,
                                                                      int mirror) {
    const unsigned amax = amax_fold_partials(part, nparts, amax_out);
    if (blockIdx.x == 0 && threadIdx.x == 0) *amax_out_t = amax;
    const float s = __uint_as_float(f16x2_scale_exp(amax) << 23);
    const long long n = (long long)Cout * kk * Cin;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        unsigned short hi, lo;
        split2(w[i], s, hi, lo);
        const long long o = (i >> 5) * 64 + (i & 31);
        planes[o] = hi;
        planes[o + 32] = lo;
    }
    const long long total = (long long)Cin * kk * Cout_pad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int nn = (int)(i % Cout_pad);
        const long long t = i / Cout_pad;
        const int tp = (int)(t % kk);
        const int tap = mirror ? kk - 1 - tp : tp;
        const int c = (int)(t / kk);
        const float v = nn < Cout ? w[((long long)nn * kk + tap) * Cin + c] : 0.0f;
        unsigned short hi, lo;
        split2(v, s, hi, lo);
        const long long o = (i >> 5) * 64 + (i & 31);
        planes_t[o] = hi;
        planes_t[o + 32] = lo;
    }
}
__global__ __launch_bounds__(256) void f16x2_transpose_split_filter_folded_kernel(const float* __restrict__ w,
                                                                                  unsigned short* __restrict__ planes, int Cout, int Cin,
                                                                                  int kk, int Cout_pad, const unsigned* __restrict__ part,
                                                                                  int nparts, unsigned* __restrict__ amax_out, int mirror) {
    // mirror: tap t is written at position kk - 1 - t, which turns the stride-1 dgrad into a FORWARD-form gather
    // (source pixel h - pad + r' with r' = k - 1 - r): conv_planes.hip runs dgrad on its forward kernel
    const unsigned amax = amax_fold_partials(part, nparts, amax_out);
    const float s = __uint_as_float(f16x2_scale_exp(amax) << 23);
    const long long total = (long long)Cin * kk * Cout_pad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i % Cout_pad);
        const long long t = i / Cout_pad;
        const int tp = (int)(t % kk);
        const int tap = mirror ? kk - 1 - tp : tp;
        const int c = (int)(t / kk);
        const float v = n < Cout ? w[((long long)n * kk + tap) * Cin + c] : 0.0f;
        unsigned short hi, lo;
        split2(v, s, hi, lo);
        const long long o = (i >> 5) * 64 + (i & 31);
        planes[o] = hi;
        planes[o + 32] = lo;
    }
}

// ---- inference: a prepared filter buffer is refreshed only when the filter's BITS changed -- judged by a 64-bit positional
// HASH of the bit patterns (order independent to compute; two different filters collide with probability 2^-64, it is not a
// proof of equality) together with the exact maximum -- decided on the device: no host sync, no version counters to trust.  ONE launch per call:
// every block fingerprints its slice and takes a ticket; the last one folds the partials and compares with the header --
// unchanged (every call but the first after a weight update): done; changed: that block re-splits the whole filter (rare,
// so its serial cost -- at most 0.4 ms for the largest filter -- does not matter).
//   header words: [0] max|w| bits  [1] scratch of the conv call  [2..3] checksum  [4] valid  [5] ticket
// Hand-off (guide, Guideline 16): partials leave as agent-scope (write-through) stores, drained before the ticket; the
// last block reads them with agent-scope loads behind a workgroup barrier.
constexpr int FP_PARTS = 256;
__global__ __launch_bounds__(256) void f16x2_refresh_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes,
                                                                   long long n, unsigned* part_max, unsigned long long* part_sum,
                                                                   unsigned* hdr) {
    __shared__ unsigned wmax[4];
    __shared__ unsigned long long wsum[4];
    __shared__ int is_last;
    unsigned m = 0u;
    unsigned long long cs = 0ull;
    auto take = [&](const float x, const unsigned long long i) {
        const unsigned bits = __float_as_uint(x);
        cs += (unsigned long long)bits * (2ull * i + 1ull) + 0x9e3779b97f4a7c15ull;
        const unsigned b = bits & 0x7fffffffu;
        if (b < 0x7f800000u && b > m) m = b;
    };
    {
        // 16-B loads, four of them in flight per thread (a one-load-per-trip loop was latency-bound: 40 us per filter)
        const long long n4 = n >> 2, stride = (long long)gridDim.x * blockDim.x;
        long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
        for (; i + 3 * stride < n4; i += 4 * stride) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(w + 4 * (i + u * stride));
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) take(v[u][e], (unsigned long long)(4 * (i + u * stride) + e));
        }
        for (; i < n4; i += stride) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(w + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) take(v[e], (unsigned long long)(4 * i + e));
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) take(w[(n4 << 2) + threadIdx.x], (unsigned long long)((n4 << 2) + threadIdx.x));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
        cs += __shfl_xor(cs, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = m; wsum[threadIdx.x >> 6] = cs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
        __hip_atomic_store(part_max + blockIdx.x, a > b ? a : b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part_sum + blockIdx.x, wsum[0] + wsum[1] + wsum[2] + wsum[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(hdr + 5, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    // ---- last block: fold, compare, (rarely) re-split
    m = 0u; cs = 0ull;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
        const unsigned v = __hip_atomic_load(part_max + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        m = v > m ? v : m;
        cs += __hip_atomic_load(part_sum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
        cs += __shfl_xor(cs, off, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = m; wsum[threadIdx.x >> 6] = cs; }
    __syncthreads();
    const unsigned a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
    const unsigned amax = a > b ? a : b;
    const unsigned long long sum = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const unsigned long long stored = (unsigned long long)hdr[2] | ((unsigned long long)hdr[3] << 32);
    const bool same = hdr[4] == 1u && stored == sum && hdr[0] == amax;
    if (!same) {
        const float s = __uint_as_float(f16x2_scale_exp(amax) << 23);
        for (long long i = threadIdx.x; i < n; i += 256) {
            unsigned short hi, lo;
            split2(w[i], s, hi, lo);
            const long long o = (i >> 5) * 64 + (i & 31);
            planes[o] = hi;
            planes[o + 32] = lo;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!same) { hdr[0] = amax; hdr[2] = (unsigned)sum; hdr[3] = (unsigned)(sum >> 32); hdr[4] = 1u; }
        hdr[5] = 0u;                                       // ticket back to zero for the next call
    }
}

int g_f16x2_shape = 16;          // MFMA shape of the f16x2 kernels: 32 (32x32x16) or 16 (16x16x32); Y4_F16X2_SHAPE overrides

template <int BM, int BN, int WM, int WN, bool TR, int MS>
int launch_gather_f16x2(const ConvGeom& g0, hipStream_t st) {
    ConvGeom g = g0;
    if (TR && g.stride == 2) {
        int t = 0;
        for (int c = 0; c < 4; ++c) {
            const int ph = (3 - c) >> 1, pw = (3 - c) & 1;
            g.cls_h[ph] = (g.Hd + 1 - ph) / 2;
            g.cls_w[pw] = (g.Wd + 1 - pw) / 2;
            g.cls_tile0[c] = t;
            const long long n = (long long)g.B * g.cls_h[ph] * g.cls_w[pw];
            t += (int)((n + BM - 1) / BM);
        }
        g.cls_tile0[4] = t;
        g.mtiles = t;
    } else {
        g.cls_slot0[0] = 0;
        g.mtiles = (g.M + BM - 1) / BM;
    }
    g.ntiles = (g.N + BN - 1) / BN;
    {
        const unsigned long long img = (unsigned long long)g.Hs * g.Ws * (unsigned long long)g.lds_ * 4ull;
        const unsigned long long wb = (unsigned long long)g.N * g.K * 4ull;
        const unsigned long long imgs_per_tile = (unsigned long long)BM / (unsigned long long)((g.Hd * g.Wd + 3) / 4 > 0 ? (g.Hd * g.Wd + 3) / 4 : 1) + 2;
        if (img * imgs_per_tile >= 0xfffffff0ull || wb >= 0xfffffff0ull) return Y4_ERR_SHAPE;
        g.src_total_bytes = (unsigned long long)g.B * img;
        if (!g.wt_planes) return Y4_ERR_WORKSPACE;
        g.wt_bytes = (unsigned)((unsigned long long)g.N * g.K * 2ull * 2ull);
    }
    size_t smem = (size_t)gather_rowm_off<BM, BN, WM, WN, MS>() + BM * sizeof(int);
    auto kern = conv_gather_f16x2<BM, BN, WM, WN, TR, MS>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    int grid = g.mtiles * g.ntiles;
    if (TR && g.stride == 2) {
        int sl = 0;
        for (int c = 0; c < 4; ++c) {
            g.cls_slot0[c] = sl;
            sl += ((g.cls_tile0[c + 1] - g.cls_tile0[c]) * g.ntiles + 7) / 8;
        }
        g.cls_slot0[4] = sl;
        grid = sl * 8;
    }
    y4::note_kernel("conv_gather_f16x2<%d, %d, %d, %d, %s, %d>", BM, BN, WM, WN, TR ? "true" : "false", MS);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

template <bool TR, int MS>
int dispatch_gather_f16x2(const ConvGeom& g, hipStream_t st, int* nparts) {
    if (nparts) *nparts = (g.M + 127) / 128;
    if (g.N > 64) {
        const long long nt = (g.N + 127) / 128;
        const long long b128 = ((long long)g.M + 127) / 128 * nt, b64 = ((long long)g.M + 63) / 64 * nt;
        const double c128 = (double)((b128 + 511) / 512) * 128.0;
        const double c64 = (double)((b64 + 511) / 512) * 64.0 * 1.10;
        if (c64 < c128 && !(TR && g.stride == 2)) {
            if (nparts) *nparts = (g.M + 63) / 64;
            return launch_gather_f16x2<64, 128, 2, 2, TR, MS>(g, st);
        }
        return launch_gather_f16x2<128, 128, 2, 2, TR, MS>(g, st);
    }
    if (g.N > 32) return launch_gather_f16x2<128, 64, 2, 2, TR, MS>(g, st);
    return launch_gather_f16x2<128, 32, 4, 1, TR, MS>(g, st);
}

template <int TN_, int TJ_, int MS>
int launch_wgrad_f16x2(const WgradGeom& g, hipStream_t st) {
    const size_t smem = 2ull * 2 * (TN_ + TJ_) * ROWB;
    auto kern = conv_wgrad_f16x2<TN_, TJ_, MS>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    y4::note_kernel("conv_wgrad_f16x2<%d, %d, %d>", TN_, TJ_, MS);
    hipLaunchKernelGGL(kern, dim3(g.ntn * g.ntj * g.splits), dim3(256), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int f16x2_shape() {
    static int s = -1;
    if (s < 0) {
        const char* e = getenv("Y4_F16X2_SHAPE");
        s = e ? atoi(e) : g_f16x2_shape;
        if (s != 16 && s != 32) s = g_f16x2_shape;
    }
    return s;
}

}  // namespace

namespace y4 {

int f16x2_gather(const ConvGeom& g, bool transposed, hipStream_t st, int* nparts) {
    if (!transposed && !g.scale && !g.shift && !g.dst_amax && g.act == Y4_ACT_LINEAR && g.pad == 1 &&
        tile_conv_ok(g.Cs, g.Cs_valid, g.N, g.k, g.stride, g.Hs, g.Ws))
        return f16x2_tile(g, st, nparts);
    if (stream1x1_f16x2_ok(g)) return dispatch_stream1x1_f16x2(g, st, nparts);
    if (halo_ok(g)) {
        if (f16x2_shape() == 16) return transposed ? launch_halo_f16x2<true, 16>(g, st, nparts) : launch_halo_f16x2<false, 16>(g, st, nparts);
        return transposed ? launch_halo_f16x2<true, 32>(g, st, nparts) : launch_halo_f16x2<false, 32>(g, st, nparts);
    }
    if (f16x2_shape() == 16)
        return transposed ? dispatch_gather_f16x2<true, 16>(g, st, nparts) : dispatch_gather_f16x2<false, 16>(g, st, nparts);
    return transposed ? dispatch_gather_f16x2<true, 32>(g, st, nparts) : dispatch_gather_f16x2<false, 32>(g, st, nparts);
}

int f16x2_wgrad(const WgradGeom& g, hipStream_t st) {
    if (f16x2_shape() == 16) {
        if (g.tn == 128 && g.tj == 128) return launch_wgrad_f16x2<128, 128, 16>(g, st);
        if (g.tn == 128) return launch_wgrad_f16x2<128, 64, 16>(g, st);
        if (g.tj == 128) return launch_wgrad_f16x2<64, 128, 16>(g, st);
        return launch_wgrad_f16x2<64, 64, 16>(g, st);
    }
    if (g.tn == 128 && g.tj == 128) return launch_wgrad_f16x2<128, 128, 32>(g, st);
    if (g.tn == 128) return launch_wgrad_f16x2<128, 64, 32>(g, st);
    if (g.tj == 128) return launch_wgrad_f16x2<64, 128, 32>(g, st);
    return launch_wgrad_f16x2<64, 64, 32>(g, st);
}

static int filter_amax_partials(const float* w, long long n, unsigned* part, hipStream_t st) {
    if (reinterpret_cast<uintptr_t>(w) & 15) return -1;
    long long blocks = (n / 4 + 1023) / 1024;
    if (blocks < 1) blocks = 1;
    if (blocks > AMAX_PART_MAX) blocks = AMAX_PART_MAX;
    hipLaunchKernelGGL(amax_partials_kernel, dim3((unsigned)blocks), dim3(256), 0, st, w, n, part);
    return (int)blocks;
}

int f16x2_refresh_prepared(const float* w, void* prepared, int Cout, int K, hipStream_t st) {
    const long long n = (long long)Cout * K;
    unsigned* hdr = static_cast<unsigned*>(prepared);
    unsigned* part_max = hdr + 16;                                            // [256] words, then [256] 64-bit sums
    unsigned long long* part_sum = reinterpret_cast<unsigned long long*>(hdr + 16 + FP_PARTS);
    unsigned short* planes = reinterpret_cast<unsigned short*>(static_cast<char*>(prepared) + 64 + 4096);
    long long blocks = (n + 4095) / 4096;
    if (blocks < 1) blocks = 1;
    if (blocks > FP_PARTS) blocks = FP_PARTS;
    hipLaunchKernelGGL(f16x2_refresh_filter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, w, planes, n, part_max, part_sum, hdr);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int f16x2_filter_planes(const float* w, unsigned short* planes, int Cout, int K, unsigned* amax_out, unsigned* part, hipStream_t st) {
    const long long n = (long long)Cout * K;
    const int np = filter_amax_partials(w, n, part, st);
    if (np < 0) return Y4_ERR_SHAPE;
    Y4_CHECK_LAUNCH();
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(f16x2_split_filter_folded_kernel, dim3(blocks), dim3(256), 0, st, w, planes, n, part, np, amax_out);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int f16x2_filter_planes_dual(const float* w, unsigned short* planes, unsigned* amax_out, unsigned* part, unsigned short* planes_t,
                             unsigned* amax_out_t, int Cout, int Cin, int kk, int Cout_pad, bool mirror, hipStream_t st) {
    const long long n = (long long)Cout * kk * Cin;
    const int np = filter_amax_partials(w, n, part, st);
    if (np < 0) return Y4_ERR_SHAPE;
    Y4_CHECK_LAUNCH();
    const long long total = (long long)Cin * kk * Cout_pad;
    const long long most = n > total ? n : total;
    const int blocks = (int)((most + 255) / 256 > 4096 ? 4096 : (most + 255) / 256);
    hipLaunchKernelGGL(f16x2_split_filter_dual_kernel, dim3(blocks), dim3(256), 0, st, w, planes, planes_t, Cout, Cin, kk, Cout_pad,
                       part, np, amax_out, amax_out_t, mirror ? 1 : 0);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int f16x2_filter_planes_transposed(const float* w, unsigned short* planes, int Cout, int Cin, int kk, int Cout_pad,
                                   unsigned* amax_out, unsigned* part, hipStream_t st, bool mirror) {
    const int np = filter_amax_partials(w, (long long)Cout * kk * Cin, part, st);
    if (np < 0) return Y4_ERR_SHAPE;
    Y4_CHECK_LAUNCH();
    const long long total = (long long)Cin * kk * Cout_pad;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(f16x2_transpose_split_filter_folded_kernel, dim3(blocks), dim3(256), 0, st, w, planes, Cout, Cin, kk,
                       Cout_pad, part, np, amax_out, mirror ? 1 : 0);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int amax_launch(const float* x, long long ld, long long M, int C, unsigned* amax_bits, hipStream_t st, bool prezeroed) {
    if (!prezeroed && hipMemsetAsync(amax_bits, 0, sizeof(unsigned), st) != hipSuccess) return Y4_ERR_LAUNCH;
    if (M <= 0 || C <= 0) return Y4_OK;
    // 16-B loads when every row starts on a 16-B boundary and a row's last vector stays inside its pitch
    if ((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ((C + 3) & ~3) <= ld) {
        const long long total = M * ((C + 3) / 4);
        const int blocks = (int)((total + 1023) / 1024 > 1024 ? 1024 : (total + 1023) / 1024);
        hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, st, x, ld, M, C, amax_bits);
    } else {
        const long long total = M * C;
        const int blocks = (int)((total + 1023) / 1024 > 1024 ? 1024 : (total + 1023) / 1024);
        hipLaunchKernelGGL(amax_strided_kernel, dim3(blocks), dim3(256), 0, st, x, ld, M, C, amax_bits);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int amax_merge(unsigned* dst, const unsigned* src, hipStream_t st) {
    hipLaunchKernelGGL(amax_merge_kernel, dim3(1), dim3(64), 0, st, dst, src);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

}  // namespace y4
