// Implicit-GEMM convolution for gfx950 on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulate).
//
//   forward / dgrad ("gather" kernel):  D[m][n] = sum_k A[m][k] * Bt[n][k]
//       m = output pixel (b,ho,wo), n = output channel, k = (r,q,c)
//       A is gathered on the fly from the NHWC activation (never materialised),
//       Bt is the KRSC filter read as a row-major [N][K] matrix.
//   wgrad:                              D[n][j] = sum_p dy[p][n] * xg[p][j]
//       p = output pixel, j = (r,q,c); both operands are K-major (pixel-major) as stored.
//
// Tile: 256 threads = 4 waves; each wave owns TM x TN tiles of 32x32 (16 accumulator VGPRs each).
// LDS: [rows][BK + 4] floats (row pitch 144 B -> ds_read_b128 conflict-free across the 16-lane
// groups), double buffered, register-staged global loads issued one K-tile ahead.
#include "common.h"
#include "conv_geom.h"

namespace {

using y4::ConvGeom;
using y4::WgradGeom;

// TRANSPOSED = false: source pixel = (hd*stride - pad + r, wd*stride - pad + q)      [forward]
// TRANSPOSED = true : source pixel = ((hd + pad - r)/stride, (wd + pad - q)/stride)   [dgrad]
//                     (stride 2: exact division is guaranteed by the parity-class tiling)
template <int BM, int BN, int WM, int WN, bool TRANSPOSED, int BKT = 32>
__global__ __launch_bounds__(256, (BKT == 16 ? 3 : 2)) void conv_gather_mfma_f32(const ConvGeom g) {
    constexpr int LPR = BKT / 4;                      // lanes per tile row (16 B each)
    constexpr int RPP = 256 / LPR;                    // rows per load pass
    constexpr int PA = BM / RPP, PB = BN / RPP;       // load passes
    constexpr int LDS_PITCH = BKT + 4;                // 144-B / 80-B row pitch: conflict-free ds_read_b128
    constexpr int BK = BKT;
    constexpr int WTM = BM / WM, WTN = BN / WN;       // wave tile
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WM * WN == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                                  // [2][BM][LDS_PITCH]
    float* Bs = smem + 2 * BM * LDS_PITCH;             // [2][BN][LDS_PITCH]
    int* row_m = reinterpret_cast<int*>(smem + 2 * (BM + BN) * LDS_PITCH);   // [BM] dest pixel of each tile row (-1: none)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    // logical tile: N-tiles innermost so the blocks of one XCD chunk reuse the same A panel
    int r0 = 0, q0 = 0, tstep = 1;
    int ph = 0, pw = 0, mt_local, nt;
    const bool classed = TRANSPOSED && g.stride == 2;
    if (!classed) {
        const int lt = y4_xcd_remap(blockIdx.x, g.mtiles * g.ntiles);
        mt_local = lt / g.ntiles;
        nt = lt - mt_local * g.ntiles;
    } else {
        // Tile cost differs 4:2:2:1 between parity classes, so a contiguous chunk per XCD would
        // leave XCD 0 with 4x the work of XCD 7.  Every XCD instead walks its own eighth of each
        // class, heaviest class (4 taps) first: balanced across XCDs, L2-local within a class.
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        int c = 0;
        while (c < 3 && slot >= g.cls_slot0[c + 1]) ++c;
        const int per = g.cls_slot0[c + 1] - g.cls_slot0[c];
        const int t = xcd * per + (slot - g.cls_slot0[c]);
        const int tiles_c = (g.cls_tile0[c + 1] - g.cls_tile0[c]) * g.ntiles;
        if (t >= tiles_c) return;                     // padding slot (whole block, before any barrier)
        mt_local = t / g.ntiles;
        nt = t - mt_local * g.ntiles;
        ph = (3 - c) >> 1; pw = (3 - c) & 1;          // slot range 0 = class (1,1): 4 taps
        r0 = (ph + g.pad) & 1; q0 = (pw + g.pad) & 1; tstep = 2;
    }
    const int n0 = nt * BN;
    const int nr = (g.k - r0 + tstep - 1) / tstep, nq = (g.k - q0 + tstep - 1) / tstep;

    const int lrow = tid / LPR, kc = tid % LPR;

    // ---- per-thread A-row bookkeeping (rows are fixed for the whole K loop); byte offsets, 32 bit
    // 32-bit buffer offsets are relative to the first image this tile touches (tensors may exceed 4 GiB)
    const int pix_per_img = classed ? g.cls_h[ph] * g.cls_w[pw] : g.Hd * g.Wd;
    const int b_first = (int)(((long long)mt_local * BM) / pix_per_img);
    const unsigned long long img_bytes = (unsigned long long)g.Hs * g.Ws * (unsigned long long)g.lds_ * 4ull;
    const unsigned long long src_skip = (unsigned long long)b_first * img_bytes;
    const unsigned long long src_left = g.src_total_bytes > src_skip ? g.src_total_bytes - src_skip : 0ull;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.src) + src_skip, (unsigned)(src_left < 0xfffffff0ull ? src_left : 0xfffffff0ull));
    const __amdgpu_buffer_rsrc_t wt_rsrc = y4_make_rsrc(g.wt, g.wt_bytes);
    const unsigned OOB = 0xffffffffu;                 // > any num_bytes: the load returns zeros
    unsigned a_base[PA];
    int a_h[PA], a_w[PA];
    bool a_ok[PA];
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int row = p * RPP + lrow;
        const int i = mt_local * BM + row;
        int b, hd, wd;
        if (!classed) {
            a_ok[p] = i < g.M;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (g.Hd * g.Wd);
            const int rem = ii - b * (g.Hd * g.Wd);
            hd = rem / g.Wd; wd = rem - hd * g.Wd;
        } else {
            const int hc = g.cls_h[ph], wc = g.cls_w[pw];
            a_ok[p] = i < g.B * hc * wc;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (hc * wc);
            const int rem = ii - b * (hc * wc);
            const int hh = rem / wc;
            hd = 2 * hh + ph; wd = 2 * (rem - hh * wc) + pw;
        }
        if (kc == 0) row_m[row] = a_ok[p] ? (b * g.Hd + hd) * g.Wd + wd : -1;
        a_base[p] = (unsigned)(b - b_first) * (unsigned)(g.Hs * g.Ws) * pix_bytes + kc * 16u;
        if (!TRANSPOSED) {
            a_h[p] = hd * g.stride - g.pad;
            a_w[p] = wd * g.stride - g.pad;
        } else {
            a_h[p] = hd + g.pad;
            a_w[p] = wd + g.pad;
        }
    }
    // ---- per-thread B rows (filter rows n): constant byte offset, the K position is a scalar offset
    unsigned b_off[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const int n = n0 + p * RPP + lrow;
        b_off[p] = n < g.N ? (unsigned)n * (unsigned)g.K * 4u + kc * 16u : OOB;
    }

    f32x4 ra[PA], rb[PB];
    const int CC = g.Cs / BK;
    int r = r0, q = q0, cc = 0;   // position of the K-tile being LOADED

    // Loads are buffer loads with hardware zero-fill for invalid rows: no branches, no selects, a
    // handful of VALU ops per row, so the K loop is one basic block the scheduler can interleave.
    auto load_tile = [&]() {
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
                if (g.stride == 2) { hi = th >> 1; wi = tw >> 1; }     // th, tw even by construction
                ok = ok && th >= 0 && tw >= 0 && hi < g.Hs && wi < g.Ws;
            }
            const unsigned off = a_base[p] + (unsigned)(hi * g.Ws + wi) * pix_bytes;
            ra[p] = y4_buf_load4(src_rsrc, ok ? off : OOB, (unsigned)(cc * BK) * 4u);
        }
        const unsigned koff = (unsigned)((r * g.k + q) * CC + cc) * (BK * 4u);
#pragma unroll
        for (int p = 0; p < PB; ++p) rb[p] = y4_buf_load4(wt_rsrc, b_off[p], koff);
        if (++cc == CC) { cc = 0; q += tstep; if (q >= g.k) { q = q0; r += tstep; } }
    };
    // pad channels of dy (Cout = 255 -> 256) may hold anything: zero them on the way to LDS
    int st_cc = 0;
    auto store_tile = [&](int buf) {
        float* as = As + buf * BM * LDS_PITCH;
        float* bs = Bs + buf * BN * LDS_PITCH;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = ra[p];
            if (TRANSPOSED) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (st_cc * BK + kc * 4 + e >= g.Cs_valid) v[e] = 0.f;
            }
            *reinterpret_cast<f32x4*>(as + (p * RPP + lrow) * LDS_PITCH + kc * 4) = v;
        }
#pragma unroll
        for (int p = 0; p < PB; ++p)
            *reinterpret_cast<f32x4*>(bs + (p * RPP + lrow) * LDS_PITCH + kc * 4) = rb[p];
        if (++st_cc == CC) st_cc = 0;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int KT = nr * nq * CC;
    load_tile();
    store_tile(0);
    __syncthreads();

    const int fr = lane & 31, fh = lane >> 5;
    const int a_frag = (wm * WTM + fr) * LDS_PITCH + fh * 4;
    const int b_frag = (wn * WTN + fr) * LDS_PITCH + fh * 4;

    auto mfma_steps = [&](const float* as, const float* bs, int u0, int u1) {
#pragma unroll
        for (int u = u0; u < u1; ++u) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(as + i * 32 * LDS_PITCH + u * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(bs + j * 32 * LDS_PITCH + u * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
        }
    };
    for (int kt = 0; kt < KT; ++kt) {
        const int cur = kt & 1;
        const float* as = As + cur * BM * LDS_PITCH + a_frag;
        const float* bs = Bs + cur * BN * LDS_PITCH + b_frag;
        // first quarter of the MFMAs is issued before the next tile's address arithmetic + buffer loads,
        // so that block runs in the shadow of MFMAs already queued on the matrix pipe
        mfma_steps(as, bs, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < KT) load_tile();                  // global loads in flight under the remaining MFMAs
        __builtin_amdgcn_sched_barrier(0);
        mfma_steps(as, bs, 1, BK / 8);
        if (kt + 1 < KT) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + fr;
        const bool nok = n < g.N;
        const float sc = (g.scale && nok) ? g.scale[n] : 1.0f;
        const float sh = (g.shift && nok) ? g.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rbase = wm * WTM + i * 32 + 4 * fh;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = row_m[rbase + (e & 3) + 8 * (e >> 2)];
                if (nok && m >= 0) {
                    float v = acc[i][j][e] * sc + sh;
                    v = y4_act(v, g.act);
                    if (g.res) v += g.res[(long long)m * g.ldr + n];
                    g.dst[(long long)m * g.ldd + n] = v;
                }
            }
        }
    }

    // ---- BatchNorm batch statistics fused into the epilogue: column sums / sums of squares of this
    // M-tile (rows beyond M were zero-filled, so they add nothing), one partial row per tile; a tiny
    // second-stage kernel folds the rows in fp64.  Saves one full read of the conv output.
    if (!TRANSPOSED && g.stats) {
        float* red = smem;                                 // [WM][BN][2]; the K loop ended with a barrier
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) { const float v = acc[i][j][e]; cs += v; css += v * v; }
            cs += __shfl_xor(cs, 32, 64);
            css += __shfl_xor(css, 32, 64);
            if (fh == 0) {
                const int c = wn * WTN + j * 32 + fr;
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
                g.stats[((long long)mt_local * 2 + 0) * g.N + n] = cs;
                g.stats[((long long)mt_local * 2 + 1) * g.N + n] = css;
            }
        }
    }
}

// =====================================================================================================
// Split-bf16 variant of the gather kernel ("bf16x3"): every fp32 operand is split EXACTLY into three bf16
// pieces (8+8+8 mantissa bits, truncation split: x = x1 + x2 + x3) when its tile is staged into LDS, and
// the product is formed on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, products exact, fp32
// accumulate) as the six leading terms  a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1.  The dropped terms are
// <= 2^-23 |a b|, i.e. the result carries fp32-grade error (comparable to an fp32 FMA chain's rounding)
// at 6/16 of the fp32-MFMA cost.  Same tiling / gather / epilogues as conv_gather_mfma_f32.
// LDS: 3 planes x [rows][32 + 8] bf16 per operand (80-B pitch: conflict-free ds_read_b128), single stage,
// register prefetch of the next K-tile under the MFMAs.
// (bf16x8, u32x2, pack_hi16 and split3x4 -- the exact three-piece truncation split -- live in common.h)

// round-to-nearest-even bf16 of 4 floats, packed (plain-bf16 mode: one plane, one MFMA per product)
__device__ __forceinline__ unsigned rn_bf16_bits(float x) {
    const unsigned u = __float_as_uint(x);
    return u + 0x7fffu + ((u >> 16) & 1u);            // upper half = RN bf16 (NaN payloads aside)
}
__device__ __forceinline__ u32x2 round1x4(const f32x4 v) {
    u32x2 p;
    p[0] = pack_hi16(rn_bf16_bits(v[1]), rn_bf16_bits(v[0]));
    p[1] = pack_hi16(rn_bf16_bits(v[3]), rn_bf16_bits(v[2]));
    return p;
}

template <int BM, int BN, int WM, int WN, bool TRANSPOSED, int NP = 3>
__global__ __launch_bounds__(256, 2) void conv_gather_bf16x3(const ConvGeom g) {
    constexpr int BK = 32;
    constexpr int PITCH_B = 80;                        // bytes per LDS row (32 bf16 + 16 B pad)
    constexpr int PA = BM / 32;
    constexpr int NB = (BN * 4 + 255) / 256;           // 16-B chunks of the B tile per thread and plane
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WM * WN == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    unsigned char* As = smem_b;                        // [NP][BM][80 B]
    unsigned char* Bs = smem_b + NP * BM * PITCH_B;    // [NP][BN][80 B]
    int* row_m = reinterpret_cast<int*>(smem_b + NP * (BM + BN) * PITCH_B);

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
        if (t >= tiles_c) return;
        mt_local = t / g.ntiles;
        nt = t - mt_local * g.ntiles;
        ph = (3 - c) >> 1; pw = (3 - c) & 1;
        r0 = (ph + g.pad) & 1; q0 = (pw + g.pad) & 1; tstep = 2;
    }
    const int n0 = nt * BN;
    const int nr = (g.k - r0 + tstep - 1) / tstep, nq = (g.k - q0 + tstep - 1) / tstep;
    // rows are dealt so that the two rows one 16-lane ds_write_b64 group covers lie 4 apart (320 B = bank +16):
    // with adjacent rows (80 B) the groups overlapped on 4 banks -- SQ_LDS_BANK_CONFLICT was 8 % of the wave cycles
    const int t3 = tid >> 3, kc = tid & 7;
    const int lrow = (t3 & 0x18) | ((t3 & 1) << 2) | ((t3 >> 1) & 3);

    // 32-bit buffer offsets are relative to the first image this tile touches (tensors may exceed 4 GiB)
    const int pix_per_img = classed ? g.cls_h[ph] * g.cls_w[pw] : g.Hd * g.Wd;
    const int b_first = (int)(((long long)mt_local * BM) / pix_per_img);
    const unsigned long long img_bytes = (unsigned long long)g.Hs * g.Ws * (unsigned long long)g.lds_ * 4ull;
    const unsigned long long src_skip = (unsigned long long)b_first * img_bytes;
    const unsigned long long src_left = g.src_total_bytes > src_skip ? g.src_total_bytes - src_skip : 0ull;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        y4_make_rsrc(reinterpret_cast<const char*>(g.src) + src_skip, (unsigned)(src_left < 0xfffffff0ull ? src_left : 0xfffffff0ull));
    const __amdgpu_buffer_rsrc_t wt_rsrc = y4_make_rsrc(g.wt_planes, g.wt_bytes);     // 3 planes of N*K bf16
    const unsigned OOB = 0xffffffffu;
    unsigned a_base[PA];
    int a_h[PA], a_w[PA];
    bool a_ok[PA];
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int row = p * 32 + lrow;
        const int i = mt_local * BM + row;
        int b, hd, wd;
        if (!classed) {
            a_ok[p] = i < g.M;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (g.Hd * g.Wd);
            const int rem = ii - b * (g.Hd * g.Wd);
            hd = rem / g.Wd; wd = rem - hd * g.Wd;
        } else {
            const int hc = g.cls_h[ph], wc = g.cls_w[pw];
            a_ok[p] = i < g.B * hc * wc;
            const int ii = a_ok[p] ? i : 0;
            b = ii / (hc * wc);
            const int rem = ii - b * (hc * wc);
            const int hh = rem / wc;
            hd = 2 * hh + ph; wd = 2 * (rem - hh * wc) + pw;
        }
        if (kc == 0) row_m[row] = a_ok[p] ? (b * g.Hd + hd) * g.Wd + wd : -1;
        a_base[p] = (unsigned)(b - b_first) * (unsigned)(g.Hs * g.Ws) * pix_bytes + kc * 16u;
        if (!TRANSPOSED) { a_h[p] = hd * g.stride - g.pad; a_w[p] = wd * g.stride - g.pad; }
        else { a_h[p] = hd + g.pad; a_w[p] = wd + g.pad; }
    }
    // B chunks: slot = tid + 256*i -> (row = slot/4, 16-B chunk = slot%4) of each plane
    unsigned b_off[NB];
    int b_lds[NB];
    const unsigned plane_bytes = (unsigned)g.N * (unsigned)g.K * 2u;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int slot = tid + 256 * i;
        const int s2 = slot >> 2, ch = slot & 3;
        const int row = (s2 & ~7) | ((s2 & 1) << 2) | ((s2 >> 1) & 3);     // same dealing for the 8-lane ds_write_b128 groups
        const bool ok = row < BN && (n0 + row) < g.N;
        b_off[i] = ok ? (unsigned)(n0 + row) * (unsigned)g.K * 2u + ch * 16u : OOB;
        b_lds[i] = row < BN ? row * PITCH_B + ch * 16 : -1;
    }

    f32x4 ra[PA];
    u32x4 rb[NB][NP];
    const int CC = g.Cs / BK;
    int r = r0, q = q0, cc = 0;
    // per-tap A offsets: the halo test and the pixel address are recomputed only when the filter tap
    // changes (every CC K-tiles); inside a tap the K position is a scalar offset of the buffer load
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
        const unsigned koff = (unsigned)((r * g.k + q) * CC + cc) * (BK * 2u);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
                rb[i][pl] = __builtin_amdgcn_raw_buffer_load_b128(wt_rsrc, (int)b_off[i], (int)(koff + pl * plane_bytes), 0);
        if (++cc == CC) { cc = 0; q += tstep; if (q >= g.k) { q = q0; r += tstep; } tap_setup(); }
    };
    int st_cc = 0;
    auto store_tile = [&]() {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            f32x4 v = ra[p];
            if (TRANSPOSED) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (st_cc * BK + kc * 4 + e >= g.Cs_valid) v[e] = 0.f;
            }
            unsigned char* d = As + (p * 32 + lrow) * PITCH_B + kc * 8;
            if constexpr (NP == 3) {
                u32x2 p1, p2, p3;
                split3x4(v, p1, p2, p3);
                *reinterpret_cast<u32x2*>(d) = p1;
                *reinterpret_cast<u32x2*>(d + BM * PITCH_B) = p2;
                *reinterpret_cast<u32x2*>(d + 2 * BM * PITCH_B) = p3;
            } else {
                *reinterpret_cast<u32x2*>(d) = round1x4(v);
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (b_lds[i] >= 0) {
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    *reinterpret_cast<u32x4*>(Bs + pl * BN * PITCH_B + b_lds[i]) = rb[i][pl];
            }
        if (++st_cc == CC) st_cc = 0;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int KT = nr * nq * CC;
    load_tile();
    store_tile();
    __syncthreads();

    const int fr = lane & 31, fh = lane >> 5;
    const unsigned char* a_frag = As + (wm * WTM + fr) * PITCH_B + fh * 16;
    const unsigned char* b_frag = Bs + (wn * WTN + fr) * PITCH_B + fh * 16;

    for (int kt = 0; kt < KT; ++kt) {
        if (kt + 1 < KT) load_tile();                  // next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 fa[TM][NP], fb[TN][NP];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    fa[i][pl] = *reinterpret_cast<const bf16x8*>(a_frag + pl * BM * PITCH_B + i * 32 * PITCH_B + ks * 32);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    fb[j][pl] = *reinterpret_cast<const bf16x8*>(b_frag + pl * BN * PITCH_B + j * 32 * PITCH_B + ks * 32);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x16 c = acc[i][j];
                    if constexpr (NP == 3) {                  // small terms first
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][2], fb[j][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][2], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
                    }
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][0], c, 0, 0, 0);
                    acc[i][j] = c;
                }
        }
        __syncthreads();                               // every wave is done reading this stage
        if (kt + 1 < KT) store_tile();                 // split + write the prefetched tile
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + fr;
        const bool nok = n < g.N;
        const float sc = (g.scale && nok) ? g.scale[n] : 1.0f;
        const float sh = (g.shift && nok) ? g.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rbase = wm * WTM + i * 32 + 4 * fh;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = row_m[rbase + (e & 3) + 8 * (e >> 2)];
                if (nok && m >= 0) {
                    float v = acc[i][j][e] * sc + sh;
                    v = y4_act(v, g.act);
                    if (g.res) v += g.res[(long long)m * g.ldr + n];
                    g.dst[(long long)m * g.ldd + n] = v;
                }
            }
        }
    }
    if (!TRANSPOSED && g.stats) {
        float* red = reinterpret_cast<float*>(smem_b);     // [WM][BN][2]; the K loop ended with a barrier
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float cs = 0.f, css = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) { const float v = acc[i][j][e]; cs += v; css += v * v; }
            cs += __shfl_xor(cs, 32, 64);
            css += __shfl_xor(css, 32, 64);
            if (fh == 0) {
                const int c = wn * WTN + j * 32 + fr;
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
                g.stats[((long long)mt_local * 2 + 0) * g.N + n] = cs;
                g.stats[((long long)mt_local * 2 + 1) * g.N + n] = css;
            }
        }
    }
}

// fp32 filter [N][K] -> three bf16 planes [3][N][K] (exact truncation split, as split3x4)
__global__ void split_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes, long long n, int np) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = w[i];
        if (np == 1) { planes[i] = (unsigned short)(rn_bf16_bits(v) >> 16); continue; }
        const unsigned h1 = __float_as_uint(v);
        const float r1 = v - __uint_as_float(h1 & 0xffff0000u);
        const unsigned h2 = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(h2 & 0xffff0000u);
        planes[i] = (unsigned short)(h1 >> 16);
        planes[n + i] = (unsigned short)(h2 >> 16);
        planes[2 * n + i] = (unsigned short)(__float_as_uint(r2) >> 16);
    }
}

// [Cout][k][k][Cin] -> [Cin][k][k][Cout4] (zero padded to a multiple of 32 output channels)
__global__ void transpose_filter_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                        int Cout, int Cin, int kk, int Cout_pad) {
    const long long total = (long long)Cin * kk * Cout_pad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i % Cout_pad);
        const long long t = i / Cout_pad;
        const int tap = (int)(t % kk);
        const int c = (int)(t / kk);
        wt[i] = n < Cout ? w[((long long)n * kk + tap) * Cin + c] : 0.0f;
    }
}

// [Cout][k][k][Cin] fp32 -> 3 bf16 planes of [Cin][k][k][Cout_pad] (dgrad filter for the bf16x3 kernels)
__global__ void transpose_split_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ planes,
                                              int Cout, int Cin, int kk, int Cout_pad, int np) {
    const long long total = (long long)Cin * kk * Cout_pad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i % Cout_pad);
        const long long t = i / Cout_pad;
        const int tap = (int)(t % kk);
        const int c = (int)(t / kk);
        const float v = n < Cout ? w[((long long)n * kk + tap) * Cin + c] : 0.0f;
        if (np == 1) { planes[i] = (unsigned short)(rn_bf16_bits(v) >> 16); continue; }
        const unsigned h1 = __float_as_uint(v);
        const float r1 = v - __uint_as_float(h1 & 0xffff0000u);
        const unsigned h2 = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(h2 & 0xffff0000u);
        planes[i] = (unsigned short)(h1 >> 16);
        planes[total + i] = (unsigned short)(h2 >> 16);
        planes[2 * total + i] = (unsigned short)(__float_as_uint(r2) >> 16);
    }
}

template <int BM, int BN, int WM, int WN, bool TR, int BKT = 32, int NP = 0>
int launch_gather(const ConvGeom& g0, hipStream_t st) {
    constexpr bool SPLIT = NP > 0;
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
        // a tile's window spans the images of BM consecutive output pixels (+1): must fit 32-bit offsets
        const unsigned long long imgs_per_tile = (unsigned long long)BM / (unsigned long long)((g.Hd * g.Wd + 3) / 4 > 0 ? (g.Hd * g.Wd + 3) / 4 : 1) + 2;
        if (img * imgs_per_tile >= 0xfffffff0ull || wb >= 0xfffffff0ull) return Y4_ERR_SHAPE;
        g.src_total_bytes = (unsigned long long)g.B * img; g.wt_bytes = (unsigned)wb;
        if (SPLIT) {
            if (!g.wt_planes) return Y4_ERR_WORKSPACE;
            g.wt_bytes = (unsigned)((unsigned long long)g.N * g.K * 2ull * NP);
        }
    }
    const size_t smem = SPLIT ? (size_t)NP * (BM + BN) * 80 + BM * sizeof(int)
                              : 2ull * (BM + BN) * (BKT + 4) * sizeof(float) + BM * sizeof(int);
    void (*kern)(const ConvGeom);
    if constexpr (SPLIT) kern = conv_gather_bf16x3<BM, BN, WM, WN, TR, (NP > 0 ? NP : 3)>;
    else kern = conv_gather_mfma_f32<BM, BN, WM, WN, TR, BKT>;
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
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

// ---------------------------------------------------------------- streaming 1x1 kernel (small K, small N)
// The 1x1 layers on the 304^2 / 152^2 maps are HBM-bound (K, N <= 128: < 64 flop per byte); the tile machinery
// above spends their time in prologues, barriers and LDS round trips.  Here the whole filter (3 bf16 planes)
// stays in LDS for the life of a persistent block, and every wave streams its own 32 pixel rows from global
// memory straight into the MFMA A-operand layout (lane = pixel, 8 consecutive channels = 32 contiguous bytes),
// splits them in registers and never meets a barrier; the next tile's loads fly under this tile's MFMAs/stores.
// Used for forward (filter planes [N][K]) and for 1x1 dgrad (planes of the transposed filter).
// NW waves per block: 4, or 8 where the filter planes allow one block per CU only (K = N = 128: 104 KB) so that every
// SIMD still holds two waves
template <int KS, int NT, int NW = 4>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void conv1x1_stream_bf16x3(const ConvGeom g) {
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
        for (int i = tid; i < 3 * N32 * CPR; i += NTHR) {
            const int pl = i / (N32 * CPR);
            const int rem = i - pl * (N32 * CPR);
            const int row = rem / CPR, ch = rem - row * CPR;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (row < g.N) v = *reinterpret_cast<const u32x4*>(wp + ((size_t)pl * g.N + row) * (K * 2) + ch * 16);
            *reinterpret_cast<u32x4*>(smem_b + (pl * N32 + row) * PITCH + ch * 16) = v;
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t src_rsrc = y4_make_rsrc(g.src, (unsigned)g.src_total_bytes);   // < 4 GiB (host)
    const unsigned pix_bytes = (unsigned)g.lds_ * 4u;
    const int mtiles = g.mtiles;
    // KH k-steps per register set: K <= 64 keeps a whole tile per set (two tiles in flight); K = 128 keeps half a tile
    // per set, the two halves of one tile alternating (the other half's loads fly under this half's MFMAs)
    constexpr int KH = KS == 8 ? 4 : KS;
    f32x4 ra0[KH][2], ra1[KH][2];
    auto load = [&](f32x4 (&ra)[KH][2], int tile, int ks0) {
        const int m = tile * TROWS + wave * 32 + fr;
        const unsigned off = m < g.M ? (unsigned)m * pix_bytes + (unsigned)fh * 32u : 0xffffffffu;
#pragma unroll
        for (int ks = 0; ks < KH; ++ks) {
            ra[ks][0] = y4_buf_load4(src_rsrc, off, (unsigned)(ks0 + ks) * 64u);
            ra[ks][1] = y4_buf_load4(src_rsrc, off, (unsigned)(ks0 + ks) * 64u + 16u);
        }
    };
    float cs[NT], css[NT];
    float sc[NT], sh[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        cs[j] = 0.f; css[j] = 0.f;
        const int n = j * 32 + fr;
        sc[j] = (g.scale && n < g.N) ? g.scale[n] : 1.0f;
        sh[j] = (g.shift && n < g.N) ? g.shift[n] : 0.0f;
    }
    const unsigned char* b_frag = smem_b + fr * PITCH + fh * 16;
    f32x16 acc[NT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    };
    auto mma = [&](f32x4 (&ra)[KH][2], int ks0) {
        // the filter fragments are loop-invariant; at K = 128 keeping them all in registers (up to 384) spills, so the
        // compiler is told the LDS may have changed and re-reads them per tile (ds_read_b128 is cheap beside 6 MFMAs)
        if constexpr (KS == 8) asm volatile("" ::: "memory");
#pragma unroll
        for (int ks = 0; ks < KH; ++ks) {
            u32x2 a1, a2, a3, b1, b2, b3;
            split3x4(ra[ks][0], a1, a2, a3);
            split3x4(ra[ks][1], b1, b2, b3);
            const u32x4 q1 = {a1[0], a1[1], b1[0], b1[1]}, q2 = {a2[0], a2[1], b2[0], b2[1]}, q3 = {a3[0], a3[1], b3[0], b3[1]};
            bf16x8 fa[3];
            fa[0] = __builtin_bit_cast(bf16x8, q1); fa[1] = __builtin_bit_cast(bf16x8, q2); fa[2] = __builtin_bit_cast(bf16x8, q3);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bf16x8 fb[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    fb[pl] = *reinterpret_cast<const bf16x8*>(b_frag + (pl * N32 + j * 32) * PITCH + (ks0 + ks) * 32);
                f32x16 c = acc[j];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2], fb[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fb[1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fb[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[0], c, 0, 0, 0);
                acc[j] = c;
            }
        }
    };
    auto epilogue = [&](int tile) {
        const int mbase = tile * TROWS + wave * 32 + 4 * fh;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = j * 32 + fr;
            const bool nok = n < g.N;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float raw = acc[j][e];
                cs[j] += raw; css[j] += raw * raw;           // rows past M are exact zeros
                const int m = mbase + (e & 3) + 8 * (e >> 2);
                if (nok && m < g.M) {
                    float v = raw * sc[j] + sh[j];
                    v = y4_act(v, g.act);
                    if (g.res) v += g.res[(long long)m * g.ldr + n];
                    g.dst[(long long)m * g.ldd + n] = v;
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
    if (g.stats) {                                        // one partial row per block: [gridDim][2][N]
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

template <int KS, int NT, int NW = 4>
int launch_stream1x1(const ConvGeom& g0, hipStream_t st, int* nparts) {
    ConvGeom g = g0;
    g.mtiles = (g.M + NW * 32 - 1) / (NW * 32);
    g.ntiles = 1;
    g.src_total_bytes = (unsigned long long)g.M * (unsigned long long)g.lds_ * 4ull;
    const size_t smem = (size_t)3 * NT * 32 * (KS * 32 + 16);
    auto kern = conv1x1_stream_bf16x3<KS, NT, NW>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    const int resident = smem > 80 * 1024 ? 256 : 512;    // blocks per CU by LDS: 1 (K = N = 128) or 2
    const int grid = g.mtiles < resident ? g.mtiles : resident;
    if (nparts) *nparts = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

// eligibility: bf16x3 arithmetic, 1x1 stride 1, K in {32,64,128}, N <= 128, filter planes <= 52 KB of LDS,
// 32-bit addressable source, every source channel valid, and enough rows to be worth a persistent launch
static bool stream1x1_ok(int mode, const ConvGeom& g) {
    if (mode != 1 || g.k != 1 || g.stride != 1 || !g.wt_planes) return false;
    if (g.Cs != 32 && g.Cs != 64 && g.Cs != 128) return false;
    if (g.Cs_valid != g.Cs || g.N > 128) return false;
    const int n32 = (g.N + 31) / 32 * 32;
    if (g.Cs * n32 > (g.Cs == 128 ? 16384 : 8192)) return false;     // filter planes: <= 52 KB (2 blocks/CU) or 104 KB at K = 128
    if ((unsigned long long)g.M * (unsigned long long)g.lds_ * 4ull >= 0xfffffff0ull) return false;
    return g.M >= 128 * 1024;
}

static int dispatch_stream1x1(const ConvGeom& g, hipStream_t st, int* nparts) {
    const int nt = (g.N + 31) / 32;
    switch (g.Cs / 16 * 10 + nt) {
        case 21: return launch_stream1x1<2, 1>(g, st, nparts);
        case 22: return launch_stream1x1<2, 2>(g, st, nparts);
        case 23: case 24: return launch_stream1x1<2, 4>(g, st, nparts);
        case 41: return launch_stream1x1<4, 1>(g, st, nparts);
        case 42: return launch_stream1x1<4, 2>(g, st, nparts);
        case 43: case 44: return launch_stream1x1<4, 4>(g, st, nparts);
        case 81: return launch_stream1x1<8, 1>(g, st, nparts);
        case 82: return launch_stream1x1<8, 2>(g, st, nparts);
        case 83: case 84: return launch_stream1x1<8, 4, 8>(g, st, nparts);
        default: return Y4_ERR_SHAPE;
    }
}

// the bf16 kernels on one tile: a single rounded plane (mode 2) or the three-piece split (mode 1)
template <int BM, int BN, int WM, int WN, bool TR>
int launch_gather_bf16(bool one, const ConvGeom& g, hipStream_t st) {
    return one ? launch_gather<BM, BN, WM, WN, TR, 32, 1>(g, st) : launch_gather<BM, BN, WM, WN, TR, 32, 3>(g, st);
}

template <bool TR>
int dispatch_gather(int mode, const ConvGeom& g, hipStream_t st, int* nparts) {
    // *nparts: number of BN-statistics partial rows the launch writes (M tiles, or blocks of the streaming kernel)
    if (nparts) *nparts = (g.M + 127) / 128;
    if (stream1x1_ok(mode, g)) return dispatch_stream1x1(g, st, nparts);
    if (mode == 1 || mode == 2) {
        const bool one = mode == 2;
        if (g.N > 64) {
            const long long nt = (g.N + 127) / 128;
            const long long b128 = ((long long)g.M + 127) / 128 * nt, b64 = ((long long)g.M + 63) / 64 * nt;
            const double c128 = (double)((b128 + 511) / 512) * 128.0;
            const double c64 = (double)((b64 + 511) / 512) * 64.0 * 1.10;
            if (c64 < c128 && !(TR && g.stride == 2)) {
                if (nparts) *nparts = (g.M + 63) / 64;
                return launch_gather_bf16<64, 128, 2, 2, TR>(one, g, st);
            }
            return launch_gather_bf16<128, 128, 2, 2, TR>(one, g, st);
        }
        if (g.N > 32) return launch_gather_bf16<128, 64, 2, 2, TR>(one, g, st);
        return launch_gather_bf16<128, 32, 4, 1, TR>(one, g, st);
    }
    if (g.N > 64) {
        // LDS allows 2 resident blocks per CU at BK = 32 (74 KB) and 3 at BK = 16 (41 KB).  1x1 convs have
        // short K loops (4..32 tiles), so prologue/epilogue time matters: the third block covers it
        // (+5..10 % measured); on the long 3x3 loops the two depths tie and BK = 32 halves the barriers.
        const bool short_k = g.k == 1;
        const long long slots = short_k ? 768 : 512;
        // When 128-row tiles fill the last round of resident blocks badly (e.g. 724 blocks = 1.41 rounds
        // at 19x19 maps), 64-row tiles (+8 % per-flop cost) win.
        const long long nt = (g.N + 127) / 128;
        const long long b128 = ((long long)g.M + 127) / 128 * nt, b64 = ((long long)g.M + 63) / 64 * nt;
        const double c128 = (double)((b128 + slots - 1) / slots) * 128.0;
        const double c64 = (double)((b64 + slots - 1) / slots) * 64.0 * 1.08;
        if (c64 < c128 && !(TR && g.stride == 2)) {
            if (nparts) *nparts = (g.M + 63) / 64;
            return short_k ? launch_gather<64, 128, 2, 2, TR, 16>(g, st) : launch_gather<64, 128, 2, 2, TR>(g, st);
        }
        return short_k ? launch_gather<128, 128, 2, 2, TR, 16>(g, st) : launch_gather<128, 128, 2, 2, TR>(g, st);
    }
    if (g.k == 1) {      // HBM-bound 1x1 layers at 304^2 / 152^2: more resident blocks = more loads in flight
        if (g.N > 32) return launch_gather<128, 64, 2, 2, TR, 16>(g, st);
    }
    if (g.N > 32) return launch_gather<128, 64, 2, 2, TR>(g, st);
    return launch_gather<128, 32, 4, 1, TR>(g, st);
}

// ------------------------------------------------------------------------------------ wgrad

// D[n][j] = sum_p dy[p][n] * xg[p][j].  Block tile TN_ x TJ_ (64 or 128 each), 4 waves as 2x2,
// K-chunks of 32 pixels, both operands kept pixel-major in LDS exactly as they lie in memory
// (rows of TN_/TJ_ floats): a half-wave's ds_read_b32 covers 32 consecutive floats, conflict-free.
template <int TN_, int TJ_>
__global__ __launch_bounds__(256, 2) void conv_wgrad_mfma_f32(const WgradGeom g) {
    constexpr int MI = TN_ / 64, MJ = TJ_ / 64;           // 32x32 MFMA tiles per wave
    constexpr int LPR_A = TN_ / 4, RPP_A = 256 / LPR_A, PA = 32 / RPP_A;
    constexpr int LPR_B = TJ_ / 4, RPP_B = 256 / LPR_B, PB = 32 / RPP_B;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                           // [2][32][TN_]  dy tile   (pixel-major)
    float* Bs = smem + 2 * 32 * TN_;            // [2][32][TJ_]  x  tile   (pixel-major)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int tiles = g.ntn * g.ntj;
    int bid = y4_xcd_remap(blockIdx.x, tiles * g.splits);   // tiles of one pixel range share an XCD's L2
    const int split = bid / tiles;
    bid -= split * tiles;
    const int tn = bid / g.ntj, tj = bid - tn * g.ntj;
    const int n0 = tn * TN_, j0 = tj * TJ_;

    const int arow = tid / LPR_A, ac4 = (tid % LPR_A) * 4;
    const int brow = tid / LPR_B, bc4 = (tid % LPR_B) * 4;
    const int Cout4 = (g.Cout + 3) & ~3;
    const bool an_ok = (n0 + ac4) < Cout4;
    const int j = j0 + bc4;
    const bool bj_ok = j < g.J;
    int jr = 0, jq = 0, jc = 0;
    if (bj_ok) { const int tap = j / g.Cin; jc = j - tap * g.Cin; jr = tap / g.k; jq = tap - jr * g.k; }

    const int chunk0 = split * g.chunks_per_split;
    int nchunks = (g.M + 31) / 32 - chunk0;
    if (nchunks > g.chunks_per_split) nchunks = g.chunks_per_split;

    // running (b, ho, wo) of this thread's B rows: advanced by 32 pixels per chunk, no divisions
    // 32-bit buffer windows start at this block's first pixel (dy) / first image (x)
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
    int pb_b[PB], pb_h[PB], pb_w[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const int pix = chunk0 * 32 + p * RPP_B + brow;
        const int pp = pix < g.M ? pix : (int)p_first;
        const int bb = pp / (g.Ho * g.Wo);
        pb_b[p] = bb - b_first;                            // image index relative to the block's window
        const int rem = pp - bb * (g.Ho * g.Wo);
        pb_h[p] = rem / g.Wo;
        pb_w[p] = rem - pb_h[p] * g.Wo;
    }
    unsigned a_off[PA];
#pragma unroll
    for (int p = 0; p < PA; ++p)
        a_off[p] = an_ok ? (unsigned)(p * RPP_A + arow) * (unsigned)g.lddy * 4u + (unsigned)(n0 + ac4) * 4u : OOB;
    const unsigned chunk_bytes = 32u * (unsigned)g.lddy * 4u;
    const unsigned x_pix_bytes = (unsigned)g.ldx * 4u;

    f32x4 ra[PA], rb[PB];
    int ld_chunk = 0;
    auto load_chunk = [&]() {
        const int pbase = (chunk0 + ld_chunk) * 32;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const bool ok = pbase + p * RPP_A + arow < g.M;
            ra[p] = y4_buf_load4(dy_rsrc, ok ? a_off[p] : OOB, (unsigned)ld_chunk * chunk_bytes);
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const int pix = pbase + p * RPP_B + brow;
            const int hi = pb_h[p] * g.stride - g.pad + jr, wi = pb_w[p] * g.stride - g.pad + jq;
            const bool ok = pix < g.M && bj_ok && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
            const unsigned off = (unsigned)((pb_b[p] * g.H + hi) * g.W + wi) * x_pix_bytes + (unsigned)jc * 4u;
            rb[p] = y4_buf_load4(x_rsrc, ok ? off : OOB, 0u);
            pb_w[p] += 32;
            while (pb_w[p] >= g.Wo) { pb_w[p] -= g.Wo; if (++pb_h[p] == g.Ho) { pb_h[p] = 0; ++pb_b[p]; } }
        }
        ++ld_chunk;
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PA; ++p)
            *reinterpret_cast<f32x4*>(As + (buf * 32 + p * RPP_A + arow) * TN_ + ac4) = ra[p];
#pragma unroll
        for (int p = 0; p < PB; ++p)
            *reinterpret_cast<f32x4*>(Bs + (buf * 32 + p * RPP_B + brow) * TJ_ + bc4) = rb[p];
    };

    f32x16 acc[MI][MJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    if (nchunks > 0) {
        load_chunk();
        store_chunk(0);
        __syncthreads();
        for (int ch = 0; ch < nchunks; ++ch) {
            const int cur = ch & 1;
            if (ch + 1 < nchunks) load_chunk();
            const float* as = As + (cur * 32 + fh) * TN_ + wm * (TN_ / 2) + fr;
            const float* bs = Bs + (cur * 32 + fh) * TJ_ + wn * (TJ_ / 2) + fr;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                float a[MI], b[MJ];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = as[(2 * t) * TN_ + i * 32];
#pragma unroll
                for (int jj = 0; jj < MJ; ++jj) b[jj] = bs[(2 * t) * TJ_ + jj * 32];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int jj = 0; jj < MJ; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[jj], acc[i][jj], 0, 0, 0);
            }
            if (ch + 1 < nchunks) store_chunk(cur ^ 1);
            __syncthreads();
        }
    }
    // D[n][j]: row index (n) on the registers, column (j) on the lane
    float* out = g.out + (long long)split * g.Cout * g.J;
#pragma unroll
    for (int jj = 0; jj < MJ; ++jj) {
        const int jcol = j0 + wn * (TJ_ / 2) + jj * 32 + fr;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int nb = n0 + wm * (TN_ / 2) + i * 32 + 4 * fh;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = nb + (e & 3) + 8 * (e >> 2);
                if (n < g.Cout && jcol < g.J) out[(long long)n * g.J + jcol] = acc[i][jj][e];
            }
        }
    }
}

// Split-bf16 ("bf16x3") wgrad: same math as conv_wgrad_mfma_f32, operands split exactly into three bf16
// planes while being transposed into LDS as [n or j][32 pixels] rows (80-B pitch), so the fragment reads
// are the plain ds_read_b128 of the gather kernel.  Each thread owns one 4-pixel x 4-channel block of
// each operand per 32-pixel chunk (4 coalesced 16-B loads, a 4x4 register transpose folded into the
// bf16 packing, 12 ds_write_b64).
template <int TN_, int TJ_, int NP = 3>
__global__ __launch_bounds__(256, 2) void conv_wgrad_bf16x3(const WgradGeom g) {
    constexpr int MI = TN_ / 64, MJ = TJ_ / 64;
    constexpr int PITCH_B = 80;
    constexpr int NBLK_A = 8 * (TN_ / 4), NBLK_B = 8 * (TJ_ / 4);     // 4x4 blocks per chunk (<= 256)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    unsigned char* As = smem_b;                          // [NP][TN_][80 B]
    unsigned char* Bs = smem_b + NP * TN_ * PITCH_B;     // [NP][TJ_][80 B]
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

    // 32-bit buffer windows start at this block's first pixel (dy) / first image (x)
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
    int pb_b[4], pb_h[4], pb_w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pix = chunk0 * 32 + pg * 4 + i;
        const int pp = pix < g.M ? pix : (int)p_first;
        const int bb = pp / (g.Ho * g.Wo);
        pb_b[i] = bb - b_first;
        const int rem = pp - bb * (g.Ho * g.Wo);
        pb_h[i] = rem / g.Wo;
        pb_w[i] = rem - pb_h[i] * g.Wo;
    }
    const unsigned a_off0 = an_ok ? (unsigned)(pg * 4) * (unsigned)g.lddy * 4u + (unsigned)(n0 + cg * 4) * 4u : OOB;
    const unsigned dy_pix_bytes = (unsigned)g.lddy * 4u;
    const unsigned chunk_bytes = 32u * dy_pix_bytes;
    const unsigned x_pix_bytes = (unsigned)g.ldx * 4u;

    f32x4 ra[4], rb[4];
    int ld_chunk = 0;
    auto load_chunk = [&]() {
        const int pbase = (chunk0 + ld_chunk) * 32 + pg * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = an_ok && pbase + i < g.M;
            ra[i] = y4_buf_load4(dy_rsrc, ok ? a_off0 + (unsigned)i * dy_pix_bytes : OOB, (unsigned)ld_chunk * chunk_bytes);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int hi = pb_h[i] * g.stride - g.pad + jr, wi = pb_w[i] * g.stride - g.pad + jq;
            const bool ok = bj_ok && pbase + i < g.M && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
            const unsigned off = (unsigned)((pb_b[i] * g.H + hi) * g.W + wi) * x_pix_bytes + (unsigned)jc * 4u;
            rb[i] = y4_buf_load4(x_rsrc, ok ? off : OOB, 0u);
            pb_w[i] += 32;
            while (pb_w[i] >= g.Wo) { pb_w[i] -= g.Wo; if (++pb_h[i] == g.Ho) { pb_h[i] = 0; ++pb_b[i]; } }
        }
        ++ld_chunk;
    };
    // split 4 pixels x 4 channels and write the 4 channel rows (3 planes each) transposed
    auto split_store = [&](const f32x4 (&v)[4], unsigned char* base, int rows) {
        if constexpr (NP == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                u32x2 p;
                p[0] = pack_hi16(rn_bf16_bits(v[1][e]), rn_bf16_bits(v[0][e]));
                p[1] = pack_hi16(rn_bf16_bits(v[3][e]), rn_bf16_bits(v[2][e]));
                *reinterpret_cast<u32x2*>(base + (cg * 4 + e) * PITCH_B + pg * 8) = p;
            }
            return;
        }
        unsigned h1[4][4], h2[4][4], h3[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h1[i][e] = __float_as_uint(v[i][e]);
                const float r1 = v[i][e] - __uint_as_float(h1[i][e] & 0xffff0000u);
                h2[i][e] = __float_as_uint(r1);
                const float r2 = r1 - __uint_as_float(h2[i][e] & 0xffff0000u);
                h3[i][e] = __float_as_uint(r2);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned char* d = base + (cg * 4 + e) * PITCH_B + pg * 8;
            u32x2 p;
            p[0] = pack_hi16(h1[1][e], h1[0][e]); p[1] = pack_hi16(h1[3][e], h1[2][e]);
            *reinterpret_cast<u32x2*>(d) = p;
            p[0] = pack_hi16(h2[1][e], h2[0][e]); p[1] = pack_hi16(h2[3][e], h2[2][e]);
            *reinterpret_cast<u32x2*>(d + rows * PITCH_B) = p;
            p[0] = pack_hi16(h3[1][e], h3[0][e]); p[1] = pack_hi16(h3[3][e], h3[2][e]);
            *reinterpret_cast<u32x2*>(d + 2 * rows * PITCH_B) = p;
        }
    };
    auto store_chunk = [&]() {
        if (a_act) split_store(ra, As, TN_);
        if (b_act) split_store(rb, Bs, TJ_);
    };

    f32x16 acc[MI][MJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const unsigned char* a_frag = As + (wm * (TN_ / 2) + fr) * PITCH_B + fh * 16;
    const unsigned char* b_frag = Bs + (wn * (TJ_ / 2) + fr) * PITCH_B + fh * 16;
    if (nchunks > 0) {
        load_chunk();
        store_chunk();
        __syncthreads();
        for (int ch = 0; ch < nchunks; ++ch) {
            if (ch + 1 < nchunks) load_chunk();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[MI][NP], fb[MJ][NP];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl)
                        fa[i][pl] = *reinterpret_cast<const bf16x8*>(a_frag + pl * TN_ * PITCH_B + i * 32 * PITCH_B + ks * 32);
#pragma unroll
                for (int jj = 0; jj < MJ; ++jj)
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl)
                        fb[jj][pl] = *reinterpret_cast<const bf16x8*>(b_frag + pl * TJ_ * PITCH_B + jj * 32 * PITCH_B + ks * 32);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int jj = 0; jj < MJ; ++jj) {
                        f32x16 c = acc[i][jj];
                        if constexpr (NP == 3) {
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][2], fb[jj][0], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[jj][1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[jj][2], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[jj][0], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[jj][1], c, 0, 0, 0);
                        }
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[jj][0], c, 0, 0, 0);
                        acc[i][jj] = c;
                    }
            }
            __syncthreads();
            if (ch + 1 < nchunks) store_chunk();
            __syncthreads();
        }
    }
    float* out = g.out + (long long)split * g.Cout * g.J;
#pragma unroll
    for (int jj = 0; jj < MJ; ++jj) {
        const int jcol = j0 + wn * (TJ_ / 2) + jj * 32 + fr;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int nb = n0 + wm * (TN_ / 2) + i * 32 + 4 * fh;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = nb + (e & 3) + 8 * (e >> 2);
                if (n < g.Cout && jcol < g.J) out[(long long)n * g.J + jcol] = acc[i][jj][e];
            }
        }
    }
}

template <int TN_, int TJ_, int NP = 0>
int launch_wgrad(const WgradGeom& g, hipStream_t st) {
    constexpr bool SPLIT = NP > 0;
    const size_t smem = SPLIT ? (size_t)NP * (TN_ + TJ_) * 80 : 2ull * 32 * (TN_ + TJ_) * sizeof(float);
    void (*kern)(const WgradGeom);
    if constexpr (SPLIT) kern = conv_wgrad_bf16x3<TN_, TJ_, (NP > 0 ? NP : 3)>;
    else kern = conv_wgrad_mfma_f32<TN_, TJ_>;
    static Y4DynLds lds_attr;                              // per device, see common.h
    if (!lds_attr.ensure(reinterpret_cast<const void*>(kern), smem)) return Y4_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(g.ntn * g.ntj * g.splits), dim3(256), smem, st, g);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

template <int NP>
int wgrad_tiles(const WgradGeom& g, hipStream_t st) {
    if (g.tn == 128 && g.tj == 128) return launch_wgrad<128, 128, NP>(g, st);
    if (g.tn == 128) return launch_wgrad<128, 64, NP>(g, st);
    if (g.tj == 128) return launch_wgrad<64, 128, NP>(g, st);
    return launch_wgrad<64, 64, NP>(g, st);
}

}  // namespace

// ---------------------------------------------------------------- what conv_api.hip calls (declared in conv_geom.h)
namespace y4 {

int igemm_filter(int mode, const float* w, void* out, int Cout, int Cin, int kk, bool transposed, hipStream_t st) {
    const int np = mode == 2 ? 1 : 3, Cout_pad = (Cout + 31) / 32 * 32;
    const long long n = (long long)Cin * kk * (transposed ? Cout_pad : Cout);
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    unsigned short* planes = static_cast<unsigned short*>(out);
    if (!transposed)
        hipLaunchKernelGGL(split_filter_kernel, dim3(blocks), dim3(256), 0, st, w, planes, n, np);
    else if (mode != 0)
        hipLaunchKernelGGL(transpose_split_filter_kernel, dim3(blocks), dim3(256), 0, st, w, planes, Cout, Cin, kk, Cout_pad, np);
    else
        hipLaunchKernelGGL(transpose_filter_kernel, dim3(blocks), dim3(256), 0, st, w, static_cast<float*>(out), Cout, Cin, kk, Cout_pad);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int igemm_gather(int mode, const ConvGeom& g, bool transposed, hipStream_t st, int* nparts) {
    return transposed ? dispatch_gather<true>(mode, g, st, nparts) : dispatch_gather<false>(mode, g, st, nparts);
}

int igemm_wgrad(int mode, const WgradGeom& g, hipStream_t st) {
    return mode == 1 ? wgrad_tiles<3>(g, st) : mode == 2 ? wgrad_tiles<1>(g, st) : wgrad_tiles<0>(g, st);
}

}  // namespace y4
