// The ImageNet classifier behind the CSPDarknet53 backbone (darknet/darknet.py:164-193, darknet/main_amp.py:184,549-562 of the
// reference): global average pool, the 1024 -> N linear layer, label-smoothed cross-entropy and top-k accuracy.
//
// All four are small beside the backbone, so the kernels are plain: 256-thread blocks, wave64 shuffles and LDS inside a
// block, a second small launch where blocks have to be combined, no block ever waits on another.  Every reduction runs in a
// fixed order (bit-identical run to run); the only atomics are the integer hit counters of the top-k kernel.
#include "common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum / max of one value per thread, the same result in every thread: butterfly inside each wave, then the
// four wave results from LDS in wave order.  `slot` is a kWaves-element LDS array that no other reduction is using.
template <typename T> __device__ __forceinline__ T block_sum(T v, T* slot) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = slot[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r += slot[w];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* slot) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = slot[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = fmaxf(r, slot[w]);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- pool
// One block: 64 channel lanes (V channels each) x 4 pixel groups of one image.  A thread sums the pixels p = g, g + 4, ...
// of its channels in that order; the four partial sums meet in LDS and are added in group order.
template <int V>
__global__ __launch_bounds__(kThreads) void avgpool_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy,
                                                               int HW, int C) {
    __shared__ float part[4][64 * V];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * V;
    const int b = blockIdx.y;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    if (c < C) {                                         // (V == 4: C % 4 == 0, so c < C covers c + 3)
        const float* xp = x + ((size_t)b * HW) * ldx + c;
        for (int p = g; p < HW; p += 4) {
            if constexpr (V == 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(xp + (size_t)p * ldx);
                acc[0] += t.x; acc[1] += t.y; acc[2] += t.z; acc[3] += t.w;
            } else {
                acc[0] += xp[(size_t)p * ldx];
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) part[g][lane * V + v] = acc[v];
    __syncthreads();
    if (g == 0 && c < C) {
        const float n = (float)HW;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int i = lane * V + v;
            y[(size_t)b * ldy + c + v] = (((part[0][i] + part[1][i]) + part[2][i]) + part[3][i]) / n;
        }
    }
}

template <int V>
__global__ __launch_bounds__(kThreads) void avgpool_bwd_kernel(const float* __restrict__ dy, int lddy, float* __restrict__ dx, int lddx,
                                                               long long total, int HW, int CV) {
    const float n = (float)HW;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const int c = (int)(i % CV) * V;
        const long long bp = i / CV;                      // pixel row b * HW + p
        const long long b = bp / HW;
        if constexpr (V == 4) {
            f32x4 t = *reinterpret_cast<const f32x4*>(dy + b * lddy + c);
            t.x /= n; t.y /= n; t.z /= n; t.w /= n;
            *reinterpret_cast<f32x4*>(dx + bp * lddx + c) = t;
        } else {
            dx[bp * lddx + c] = dy[b * lddy + c] / n;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// -------------------------------------------------------------------------------------------------------------- linear
// out[i][j] = sum_r A(i, r) * B(j, r) (+ bias[j]),  A(i, r) = a[i * sai + r * sar],  B(j, r) = b[j * sbj + r * sbr].
// 64 x 64 output tile per block, 4 x 4 per thread, 32 reduction steps per LDS stage; fp32 fma chain in r order, so an
// element's value does not depend on the grid.  AR / BR: the operand's r index is the contiguous one (lanes run along r
// when staging it), else its tile index is.  Elements outside the problem are staged as zeros.  The next stage's global
// loads are issued into registers before the current stage is multiplied, so their latency hides behind the fma block.
constexpr int kTile = 64, kStep = 32, kPitch = kTile + 4, kPerThread = kTile * kStep / kThreads;

template <bool RCONTIG>
__device__ __forceinline__ void fetch_tile(float (&v)[kPerThread], const float* __restrict__ p, long long st, long long sr, int t0,
                                           int T, int r0, int R) {
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
        const int idx = threadIdx.x + e * kThreads;
        const int t = RCONTIG ? idx / kStep : idx % kTile;
        const int r = RCONTIG ? idx % kStep : idx / kTile;
        v[e] = (t0 + t < T && r0 + r < R) ? p[(long long)(t0 + t) * st + (long long)(r0 + r) * sr] : 0.0f;
    }
}
template <bool RCONTIG> __device__ __forceinline__ void stage_tile(float (*s)[kPitch], const float (&v)[kPerThread]) {
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
        const int idx = threadIdx.x + e * kThreads;
        s[RCONTIG ? idx % kStep : idx / kTile][RCONTIG ? idx / kStep : idx % kTile] = v[e];
    }
}

template <bool AR, bool BR>
__global__ __launch_bounds__(kThreads) void gemm_nt_kernel(const float* __restrict__ a, long long sai, long long sar,
                                                           const float* __restrict__ b, long long sbj, long long sbr,
                                                           const float* __restrict__ bias, float* __restrict__ out, long long ldo,
                                                           int I, int J, int R) {
    __shared__ __attribute__((aligned(16))) float As[kStep][kPitch];
    __shared__ __attribute__((aligned(16))) float Bs[kStep][kPitch];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int ti = (threadIdx.x >> 4) * 4, tj = (threadIdx.x & 15) * 4;
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0f;
    float ra[kPerThread], rb[kPerThread];
    fetch_tile<AR>(ra, a, sai, sar, i0, I, 0, R);
    fetch_tile<BR>(rb, b, sbj, sbr, j0, J, 0, R);
    for (int r0 = 0; r0 < R; r0 += kStep) {
        stage_tile<AR>(As, ra);
        stage_tile<BR>(Bs, rb);
        __syncthreads();
        if (r0 + kStep < R) {
            fetch_tile<AR>(ra, a, sai, sar, i0, I, r0 + kStep, R);
            fetch_tile<BR>(rb, b, sbj, sbr, j0, J, r0 + kStep, R);
        }
#pragma unroll
        for (int r = 0; r < kStep; ++r) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&As[r][ti]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[r][tj]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], bv[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ti + u;
        if (i >= I) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tj + v;
            if (j < J) out[(long long)i * ldo + j] = acc[u][v] + (bias ? bias[j] : 0.0f);
        }
    }
}

// dbias[n] = sum_m dy[m][n], m ascending: one thread per column
__global__ __launch_bounds__(kThreads) void colsum_kernel(const float* __restrict__ dy, int lddy, float* __restrict__ dbias, int M, int N) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
    for (int m = 0; m < M; ++m) s += dy[(size_t)m * lddy + n];
    dbias[n] = s;
}

template <bool AR, bool BR>
int launch_gemm(const float* a, long long sai, long long sar, const float* b, long long sbj, long long sbr, const float* bias,
                float* out, long long ldo, int I, int J, int R, hipStream_t st) {
    const dim3 grid((J + kTile - 1) / kTile, (I + kTile - 1) / kTile);
    hipLaunchKernelGGL((gemm_nt_kernel<AR, BR>), grid, dim3(kThreads), 0, st, a, sai, sar, b, sbj, sbr, bias, out, ldo, I, J, R);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

// --------------------------------------------------------------------------------------------------- cross-entropy
constexpr long long kIgnore = -100;                       // torch's default ignore_index

struct RowStats {
    float m;        // max_j z_j
    float sum_e;    // sum_j exp(z_j - m)
    float sum_z;    // sum_j z_j
    float z_t;      // z at the label (0 if the label matches no column)
};

// The label is only COMPARED with the column index (a select inside the sweep): no address is ever computed from it, so a
// label outside [0, N) cannot read out of bounds.
__device__ __forceinline__ RowStats row_stats(const float* __restrict__ z, int N, long long t, float* lds) {
    float m = -INFINITY, sz = 0.0f, zt = 0.0f;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const float v = z[j];
        m = fmaxf(m, v);
        sz += v;
        zt = ((long long)j == t) ? v : zt;
    }
    RowStats r;
    r.m = block_max(m, lds);
    r.sum_z = block_sum(sz, lds + kWaves);
    r.z_t = block_sum(zt, lds + 2 * kWaves);               // (exactly one thread holds a non-zero term)
    float se = 0.0f;
    for (int j = threadIdx.x; j < N; j += kThreads) se += expf(z[j] - r.m);
    r.sum_e = block_sum(se, lds + 3 * kWaves);
    return r;
}

__global__ __launch_bounds__(kThreads) void ce_fwd_rows_kernel(const float* __restrict__ logits, int ldl, const long long* __restrict__ target,
                                                               int N, double eps, float* __restrict__ row_loss) {
    __shared__ float lds[4 * kWaves];
    const int b = blockIdx.x;
    const long long t = target[b];
    if (t == kIgnore) {
        if (threadIdx.x == 0) row_loss[b] = 0.0f;
        return;
    }
    const RowStats s = row_stats(logits + (size_t)b * ldl, N, t, lds);
    if (threadIdx.x == 0) {
        const double lse = (double)s.m + log((double)s.sum_e);
        const double row = lse - (1.0 - eps) * (double)s.z_t - eps * ((double)s.sum_z / (double)N);
        row_loss[b] = (t < 0 || t >= N) ? NAN : (float)row;
    }
}

// loss_out[0] = sum of the counted rows / their number (NaN when there is none, as in torch), loss_out[1] = that number;
// one block, rows b = tid, tid + 256, ... in double, then the block reduction
__global__ __launch_bounds__(kThreads) void ce_mean_kernel(const float* __restrict__ row_loss, const long long* __restrict__ target, int B,
                                                           double* __restrict__ loss_out) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0, n = 0.0;
    for (int b = threadIdx.x; b < B; b += kThreads)
        if (target[b] != kIgnore) {
            s += (double)row_loss[b];
            n += 1.0;
        }
    s = block_sum(s, lds);
    n = block_sum(n, lds + kWaves);
    if (threadIdx.x == 0) {
        loss_out[0] = s / n;
        loss_out[1] = n;
    }
}

__global__ __launch_bounds__(kThreads) void ce_bwd_kernel(const float* __restrict__ logits, int ldl, const long long* __restrict__ target,
                                                          const double* __restrict__ loss_out, const float* __restrict__ gscale,
                                                          float* __restrict__ dlogits, int lddl, int N, double eps) {
    __shared__ float lds[4 * kWaves];
    const int b = blockIdx.x;
    const long long t = target[b];
    float* d = dlogits + (size_t)b * lddl;
    if (t == kIgnore) {
        for (int j = threadIdx.x; j < N; j += kThreads) d[j] = 0.0f;
        return;
    }
    const float* z = logits + (size_t)b * ldl;
    const RowStats s = row_stats(z, N, t, lds);
    const double scale = (double)gscale[0] / loss_out[1];
    const double inv = 1.0 / (double)s.sum_e, uni = eps / (double)N;
    const bool bad = t < 0 || t >= N;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const double p = (double)expf(z[j] - s.m) * inv;
        const double q = (((long long)j == t) ? 1.0 - eps : 0.0) + uni;
        d[j] = bad ? NAN : (float)(scale * (p - q));
    }
}

// --------------------------------------------------------------------------------------------------------------- top-k
struct TopKs {
    int k[8];
};

__global__ void zero_i32_kernel(int* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0;
}

// rank_b = #{j: z_j > z_t} + #{j < t: z_j == z_t}; N for a row that holds a NaN or whose label is outside [0, N)
__global__ __launch_bounds__(kThreads) void topk_rows_kernel(const float* __restrict__ logits, int ldl, const long long* __restrict__ target,
                                                             int N, TopKs ks, int nk, int* __restrict__ correct, int* __restrict__ rank) {
    __shared__ int lds[2 * kWaves];
    const int b = blockIdx.x;
    const long long t = target[b];
    const bool in_range = t >= 0 && t < N;
    const float* z = logits + (size_t)b * ldl;
    const float zt = in_range ? z[t] : 0.0f;              // (read only after the bounds check)
    int ahead = 0, has_nan = 0;
    for (int j = threadIdx.x; j < N; j += kThreads) {
        const float v = z[j];
        ahead += (v > zt || (v == zt && (long long)j < t)) ? 1 : 0;
        has_nan |= (v != v) ? 1 : 0;
    }
    ahead = block_sum(ahead, lds);
    has_nan = block_sum(has_nan, lds + kWaves);
    if (threadIdx.x == 0) {
        const int r = (in_range && has_nan == 0) ? ahead : N;
        if (rank) rank[b] = r;
        for (int i = 0; i < nk; ++i)
            if (r < ks.k[i]) atomicAdd(correct + i, 1);
    }
}

}  // namespace

extern "C" {

int y4_avgpool_global_fwd_f32(const float* x, int ldx, float* y, int ldy, int B, int HW, int C, void* stream) {
    if (!x || !y) return Y4_ERR_NULL;
    if (B < 1 || HW < 1 || C < 1 || ldx < C || ldy < C || B > 65535) return Y4_ERR_SHAPE;
    const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);
    const int per_block = 64 * (vec ? 4 : 1);
    const dim3 grid((C + per_block - 1) / per_block, B);
    if (vec)
        hipLaunchKernelGGL(avgpool_fwd_kernel<4>, grid, dim3(kThreads), 0, y4_stream(stream), x, ldx, y, ldy, HW, C);
    else
        hipLaunchKernelGGL(avgpool_fwd_kernel<1>, grid, dim3(kThreads), 0, y4_stream(stream), x, ldx, y, ldy, HW, C);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_avgpool_global_bwd_f32(const float* dy, int lddy, float* dx, int lddx, int B, int HW, int C, void* stream) {
    if (!dy || !dx) return Y4_ERR_NULL;
    if (B < 1 || HW < 1 || C < 1 || lddy < C || lddx < C) return Y4_ERR_SHAPE;
    const bool vec = C % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && aligned16(dy) && aligned16(dx);
    const int CV = vec ? C / 4 : C;
    const long long total = (long long)B * HW * CV;
    const long long want = (total + kThreads - 1) / kThreads;
    const int blocks = (int)(want < 8192 ? want : 8192);
    if (vec)
        hipLaunchKernelGGL(avgpool_bwd_kernel<4>, dim3(blocks), dim3(kThreads), 0, y4_stream(stream), dy, lddy, dx, lddx, total, HW, CV);
    else
        hipLaunchKernelGGL(avgpool_bwd_kernel<1>, dim3(blocks), dim3(kThreads), 0, y4_stream(stream), dy, lddy, dx, lddx, total, HW, CV);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

static bool gemm_dims_ok(int M, int K, int N) {
    // (grid.y carries a 64-row tile index)
    return M >= 1 && K >= 1 && N >= 1 && M <= 65535 * kTile && K <= 65535 * kTile && N <= 65535 * kTile;
}

int y4_linear_fwd_f32(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int M, int K, int N, void* stream) {
    if (!x || !w || !y) return Y4_ERR_NULL;
    if (!gemm_dims_ok(M, K, N) || ldx < K || ldy < N) return Y4_ERR_SHAPE;
    // y[m][n] = sum_k x[m][k] w[n][k] + bias[n]
    return launch_gemm<true, true>(x, ldx, 1, w, K, 1, bias, y, ldy, M, N, K, y4_stream(stream));
}

int y4_linear_bwd_f32(const float* x, int ldx, const float* w, const float* dy, int lddy, float* dx, int lddx, float* dw, float* dbias,
                      int M, int K, int N, void* stream) {
    if (!dy || (!dx && !dw && !dbias) || (dx && !w) || (dw && !x)) return Y4_ERR_NULL;
    if (!gemm_dims_ok(M, K, N) || lddy < N || (dx && lddx < K) || (dw && ldx < K)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    if (dx) {          // dx[m][k] = sum_n dy[m][n] w[n][k]
        const int rc = launch_gemm<true, false>(dy, lddy, 1, w, 1, K, nullptr, dx, lddx, M, K, N, st);
        if (rc != Y4_OK) return rc;
    }
    if (dw) {          // dw[n][k] = sum_m dy[m][n] x[m][k]: the whole M range inside one block, nothing to combine
        const int rc = launch_gemm<false, false>(dy, 1, lddy, x, 1, ldx, nullptr, dw, K, N, K, M, st);
        if (rc != Y4_OK) return rc;
    }
    if (dbias) {
        hipLaunchKernelGGL(colsum_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, dy, lddy, dbias, M, N);
        Y4_CHECK_LAUNCH();
    }
    return Y4_OK;
}

int y4_ce_smooth_fwd_f32(const float* logits, int ldl, const long long* target, int B, int N, double smoothing, float* row_loss,
                         double* loss_out, void* stream) {
    if (!logits || !target || !row_loss || !loss_out) return Y4_ERR_NULL;
    if (B < 1 || N < 1 || ldl < N || !(smoothing >= 0.0 && smoothing <= 1.0)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(ce_fwd_rows_kernel, dim3(B), dim3(kThreads), 0, st, logits, ldl, target, N, smoothing, row_loss);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(kThreads), 0, st, row_loss, target, B, loss_out);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_ce_smooth_bwd_f32(const float* logits, int ldl, const long long* target, const double* loss_out, const float* gscale,
                         float* dlogits, int lddl, int B, int N, double smoothing, void* stream) {
    if (!logits || !target || !loss_out || !gscale || !dlogits) return Y4_ERR_NULL;
    if (B < 1 || N < 1 || ldl < N || lddl < N || !(smoothing >= 0.0 && smoothing <= 1.0)) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(B), dim3(kThreads), 0, y4_stream(stream), logits, ldl, target, loss_out, gscale, dlogits,
                       lddl, N, smoothing);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_topk_correct_f32(const float* logits, int ldl, const long long* target, int B, int N, const int* ks_host, int nk, int* correct,
                        int* rank, void* stream) {
    if (!logits || !target || !ks_host || !correct) return Y4_ERR_NULL;
    if (B < 1 || N < 1 || ldl < N || nk < 1 || nk > 8) return Y4_ERR_SHAPE;
    TopKs ks;
    for (int i = 0; i < 8; ++i) ks.k[i] = i < nk ? ks_host[i] : 0;
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(zero_i32_kernel, dim3(1), dim3(64), 0, st, correct, nk);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(topk_rows_kernel, dim3(B), dim3(kThreads), 0, st, logits, ldl, target, N, ks, nk, correct, rank);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

}  // extern "C"
