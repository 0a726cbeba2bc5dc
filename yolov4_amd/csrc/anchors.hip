// Anchor fitting on label shapes (Darknet's `detector calc_anchors`, the evolution stage of YOLOv5's autoanchor) as two
// kernels: the assignment pass of one Lloyd iteration, and the fitness of many candidate anchor sets in one launch.
// The shape IoU is the loss's (yolo_loss.hip, yolo_assign_kernel): fp32, unfused (this file is built with
// -ffp-contract=off), IEEE division, first maximum wins.  Every sum is a sum of int64 fixed-point values (w, h: 2^-16;
// IoU: 2^-30), so the results do not depend on block shape or arrival order.  Semantics: include/yolov4_amd.h, DESIGN.md §20.
#include "common.h"

namespace {

constexpr int kMaxA = 32;              // anchors per set
constexpr int kMaxN = 1 << 24;         // shapes
constexpr int kMaxG = 65535;           // candidate sets per launch
constexpr int kThreads = 256;
constexpr int kAssignBlocks = 512;     // grid cap of the assignment pass (blocks stride over the shapes)
constexpr int kSpt = 8;                // fitness: shapes a thread keeps in registers
constexpr int kTile = kThreads * kSpt; // fitness: shapes of one tile
constexpr int kGc = 8;                 // fitness: candidate sets per block (their anchors: 8 * 32 * 16 B = 4 KB of LDS)
constexpr int kFitBlocks = 8192;       // fitness: aimed-at number of blocks; beyond it blocks stride over the tiles

typedef unsigned long long u64;

__device__ __forceinline__ float shape_iou(float tw, float th, float tarea, float aw, float ah, float aarea) {
    const float brx = fminf(tw, aw), bry = fminf(th, ah);
    const float ai = brx * bry;
    return ai / ((tarea + aarea) - ai);
}
__device__ __forceinline__ long long q16(float v) { return (long long)rint((double)v * 65536.0); }
__device__ __forceinline__ long long q30(float v) { return (long long)rint((double)v * 1073741824.0); }

// One Lloyd assignment pass.  acc[a] = (count, sum qw, sum qh, sum qiou, hits).  The three sums are keyed by the lane's own
// arg-max, so they go to the block's LDS table by 64-bit LDS adds; count and hits are wave ballots, one LDS add per wave
// and anchor.  One global add per non-zero table entry per block.
__global__ __launch_bounds__(kThreads) void anchor_assign_kernel(const float2* __restrict__ wh, int N,
                                                                 const float2* __restrict__ anchors, int A, float iou_thresh,
                                                                 unsigned char* __restrict__ assign,
                                                                 float* __restrict__ best_iou, u64* __restrict__ acc) {
    __shared__ float4 s_a[kMaxA];                         // (w, h, w * h, -)
    __shared__ u64 s_acc[kMaxA * 5];
    const int tid = threadIdx.x;
    if (tid < A) {
        const float2 a = anchors[tid];
        s_a[tid] = make_float4(a.x, a.y, a.x * a.y, 0.f);
    }
    if (tid < A * 5) s_acc[tid] = 0ull;
    __syncthreads();
    const int rounds = (N + kThreads * (int)gridDim.x - 1) / (kThreads * (int)gridDim.x);   // the same for every lane: ballots
    for (int r = 0; r < rounds; ++r) {
        const int i = (r * (int)gridDim.x + (int)blockIdx.x) * kThreads + tid;
        const bool valid = i < N;
        int best = -1;
        unsigned hit = 0u;
        if (valid) {
            const float2 t = wh[i];
            const float tarea = t.x * t.y;
            float bi = -1.0f;
            for (int k = 0; k < A; ++k) {
                const float4 a = s_a[k];
                const float iou = shape_iou(t.x, t.y, tarea, a.x, a.y, a.z);
                if (iou > bi) { bi = iou; best = k; }     // strict: the first maximum stays
                hit |= (iou > iou_thresh ? 1u : 0u) << k;
            }
            hit |= 1u << best;
            if (assign) assign[i] = (unsigned char)best;
            if (best_iou) best_iou[i] = bi;
            atomicAdd(&s_acc[best * 5 + 1], (u64)q16(t.x));
            atomicAdd(&s_acc[best * 5 + 2], (u64)q16(t.y));
            atomicAdd(&s_acc[best * 5 + 3], (u64)q30(bi));
        }
        for (int k = 0; k < A; ++k) {
            const u64 mb = __ballot(best == k), mh = __ballot((hit >> k) & 1u);
            if ((tid & 63) == 0) {
                if (mb) atomicAdd(&s_acc[k * 5 + 0], (u64)__popcll(mb));
                if (mh) atomicAdd(&s_acc[k * 5 + 4], (u64)__popcll(mh));
            }
        }
    }
    __syncthreads();
    if (tid < A * 5) {
        const u64 v = s_acc[tid];
        if (v) atomicAdd(&acc[tid], v);
    }
}

// Fitness of G candidate sets.  Block (x, y) takes the candidates [y * kGc, y * kGc + kGc) -- their anchors sit in LDS --
// and the tiles x, x + gridDim.x, ...: a thread loads its kSpt shapes of a tile once and scores them against every candidate
// of the block.  Per (tile, candidate) a thread's sum of qiou (< 2^34) and its count of shapes above thr (<= 8) travel as
// ONE 64-bit word, count << 48 | sum, through the wave reduction (the wave's sum stays below 2^40), then one LDS add per
// wave; one global add per non-zero entry per block.
__global__ __launch_bounds__(kThreads) void anchor_fitness_kernel(const float2* __restrict__ wh, int N,
                                                                  const float2* __restrict__ cand, int G, int A, float thr,
                                                                  int tiles, u64* __restrict__ out) {
    __shared__ float4 s_c[kGc * kMaxA];
    __shared__ u64 s_out[kGc * 2];
    const int tid = threadIdx.x;
    const int g0 = (int)blockIdx.y * kGc;
    const int ng = min(kGc, G - g0);
    for (int j = tid; j < ng * A; j += kThreads) {
        const float2 a = cand[(size_t)g0 * A + j];
        s_c[j] = make_float4(a.x, a.y, a.x * a.y, 0.f);
    }
    if (tid < kGc * 2) s_out[tid] = 0ull;
    __syncthreads();
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        float tw[kSpt], th[kSpt], ta[kSpt];
        bool ok[kSpt];
#pragma unroll
        for (int s = 0; s < kSpt; ++s) {
            const int i = tile * kTile + s * kThreads + tid;
            ok[s] = i < N;
            const float2 t = ok[s] ? wh[i] : make_float2(1.f, 1.f);
            tw[s] = t.x;
            th[s] = t.y;
            ta[s] = t.x * t.y;
        }
        for (int g = 0; g < ng; ++g) {
            float bi[kSpt];
#pragma unroll
            for (int s = 0; s < kSpt; ++s) bi[s] = -1.0f;
            for (int k = 0; k < A; ++k) {
                const float4 a = s_c[g * A + k];
#pragma unroll
                for (int s = 0; s < kSpt; ++s) bi[s] = fmaxf(bi[s], shape_iou(tw[s], th[s], ta[s], a.x, a.y, a.z));
            }
            u64 v = 0ull;
#pragma unroll
            for (int s = 0; s < kSpt; ++s)
                if (ok[s]) v += (u64)q30(bi[s]) + ((bi[s] > thr ? 1ull : 0ull) << 48);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += (u64)__shfl_xor((long long)v, off, 64);
            if ((tid & 63) == 0) {
                const u64 sum = v & ((1ull << 48) - 1ull), cnt = v >> 48;
                if (sum) atomicAdd(&s_out[g * 2], sum);
                if (cnt) atomicAdd(&s_out[g * 2 + 1], cnt);
            }
        }
    }
    __syncthreads();
    if (tid < ng * 2) {
        const u64 v = s_out[tid];
        if (v) atomicAdd(&out[(size_t)g0 * 2 + tid], v);
    }
}

// (w, h) pairs are loaded as 8-byte words, the tables are 64-bit words
bool misaligned8(const void* a, const void* b, const void* c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 7u) != 0;
}

}  // namespace

extern "C" int y4_anchor_assign_f32(const float* wh, int N, const float* anchors, int A, float iou_thresh,
                                    unsigned char* assign, float* best_iou, long long* acc, void* stream) {
    if (!wh || !anchors || !acc) return Y4_ERR_NULL;
    if (N < 1 || N > kMaxN || A < 1 || A > kMaxA || misaligned8(wh, anchors, acc)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    if (hipMemsetAsync(acc, 0, (size_t)A * 5 * sizeof(long long), st) != hipSuccess) return Y4_ERR_LAUNCH;
    const int blocks = min((N + kThreads - 1) / kThreads, kAssignBlocks);
    hipLaunchKernelGGL(anchor_assign_kernel, dim3(blocks), dim3(kThreads), 0, st, reinterpret_cast<const float2*>(wh), N,
                       reinterpret_cast<const float2*>(anchors), A, iou_thresh, assign, best_iou, reinterpret_cast<u64*>(acc));
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_anchor_fitness_f32(const float* wh, int N, const float* cand, int G, int A, float thr, long long* out,
                                     void* stream) {
    if (!wh || !cand || !out) return Y4_ERR_NULL;
    if (N < 1 || N > kMaxN || A < 1 || A > kMaxA || G < 1 || G > kMaxG || misaligned8(wh, cand, out)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    if (hipMemsetAsync(out, 0, (size_t)G * 2 * sizeof(long long), st) != hipSuccess) return Y4_ERR_LAUNCH;
    const int tiles = (N + kTile - 1) / kTile;
    const int chunks = (G + kGc - 1) / kGc;
    const int bx = min(tiles, max(1, kFitBlocks / chunks));
    hipLaunchKernelGGL(anchor_fitness_kernel, dim3(bx, chunks), dim3(kThreads), 0, st, reinterpret_cast<const float2*>(wh), N,
                       reinterpret_cast<const float2*>(cand), G, A, thr, tiles, reinterpret_cast<u64*>(out));
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
