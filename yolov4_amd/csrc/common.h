// Shared device helpers for libyolov4_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yolov4_amd.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define Y4_CHECK_LAUNCH()                                   \
    do {                                                    \
        if (hipGetLastError() != hipSuccess) return Y4_ERR_LAUNCH; \
    } while (0)

static inline hipStream_t y4_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: one flag word per launcher
// instantiation, bit d = "set on device d" (devices >= 64: set on every launch).  Two threads racing through their first
// launch both set the attribute, which is idempotent.
#include <atomic>
struct Y4DynLds {
    std::atomic<unsigned long long> done{0ull};
    bool ensure(const void* kernel, size_t bytes) {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) return false;
        if (d >= 0 && d < 64 && ((done.load(std::memory_order_acquire) >> d) & 1ull)) return true;
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
        if (d >= 0 && d < 64) done.fetch_or(1ull << d, std::memory_order_release);
        return true;
    }
};

// darknet/darknet.py:14-20: x * tanh(softplus(x)).  With n = e^x:
// tanh(log(1+n)) = ((1+n)^2-1)/((1+n)^2+1) = n(n+2)/(n(n+2)+2); softplus threshold 20 of
// torch (returns x above it) coincides with the ratio being exactly 1.0f there.
// One v_exp_f32 + one v_rcp_f32 (both ~1 ulp): these kernels are HBM-bound only if the
// activation costs a handful of VALU ops per element.
//
// n = e^min(x, 20).  v_exp_f32 flushes a denormal RESULT to zero, so below x = -87.34 (e^x < 2^-126) n is 0 and Mish and its
// derivative come out as -0 / 0 where they are x e^x and (1 + x) e^x: up to 1.2e-36 in magnitude, 100 times the smallest
// normal number.  DENORM = true raises the exponent by 64 below 2^-126 and scales the result back (both exact: powers of two;
// the same bits as DENORM = false everywhere else) for five more VALU operations.  The flat activation kernels take it; the
// fused epilogues and the BatchNorm sweeps, which have no VALU operation to spare, keep the flush and with it an ABSOLUTE
// error of at most 1.2e-36 for pre-activations in [-103.3, -87.34].
template <bool DENORM = false> __device__ __forceinline__ float y4_mish_exp(float x) {
    if constexpr (!DENORM) return __expf(fminf(x, 20.0f));
    const float t = fminf(x, 20.0f) * 1.44269504088896341f;              // as __expf: 2^(x log2 e)
    const bool low = t < -126.0f;
    return __builtin_amdgcn_exp2f(low ? t + 64.0f : t) * (low ? 0x1p-64f : 1.0f);
}
template <bool DENORM = false> __device__ __forceinline__ float y4_mish(float x) {
    const float n = y4_mish_exp<DENORM>(x);
    const float w = n * (n + 2.0f);
    return x * (w * __frcp_rn(w + 2.0f));
}
// d/dx [x * t(x)], t = tanh(softplus(x)):  t + x * (1 - t^2) * sigmoid(x).  With w = n(n + 2), d = w + 2:
// t = w / d, 1 - t^2 = 4 (w + 1) / d^2 = 4 (n + 1)^2 / d^2, sigmoid = n / (n + 1)  =>  (1 - t^2) sigmoid = 4 n (n + 1) / d^2,
// so the derivative is (w + 4 x n (n + 1) / d) / d: ONE v_rcp_f32 beside the v_exp_f32 (no cancellation: every term but x
// is positive).  The BatchNorm backward sweeps evaluate this twice per element and run close to the VALU rate with it.
// Above the clamp n stays e^20 while x grows: the second term would read 4 x / n^2 instead of 4 x e^-2x -- 1.7 at
// x = 1e17, +inf from 1.45e21 on (and then NaN for a zero upstream gradient) -- where the derivative is 1 to 4e-16.  Hence
// the select; a NaN compares false and takes the formula's NaN.
template <bool DENORM = false> __device__ __forceinline__ float y4_mish_grad(float x) {
    const float n = y4_mish_exp<DENORM>(x);
    const float w = n * (n + 2.0f);
    const float rd = __frcp_rn(w + 2.0f);
    const float q = fmaf(n, n, n);                         // n (n + 1)
    const float d = fmaf(4.0f * (x * q), rd, w) * rd;
    return x > 20.0f ? 1.0f : d;
}
template <bool DENORM = false> __device__ __forceinline__ float y4_act(float x, int act) {
    switch (act) {
        case Y4_ACT_LEAKY: return x > 0.0f ? x : 0.1f * x;
        case Y4_ACT_MISH: return y4_mish<DENORM>(x);
        case Y4_ACT_RELU: return x < 0.0f ? 0.0f : x;      // (not fmaxf: a NaN stays a NaN, as in torch)
        default: return x;
    }
}
template <bool DENORM = false> __device__ __forceinline__ float y4_act_grad(float x, int act) {
    switch (act) {
        case Y4_ACT_LEAKY: return x > 0.0f ? 1.0f : 0.1f;
        case Y4_ACT_MISH: return y4_mish_grad<DENORM>(x);
        case Y4_ACT_RELU: return x > 0.0f ? 1.0f : 0.0f;
        default: return 1.0f;
    }
}

// the same with the activation a compile-time constant (the BatchNorm sweeps: no branch per element, full unrolling)
template <int ACT> __device__ __forceinline__ float y4_act_t(float x) {
    if constexpr (ACT == Y4_ACT_LEAKY) return x > 0.0f ? x : 0.1f * x;
    else if constexpr (ACT == Y4_ACT_MISH) return y4_mish(x);
    else if constexpr (ACT == Y4_ACT_RELU) return x < 0.0f ? 0.0f : x;
    else return x;
}
template <int ACT> __device__ __forceinline__ float y4_act_grad_t(float x) {
    if constexpr (ACT == Y4_ACT_LEAKY) return x > 0.0f ? 1.0f : 0.1f;
    else if constexpr (ACT == Y4_ACT_MISH) return y4_mish_grad(x);
    else if constexpr (ACT == Y4_ACT_RELU) return x > 0.0f ? 1.0f : 0.0f;
    else return 1.0f;
}

// XCD-aware block remap (MI355X: 8 XCDs, blocks dealt round-robin, private L2 each): give every
// XCD a contiguous chunk of the logical tile sequence so neighbouring tiles (shared halo rows /
// shared filter panels) hit the same L2.  Bijective for any nwg (guide §5 "XCD swizzle").
__device__ __forceinline__ int y4_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// Raw buffer loads (SRD in SGPRs, 32-bit byte offsets): an offset >= num_bytes returns zeros in
// hardware, which replaces both the branch around a masked load and the select on its result.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t y4_make_rsrc(const void* base, unsigned num_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)num_bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 y4_buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff_bytes, (int)soff_bytes, 0);
    return __builtin_bit_cast(f32x4, v);
}

// ---- the bf16x3 split (conv_igemm.hip, conv_stem.hip, stem_fused.hip): an fp32 value as the exact sum of three truncated bf16 pieces
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// pack the upper halves (= truncated bf16) of two fp32 words: result = {hi16(x1), hi16(x0)}
__device__ __forceinline__ unsigned pack_hi16(unsigned x1, unsigned x0) { return __builtin_amdgcn_perm(x1, x0, 0x07060302u); }
__device__ __forceinline__ void split3x4(const f32x4 v, u32x2& p1, u32x2& p2, u32x2& p3) {
    unsigned h1[4], h2[4], h3[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h1[e] = __float_as_uint(v[e]);
        const float r1 = v[e] - __uint_as_float(h1[e] & 0xffff0000u);     // exact
        h2[e] = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(h2[e] & 0xffff0000u);       // exact, <= 8 significant bits left
        h3[e] = __float_as_uint(r2);
    }
    p1[0] = pack_hi16(h1[1], h1[0]); p1[1] = pack_hi16(h1[3], h1[2]);
    p2[0] = pack_hi16(h2[1], h2[0]); p2[1] = pack_hi16(h2[3], h2[2]);
    p3[0] = pack_hi16(h3[1], h3[0]); p3[1] = pack_hi16(h3[3], h3[2]);
}

// ---- optional by-product of the sweeps that PRODUCE a conv operand (pointwise.hip, stem_fused.hip): bit pattern of
// max|finite output| folded into *out with an integer atomicMax (order independent); conv mode 3 ("f16x2") scales its
// operands by it
__device__ __forceinline__ void amax_track1(unsigned& m, const float o) {
    const unsigned b = __float_as_uint(o) & 0x7fffffffu;
    if (b < 0x7f800000u && b > m) m = b;
}
__device__ __forceinline__ void amax_track(unsigned& m, const f32x4 o) {
#pragma unroll
    for (int e = 0; e < 4; ++e) amax_track1(m, o[e]);
}
// (blocks of 256 threads, every thread calls it)
__device__ __forceinline__ void amax_commit(unsigned m, unsigned* out) {
    // waves folded through LDS, ONE atomic per block, and only when it would raise the word (it only grows; a stale
    // read merely costs an atomic).  Per-wave atomics on one address serialised: +150 us per BatchNorm sweep, measured.
    __shared__ unsigned wmax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = wmax[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) v = wmax[w] > v ? wmax[w] : v;
        if (v > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, v);
    }
}

// ---- host-side pieces other translation units launch for stem_fused.hip
namespace y4 {
// pointwise.hip: per-block rows part[nparts][2][C] of (sum g, sum g xhat) -> dbeta, dgamma and the fp64 words acc[2C] at the
// head of `workspace` (y4_bn_finalize_workspace(C) bytes), fixed order
int bn_bwd_fold_finalize(const float* part, long long nparts, long long M, int C, void* workspace, float* dgamma, float* dbeta,
                         const float* gamma, const float* invstd, hipStream_t st);
// pointwise.hip: reduce (with the bound words [0..4] of the 6 zeroed words `bounds`), fold and finalize of the BatchNorm backward
// over dz, y -> dbeta, dgamma and the fp64 words acc[2C] at the head of `workspace` (y4_bn_workspace(M, C) bytes)
int bn_bwd_reduce_finalize_bounds(const float* dz, int lddz, const float* y, int ldy, const float* mean, const float* invstd,
                                  const float* gamma, const float* beta, int act, long long M, int C, void* workspace,
                                  float* dgamma, float* dbeta, unsigned* bounds, hipStream_t st);
// conv_stem.hip: per-wave slabs [nslabs][32 n][32 j] -> dw[Cout][27] through part[64][1024] doubles, fixed order
int stem_wgrad_fold(const float* slabs, int nslabs, double* part, float* dw, int Cout, hipStream_t st);
}  // namespace y4
