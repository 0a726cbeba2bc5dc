// The two-piece fp16 operand split ("f16x2", conv mode 3) as the register-staged kernels form it: the power-of-two operand
// scale, the split itself and the swizzled LDS row image (conv_f16x2.hip, conv1x1_bwd_fused.hip).
#pragma once
#include "common.h"

namespace y4x2 {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

// ---- operand scale: power of two s with max|T| * s in [2^14, 2^15); amax_bits = bit pattern of max|finite x|
__device__ __host__ __forceinline__ unsigned f16x2_scale_exp(unsigned amax_bits) {
    const unsigned e = (amax_bits >> 23) & 0xffu;
    if (e == 0u || e == 255u) return 127u;                 // all-zero / subnormal / unknown tensor: s = 1
    int se = 268 - (int)e;                                 // 127 + 14 - (e - 127)
    if (se < 2) se = 2;
    if (se > 252) se = 252;
    return (unsigned)se;
}
__device__ __forceinline__ float f16x2_scale(const unsigned* amax) {
    return __uint_as_float(f16x2_scale_exp(amax ? *amax : 0u) << 23);
}
__device__ __forceinline__ float f16x2_unscale(const unsigned* amax) {
    return __uint_as_float((254u - f16x2_scale_exp(amax ? *amax : 0u)) << 23);
}

// 4 consecutive fp32 values -> 4 hi halfs (hi[0..1]) and 4 scaled lo halfs.
// Y4_SPLIT_ASM=1 (off by default) replaces the compiler's 3.5 VALU per element (two of them packed-fp32 ops) by 3 on the
// mixed-precision fma unit (v_fma_mixlo/mixhi_f16 scale + round + pack in one instruction, v_fma_mix_f32 forms x s - hi
// with the fp16 half as an operand).  Measured A/B on one box, whole step: 357-359 img/s with it, 360 without -- the
// split VALU is not what bounds these kernels -- and fragments that go from the asm block straight into an MFMA (the
// streaming 1x1 kernel) would need manual wait states (hipcc pads nothing after inline asm).  Kept for the record.
#ifndef Y4_SPLIT_ASM
#define Y4_SPLIT_ASM 0
#endif
__device__ __forceinline__ void split2_pair(const float x0, const float x1, const float s, unsigned& hi, unsigned& lo) {
#if Y4_SPLIT_ASM
    unsigned h, l;
    float r0, r1;
    asm("v_fma_mixlo_f16 %0, %4, %6, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %5, %6, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mix_f32 %2, %4, %6, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mix_f32 %3, %5, %6, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %1, %2, %7, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %3, %7, 0 op_sel_hi:[0,0,0]"
        : "=&v"(h), "=&v"(l), "=&v"(r0), "=&v"(r1)
        : "v"(x0), "v"(x1), "v"(s), "v"(2048.0f));
    hi = h; lo = l;
#else
    f16x2v h, l;
    const float t0 = x0 * s, t1 = x1 * s;
    h[0] = (_Float16)t0; h[1] = (_Float16)t1;
    l[0] = (_Float16)((t0 - (float)h[0]) * 2048.f); l[1] = (_Float16)((t1 - (float)h[1]) * 2048.f);
    hi = __builtin_bit_cast(unsigned, h); lo = __builtin_bit_cast(unsigned, l);
#endif
}
__device__ __forceinline__ void split2x4(const f32x4 v, const float s, u32x2& hi, u32x2& lo) {
    unsigned h0, l0, h1, l1;
    split2_pair(v[0], v[1], s, h0, l0);
    split2_pair(v[2], v[3], s, h1, l1);
    hi[0] = h0; hi[1] = h1; lo[0] = l0; lo[1] = l1;
}
__device__ __forceinline__ void split2(const float x, const float s, unsigned short& hi, unsigned short& lo) {
    const float xs = x * s;
    const _Float16 h = (_Float16)xs;
    const _Float16 l = (_Float16)((xs - (float)h) * 2048.f);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}

// ---- LDS image: rows of 32 fp16 (64 B = four 16-B chunks), unpadded.  Chunk c of row r lives at chunk c ^ swz(r).
//   32x32x16: a 16-lane ds_read_b128 group reads 16 rows (r mod 4 each residue 4 times) at one chunk: XOR with
//             (r >> 2) & 3 spreads every residue class over the four chunks.
//   16x16x32: a group reads rows {0-3,12-15} at chunk q and rows {4-11} at chunk q ^ 1 (or the mirrored set):
//             XOR with g[(r >> 2) & 3], g = {0, 2, 3, 1}, makes the 16 (residue, chunk) slots distinct.
template <int MS>
__device__ __forceinline__ int lds_swz(int row) {
    const int q = (row >> 2) & 3;
    if constexpr (MS == 32) return q;
    else return (0x78 >> (2 * q)) & 3;                     // {0, 2, 3, 1}[q] packed two bits each: 0b01'11'10'00
}

constexpr int ROWB = 64;                                   // bytes per LDS row (32 fp16)

}  // namespace y4x2
