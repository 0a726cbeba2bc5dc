// What the two resized-crop gather kernels of the classifier's input pipeline share: the fp32 gather of resample.hip
// (y4_rcrop_u8_f32) and the uint8 gather in front of RandAugment (randaug.hip).  Their common body is rcrop_gather_body.inc;
// both compute the same pixels and differ in the store alone (and the uint8 one knows no paste).  See resample.hip for the
// shape of the gather and include/yolov4_amd.h for the arithmetic.  Include only from translation units compiled with
// -ffp-contract=off.
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"

namespace y4 {
struct rc_norm {
    float mean[3], std[3];
};
}  // namespace y4

namespace {

using y4::rc_norm;

constexpr int kTileX = 64;          // output columns per block = threads per block (one wave)
constexpr int kTileY = 6;           // output rows per block: 18 int32 accumulators per thread (6 beat 4, 8, 12, 16)
constexpr int kPrecBits = 22;       // Pillow's PRECISION_BITS for 8-bit pixels (32 - 8 - 2)
constexpr int kMaxSide = 65535;

// taps per output index of one axis: Pillow's ksize for the bilinear filter (support 1.0)
__host__ __device__ inline int rc_ksize(int in, int out) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(fs) * 2 + 1;
}
// int32 words of one axis' table: bounds[S][2], then k[S][ksize]
__host__ __device__ inline long long rc_axis_words(int S, int ksize) { return (long long)S * (2 + ksize); }

__device__ __forceinline__ int rc_clip8(int v) {
    v >>= kPrecBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace

// host-side pieces of resample.hip that randaug.hip calls
namespace y4 {
// every check of y4_rcrop_u8_f32 that concerns the job table and its workspace; nothing may be launched unless Y4_OK
int rcrop_check(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, const void* workspace, size_t ws_bytes);
// mean / std into `nm`; Y4_ERR_SHAPE for a value that is not finite or a zero std
int rcrop_norm(const float* mean3_host, const float* std3_host, rc_norm* nm);
void rcrop_launch_coeffs(const y4_rcrop_job* jobs_dev, int n, int S, void* workspace, hipStream_t st);
void rcrop_launch_gather_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, const void* workspace,
                             const rc_norm& nm, float* dst, long long dsb, long long dsc, long long dsh, long long dsw,
                             hipStream_t st);
}  // namespace y4
