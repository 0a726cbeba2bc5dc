// The classifier's input pipeline (reference: darknet/main_amp.py:205-332 -- RandomResizedCrop + RandomHorizontalFlip for
// training, Resize + CenterCrop for validation, uint8 collate, float().sub_(mean).div_(std)), fused into ONE gather per batch:
// crop, Pillow's antialiased bilinear resample of the crop to res_h x res_w, an S x S window of that image, horizontal flip,
// CutMix paste and the normalisation.  No crop image, resized image or uint8 batch is materialised.
// The arithmetic restates Pillow's Image.crop(box).resize((res_w, res_h), Image.BILINEAR) for 8-bit RGB (libImaging
// Resample.c: precompute_coeffs in double, normalize_coeffs_8bpc to 22 fractional bits, the horizontal pass stored as uint8,
// then the vertical pass); see include/yolov4_amd.h for the exact statement.  Compiled with -ffp-contract=off.
//
// Two launches: the coefficient tables of the window's S columns and S rows of every job (one thread per entry, fp64), then
// the gather.  Gather shape: a block owns a tile of kTileX output columns x kTileY output rows of one sample; a thread owns
// one output column and keeps the tile's kTileY x 3 row accumulators in registers.  The block walks the source rows the tile
// needs ONCE: each thread forms the horizontal result of that row for its column (a tap loop of the table's length, no
// fixed ksize), rounds it to 8 bits as Pillow stores it, and adds it into every accumulator whose vertical window holds the
// row (block-uniform tests and scalar coefficient loads).  A horizontal result is thus computed once per output column and
// source row of a tile, not once per output row.  No LDS, no MFMA; byte loads, int32 multiply-adds, coalesced plane stores.
// CutMix: a batch with a paste doubles the grid's z; the second half writes, inside each sample's rectangle, the pixels its
// partner's record and tables give at the same place, the first half everything outside it.
// The gather's body lives in rcrop_gather_body.inc: randaug.hip compiles the same text with a uint8 store for RandAugment.
#include "rcrop_gather.h"

namespace {

size_t rc_job_bytes(const y4_rcrop_job& j, int S) {
    const long long words = rc_axis_words(S, rc_ksize(j.crop_w, j.res_w)) + rc_axis_words(S, rc_ksize(j.crop_h, j.res_h));
    return ((size_t)words * 4 + 15) & ~(size_t)15;
}

__device__ __forceinline__ double rc_tap(int x, int xmin, double center, double ss) {
    double v = (x + xmin - center + 0.5) * ss;
    if (v < 0.0) v = -v;
    return v < 1.0 ? 1.0 - v : 0.0;
}

// one thread per (job, axis, window index): bounds and the 22-bit taps of resized index win + i
__global__ void __launch_bounds__(256)
rcrop_coeffs_kernel(const y4_rcrop_job* __restrict__ jobs, int S, int* __restrict__ ws) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const int axis = blockIdx.y;
    const y4_rcrop_job jb = jobs[blockIdx.z];
    const int in = axis ? jb.crop_h : jb.crop_w, out = axis ? jb.res_h : jb.res_w, win = axis ? jb.win_y : jb.win_x;
    const int ks = rc_ksize(in, out);
    int* base = ws + jb.ws_offset / 4 + (axis ? rc_axis_words(S, rc_ksize(jb.crop_w, jb.res_w)) : 0ll);
    int* k = base + 2ll * S + (long long)i * ks;

    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = ((win + i) + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int n = xmax - xmin;
    n = n < 0 ? 0 : (n > ks ? ks : n);          // (never taken: 2 support + 1 <= ksize; keeps every store inside the row)
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += rc_tap(x, xmin, center, ss);
    for (int x = 0; x < ks; ++x) {
        int v = 0;
        if (x < n) {
            double w = rc_tap(x, xmin, center, ss);
            if (ww != 0.0) w = w / ww;
            v = (int)(0.5 + w * 4194304.0);
        }
        k[x] = v;
    }
    base[2ll * i] = xmin;
    base[2ll * i + 1] = n;
}

__global__ void __launch_bounds__(kTileX)
rcrop_gather_kernel(const y4_rcrop_job* __restrict__ jobs, int n, int S, const int* __restrict__ ws, rc_norm nm,
                    float* __restrict__ dst, long long dsb, long long dsc, long long dsh, long long dsw) {
#define RC_GATHER_U8 0
#include "rcrop_gather_body.inc"
#undef RC_GATHER_U8
}

}  // namespace

// every check of the entry points that concerns the job table; nothing is launched unless this returns Y4_OK
int y4::rcrop_check(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs, int n, int S, const void* workspace,
                    size_t ws_bytes) {
    if (!jobs_dev || !jobs || !workspace) return Y4_ERR_NULL;
    if (n < 1 || n > 65535 || S < 1 || S > kMaxSide) return Y4_ERR_SHAPE;
    for (int i = 0; i < n; ++i) {
        const y4_rcrop_job& j = jobs[i];
        if (!j.src) return Y4_ERR_NULL;
        if (j.src_h < 1 || j.src_w < 1 || j.src_h > kMaxSide || j.src_w > kMaxSide || j.src_pitch < 3ll * j.src_w)
            return Y4_ERR_SHAPE;
        if (j.crop_w < 1 || j.crop_h < 1 || j.crop_x < 0 || j.crop_y < 0 || j.crop_x > j.src_w - j.crop_w ||
            j.crop_y > j.src_h - j.crop_h)
            return Y4_ERR_SHAPE;
        if (j.res_w < 1 || j.res_h < 1 || j.res_w > kMaxSide || j.res_h > kMaxSide) return Y4_ERR_SHAPE;
        if (j.win_x < 0 || j.win_y < 0 || j.win_x > j.res_w - S || j.win_y > j.res_h - S) return Y4_ERR_SHAPE;
        if (j.paste_from < -1 || j.paste_from >= n) return Y4_ERR_SHAPE;
        if (j.paste_from >= 0 && (j.paste_x0 < 0 || j.paste_x0 > j.paste_x1 || j.paste_x1 > S || j.paste_y0 < 0 ||
                                  j.paste_y0 > j.paste_y1 || j.paste_y1 > S))
            return Y4_ERR_SHAPE;
        if (j.ws_offset < 0 || (j.ws_offset & 15)) return Y4_ERR_SHAPE;
    }
    for (int i = 0; i < n; ++i)
        if ((unsigned long long)jobs[i].ws_offset + rc_job_bytes(jobs[i], S) > ws_bytes) return Y4_ERR_WORKSPACE;
    return Y4_OK;
}

void y4::rcrop_launch_coeffs(const y4_rcrop_job* jobs_dev, int n, int S, void* workspace, hipStream_t st) {
    hipLaunchKernelGGL(rcrop_coeffs_kernel, dim3((S + 255) / 256, 2, n), dim3(256), 0, st, jobs_dev, S, (int*)workspace);
}

int y4::rcrop_norm(const float* mean3_host, const float* std3_host, rc_norm* nm) {
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(mean3_host[c]) || !isfinite(std3_host[c]) || std3_host[c] == 0.0f) return Y4_ERR_SHAPE;
        nm->mean[c] = mean3_host[c];
        nm->std[c] = std3_host[c];
    }
    return Y4_OK;
}

void y4::rcrop_launch_gather_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S,
                                 const void* workspace, const rc_norm& nm, float* dst, long long dsb, long long dsc,
                                 long long dsh, long long dsw, hipStream_t st) {
    bool pastes = false;
    for (int i = 0; i < n; ++i) pastes = pastes || jobs_host[i].paste_from >= 0;
    hipLaunchKernelGGL(rcrop_gather_kernel, dim3((S + kTileX - 1) / kTileX, (S + kTileY - 1) / kTileY, pastes ? 2 * n : n),
                       dim3(kTileX), 0, st, jobs_dev, n, S, (const int*)workspace, nm, dst, dsb, dsc, dsh, dsw);
}

extern "C" size_t y4_rcrop_workspace(const y4_rcrop_job* jobs_host, int n, int S) {
    if (!jobs_host || n < 1 || S < 1 || S > kMaxSide) return 0;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        const y4_rcrop_job& j = jobs_host[i];
        if (j.crop_w < 1 || j.crop_h < 1 || j.res_w < 1 || j.res_h < 1 || j.crop_w > kMaxSide || j.crop_h > kMaxSide) return 0;
        total += rc_job_bytes(j, S);
    }
    return total;
}

extern "C" int y4_rcrop_coeffs_i32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, void* workspace,
                                   size_t ws_bytes, void* stream) {
    const int rc = y4::rcrop_check(jobs_dev, jobs_host, n, S, workspace, ws_bytes);
    if (rc != Y4_OK) return rc;
    y4::rcrop_launch_coeffs(jobs_dev, n, S, workspace, y4_stream(stream));
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_rcrop_u8_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S,
                               const float* mean3_host, const float* std3_host, float* dst, long long dst_sb, long long dst_sc,
                               long long dst_sh, long long dst_sw, void* workspace, size_t ws_bytes, void* stream) {
    if (!mean3_host || !std3_host || !dst) return Y4_ERR_NULL;
    int rc = y4::rcrop_check(jobs_dev, jobs_host, n, S, workspace, ws_bytes);
    if (rc != Y4_OK) return rc;
    rc_norm nm;
    rc = y4::rcrop_norm(mean3_host, std3_host, &nm);
    if (rc != Y4_OK) return rc;
    y4::rcrop_launch_coeffs(jobs_dev, n, S, workspace, y4_stream(stream));
    Y4_CHECK_LAUNCH();
    y4::rcrop_launch_gather_f32(jobs_dev, jobs_host, n, S, workspace, nm, dst, dst_sb, dst_sc, dst_sh, dst_sw, y4_stream(stream));
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
