// YOLO head: anchor decode, target assignment + detection loss (+ its gradient), and the
// per-class greedy NMS of the post-processing.  No MFMA here: HBM-bound sweeps, wavefront /
// block reductions, and one block-wide bitonic sort + bitmask NMS per (image, class) segment.
//
// This file is compiled with -ffp-contract=off: IoU comparisons against thresholds must follow
// the reference's separate fp32 multiply / add / divide sequence bit for bit
// (yolo/model/yololoss.py:56-91, yolo/util/utils.py:64-77).
//
// Post-processing options (include/yolov4_amd.h): the overlap measure (IoU | DIoU) is a template
// parameter of the suppression kernels, segments are (image, class) or whole images (AGN), Soft-NMS (linear | Gaussian
// decay) is one block per segment with its state in LDS, a per-image cap sorts the kept rows of an image.  The measure's
// fp32 operation order is written out at nms_measure; a float32 restatement of it is bit-equal (no fma contraction here).
#include <stdlib.h>
#include "common.h"

namespace {

struct Anchors { float w[16]; float h[16]; };

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ------------------------------------------------------------------------------------ decode
// The eval centre with scale_x_y = s != 1, ((sigma * s) - h + cell) * stride with h = (s - 1) / 2, cancels where sigma * s is near
// h in the first column / row (cell = 0): an fp32 sigmoid that is a few 2^-24 off is then arbitrarily far off RELATIVE to the
// result.  These two of the 5 + C channels are therefore evaluated in fp64 from the logit and rounded to fp32 once (error
// 2^-24 of the result itself); s = 1 has no cancellation (sigma + cell >= sigma) and keeps its fp32 code and bits.
__device__ __forceinline__ float eval_centre64(float v, float sxy, float hxy, int cell, float stride) {
    const double sg = 1.0 / (1.0 + exp(-(double)v));
    return (float)((((sg * (double)sxy) - (double)hxy) + (double)cell) * (double)stride);
}

// one block sweeps pixels; thread t <-> logit channel t = a*n_ch + ch of that pixel
// RECT: the map is Fh rows of F columns (eval only); without it Fh_arg is not read and the code is the square form's
template <bool EVAL, bool RECT = false>
__global__ __launch_bounds__(256) void yolo_decode_kernel(const float* __restrict__ logits, long long ldl,
                                                          float* __restrict__ output, float* __restrict__ pred,
                                                          long long n_total, long long box_off, float stride,
                                                          int B, int F, int A, int n_ch, Anchors anc,
                                                          float sxy, float hxy, int Fh_arg) {
    const int Fh = RECT ? Fh_arg : F;
    const long long npix = (long long)B * Fh * F;
    const int nt = A * n_ch;
    for (int t = threadIdx.x; t < nt; t += blockDim.x) {
        const int a = t / n_ch, ch = t - a * n_ch;
        for (long long p = blockIdx.x; p < npix; p += gridDim.x) {
            const int i = (int)(p % F);
            const int j = (int)((p / F) % Fh);
            const long long b = p / ((long long)Fh * F);
            const float v = logits[p * ldl + t];
            float o = v, pv = v;
            if (ch != 2 && ch != 3) { o = sigmoidf_(v); pv = o; }
            // scale_x_y: ((o * s) - h) + i, h = (s - 1) / 2.  s = 1: o * 1 and o - 0 are exact, the bits of o + i
            if (ch == 0) pv = ((o * sxy) - hxy) + (float)i;
            else if (ch == 1) pv = ((o * sxy) - hxy) + (float)j;
            else if (ch == 2) pv = expf(v) * anc.w[a];
            else if (ch == 3) pv = expf(v) * anc.h[a];
            if (EVAL) {
                if (ch < 4) pv = pv * stride;
                // scale_x_y != 1 (eval): the centre in fp64, rounded once (see eval_centre64)
                if (ch < 2 && sxy != 1.0f) pv = eval_centre64(v, sxy, hxy, ch == 0 ? i : j, stride);
                output[(b * n_total + box_off + ((long long)a * Fh + j) * F + i) * n_ch + ch] = pv;
            } else {
                const long long cell = ((b * A + a) * F + j) * F + i;
                output[cell * n_ch + ch] = o;
                if (ch < 4) pred[cell * 4 + ch] = pv;
            }
        }
    }
}

// Tiled form of the decode: a block takes DEC_TP consecutive pixels of ONE image with all their A * n_ch logit channels.
//   phase 1: coalesced 16-B loads of whole pixel rows (a thread's four columns -- hence its anchor / channel roles -- are
//            fixed for the whole tile: no division per element), activation applied on the way into an LDS image
//            [pixel][column];
//   phase 2: for an anchor a, the tile's part of the result is ONE contiguous run of cnt * n_ch floats (rows of n_ch
//            floats of consecutive pixels follow each other in [B, N, n_ch] / [B, A, F, F, n_ch]): written with aligned
//            16-B stores gathered from the LDS image (scalar stores for the <= 3 floats at either end of the run).
// The per-channel kernel above read 4 bytes per lane with a 1-KiB stride between lanes' pixels and wrote three 340-B
// segments per pixel (0.22 of the HBM peak) and spent 30 VALU per element on IEEE expf + division; this one moves whole
// lines both ways with one v_exp_f32 + one v_rcp_f32 per element (~1e-7 relative, far inside the 1e-4 parity bar):
// 4.6 - 4.9 TB/s algorithmic on the 76 x 76 layer at bs = 32 (rows of 32 pixels; 16 on small maps for occupancy).
// SCALED: scale_x_y != 1.  The instance without it has s = 1, h = 0 folded away at compile time: the default path runs the
// code it always ran (a run-time s = 1 gave the same bits but measured 6 % slower in the eval decode of bench.py).
// RECT (eval only): Fh_arg rows of F columns; pixel p of an image is (j, i) = (p / F, p % F) either way, so only the pixel
// count differs.  The square instances do not read Fh_arg: their code is what it was before the option existed.
template <bool EVAL, int DEC_TP, bool SCALED, bool RECT = false>     // DEC_TP pixels per tile: DEC_TP x 256 floats of LDS
__global__ __launch_bounds__(256) void yolo_decode_tiled_kernel(const float* __restrict__ logits, long long ldl,
                                                                float* __restrict__ output, float* __restrict__ pred,
                                                                long long n_total, long long box_off, float stride,
                                                                int F, int A, int n_ch, Anchors anc, int tiles_per_img,
                                                                float sxy_arg, float hxy_arg, int Fh_arg) {
    const float sxy = SCALED ? sxy_arg : 1.0f, hxy = SCALED ? hxy_arg : 0.0f;
    __shared__ __attribute__((aligned(16))) float tile[DEC_TP][256];
    __shared__ __attribute__((aligned(16))) float predt[EVAL ? 1 : 4][DEC_TP][4];      // train: decoded boxes per anchor
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_img, t = blockIdx.x - b * tiles_per_img;
    const int FF = (RECT ? Fh_arg : F) * F;
    const int p0 = t * DEC_TP;
    const int cnt = FF - p0 < DEC_TP ? FF - p0 : DEC_TP;
    const int nt = A * n_ch;
    // ---- phase 1.  Per column (fixed for the thread): value = rcp(exp(-v) + one) * mul + (ci * (i - h) + cj * (j - h))
    //   sigmoid channels: one = 1 (1 / (1 + e^-v)); exp channels (w, h): one = 0 (1 / e^-v = e^v), mul = anchor (* stride)
    //   x / y with scale_x_y = s: mul = s (* stride), h = (s - 1) / 2 taken off the cell index once per pixel row; s = 1
    //   gives mul = 1 (* stride) and i - 0 = i: the bits of the form without the option, at its instruction count
    // -> one v_exp, one v_rcp and three plain VALU per element, no per-element role tests
    const int col4 = tid & 63, r0 = tid >> 6;
    f32x4 one, mul, ci, cj;
    int ca[4], cch[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * col4 + e;
        const int a = c < nt ? c / n_ch : -1;
        const int ch = c < nt ? c - a * n_ch : 4;
        ca[e] = a; cch[e] = ch;
        const float sc = (EVAL && ch < 4) ? stride : 1.0f;
        one[e] = (ch == 2 || ch == 3) ? 0.f : 1.f;
        mul[e] = ch == 2 ? anc.w[a < 0 ? 0 : a] * sc : ch == 3 ? anc.h[a < 0 ? 0 : a] * sc : ch < 2 ? sxy * sc : sc;
        ci[e] = ch == 0 ? sc : 0.f;
        cj[e] = ch == 1 ? sc : 0.f;
    }
    const bool anyc = 4 * col4 < nt;
    // all of a thread's DEC_TP / 4 row loads go out before the first is used (the loop was latency-bound otherwise)
    f32x4 vv[DEC_TP / 4];
#pragma unroll
    for (int u = 0; u < DEC_TP / 4; ++u) {
        const int r = r0 + 4 * u;
        vv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (anyc && r < cnt) vv[u] = *reinterpret_cast<const f32x4*>(logits + ((long long)b * FF + p0 + r) * ldl + 4 * col4);
    }
#pragma unroll
    for (int u = 0; u < DEC_TP / 4; ++u) {
        const int r = r0 + 4 * u;
        if (r >= cnt) break;
        const int pix = p0 + r;
        const int j = pix / F, i = pix - j * F;
        const float fi = (float)i - hxy, fj = (float)j - hxy;
        const f32x4 v = vv[u];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = __expf(-v[e]);
            const float rr = __frcp_rn(t + one[e]);
            const float pv = rr * mul[e] + (ci[e] * fi + cj[e] * fj);
            if (EVAL) {
                o[e] = pv;
            } else {
                const int ch = cch[e];
                o[e] = (ch == 2 || ch == 3) ? v[e] : rr;          // `output` keeps the raw w / h logits (yololayer.py:136-139)
                if (ca[e] >= 0 && ch < 4) predt[ca[e]][r][ch] = pv;
            }
        }
        *reinterpret_cast<f32x4*>(&tile[r][4 * col4]) = o;
    }
    if (EVAL && SCALED) {
        // the 2 * A centres of each of the tile's pixels again, in fp64 (eval_centre64): one element per thread (cnt <= 32,
        // A <= 4), its logit re-read from the row phase 1 has just loaded; a barrier of its own, in these instances only
        __syncthreads();
        const int per = 2 * A;
        if (tid < cnt * per) {
            const int r = tid / per, q = tid - r * per;
            const int a = q >> 1, ch = q & 1;
            const int pix = p0 + r;
            const int j = pix / F, i = pix - j * F;
            const float v = logits[((long long)b * FF + pix) * ldl + a * n_ch + ch];
            tile[r][a * n_ch + ch] = eval_centre64(v, sxy, hxy, ch ? j : i, stride);
        }
    }
    __syncthreads();
    // ---- phase 2
    for (int a = 0; a < A; ++a) {
        const long long row0 = EVAL ? (long long)b * n_total + box_off + (long long)a * FF + p0
                                    : ((long long)b * A + a) * FF + p0;
        float* dst = output + row0 * n_ch;                 // the run [dst, dst + cnt * n_ch)
        const int len = cnt * n_ch;
        const int mis = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);      // floats past a 16-B boundary
        const int head = mis ? 4 - mis : 0;                // scalar floats before the first aligned float4
        const int nv = len > head ? (len - head) >> 2 : 0;
        const int colbase = a * n_ch;
        // (row, channel) of a thread's float4 advance by 1024 floats per trip: one division up front, none in the loop
        const int adv_pl = 1024 / n_ch, adv_ch = 1024 - adv_pl * n_ch;
        int pl0 = (head + 4 * tid) / n_ch, ch0 = head + 4 * tid - pl0 * n_ch;
        for (int q = tid; q < nv; q += 256) {
            const int o0 = head + 4 * q;
            int pl = pl0, ch = ch0;
            f32x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w[e] = tile[pl][colbase + ch];
                if (++ch == n_ch) { ch = 0; ++pl; }
            }
            *reinterpret_cast<f32x4*>(dst + o0) = w;
            pl0 += adv_pl; ch0 += adv_ch;
            if (ch0 >= n_ch) { ch0 -= n_ch; ++pl0; }
        }
        const int tail0 = head + 4 * nv;                   // scalar ends: [0, head) and [tail0, len)
        if (tid < head && tid < len) { const int pl = tid / n_ch; dst[tid] = tile[pl][colbase + tid - pl * n_ch]; }
        if (tid >= 4 && tid < 4 + (len - tail0) && len > head) {
            const int o = tail0 + tid - 4;
            const int pl = o / n_ch;
            dst[o] = tile[pl][colbase + o - pl * n_ch];
        }
        if (!EVAL) {
            // pred [B, A, F, F, 4]: one float4 per cell, always 16-B aligned
            if (tid < cnt)
                *reinterpret_cast<f32x4*>(pred + (((long long)b * A + a) * FF + p0 + tid) * 4) = *reinterpret_cast<const f32x4*>(predt[a][tid]);
        }
    }
}

static int decode_tp(long long npix) { return npix >= 100000 ? 32 : 16; }      // tile height: measured best per map size
static bool decode_tiled_ok(const float* logits, int ldl, int A, int n_ch, const float* output, const float* pred) {
    return A * n_ch <= 256 && A <= 4 && (ldl & 3) == 0 && ldl >= ((A * n_ch + 3) & ~3) &&
           (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(output) & 3) == 0 &&
           (!pred || (reinterpret_cast<uintptr_t>(pred) & 15) == 0);
}

__global__ __launch_bounds__(256) void yolo_decode_bwd_kernel(const float* __restrict__ logits, long long ldl,
                                                              const float* __restrict__ g_out,
                                                              const float* __restrict__ g_pred,
                                                              float* __restrict__ g_logits,
                                                              int B, int F, int A, int n_ch, Anchors anc, float sxy) {
    const long long npix = (long long)B * F * F;
    const int nt = A * n_ch;
    for (int t = threadIdx.x; t < (int)ldl; t += blockDim.x) {
        const int a = t / n_ch, ch = t - a * n_ch;
        for (long long p = blockIdx.x; p < npix; p += gridDim.x) {
            float g = 0.f;
            if (t < nt) {
                const int i = (int)(p % F);
                const int j = (int)((p / F) % F);
                const long long b = p / ((long long)F * F);
                const long long cell = ((b * A + a) * F + j) * F + i;
                const float v = logits[p * ldl + t];
                if (g_out) g = g_out[cell * n_ch + ch];
                if (ch < 4 && g_pred) {
                    const float gp = g_pred[cell * 4 + ch];
                    if (ch < 2) g += sxy * gp;                    // d pred / d output = scale_x_y (1 * gp is exact)
                    else g += gp * (expf(v) * (ch == 2 ? anc.w[a] : anc.h[a]));
                }
                if (ch != 2 && ch != 3) {
                    const float o = sigmoidf_(v);
                    g = g * ((1.0f - o) * o);
                }
            }
            g_logits[p * ldl + t] = g;
        }
    }
}

// ------------------------------------------------------------------------------------ pairwise IoU
// bboxes_iou, yolo/model/yololoss.py:16-91: [Na,4] x [Nb,4] -> [Na,Nb]; xyxy corners or centre/size; the intersection
// counts only where tl < br on both axes; area_i / (area_a + area_b - area_i), no epsilon.  torch.max/min
// propagate NaN (fmaxf/fminf do not), kept here.  One thread per (a, b) pair, the fp32 operation sequence of the
// reference (this file is built with -ffp-contract=off).
__device__ __forceinline__ float tmax_(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }
__device__ __forceinline__ float tmin_(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }
__global__ __launch_bounds__(256) void bboxes_iou_kernel(const float* __restrict__ A_, long long Na, const float* __restrict__ B_,
                                                         long long Nb, int xyxy, float* __restrict__ out) {
    const long long total = Na * Nb;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long ia = i / Nb, ib = i - ia * Nb;
        const float a0 = A_[ia * 4], a1 = A_[ia * 4 + 1], a2 = A_[ia * 4 + 2], a3 = A_[ia * 4 + 3];
        const float b0 = B_[ib * 4], b1 = B_[ib * 4 + 1], b2 = B_[ib * 4 + 2], b3 = B_[ib * 4 + 3];
        float tlx, tly, brx, bry, area_a, area_b;
        if (xyxy) {
            tlx = tmax_(a0, b0); tly = tmax_(a1, b1);
            brx = tmin_(a2, b2); bry = tmin_(a3, b3);
            area_a = (a2 - a0) * (a3 - a1);
            area_b = (b2 - b0) * (b3 - b1);
        } else {
            tlx = tmax_(a0 - a2 / 2.f, b0 - b2 / 2.f); tly = tmax_(a1 - a3 / 2.f, b1 - b3 / 2.f);
            brx = tmin_(a0 + a2 / 2.f, b0 + b2 / 2.f); bry = tmin_(a1 + a3 / 2.f, b1 + b3 / 2.f);
            area_a = a2 * a3;
            area_b = b2 * b3;
        }
        const float en = ((tlx < brx) ? 1.f : 0.f) * ((tly < bry) ? 1.f : 0.f);
        const float area_i = ((brx - tlx) * (bry - tly)) * en;
        out[i] = area_i / ((area_a + area_b) - area_i);
    }
}

// ------------------------------------------------------------------------------------ loss
struct LossWs {
    size_t nlabel, npos, truth, pos_cell, pos_val, pos_cls, pos_index, partials, pos_box, pos_obj, total;
    int cw, nblocks;
};
static inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
constexpr int LOSS_BLOCK = 256;
// R: records an image can hold per layer.  One positive anchor per label (iou_thresh >= 1): R = K.  Several (iou_thresh
// < 1): every label can be positive on each of the layer's A anchors, R = K * A.  With R = K the layout is unchanged.
static inline int loss_rec_cap(int K, int A, float iou_thresh) { return iou_thresh < 1.f ? K * A : K; }
static inline bool loss_opts_ok(float iou_thresh, float label_smooth) {          // false for NaN too
    return iou_thresh > 0.f && iou_thresh <= 1.f && label_smooth >= 0.f && label_smooth < 1.f;
}
static inline bool scale_xy_ok(float s) { return s >= 1.f && s <= 2.f; }
// iou_obj (obj_iou_ratio > 0): pos_obj [B, R] is appended; without it offsets and total are what they were.
static LossWs loss_ws(int B, int F, int A, int K, int C, int R, bool iou_obj = false) {
    LossWs w;
    w.cw = (C + 31) / 32;
    const long long cells = (long long)B * A * F * F;
    w.nblocks = (int)((cells + LOSS_BLOCK - 1) / LOSS_BLOCK);
    size_t o = 0;
    w.nlabel = o; o = al16(o + (size_t)B * 4);
    w.npos = o; o = al16(o + (size_t)B * 4);
    w.truth = o; o = al16(o + (size_t)B * K * 4 * 4);
    w.pos_cell = o; o = al16(o + (size_t)B * R * 4);
    w.pos_val = o; o = al16(o + (size_t)B * R * 5 * 4);
    w.pos_cls = o; o = al16(o + (size_t)B * R * w.cw * 4);
    w.pos_index = o; o = al16(o + (size_t)cells * 4);
    w.partials = o; o = al16(o + (size_t)w.nblocks * 4 * 8);
    w.pos_box = o; o = al16(o + (size_t)B * R * 4 * 4);       // appended: every offset above is what it was without it
    w.pos_obj = o;
    if (iou_obj) o = al16(o + (size_t)B * R * 4);
    w.total = o;
    return w;
}

struct LossPtrs {
    int* nlabel; int* npos; float* truth; int* pos_cell; float* pos_val; unsigned* pos_cls; int* pos_index;
    double* partials;
    float* pos_box;                                            // [B, K, 4]: a record's truth box (xc, yc, w, h), grid units
};
static LossPtrs loss_ptrs(const void* ws, const LossWs& l) {
    char* b = static_cast<char*>(const_cast<void*>(ws));
    LossPtrs p;
    p.nlabel = reinterpret_cast<int*>(b + l.nlabel);
    p.npos = reinterpret_cast<int*>(b + l.npos);
    p.truth = reinterpret_cast<float*>(b + l.truth);
    p.pos_cell = reinterpret_cast<int*>(b + l.pos_cell);
    p.pos_val = reinterpret_cast<float*>(b + l.pos_val);
    p.pos_cls = reinterpret_cast<unsigned*>(b + l.pos_cls);
    p.pos_index = reinterpret_cast<int*>(b + l.pos_index);
    p.partials = reinterpret_cast<double*>(b + l.partials);
    p.pos_box = reinterpret_cast<float*>(b + l.pos_box);
    return p;
}

// What the kernels need of the options.  fobj / fcls: the objectness / class BCE terms are focal (gamma > 0 and the bit
// of focal_terms).  r > 0: the objectness target of a record is (1 - r) + r * max(X, 0), kept per record in pos_obj.
struct LossOptK {
    float gamma, alpha;
    int fobj, fcls;
    float r;
    int kind;
    float obj_gain, cls_gain;
    float* pos_obj;                                            // [B, R]; NULL with r = 0
};

// y4_loss_opts: the defaults with the two options of the _ex entries; the range check (false for NaN too; alpha, the
// term bits and the kind count only where gamma / the ratio switch them on); whether anything beyond the _ex options is
// on, i.e. whether the option kernels have to run at all.
static inline y4_loss_opts loss_opts_default(float iou_thresh, float label_smooth) {
    y4_loss_opts o;
    o.iou_thresh = iou_thresh; o.label_smooth = label_smooth;
    o.focal_gamma = 0.f; o.focal_alpha = 0.25f; o.focal_terms = 3;
    o.obj_iou_ratio = 0.f; o.obj_iou_kind = Y4_BOX_CIOU;
    o.obj_gain = 1.f; o.cls_gain = 1.f;
    return o;
}
static inline bool gain_ok(float g) { return g > 0.f && g <= 3.402823466e38f; }
static bool loss_opts_all_ok(const y4_loss_opts* o) {
    if (!loss_opts_ok(o->iou_thresh, o->label_smooth)) return false;
    const float g = o->focal_gamma, a = o->focal_alpha, r = o->obj_iou_ratio;
    if (!(g == 0.f || (g >= 0.5f && g <= 5.f))) return false;
    if (g > 0.f && (!(a >= 0.f && a < 1.f) || o->focal_terms < 1 || o->focal_terms > 3)) return false;
    if (!(r >= 0.f && r <= 1.f)) return false;
    if (r > 0.f && (o->obj_iou_kind < Y4_BOX_IOU || o->obj_iou_kind > Y4_BOX_CIOU)) return false;
    return gain_ok(o->obj_gain) && gain_ok(o->cls_gain);
}
static inline bool loss_opts_any(const y4_loss_opts* o) {
    return o->focal_gamma > 0.f || o->obj_iou_ratio > 0.f || o->obj_gain != 1.f || o->cls_gain != 1.f;
}
static LossOptK loss_opt_k(const y4_loss_opts* o, const void* ws, const LossWs& l) {
    LossOptK k;
    k.gamma = o->focal_gamma; k.alpha = o->focal_alpha;
    k.fobj = (o->focal_gamma > 0.f && (o->focal_terms & 1)) ? 1 : 0;
    k.fcls = (o->focal_gamma > 0.f && (o->focal_terms & 2)) ? 1 : 0;
    k.r = o->obj_iou_ratio; k.kind = o->obj_iou_kind;
    k.obj_gain = o->obj_gain; k.cls_gain = o->cls_gain;
    k.pos_obj = o->obj_iou_ratio > 0.f ? reinterpret_cast<float*>(static_cast<char*>(const_cast<void*>(ws)) + l.pos_obj) : nullptr;
    return k;
}

// yololoss.py:196-265,304-369: one thread per image walks its <= K labels in order (the
// sequential semantics -- last writer wins for xy/wh/scale, class bits OR -- are kept by
// construction); cost is negligible (B*K*9 IoUs).
//
// MULTI (iou_thresh < 1, Darknet's iou_thresh): the positive anchors of a label are its arg-max anchor and every anchor
// whose shape IoU is > iou_thresh (strict; a NaN IoU never is).  The (label, anchor slot) pairs of a layer go through the
// steps of the single pair in the order of t, then of the slot a; records (R = K * A per image) are numbered by first hit
// in that order.  The host only takes masks with mask[a] % 3 == a here, so the arg-max's slot best % 3 is its position.
template <bool MULTI>
__global__ void yolo_assign_kernel(const float* __restrict__ labels, int K, int R, int B, int F, int A, int C, int cw,
                                   float stride, Anchors all_anc, int n_all, int m0, int m1, int m2,
                                   Anchors masked, float iou_thresh, LossPtrs w) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* lab = labels + (long long)b * K * 5;
    int n = 0;
    for (int t = 0; t < K; ++t) {
        const float s = (((lab[t * 5] + lab[t * 5 + 1]) + lab[t * 5 + 2]) + lab[t * 5 + 3]) + lab[t * 5 + 4];
        if (s > 0.f) ++n;
    }
    w.nlabel[b] = n;
    int np = 0;
    const float Ff = (float)F;
    for (int t = 0; t < n; ++t) {
        const float tx = lab[t * 5] / stride, ty = lab[t * 5 + 1] / stride;
        const float tw = lab[t * 5 + 2] / stride, th = lab[t * 5 + 3] / stride;
        float* tr = w.truth + ((long long)b * K + t) * 4;
        tr[0] = tx; tr[1] = ty; tr[2] = tw; tr[3] = th;
        // IoU of (0,0,tw,th) against the n_all anchors (0,0,aw,ah), xyxy form, first max wins
        int best = 0;
        float best_iou = -INFINITY;
        float im0 = 0.f, im1 = 0.f, im2 = 0.f;                 // the IoU against the layer's own three anchors
        bool first = true;
        for (int k = 0; k < n_all; ++k) {
            const float aw = all_anc.w[k], ah = all_anc.h[k];
            const float brx = fminf(tw, aw), bry = fminf(th, ah);
            const float en = (0.f < brx && 0.f < bry) ? 1.f : 0.f;
            const float ai = (brx * bry) * en;
            const float iou = ai / ((tw * th + aw * ah) - ai);
            // torch.argmax: NaN counts as maximal; first occurrence wins
            if (first || iou > best_iou || (iou != iou && !(best_iou != best_iou))) { best = k; best_iou = iou; first = false; }
            if (k == m0) im0 = iou;
            if (k == m1) im1 = iou;
            if (k == m2) im2 = iou;
        }
        const bool best_here = best == m0 || best == m1 || best == m2;
        if (!MULTI && !best_here) continue;
        const int i = (int)(short)(int)tx, j = (int)(short)(int)ty;                    // .to(torch.int16): truncation
        if (i < 0 || i >= F || j < 0 || j >= F) continue;                    // reference would raise / wrap: skipped
        const int cls = (int)(short)(int)lab[t * 5 + 4];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int mk = a == 0 ? m0 : a == 1 ? m1 : m2;
            const float ia = a == 0 ? im0 : a == 1 ? im1 : im2;
            const bool hit = MULTI ? (mk == best || ia > iou_thresh) : (a == best % 3);
            if (!hit || a >= A) continue;
            const int cell = (a * F + j) * F + i;
            int rec = w.pos_index[(long long)b * A * F * F + cell];         // -1 (the host's memset) until a pair hits the cell
            if (rec < 0) {
                rec = np++;
                w.pos_cell[(long long)b * R + rec] = cell;
                for (int q = 0; q < cw; ++q) w.pos_cls[((long long)b * R + rec) * cw + q] = 0u;
                w.pos_index[(long long)b * A * F * F + cell] = rec;
            }
            float* pv = w.pos_val + ((long long)b * R + rec) * 5;
            pv[0] = tx - (float)(short)(int)tx;
            pv[1] = ty - (float)(short)(int)ty;
            pv[2] = logf(tw / (a == 0 ? masked.w[0] : a == 1 ? masked.w[1] : masked.w[2]) + 1e-16f);
            pv[3] = logf(th / (a == 0 ? masked.h[0] : a == 1 ? masked.h[1] : masked.h[2]) + 1e-16f);
            pv[4] = sqrtf(2.0f - tw * th / Ff / Ff);
            float* pb = w.pos_box + ((long long)b * R + rec) * 4;            // last writer wins, like pv
            pb[0] = tx; pb[1] = ty; pb[2] = tw; pb[3] = th;
            if (cls >= 0 && cls < C) w.pos_cls[((long long)b * R + rec) * cw + (cls >> 5)] |= 1u << (cls & 31);
        }
    }
    w.npos[b] = np;
}

// The same assignment with one wave per image (K <= 64 labels, one lane each): the per-label work (anchor argmax, cell,
// regression targets) is independent; the sequential rules of the loop above become lane-order rules -- a cell's record
// belongs to the first label that hits it (records numbered in that order), its values come from the LAST such label,
// its class bits are the OR over all of them.
__global__ __launch_bounds__(64) void yolo_assign_wave_kernel(const float* __restrict__ labels, int K, int B, int F, int A,
                                                              int C, int cw, float stride, Anchors all_anc, int n_all,
                                                              int m0, int m1, int m2, Anchors masked, LossPtrs w) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* lab = labels + (long long)b * K * 5;
    float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f, l4 = 0.f;
    if (t < K) { l0 = lab[t * 5]; l1 = lab[t * 5 + 1]; l2 = lab[t * 5 + 2]; l3 = lab[t * 5 + 3]; l4 = lab[t * 5 + 4]; }
    const float s = (((l0 + l1) + l2) + l3) + l4;
    const int n = __popcll(__ballot(t < K && s > 0.f));
    if (t == 0) w.nlabel[b] = n;
    const bool act = t < n;
    const float tx = l0 / stride, ty = l1 / stride, tw = l2 / stride, th = l3 / stride;
    if (act) {
        float* tr = w.truth + ((long long)b * K + t) * 4;
        tr[0] = tx; tr[1] = ty; tr[2] = tw; tr[3] = th;
    }
    int best = 0;
    float best_iou = -INFINITY;
    bool first = true;
    for (int k = 0; k < n_all; ++k) {
        const float aw = all_anc.w[k], ah = all_anc.h[k];
        const float brx = fminf(tw, aw), bry = fminf(th, ah);
        const float en = (0.f < brx && 0.f < bry) ? 1.f : 0.f;
        const float ai = (brx * bry) * en;
        const float iou = ai / ((tw * th + aw * ah) - ai);
        if (first || iou > best_iou || (iou != iou && !(best_iou != best_iou))) { best = k; best_iou = iou; first = false; }
    }
    const int a = best % 3;
    const int i = (int)(short)(int)tx, j = (int)(short)(int)ty;
    const bool pos = act && (best == m0 || best == m1 || best == m2) && i >= 0 && i < F && j >= 0 && j < F && a < A;
    const int cell = pos ? (a * F + j) * F + i : -1 - t;                      // non-positive lanes never match anyone
    const int cls = (int)(short)(int)l4;
    const unsigned long long pm = __ballot(pos);
    int owner = t;
    bool later_same = false;
    for (int u = 0; u < 64; ++u) {
        const int cu = __shfl(cell, u, 64);
        if (((pm >> u) & 1ull) && cu == cell) {
            if (u < owner) owner = u;
            if (u > t) later_same = true;
        }
    }
    const bool is_owner = pos && owner == t;
    const unsigned long long om = __ballot(is_owner);
    const int my_rank = __popcll(om & ((1ull << t) - 1ull));
    const int rec = __shfl(my_rank, owner, 64);
    for (int q = 0; q < cw; ++q) {
        unsigned word = 0u;
        for (int u = 0; u < 64; ++u) {
            const int cu = __shfl(cell, u, 64), ku = __shfl(cls, u, 64);
            if (((pm >> u) & 1ull) && cu == cell && ku >= 0 && ku < C && (ku >> 5) == q) word |= 1u << (ku & 31);
        }
        if (is_owner) w.pos_cls[((long long)b * K + rec) * cw + q] = word;
    }
    if (is_owner) {
        w.pos_cell[(long long)b * K + rec] = cell;
        w.pos_index[(long long)b * A * F * F + cell] = rec;
    }
    if (pos && !later_same) {
        const float Ff = (float)F;
        float* pv = w.pos_val + ((long long)b * K + rec) * 5;
        pv[0] = tx - (float)(short)(int)tx;
        pv[1] = ty - (float)(short)(int)ty;
        pv[2] = logf(tw / masked.w[a] + 1e-16f);
        pv[3] = logf(th / masked.h[a] + 1e-16f);
        pv[4] = sqrtf(2.0f - tw * th / Ff / Ff);
        float* pb = w.pos_box + ((long long)b * K + rec) * 4;
        pb[0] = tx; pb[1] = ty; pb[2] = tw; pb[3] = th;
    }
    if (t == 0) w.npos[b] = __popcll(om);
}

// The wave form with several positive anchors per label (iou_thresh < 1; the kernel above stays as it is for the default
// path, where it measured 2 us per call faster than a one-round instance of this one).  The three anchor slots are three
// independent rounds of the same rules (a cell includes its slot, so labels collide only within a round); a record's
// number is the count of owner (label, slot) pairs before its own in (t, a) order, from the three owner ballots.  Every
// per-round array below is indexed by fully unrolled loops only (registers, no scratch).
__global__ __launch_bounds__(64) void yolo_assign_wave_multi_kernel(const float* __restrict__ labels, int K, int R, int B,
                                                                    int F, int A, int C, int cw, float stride,
                                                                    Anchors all_anc, int n_all, int m0, int m1, int m2,
                                                                    Anchors masked, float iou_thresh, LossPtrs w) {
    constexpr int NR = 3;
    const int b = blockIdx.x, t = threadIdx.x;
    const float* lab = labels + (long long)b * K * 5;
    float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f, l4 = 0.f;
    if (t < K) { l0 = lab[t * 5]; l1 = lab[t * 5 + 1]; l2 = lab[t * 5 + 2]; l3 = lab[t * 5 + 3]; l4 = lab[t * 5 + 4]; }
    const float s = (((l0 + l1) + l2) + l3) + l4;
    const int n = __popcll(__ballot(t < K && s > 0.f));
    if (t == 0) w.nlabel[b] = n;
    const bool act = t < n;
    const float tx = l0 / stride, ty = l1 / stride, tw = l2 / stride, th = l3 / stride;
    if (act) {
        float* tr = w.truth + ((long long)b * K + t) * 4;
        tr[0] = tx; tr[1] = ty; tr[2] = tw; tr[3] = th;
    }
    int best = 0;
    float best_iou = -INFINITY;
    float im0 = 0.f, im1 = 0.f, im2 = 0.f;                     // the IoU against the layer's own three anchors
    bool first = true;
    for (int k = 0; k < n_all; ++k) {
        const float aw = all_anc.w[k], ah = all_anc.h[k];
        const float brx = fminf(tw, aw), bry = fminf(th, ah);
        const float en = (0.f < brx && 0.f < bry) ? 1.f : 0.f;
        const float ai = (brx * bry) * en;
        const float iou = ai / ((tw * th + aw * ah) - ai);
        if (first || iou > best_iou || (iou != iou && !(best_iou != best_iou))) { best = k; best_iou = iou; first = false; }
        if (k == m0) im0 = iou;
        if (k == m1) im1 = iou;
        if (k == m2) im2 = iou;
    }
    const int i = (int)(short)(int)tx, j = (int)(short)(int)ty;
    const bool inmap = act && i >= 0 && i < F && j >= 0 && j < F;
    const int cls = (int)(short)(int)l4;
    int slot[NR], cell[NR], owner[NR];
    bool pos[NR], later_same[NR];
    unsigned long long pm[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int mk = r == 0 ? m0 : r == 1 ? m1 : m2;
        const float ir = r == 0 ? im0 : r == 1 ? im1 : im2;
        slot[r] = r;
        pos[r] = inmap && r < A && (mk == best || ir > iou_thresh);
        cell[r] = pos[r] ? (slot[r] * F + j) * F + i : -1 - t;               // non-positive lanes never match anyone
        pm[r] = __ballot(pos[r]);
        owner[r] = t;
        later_same[r] = false;
    }
    for (int u = 0; u < 64; ++u) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int cu = __shfl(cell[r], u, 64);
            if (((pm[r] >> u) & 1ull) && cu == cell[r]) {
                if (u < owner[r]) owner[r] = u;
                if (u > t) later_same[r] = true;
            }
        }
    }
    bool is_owner[NR];
    unsigned long long om[NR];
    int before = 0;                                            // owner pairs of the labels before t, over all rounds
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        is_owner[r] = pos[r] && owner[r] == t;
        om[r] = __ballot(is_owner[r]);
        before += __popcll(om[r] & ((1ull << t) - 1ull));
    }
    int rec[NR];
    int mine = 0;                                              // owner pairs of label t in the rounds before r
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int my_rank = before + mine;
        rec[r] = __shfl(my_rank, owner[r], 64);
        mine += is_owner[r] ? 1 : 0;
    }
    for (int q = 0; q < cw; ++q) {
        unsigned word[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) word[r] = 0u;
        for (int u = 0; u < 64; ++u) {
            const int ku = __shfl(cls, u, 64);
            const bool kq = ku >= 0 && ku < C && (ku >> 5) == q;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int cu = __shfl(cell[r], u, 64);
                if (((pm[r] >> u) & 1ull) && cu == cell[r] && kq) word[r] |= 1u << (ku & 31);
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (is_owner[r]) w.pos_cls[((long long)b * R + rec[r]) * cw + q] = word[r];
    }
    int np = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (is_owner[r]) {
            w.pos_cell[(long long)b * R + rec[r]] = cell[r];
            w.pos_index[(long long)b * A * F * F + cell[r]] = rec[r];
        }
        if (pos[r] && !later_same[r]) {
            const float Ff = (float)F;
            const int a = slot[r];
            float* pv = w.pos_val + ((long long)b * R + rec[r]) * 5;
            pv[0] = tx - (float)(short)(int)tx;
            pv[1] = ty - (float)(short)(int)ty;
            pv[2] = logf(tw / masked.w[a] + 1e-16f);
            pv[3] = logf(th / masked.h[a] + 1e-16f);
            pv[4] = sqrtf(2.0f - tw * th / Ff / Ff);
            float* pb = w.pos_box + ((long long)b * R + rec[r]) * 4;
            pb[0] = tx; pb[1] = ty; pb[2] = tw; pb[3] = th;
        }
        np += __popcll(om[r]);
    }
    if (t == 0) w.npos[b] = np;
}

__device__ __forceinline__ float bce_term(float o, float t) {
    const float lo = fmaxf(logf(o), -100.f), l1 = fmaxf(logf(1.0f - o), -100.f);
    return -(t * lo + (1.0f - t) * l1);
}
__device__ __forceinline__ float bce_grad(float o, float t) { return (o - t) / fmaxf((1.0f - o) * o, 1e-12f); }

// ---- focal loss, IoU-aware objectness, obj / cls gains (y4_loss_opts)
// The soft-target focal term of YOLOv5 on one element: with p_t = t o + (1 - t)(1 - o), q = 1 - p_t and
// a = alpha > 0 ? t alpha + (1 - t)(1 - alpha) : 1 the loss is (bce a) q^gamma and its exact derivative
// a (bce_grad q^gamma - ((bce gamma) q^(gamma - 1)) (2 t - 1)); both are 0 at q = 0.  q^(gamma - 1) is
// exp2(e log2 q), relative error about |e log2 q| 2^-24 (at most 6e-6 at q = 2^-24, gamma = 5), and q^gamma is that
// times q: one transcendental pair per element for both powers.
struct FocalW { float a, m, m1; };
__device__ __forceinline__ FocalW focal_weights(float o, float t, float gamma, float alpha) {
    const float pt = t * o + (1.0f - t) * (1.0f - o);
    const float q = 1.0f - pt;
    FocalW f;
    f.a = alpha > 0.f ? t * alpha + (1.0f - t) * (1.0f - alpha) : 1.0f;
    f.m1 = q > 0.f ? exp2f((gamma - 1.0f) * log2f(q)) : 0.f;
    f.m = q > 0.f ? f.m1 * q : 0.f;
    return f;
}
__device__ __forceinline__ float focal_term(float o, float t, float gamma, float alpha) {
    const FocalW f = focal_weights(o, t, gamma, alpha);
    return (bce_term(o, t) * f.a) * f.m;
}
__device__ __forceinline__ float focal_grad(float o, float t, float gamma, float alpha) {
    const FocalW f = focal_weights(o, t, gamma, alpha);
    return f.a * (bce_grad(o, t) * f.m - ((bce_term(o, t) * gamma) * f.m1) * (2.0f * t - 1.0f));
}

struct BoxTerm { float loss, g0, g1, g2, g3; };                // g: d loss / d(px, py, log pw, log ph)
template <bool GRAD>
__device__ __forceinline__ BoxTerm box_term(int kind, float px, float py, float pw, float ph, float tx, float ty,
                                            float tw, float th);

// The option kernels take a LossOptK as their last argument, the default instances (OPT = false) nothing: those keep the
// arguments and the code they had before the options existed.
__device__ __forceinline__ LossOptK loss_opt_of() { return LossOptK{}; }
__device__ __forceinline__ LossOptK loss_opt_of(const LossOptK& op) { return op; }

// yololoss.py:276-301 (ignore mask) + :402-427 (loss terms), one thread per cell.
template <bool OPT, typename... Op>
__global__ __launch_bounds__(LOSS_BLOCK) void yolo_loss_dense_kernel(
    const float* __restrict__ output, const float* __restrict__ pred, int B, int F, int A, int K, int R, int C, int cw,
    float thresh, float cls_lo, float cls_hi, float* __restrict__ obj_mask, LossPtrs w, Op... opk) {
    const LossOptK op = loss_opt_of(opk...);
    __shared__ double red[4][LOSS_BLOCK / 64];
    const long long cells = (long long)B * A * F * F;
    const long long cell = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int n_ch = 5 + C;
    double part[4] = {0, 0, 0, 0};
    if (cell < cells) {
        const int per_img = A * F * F;
        const int b = (int)(cell / per_img);
        const int n = w.nlabel[b];
        const float px = pred[cell * 4], py = pred[cell * 4 + 1], pw = pred[cell * 4 + 2], ph = pred[cell * 4 + 3];
        const float pl = px - pw / 2.f, pr = px + pw / 2.f, pt = py - ph / 2.f, pb = py + ph / 2.f;
        const float area_a = pw * ph;
        float best = -INFINITY;
        bool nan_seen = false;
        const float* tr = w.truth + (long long)b * K * 4;
        for (int t = 0; t < n; ++t) {
            const float tx = tr[t * 4], ty = tr[t * 4 + 1], tw = tr[t * 4 + 2], th = tr[t * 4 + 3];
            const float tlx = fmaxf(pl, tx - tw / 2.f), tly = fmaxf(pt, ty - th / 2.f);
            const float brx = fminf(pr, tx + tw / 2.f), bry = fminf(pb, ty + th / 2.f);
            // torch.max/min propagate NaN, fmaxf does not: track NaN inputs explicitly
            const bool in_nan = (pl != pl) || (pr != pr) || (pt != pt) || (pb != pb);
            const float en = (tlx < brx && tly < bry) ? 1.f : 0.f;
            const float ai = ((brx - tlx) * (bry - tly)) * en;
            const float iou = ai / ((area_a + tw * th) - ai);
            if (in_nan || iou != iou) nan_seen = true;
            else best = fmaxf(best, iou);
        }
        const bool ignore = !nan_seen && best > thresh;
        const int rec = w.pos_index[cell];
        const float m = (rec >= 0 || !ignore) ? 1.f : 0.f;
        obj_mask[cell] = m;
        const float* o = output + cell * n_ch;
        float t_obj = rec >= 0 ? 1.f : 0.f;
        if (OPT) {
            if (rec >= 0 && op.r > 0.f) {
                // X on box_record()'s operands: both boxes relative to the cell origin, so the bits are the box loss's
                const int c = (int)(cell - (long long)b * per_img);
                const float fi = (float)(c % F), fj = (float)((c / F) % F);
                const float* tb = w.pos_box + ((long long)b * R + rec) * 4;
                const float x = 1.0f - box_term<false>(op.kind, px - fi, py - fj, pw, ph, tb[0] - fi, tb[1] - fj, tb[2],
                                                       tb[3]).loss;
                t_obj = (1.0f - op.r) + op.r * fmaxf(x, 0.f);
                if (x != x) t_obj = NAN;                       // fmaxf drops the NaN of a NaN pred
                op.pos_obj[(long long)b * R + rec] = t_obj;
            }
        }
        if (m != 0.f) {
            if (OPT && op.fobj) part[2] = (double)focal_term(o[4], t_obj, op.gamma, op.alpha);
            else part[2] = (double)bce_term(o[4], t_obj);
        }
        if (rec >= 0) {
            const float* pv = w.pos_val + ((long long)b * R + rec) * 5;
            const unsigned* pc = w.pos_cls + ((long long)b * R + rec) * cw;
            const float s = pv[4];
            const float ww = s * s;
            part[0] = (double)(ww * bce_term(o[0], pv[0])) + (double)(ww * bce_term(o[1], pv[1]));
            const float d2 = o[2] * s - pv[2] * s, d3 = o[3] * s - pv[3] * s;
            part[1] = ((double)(d2 * d2) + (double)(d3 * d3)) * 0.5;
            double c = 0;
            if (OPT && op.fcls) {
                for (int k = 0; k < C; ++k)
                    c += (double)focal_term(o[5 + k], ((pc[k >> 5] >> (k & 31)) & 1u) ? cls_hi : cls_lo, op.gamma, op.alpha);
            } else {
                for (int k = 0; k < C; ++k) c += (double)bce_term(o[5 + k], ((pc[k >> 5] >> (k & 31)) & 1u) ? cls_hi : cls_lo);
            }
            part[3] = c;
        }
    }
    // block reduction (wave shuffles, then 4 waves through LDS), fixed order -> deterministic
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = part[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = 0;
        for (int k = 0; k < LOSS_BLOCK / 64; ++k) v += red[threadIdx.x][k];
        w.partials[(long long)blockIdx.x * 4 + threadIdx.x] = v;
    }
}

// GAIN: parts[2] *= obj_gain, parts[3] *= cls_gain, once, in fp64, on the reduced sums
template <bool GAIN, typename... Op>
__global__ __launch_bounds__(256) void yolo_loss_final_kernel(const double* __restrict__ partials, int nblocks,
                                                              double* __restrict__ out, Op... opk) {
    const LossOptK op = loss_opt_of(opk...);
    __shared__ double red[4][256];
    double v[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblocks; i += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += partials[(long long)i * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) {
        double v = red[threadIdx.x][0];
        if (GAIN) {
            if (threadIdx.x == 2) v = v * (double)op.obj_gain;
            if (threadIdx.x == 3) v = v * (double)op.cls_gain;
        }
        out[threadIdx.x] = v;
    }
}

// grad wrt `output`, dense: thread per element.  OPT as in yolo_loss_dense_kernel.
template <bool OPT, typename... Op>
__global__ __launch_bounds__(256) void yolo_loss_bwd_kernel(const float* __restrict__ output, int masked,
                                                            const float* __restrict__ obj_mask,
                                                            const float* __restrict__ gscale_p,
                                                            float* __restrict__ g_out, int B, int F, int A, int R,
                                                            int C, int cw, float cls_lo, float cls_hi, LossPtrs w,
                                                            Op... opk) {
    const LossOptK op = loss_opt_of(opk...);
    const int n_ch = 5 + C;
    const long long total = (long long)B * A * F * F * n_ch;
    const int per_img = A * F * F;
    const float gscale = *gscale_p;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long cell = e / n_ch;
        const int ch = (int)(e - cell * n_ch);
        const int rec = w.pos_index[cell];
        float g = 0.f;
        if (ch == 4) {
            if (obj_mask[cell] != 0.f) {
                float t = rec >= 0 ? 1.f : 0.f;
                if (OPT) {
                    if (rec >= 0 && op.r > 0.f) t = op.pos_obj[(long long)(cell / per_img) * R + rec];
                    g = op.fobj ? focal_grad(output[e], t, op.gamma, op.alpha) : bce_grad(output[e], t);
                    g = g * op.obj_gain;
                } else {
                    g = bce_grad(output[e], t);
                }
            }
        } else if (rec >= 0) {
            const int b = (int)(cell / per_img);
            const float* pv = w.pos_val + ((long long)b * R + rec) * 5;
            const float s = pv[4];
            const float o = output[e];
            if (ch < 2) g = (s * s) * bce_grad(o, pv[ch]);
            else if (ch < 4) g = ((masked ? o : o * s) - pv[ch] * s) * s;
            else {
                const int k = ch - 5;
                const unsigned bit = (w.pos_cls[((long long)b * R + rec) * cw + (k >> 5)] >> (k & 31)) & 1u;
                if (OPT) {
                    g = op.fcls ? focal_grad(o, bit ? cls_hi : cls_lo, op.gamma, op.alpha) : bce_grad(o, bit ? cls_hi : cls_lo);
                    g = g * op.cls_gain;
                } else {
                    g = bce_grad(o, bit ? cls_hi : cls_lo);
                }
            }
        }
        g_out[e] = g * gscale;
    }
}



// yololoss.py:402-407: output[...,4]*=obj_mask; output[...,{0-3,5..}]*=tgt_mask; output[...,2:4]*=tgt_scale
__global__ __launch_bounds__(256) void yolo_loss_mask_output_kernel(float* __restrict__ output,
                                                                    const float* __restrict__ obj_mask,
                                                                    int B, int F, int A, int R, int C, LossPtrs w) {
    const int n_ch = 5 + C;
    const long long total = (long long)B * A * F * F * n_ch;
    const int per_img = A * F * F;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long cell = e / n_ch;
        const int ch = (int)(e - cell * n_ch);
        const int rec = w.pos_index[cell];
        float v = output[e];
        if (ch == 4) v = v * obj_mask[cell];
        else {
            v = v * (rec >= 0 ? 1.f : 0.f);
            if (ch == 2 || ch == 3) {
                const int b = (int)(cell / per_img);
                v = v * (rec >= 0 ? w.pos_val[((long long)b * R + rec) * 5 + 4] : 0.f);
            }
        }
        output[e] = v;
    }
}

__global__ void yolo_dense_targets_kernel(float* __restrict__ target, float* __restrict__ tgt_mask,
                                          float* __restrict__ tgt_scale, int B, int F, int A, int R, int C, int cw,
                                          float cls_lo, float cls_hi, LossPtrs w, const float* __restrict__ pos_obj) {
    // one thread per (image, record slot); pos_obj: the records' objectness targets (obj_iou_ratio > 0) or NULL for 1
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * R) return;
    const int b = (int)(idx / R), rec = (int)(idx - (long long)b * R);
    if (rec >= w.npos[b]) return;
    const long long cell = (long long)b * A * F * F + w.pos_cell[idx];
    const int n_ch = 5 + C;
    const float* pv = w.pos_val + (long long)idx * 5;
    float* t = target + cell * n_ch;
    t[0] = pv[0]; t[1] = pv[1]; t[2] = pv[2]; t[3] = pv[3]; t[4] = pos_obj ? pos_obj[idx] : 1.f;
    for (int k = 0; k < C; ++k)                                // label smoothing off: 1 and the 0 the host's memset left
        t[5 + k] = ((w.pos_cls[(long long)idx * cw + (k >> 5)] >> (k & 31)) & 1u) ? cls_hi : cls_lo;
    float* tm = tgt_mask + cell * (4 + C);
    for (int k = 0; k < 4 + C; ++k) tm[k] = 1.f;
    tgt_scale[cell * 2] = pv[4];
    tgt_scale[cell * 2 + 1] = pv[4];
}

// ------------------------------------------------------------------------------------ IoU-family box loss
// 1 - X over the positive records, X = IoU | GIoU | DIoU | CIoU of the decoded box p = pred[cell] against the record's
// truth box (pos_box), both as (xc, yc, w, h) in grid units.  Centres come in relative to the cell origin, so the corner
// differences do not cancel against the grid offset.  px - i and tx - i are exact in fp32: tx is in [i, i + 1) with
// i = trunc(tx); px is in [i - h, i + 1 + h] with h = (scale_x_y - 1) / 2 <= 0.5, where px and i are both multiples of
// u = ulp(px) (u <= 1; i = 0 is trivial, else px >= 0.5 and u >= 2^-24) and |px - i| <= 1.5 (<= 0.5 where px < 1) is
// below 2^24 u, so the difference is representable.  Ties: a corner of p counts as the selected one of min / max only under a strict inequality, the clamp of the
// intersection passes a gradient only when the raw extent is > 0.  CIoU's alpha is a constant in the gradient.
// fmaxf / fminf drop NaN operands: a NaN in p is carried to the result explicitly.
constexpr float BOX_EPS = 1e-7f;

template <bool GRAD>
__device__ __forceinline__ BoxTerm box_term(int kind, float px, float py, float pw, float ph, float tx, float ty,
                                            float tw, float th) {
    const float pl = px - pw / 2.f, pr = px + pw / 2.f, pt = py - ph / 2.f, pb = py + ph / 2.f;
    const float tl = tx - tw / 2.f, tr = tx + tw / 2.f, tt = ty - th / 2.f, tb = ty + th / 2.f;
    const float iwr = fminf(pr, tr) - fmaxf(pl, tl), ihr = fminf(pb, tb) - fmaxf(pt, tt);
    const float iw = fmaxf(0.f, iwr), ih = fmaxf(0.f, ihr);
    const float inter = iw * ih;
    const float uni = ((pw * ph + tw * th) - inter) + BOX_EPS;
    const float iou = inter / uni;
    float x = iou;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;              // d X / d(px, py, pw, ph)
    float dU0 = 0.f, dU1 = 0.f, dU2 = 0.f, dU3 = 0.f;
    if (GRAD) {
        const float ar = (pr < tr && iwr > 0.f) ? 1.f : 0.f, al = (pl > tl && iwr > 0.f) ? 1.f : 0.f;
        const float ab = (pb < tb && ihr > 0.f) ? 1.f : 0.f, at = (pt > tt && ihr > 0.f) ? 1.f : 0.f;
        const float dI0 = ih * (ar - al), dI1 = iw * (ab - at);
        const float dI2 = ih * ((ar + al) / 2.f), dI3 = iw * ((ab + at) / 2.f);
        dU0 = -dI0; dU1 = -dI1; dU2 = ph - dI2; dU3 = pw - dI3;
        d0 = (dI0 - iou * dU0) / uni; d1 = (dI1 - iou * dU1) / uni;
        d2 = (dI2 - iou * dU2) / uni; d3 = (dI3 - iou * dU3) / uni;
    }
    if (kind != Y4_BOX_IOU) {
        const float cw = fmaxf(pr, tr) - fminf(pl, tl), ch = fmaxf(pb, tb) - fminf(pt, tt);
        float dcw0 = 0.f, dcw2 = 0.f, dch1 = 0.f, dch3 = 0.f;
        if (GRAD) {
            const float cr = pr > tr ? 1.f : 0.f, cl = pl < tl ? 1.f : 0.f;
            const float cb = pb > tb ? 1.f : 0.f, ct = pt < tt ? 1.f : 0.f;
            dcw0 = cr - cl; dcw2 = (cr + cl) / 2.f;
            dch1 = cb - ct; dch3 = (cb + ct) / 2.f;
        }
        if (kind == Y4_BOX_GIOU) {
            const float ca = cw * ch + BOX_EPS;
            x = iou - (ca - uni) / ca;
            if (GRAD) {
                const float ca2 = ca * ca;
                d0 = (d0 + dU0 / ca) - uni * (ch * dcw0) / ca2;
                d1 = (d1 + dU1 / ca) - uni * (cw * dch1) / ca2;
                d2 = (d2 + dU2 / ca) - uni * (ch * dcw2) / ca2;
                d3 = (d3 + dU3 / ca) - uni * (cw * dch3) / ca2;
            }
        } else {
            const float c2 = (cw * cw + ch * ch) + BOX_EPS;
            const float ex = px - tx, ey = py - ty;
            const float rho2 = ex * ex + ey * ey;
            x = iou - rho2 / c2;
            if (GRAD) {
                const float c4 = c2 * c2;
                d0 = d0 - ((2.f * ex) * c2 - rho2 * ((2.f * cw) * dcw0)) / c4;
                d1 = d1 - ((2.f * ey) * c2 - rho2 * ((2.f * ch) * dch1)) / c4;
                d2 = d2 + (rho2 * ((2.f * cw) * dcw2)) / c4;
                d3 = d3 + (rho2 * ((2.f * ch) * dch3)) / c4;
            }
            if (kind == Y4_BOX_CIOU) {
                const float phe = ph + BOX_EPS;
                const float da = atanf(tw / (th + BOX_EPS)) - atanf(pw / phe);
                const float v = (0.40528473456935109f * da) * da;          // 4 / pi^2
                const float alpha = v / (((1.f - iou) + v) + BOX_EPS);
                x = x - alpha * v;
                if (GRAD) {
                    const float den = phe * phe + pw * pw;
                    const float k = 0.81056946913870217f * da;            // 8 / pi^2
                    d2 = d2 + alpha * ((k * phe) / den);
                    d3 = d3 - alpha * ((k * pw) / den);
                }
            }
        }
    }
    BoxTerm r;
    r.loss = 1.f - x;
    r.g0 = -d0; r.g1 = -d1; r.g2 = -(d2 * pw); r.g3 = -(d3 * ph);
    if (px != px || py != py || pw != pw || ph != ph) { r.loss = NAN; r.g0 = NAN; r.g1 = NAN; r.g2 = NAN; r.g3 = NAN; }
    return r;
}

// the boxes of record slot s = b * R + rec; false for an empty slot
__device__ __forceinline__ bool box_record(const float* __restrict__ pred, int F, int A, int R, const LossPtrs& w,
                                           long long s, long long& cell_out, float* p, float* t) {
    const int b = (int)(s / R), rec = (int)(s - (long long)b * R);
    if (rec >= w.npos[b]) return false;
    const int per_img = A * F * F;
    const int cell = w.pos_cell[s];
    if (cell < 0 || cell >= per_img) return false;             // never so on a workspace the loss forward filled
    const int i = cell % F, j = (cell / F) % F;
    cell_out = (long long)b * per_img + cell;
    const float* pp = pred + cell_out * 4;
    const float* tb = w.pos_box + s * 4;
    p[0] = pp[0] - (float)i; p[1] = pp[1] - (float)j; p[2] = pp[2]; p[3] = pp[3];
    t[0] = tb[0] - (float)i; t[1] = tb[1] - (float)j; t[2] = tb[2]; t[3] = tb[3];
    return true;
}

// One block: a thread adds its slots in slot order, then wave shuffles, then the 16 wave sums in order through LDS.
constexpr int BOX_BLOCK = 1024;
__global__ __launch_bounds__(BOX_BLOCK) void yolo_box_loss_fwd_kernel(const float* __restrict__ pred, int kind, float gain,
                                                                      int B, int F, int A, int R, LossPtrs w,
                                                                      double* __restrict__ out) {
    __shared__ double red[BOX_BLOCK / 64];
    const long long slots = (long long)B * R;
    double acc = 0;
    for (long long s = threadIdx.x; s < slots; s += BOX_BLOCK) {
        long long cell;
        float p[4], t[4];
        if (box_record(pred, F, A, R, w, s, cell, p, t))
            acc += (double)box_term<false>(kind, p[0], p[1], p[2], p[3], t[0], t[1], t[2], t[3]).loss;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0;
        for (int k = 0; k < BOX_BLOCK / 64; ++k) v += red[k];
        out[0] = v * (double)gain;
        out[1] = 0.0;
    }
}

// One thread per record slot: the four box channels of its cell, over what the dense backward wrote there.
__global__ __launch_bounds__(256) void yolo_box_loss_bwd_kernel(const float* __restrict__ pred, int kind, float gain,
                                                                const float* __restrict__ gscale_p,
                                                                float* __restrict__ g_out, int B, int F, int A, int R,
                                                                int n_ch, float sxy, LossPtrs w) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= (long long)B * R) return;
    long long cell;
    float p[4], t[4];
    if (!box_record(pred, F, A, R, w, s, cell, p, t)) return;
    const BoxTerm r = box_term<true>(kind, p[0], p[1], p[2], p[3], t[0], t[1], t[2], t[3]);
    const float gscale = *gscale_p;
    float* g = g_out + cell * n_ch;
    g[0] = ((r.g0 * gain) * sxy) * gscale;                    // d pred / d output = scale_x_y on x and y (x * 1 is exact)
    g[1] = ((r.g1 * gain) * sxy) * gscale;
    g[2] = (r.g2 * gain) * gscale;
    g[3] = (r.g3 * gain) * gscale;
}

// ------------------------------------------------------------------------------------ training statistics of the loss
// Darknet's per-layer line (count, Avg IOU, .5R, .75R, Obj, No Obj, Class) from what the loss forward left behind: one
// thread per cell, as in yolo_loss_dense_kernel (channel 4 of the 5 + C row; a positive cell also walks its class
// channels).  X is t_obj's expression with the kind fixed to IoU.  Eleven block partials ([nblocks, 11] doubles: the
// seven counts are exact integers there), folded in a fixed order by the second kernel, which ADDS them to the caller's
// row: the sums are bit-reproducible for a given shape.  Row entry 0 (n_cells) is added by the fold.
constexpr int STATS_N = 12;
constexpr int STATS_P = STATS_N - 1;                           // partial q holds row entry q + 1
__global__ __launch_bounds__(LOSS_BLOCK) void yolo_loss_stats_kernel(
    const float* __restrict__ output, const float* __restrict__ pred, const float* __restrict__ obj_mask, int B, int F,
    int A, int R, int C, int cw, LossPtrs w, double* __restrict__ partials) {
    __shared__ double red[STATS_P][LOSS_BLOCK / 64];
    const long long cells = (long long)B * A * F * F;
    const long long cell = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int n_ch = 5 + C;
    // q + 1: 1 n_pos, 2 n_ign, 3 sum_iou, 4 n_iou50, 5 n_iou75, 6 sum_obj_pos, 7 sum_obj_bg, 8 n_bg, 9 sum_cls, 10 n_cls,
    // 11 n_top1
    double v[STATS_P];
#pragma unroll
    for (int q = 0; q < STATS_P; ++q) v[q] = 0.0;
    if (cell < cells) {
        const int per_img = A * F * F;
        const int b = (int)(cell / per_img);
        const int rec = w.pos_index[cell];
        const float m = obj_mask[cell];
        const float* o = output + cell * n_ch;
        const float obj = o[4];
        if (m == 0.f) v[1] = 1.0;
        if (rec >= 0) {
            const int c = (int)(cell - (long long)b * per_img);
            const float fi = (float)(c % F), fj = (float)((c / F) % F);
            const long long s = (long long)b * R + rec;
            const float* tb = w.pos_box + s * 4;
            const float px = pred[cell * 4], py = pred[cell * 4 + 1], pw = pred[cell * 4 + 2], ph = pred[cell * 4 + 3];
            const float x = 1.0f - box_term<false>(Y4_BOX_IOU, px - fi, py - fj, pw, ph, tb[0] - fi, tb[1] - fj, tb[2],
                                                   tb[3]).loss;
            v[0] = 1.0;
            v[2] = (double)x;                                   // a NaN pred: NaN here, and neither comparison holds
            if (x > 0.5f) v[3] = 1.0;
            if (x > 0.75f) v[4] = 1.0;
            v[5] = (double)obj;
            const unsigned* pc = w.pos_cls + s * cw;
            double sc = 0.0;
            int nc = 0, top = 0;
            float best = o[5];
            for (int k = 0; k < C; ++k) {
                const float p = o[5 + k];
                if ((pc[k >> 5] >> (k & 31)) & 1u) { sc += (double)p; ++nc; }
                if (p > best) { best = p; top = k; }            // strict: the lowest index wins a tie
            }
            v[8] = sc;
            v[9] = (double)nc;
            if ((pc[top >> 5] >> (top & 31)) & 1u) v[10] = 1.0;
        } else if (m != 0.f) {
            v[6] = (double)obj;
            v[7] = 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < STATS_P; ++q) {
        double r = v[q];
        for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x < STATS_P) {
        double r = 0;
        for (int k = 0; k < LOSS_BLOCK / 64; ++k) r += red[threadIdx.x][k];
        partials[(long long)blockIdx.x * STATS_P + threadIdx.x] = r;
    }
}

__global__ __launch_bounds__(256) void yolo_loss_stats_fold_kernel(const double* __restrict__ partials, int nblocks,
                                                                   double n_cells, double* __restrict__ row) {
    __shared__ double red[STATS_P][256];
    double v[STATS_P];
#pragma unroll
    for (int q = 0; q < STATS_P; ++q) v[q] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256)
#pragma unroll
        for (int q = 0; q < STATS_P; ++q) v[q] += partials[(long long)i * STATS_P + q];
#pragma unroll
    for (int q = 0; q < STATS_P; ++q) red[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
#pragma unroll
            for (int q = 0; q < STATS_P; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < STATS_P) row[1 + threadIdx.x] += red[threadIdx.x][0];
    else if (threadIdx.x == STATS_P) row[0] += n_cells;
}

// ------------------------------------------------------------------------------------ postprocess
// The prediction rows are [5 + C] floats (340 B at C = 80): one thread per row reads 4 B from 64 different lines per
// load (measured: 25x the tensor's bytes on the fabric, 276 GB/s).  The tiled forms below copy POST_ROWS consecutive rows
// -- a contiguous span -- into LDS with coalesced loads (row pitch forced odd: conflict-free column walks) and let
// thread (row, class) pairs read them from there; candidate counts go through an LDS histogram first.
constexpr int POST_ROWS = 64;
constexpr int POST_MAX_NCH = 255;                          // 64 rows x 255 floats = 63.8 KB of LDS

__device__ __forceinline__ void post_load_tile(const float* __restrict__ pred, long long row0, int rows, int n_ch,
                                               int pitch, float* __restrict__ tile) {
    const float* src = pred + row0 * n_ch;
    const int total = rows * n_ch;
    int e = threadIdx.x;
    int r = e / n_ch, c = e - r * n_ch;
    const int dr = 256 / n_ch, dc = 256 - dr * n_ch;
    for (; e < total; e += 256) {
        tile[r * pitch + c] = src[e];
        r += dr; c += dc;
        if (c >= n_ch) { c -= n_ch; ++r; }
    }
}

// AGN (class-agnostic segments): one segment per image, counts[b]; else counts[b * C + c]
template <bool AGN>
__global__ __launch_bounds__(256) void post_count_tiled_kernel(float* __restrict__ pred, int B, long long N, int C,
                                                               float conf, int convert, int* __restrict__ counts) {
    extern __shared__ float post_smem[];
    const int n_ch = 5 + C, pitch = n_ch | 1;
    float* tile = post_smem;
    int* hist = reinterpret_cast<int*>(post_smem + POST_ROWS * pitch);       // [2][C]: the tile's first / second image
    const long long total = (long long)B * N;
    const long long ntiles = (total + POST_ROWS - 1) / POST_ROWS;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long row0 = t * POST_ROWS;
        const int rows = (int)((total - row0) < POST_ROWS ? (total - row0) : POST_ROWS);
        post_load_tile(pred, row0, rows, n_ch, pitch, tile);
        for (int i = threadIdx.x; i < 2 * C; i += 256) hist[i] = 0;
        __syncthreads();
        const int b0 = (int)(row0 / N);
        const long long b0_end = (long long)(b0 + 1) * N;                     // rows >= b0_end belong to image b0 + 1 ...
        if (convert && threadIdx.x < rows) {                                  // utils.py:117-126, written back in place
            float* q = tile + threadIdx.x * pitch;
            const float x = q[0], y = q[1], w = q[2], h = q[3];
            float* p = pred + (row0 + threadIdx.x) * n_ch;
            p[0] = x - w / 2.f; p[1] = y - h / 2.f; p[2] = x + w / 2.f; p[3] = y + h / 2.f;
        }
        for (int e = threadIdx.x; e < POST_ROWS * C; e += 256) {
            const int r = e & (POST_ROWS - 1), c = e / POST_ROWS;
            if (r < rows) {
                const float* q = tile + r * pitch;
                if (q[5 + c] * q[4] >= conf) {
                    // ... or a later one when N < POST_ROWS: those go straight to the global counter
                    const long long i = row0 + r;
                    if (i < b0_end) atomicAdd(&hist[c], 1);
                    else if (i < b0_end + N) atomicAdd(&hist[C + c], 1);
                    else atomicAdd(&counts[AGN ? (int)(i / N) : (int)(i / N) * C + c], 1);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C; i += 256) {
            const int v = hist[i];
            const int b = b0 + (i >= C ? 1 : 0);
            if (v && b < B) atomicAdd(&counts[AGN ? b : b * C + (i >= C ? i - C : i)], v);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned long long make_key(float score, unsigned idx);

// AGN: the key's low word is box * C + c (ties: lower box, then lower class); else the box index
template <bool AGN>
__global__ __launch_bounds__(256) void post_fill_tiled_kernel(const float* __restrict__ pred, int B, long long N, int C,
                                                              float conf, const int* __restrict__ seg_off,
                                                              int* __restrict__ cursor,
                                                              unsigned long long* __restrict__ keys) {
    extern __shared__ float post_smem[];
    const int n_ch = 5 + C, pitch = n_ch | 1;
    float* tile = post_smem;
    const long long total = (long long)B * N;
    const long long ntiles = (total + POST_ROWS - 1) / POST_ROWS;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long row0 = t * POST_ROWS;
        const int rows = (int)((total - row0) < POST_ROWS ? (total - row0) : POST_ROWS);
        post_load_tile(pred, row0, rows, n_ch, pitch, tile);
        __syncthreads();
        for (int e = threadIdx.x; e < POST_ROWS * C; e += 256) {
            const int r = e & (POST_ROWS - 1), c = e / POST_ROWS;
            if (r < rows) {
                const float* q = tile + r * pitch;
                const float obj = q[4], cc = q[5 + c];
                if (cc * obj >= conf) {
                    const long long i = row0 + r;
                    const int b = (int)(i / N);
                    const int seg = AGN ? b : b * C + c;
                    const int slot = atomicAdd(&cursor[seg], 1);
                    const unsigned box = (unsigned)(i - (long long)b * N);
                    // (a segment truncated by a too-small candidate buffer takes what fits; the host re-runs with room)
                    if (slot < seg_off[seg + 1] - seg_off[seg])
                        keys[seg_off[seg] + slot] = make_key(obj * cc, AGN ? box * (unsigned)C + (unsigned)c : box);   // utils.py:209
                }
            }
        }
        __syncthreads();
    }
}

template <bool AGN>
__global__ __launch_bounds__(256) void post_count_kernel(float* __restrict__ pred, int B, long long N, int C,
                                                         float conf, int convert, int* __restrict__ counts) {
    const long long total = (long long)B * N;
    const int n_ch = 5 + C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        float* p = pred + i * n_ch;
        if (convert) {                                           // utils.py:117-126
            const float x = p[0], y = p[1], w = p[2], h = p[3];
            p[0] = x - w / 2.f; p[1] = y - h / 2.f; p[2] = x + w / 2.f; p[3] = y + h / 2.f;
        }
        const int b = (int)(i / N);
        const float obj = p[4];
        for (int c = 0; c < C; ++c)
            if (p[5 + c] * obj >= conf) atomicAdd(&counts[AGN ? b : b * C + c], 1);
    }
}

// key: high 32 = ~ordered(score) (so ascending key = descending score), low 32 = box index
__device__ __forceinline__ unsigned long long make_key(float score, unsigned idx) {
    unsigned u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // total order on floats
    return ((unsigned long long)(~u) << 32) | idx;
}

template <bool AGN>
__global__ __launch_bounds__(256) void post_fill_kernel(const float* __restrict__ pred, int B, long long N, int C,
                                                        float conf, const int* __restrict__ seg_off,
                                                        int* __restrict__ cursor, unsigned long long* __restrict__ keys) {
    const long long total = (long long)B * N;
    const int n_ch = 5 + C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const float* p = pred + i * n_ch;
        const int b = (int)(i / N);
        const unsigned box = (unsigned)(i - (long long)b * N);
        const float obj = p[4];
        for (int c = 0; c < C; ++c) {
            const float cc = p[5 + c];
            if (cc * obj >= conf) {
                const int seg = AGN ? b : b * C + c;
                const int slot = atomicAdd(&cursor[seg], 1);
                if (slot < seg_off[seg + 1] - seg_off[seg])
                    keys[seg_off[seg] + slot] = make_key(obj * cc, AGN ? box * (unsigned)C + (unsigned)c : box);  // utils.py:209 score = obj*cls_conf
            }
        }
    }
}

// Block-wide bitonic sort of n keys in global memory, n arbitrary.  All-ascending network (the
// first step of every merge mirrors the upper half), so virtual +inf padding at indices >= n
// never moves and a compare-exchange whose upper index is >= n is simply skipped.
__device__ void block_bitonic_sort(unsigned long long* k, int n) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int size = 2; size <= np2; size <<= 1) {
        const int half = size >> 1;
        for (int t = threadIdx.x; t < np2 / 2; t += blockDim.x) {
            const int blk = t / half, off = t - blk * half;
            const int lo = blk * size + off, hi = blk * size + size - 1 - off;
            if (hi < n) {
                const unsigned long long a = k[lo], b = k[hi];
                if (a > b) { k[lo] = b; k[hi] = a; }
            }
        }
        __syncthreads();
        for (int stride = half >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < np2 / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                if (hi < n) {
                    const unsigned long long a = k[lo], b = k[hi];
                    if (a > b) { k[lo] = b; k[hi] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// utils.py:64-81 greedy suppression on a sorted list.  box(i): xyxy of sorted candidate i.
// Chunks of 256 candidates: (A) test against everything kept so far, (B) 256x256 bitmask of
// intra-chunk suppression + a serial scan by one thread.  keep_flag[i] in sorted order.
struct NmsShared {
    float4 kb[256];
    float ka[256];
    unsigned long long mask[256][4];
    unsigned long long alive[4];
    int kept_in_chunk[256];
    int nk;
};

// The overlap of candidate a against the already selected box o, areas (x2 - x1) * (y2 - y1) computed by the caller.
// Y4_NMS_IOU: utils.py:64-77.  Y4_NMS_DIOU: iou - rho2 / c2 with, each step one fp32 operation in this order,
//   dx = ((a.x1 + a.x2) - (o.x1 + o.x2)) * 0.5, dy likewise, rho2 = dx * dx + dy * dy,
//   ew = max(a.x2, o.x2) - min(a.x1, o.x1), eh likewise, c2 = ew * ew + eh * eh, penalty = c2 == 0 ? 0 : rho2 / c2.
template <int MEASURE>
__device__ __forceinline__ float nms_measure(const float4 a, float area_a, const float4 o, float area_o) {
    const float tlx = fmaxf(a.x, o.x), tly = fmaxf(a.y, o.y);
    const float brx = fminf(a.z, o.z), bry = fminf(a.w, o.w);
    const float en = (tlx < brx && tly < bry) ? 1.f : 0.f;
    const float inter = ((brx - tlx) * (bry - tly)) * en;
    const float iou = inter / ((area_a + area_o) - inter);
    if (MEASURE == Y4_NMS_IOU) return iou;
    const float dx = ((a.x + a.z) - (o.x + o.z)) * 0.5f, dy = ((a.y + a.w) - (o.y + o.w)) * 0.5f;
    const float rho2 = dx * dx + dy * dy;
    const float ew = fmaxf(a.z, o.z) - fminf(a.x, o.x), eh = fmaxf(a.w, o.w) - fminf(a.y, o.y);
    const float c2 = ew * ew + eh * eh;
    const float pen = c2 == 0.f ? 0.f : rho2 / c2;
    return iou - pen;
}

template <int MEASURE, typename BoxFn>
__device__ int block_greedy_nms(int n, float thresh, int limit, BoxFn box_of, float4* kept_box, float* kept_area,
                                int* kept_sorted_pos, NmsShared& sh) {
    int kept = 0;                                               // uniform
    for (int s = 0; s < n && (limit <= 0 || kept < limit); s += 256) {
        const int i = s + threadIdx.x;
        const bool valid = i < n;
        float4 bx = make_float4(0, 0, 0, 0);
        if (valid) bx = box_of(i);
        const float area = (bx.z - bx.x) * (bx.w - bx.y);
        bool alive = valid;
        // (A) against earlier kept boxes, staged through LDS 256 at a time
        for (int k0 = 0; k0 < kept; k0 += 256) {
            __syncthreads();
            if (k0 + (int)threadIdx.x < kept) { sh.kb[threadIdx.x] = kept_box[k0 + threadIdx.x]; sh.ka[threadIdx.x] = kept_area[k0 + threadIdx.x]; }
            __syncthreads();
            const int kn = min(256, kept - k0);
            if (alive)
                for (int k = 0; k < kn; ++k) {
                    if (nms_measure<MEASURE>(bx, area, sh.kb[k], sh.ka[k]) >= thresh) { alive = false; break; }
                }
        }
        // (B) intra-chunk
        __syncthreads();
        sh.kb[threadIdx.x] = bx;
        sh.ka[threadIdx.x] = area;
        if (threadIdx.x < 4) sh.alive[threadIdx.x] = 0ull;
        __syncthreads();
        {
            const unsigned long long bal = __ballot(alive);
            if ((threadIdx.x & 63) == 0) sh.alive[threadIdx.x >> 6] = bal;
        }
        unsigned long long mk[4] = {0, 0, 0, 0};
        if (alive)
            for (int u = threadIdx.x + 1; u < 256 && s + u < n; ++u) {
                // candidate u is tested against already-selected t: area_u + area_t (utils.py:76)
                if (nms_measure<MEASURE>(sh.kb[u], sh.ka[u], bx, area) >= thresh) mk[u >> 6] |= 1ull << (u & 63);
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) sh.mask[threadIdx.x][q] = mk[q];
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long al[4] = {sh.alive[0], sh.alive[1], sh.alive[2], sh.alive[3]};
            int nk = 0;
            int room = limit > 0 ? limit - kept : 0x7fffffff;
            for (int t = 0; t < 256 && room > 0; ++t) {
                if ((al[t >> 6] >> (t & 63)) & 1ull) {
                    sh.kept_in_chunk[nk++] = t;
                    --room;
#pragma unroll
                    for (int q = 0; q < 4; ++q) al[q] &= ~sh.mask[t][q];
                }
            }
            sh.nk = nk;
        }
        __syncthreads();
        const int nk = sh.nk;
        if ((int)threadIdx.x < nk) {
            const int t = sh.kept_in_chunk[threadIdx.x];
            kept_box[kept + threadIdx.x] = sh.kb[t];
            kept_area[kept + threadIdx.x] = sh.ka[t];
            kept_sorted_pos[kept + threadIdx.x] = s + t;
        }
        kept += nk;
        __syncthreads();
    }
    return kept;
}

constexpr int NMS_LDS_KEYS = 2048;

// AGN: segment = image, key low word = box * C + c; `limit` > 0 stops a segment at that many survivors
template <int MEASURE, bool AGN>
__global__ __launch_bounds__(256) void post_nms_kernel(const float* __restrict__ pred, long long N, int C,
                                                       float thresh, int limit, const int* __restrict__ seg_off,
                                                       unsigned long long* __restrict__ keys,
                                                       float4* __restrict__ kbox, float* __restrict__ karea,
                                                       int* __restrict__ kpos, float* __restrict__ det_rows,
                                                       int* __restrict__ kept_out) {
    __shared__ NmsShared sh;
    const int seg = blockIdx.x;
    const int off = seg_off[seg];
    const int n = seg_off[seg + 1] - off;
    if (n == 0) { if (threadIdx.x == 0) kept_out[seg] = 0; return; }
    const int b = AGN ? seg : seg / C, c = AGN ? 0 : seg - b * C;
    const int n_ch = 5 + C;
    unsigned long long* k = keys + off;
    if (n <= NMS_LDS_KEYS) {
        // the usual segment (a few hundred candidates): the bitonic network runs on an LDS copy of the keys
        __shared__ unsigned long long skeys[NMS_LDS_KEYS];
        for (int i = threadIdx.x; i < n; i += blockDim.x) skeys[i] = k[i];
        __syncthreads();
        block_bitonic_sort(skeys, n);
        for (int i = threadIdx.x; i < n; i += blockDim.x) k[i] = skeys[i];
        __syncthreads();
    } else {
        block_bitonic_sort(k, n);
    }
    const float* img = pred + (long long)b * N * n_ch;
    auto box_of = [&](int i) {
        const unsigned low = (unsigned)(k[i] & 0xffffffffull);
        const unsigned idx = AGN ? low / (unsigned)C : low;
        const float* p = img + (long long)idx * n_ch;
        return make_float4(p[0], p[1], p[2], p[3]);
    };
    const int kept = block_greedy_nms<MEASURE>(n, thresh, limit, box_of, kbox + off, karea + off, kpos + off, sh);
    for (int r = threadIdx.x; r < kept; r += blockDim.x) {
        const unsigned low = (unsigned)(k[kpos[off + r]] & 0xffffffffull);
        const unsigned idx = AGN ? low / (unsigned)C : low;
        const int cls = AGN ? (int)(low - idx * (unsigned)C) : c;
        const float* p = img + (long long)idx * n_ch;
        float* o = det_rows + (long long)(off + r) * 7;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; o[4] = p[4]; o[5] = p[5 + cls]; o[6] = (float)cls;
    }
    if (threadIdx.x == 0) kept_out[seg] = kept;
}

// ---- Soft-NMS (Bodla et al.), one block per segment.  Candidate j = sorted position j (score descending, key index
// ascending) carries a weight W_j (1 at the start) and the current score s0_j * W_j.  A round emits the alive candidate with
// the largest current score (ties: lower sorted position) and decays every other alive j by
//   ov = measure(j, selected) > 0 ? measure : 0;   linear: w = ov >= thresh ? 1 - ov : 1;   gaussian: w = expf(-(ov * ov) / sigma)
//   W_j = W_j * w;   j leaves when s0_j * W_j < conf.
// The decay sweep of one round is also the arg-max of the next: a thread keeps the best (score, position) of what it
// swept, 64 lanes fold by shuffles, the four waves through LDS (two buffers in turn: one barrier per round).  Every loop is
// bounded by n or by `rounds` = min(n, limit or n), both read before it starts.
struct SoftRed { float v[2][4]; int j[2][4]; };

__device__ __forceinline__ float key_score(unsigned long long key) {
    const unsigned u = ~(unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

template <int MEASURE>
__device__ __forceinline__ int soft_nms_rounds(int n, int rounds, int soft, float thresh, float sigma, float conf,
                                               const float4* sb, const float* ss0, float* sW, unsigned char* sal,
                                               int* epos, float* ew, SoftRed& red) {
    int sel = 0, e = 0;                                         // uniform; position 0 holds the largest s0 and every W is 1
    for (int r = 0; r < rounds; ++r) {
        const float4 bs = sb[sel];
        const float as = (bs.z - bs.x) * (bs.w - bs.y);
        if (threadIdx.x == 0) { epos[e] = sel; ew[e] = sW[sel]; sal[sel] = 0; }
        ++e;
        if (r + 1 == rounds) break;
        float bv = 0.f;
        int bj = -1;
        for (int j = threadIdx.x; j < n; j += 256) {
            if (j == sel || !sal[j]) continue;
            const float4 bx = sb[j];
            const float m = nms_measure<MEASURE>(bx, (bx.z - bx.x) * (bx.w - bx.y), bs, as);
            const float ov = m > 0.f ? m : 0.f;
            const float w = soft == Y4_SOFT_LINEAR ? (ov >= thresh ? 1.f - ov : 1.f) : expf(-(ov * ov) / sigma);
            const float W = sW[j] * w;
            sW[j] = W;
            const float cur = ss0[j] * W;
            if (cur < conf) sal[j] = 0;
            else if (bj < 0 || cur > bv) { bv = cur; bj = j; }  // ascending j: the first of equal scores stays
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_down(bv, off, 64);
            const int oj = __shfl_down(bj, off, 64);
            if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
        }
        const int buf = r & 1;
        if ((threadIdx.x & 63) == 0) { red.v[buf][threadIdx.x >> 6] = bv; red.j[buf][threadIdx.x >> 6] = bj; }
        __syncthreads();
        bv = red.v[buf][0]; bj = red.j[buf][0];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float ov = red.v[buf][q];
            const int oj = red.j[buf][q];
            if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
        }
        if (bj < 0) break;                                      // nothing remains
        sel = bj;
    }
    return e;
}

template <int MEASURE, bool AGN>
__global__ __launch_bounds__(256) void post_soft_nms_kernel(const float* __restrict__ pred, long long N, int C, float thresh,
                                                            int soft, float sigma, float conf, int limit,
                                                            const int* __restrict__ seg_off,
                                                            unsigned long long* __restrict__ keys,
                                                            float4* __restrict__ gbox, float* __restrict__ gs0,
                                                            float* __restrict__ gW, unsigned char* __restrict__ galive,
                                                            int* __restrict__ epos, float* __restrict__ ew,
                                                            float* __restrict__ det_rows, int* __restrict__ kept_out) {
    // boxes 32 KiB | s0 8 KiB | W 8 KiB | alive 2 KiB; the sort's key copy (16 KiB) uses the box area before the boxes do
    __shared__ __attribute__((aligned(16))) unsigned char lds[NMS_LDS_KEYS * 25];
    __shared__ SoftRed red;
    const int seg = blockIdx.x;
    const int off = seg_off[seg];
    const int n = seg_off[seg + 1] - off;
    if (n == 0) { if (threadIdx.x == 0) kept_out[seg] = 0; return; }
    const int b = AGN ? seg : seg / C, c = AGN ? 0 : seg - b * C;
    const int n_ch = 5 + C;
    unsigned long long* k = keys + off;
    const bool in_lds = n <= NMS_LDS_KEYS;
    if (in_lds) {
        unsigned long long* skeys = reinterpret_cast<unsigned long long*>(lds);
        for (int i = threadIdx.x; i < n; i += 256) skeys[i] = k[i];
        __syncthreads();
        block_bitonic_sort(skeys, n);
        for (int i = threadIdx.x; i < n; i += 256) k[i] = skeys[i];
        __syncthreads();
    } else {
        block_bitonic_sort(k, n);
    }
    const float* img = pred + (long long)b * N * n_ch;
    float4* sb = in_lds ? reinterpret_cast<float4*>(lds) : gbox + off;
    float* ss0 = in_lds ? reinterpret_cast<float*>(lds + NMS_LDS_KEYS * 16) : gs0 + off;
    float* sW = in_lds ? reinterpret_cast<float*>(lds + NMS_LDS_KEYS * 20) : gW + off;
    unsigned char* sal = in_lds ? lds + NMS_LDS_KEYS * 24 : galive + off;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long key = k[i];
        const unsigned low = (unsigned)(key & 0xffffffffull);
        const unsigned idx = AGN ? low / (unsigned)C : low;
        const float* p = img + (long long)idx * n_ch;
        sb[i] = make_float4(p[0], p[1], p[2], p[3]);
        ss0[i] = key_score(key);
        sW[i] = 1.f;
        sal[i] = 1;
    }
    __syncthreads();
    const int rounds = (limit > 0 && limit < n) ? limit : n;
    int kept;
    if (in_lds)
        kept = soft_nms_rounds<MEASURE>(n, rounds, soft, thresh, sigma, conf, reinterpret_cast<const float4*>(lds),
                                        reinterpret_cast<const float*>(lds + NMS_LDS_KEYS * 16),
                                        reinterpret_cast<float*>(lds + NMS_LDS_KEYS * 20), lds + NMS_LDS_KEYS * 24,
                                        epos + off, ew + off, red);
    else
        kept = soft_nms_rounds<MEASURE>(n, rounds, soft, thresh, sigma, conf, gbox + off, gs0 + off, gW + off, galive + off,
                                        epos + off, ew + off, red);
    __syncthreads();
    for (int r = threadIdx.x; r < kept; r += 256) {
        const unsigned low = (unsigned)(k[epos[off + r]] & 0xffffffffull);
        const unsigned idx = AGN ? low / (unsigned)C : low;
        const int cls = AGN ? (int)(low - idx * (unsigned)C) : c;
        const float* p = img + (long long)idx * n_ch;
        float* o = det_rows + (long long)(off + r) * 7;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; o[4] = p[4]; o[5] = p[5 + cls] * ew[off + r]; o[6] = (float)cls;
    }
    if (threadIdx.x == 0) kept_out[seg] = kept;
}

// ---- Weighted box fusion (Solovyev et al.), one block per segment.  Candidates are walked in key order j = 0 .. n-1; cluster
// t holds its fused box F_t, the score-weighted corner sums, the score sum S_t, its member count and its class.  Per
// candidate: every thread measures it against the clusters t = tid, tid + 256, ... (a = the candidate, o = F_t, the 'iou'
// sequence of nms_measure), keeps the best strict match (value descending, index ascending: any fold order gives the same
// winner), 64 lanes fold by shuffles and the four waves through LDS (two buffers in turn: ONE barrier per candidate).  The
// update is one thread's work: cluster t is only ever read and written by thread t % 256, so the next candidate's scan sees it
// without a second barrier.  Scores do not decay: a segment always takes n steps, n read before the loop starts.
// Candidates (box, score, class) are gathered once into the workspace and read one step ahead of their use.
constexpr int WBF_LDS_CLUSTERS = 1024;                      // cluster state in LDS up to here (44 B each), else the workspace

struct WbfState { float4* F; float4* sum; float* S; int* cnt; int* cls; };

__device__ __forceinline__ int wbf_walk(int n, float thresh, const float4* cbox, const float* cs, const int* ccls,
                                        const WbfState st, SoftRed& red) {
    int T = 0;                                                  // uniform
    float4 bx = cbox[0];
    float s = cs[0];
    int cl = ccls[0];
    for (int j = 0; j < n; ++j) {
        const float4 a = bx;
        const float sa = s;
        const int ca = cl;
        if (j + 1 < n) { bx = cbox[j + 1]; s = cs[j + 1]; cl = ccls[j + 1]; }
        const float area = (a.z - a.x) * (a.w - a.y);
        float bv = 0.f;
        int bj = -1;
        for (int t = threadIdx.x; t < T; t += 256) {
            const float4 o = st.F[t];
            const float m = nms_measure<Y4_NMS_IOU>(a, area, o, (o.z - o.x) * (o.w - o.y));
            if (m > thresh && (bj < 0 || m > bv)) { bv = m; bj = t; }      // NaN: no match; ascending t: the first of equals stays
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_down(bv, off, 64);
            const int oj = __shfl_down(bj, off, 64);
            if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
        }
        const int buf = j & 1;
        if ((threadIdx.x & 63) == 0) { red.v[buf][threadIdx.x >> 6] = bv; red.j[buf][threadIdx.x >> 6] = bj; }
        __syncthreads();
        bv = red.v[buf][0]; bj = red.j[buf][0];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float ov = red.v[buf][q];
            const int oj = red.j[buf][q];
            if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
        }
        const int t = bj >= 0 ? bj : T;
        if ((int)threadIdx.x == (t & 255)) {
            const float px1 = sa * a.x, py1 = sa * a.y, px2 = sa * a.z, py2 = sa * a.w;
            if (bj >= 0) {
                float4 sm = st.sum[t];
                sm.x = sm.x + px1; sm.y = sm.y + py1; sm.z = sm.z + px2; sm.w = sm.w + py2;
                const float S = st.S[t] + sa;
                st.sum[t] = sm;
                st.S[t] = S;
                st.cnt[t] = st.cnt[t] + 1;
                st.F[t] = make_float4(sm.x / S, sm.y / S, sm.z / S, sm.w / S);
            } else {
                st.sum[t] = make_float4(px1, py1, px2, py2);
                st.S[t] = sa;
                st.cnt[t] = 1;
                st.cls[t] = ca;
                st.F[t] = a;
            }
        }
        if (bj < 0) ++T;
    }
    return T;
}

// rows (F, 1, S / n * min(n, views) / views, class) in creation order; thread t % 256 reads what it wrote itself
__device__ __forceinline__ void wbf_emit(int T, int n_views, const WbfState st, float* __restrict__ rows) {
    const float fv = (float)n_views;
    for (int t = threadIdx.x; t < T; t += 256) {
        const float4 F = st.F[t];
        const int cnt = st.cnt[t];
        const float mean = st.S[t] / (float)cnt;
        const float f = (float)min(cnt, n_views) / fv;
        float* o = rows + (long long)t * 7;
        o[0] = F.x; o[1] = F.y; o[2] = F.z; o[3] = F.w; o[4] = 1.f; o[5] = mean * f; o[6] = (float)st.cls[t];
    }
}

template <bool AGN>
__global__ __launch_bounds__(256) void post_wbf_kernel(const float* __restrict__ pred, long long N, int C, float thresh,
                                                       int n_views, const int* __restrict__ seg_off,
                                                       unsigned long long* __restrict__ keys, float4* cbox, float* cs,
                                                       int* ccls, float4* gF, float4* gsum, float* gS, int* gcnt, int* gcls,
                                                       float* __restrict__ det_rows, int* __restrict__ kept_out) {
    // F 16 KiB | sums 16 KiB | S 4 KiB | count 4 KiB | class 4 KiB; the sort's key copy (16 KiB) uses the front before they do
    __shared__ __attribute__((aligned(16))) unsigned char lds[WBF_LDS_CLUSTERS * 44];
    __shared__ SoftRed red;
    static_assert(WBF_LDS_CLUSTERS * 44 >= NMS_LDS_KEYS * 8, "the key copy must fit");
    const int seg = blockIdx.x;
    const int off = seg_off[seg];
    const int n = seg_off[seg + 1] - off;
    if (n == 0) { if (threadIdx.x == 0) kept_out[seg] = 0; return; }
    const int b = AGN ? seg : seg / C, c = AGN ? 0 : seg - b * C;
    const int n_ch = 5 + C;
    unsigned long long* k = keys + off;
    if (n <= NMS_LDS_KEYS) {
        unsigned long long* skeys = reinterpret_cast<unsigned long long*>(lds);
        for (int i = threadIdx.x; i < n; i += 256) skeys[i] = k[i];
        __syncthreads();
        block_bitonic_sort(skeys, n);
        for (int i = threadIdx.x; i < n; i += 256) k[i] = skeys[i];
        __syncthreads();
    } else {
        block_bitonic_sort(k, n);
    }
    const float* img = pred + (long long)b * N * n_ch;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long key = k[i];
        const unsigned low = (unsigned)(key & 0xffffffffull);
        const unsigned idx = AGN ? low / (unsigned)C : low;
        const float* p = img + (long long)idx * n_ch;
        cbox[off + i] = make_float4(p[0], p[1], p[2], p[3]);
        cs[off + i] = key_score(key);
        ccls[off + i] = AGN ? (int)(low - idx * (unsigned)C) : c;
    }
    __syncthreads();
    int T;                                                      // (two calls: each inlines with its own address space)
    if (n <= WBF_LDS_CLUSTERS) {
        const WbfState st = {reinterpret_cast<float4*>(lds), reinterpret_cast<float4*>(lds + WBF_LDS_CLUSTERS * 16),
                             reinterpret_cast<float*>(lds + WBF_LDS_CLUSTERS * 32),
                             reinterpret_cast<int*>(lds + WBF_LDS_CLUSTERS * 36),
                             reinterpret_cast<int*>(lds + WBF_LDS_CLUSTERS * 40)};
        T = wbf_walk(n, thresh, cbox + off, cs + off, ccls + off, st, red);
        wbf_emit(T, n_views, st, det_rows + (long long)off * 7);
    } else {
        const WbfState st = {gF + off, gsum + off, gS + off, gcnt + off, gcls + off};
        T = wbf_walk(n, thresh, cbox + off, cs + off, ccls + off, st, red);
        wbf_emit(T, n_views, st, det_rows + (long long)off * 7);
    }
    if (threadIdx.x == 0) kept_out[seg] = T;
}

__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ scores, long long R,
                                                       unsigned long long* __restrict__ keys) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < R; i += (long long)gridDim.x * blockDim.x)
        keys[i] = scores ? make_key(scores[i], (unsigned)i) : (unsigned long long)i;
}

__global__ __launch_bounds__(256) void nms_single_kernel(const float* __restrict__ boxes, int R, float thresh, int limit,
                                                         unsigned long long* __restrict__ keys, float4* kbox,
                                                         float* karea, int* kpos, int* __restrict__ keep_idx,
                                                         int* __restrict__ n_keep) {
    __shared__ NmsShared sh;
    block_bitonic_sort(keys, R);
    auto box_of = [&](int i) {
        const unsigned idx = (unsigned)(keys[i] & 0xffffffffull);
        return make_float4(boxes[idx * 4], boxes[idx * 4 + 1], boxes[idx * 4 + 2], boxes[idx * 4 + 3]);
    };
    const int kept = block_greedy_nms<Y4_NMS_IOU>(R, thresh, limit, box_of, kbox, karea, kpos, sh);
    for (int r = threadIdx.x; r < kept; r += blockDim.x) keep_idx[r] = (int)(keys[kpos[r]] & 0xffffffffull);
    if (threadIdx.x == 0) *n_keep = kept;
}

// ---- device-side prefix sums of the postprocess: segment offsets from the candidate counts, output offsets from the
// survivor counts.  One block; thread t owns a run of consecutive segments, runs are combined by an LDS scan.
__device__ __forceinline__ long long block_exclusive_scan_1024(long long v, long long* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t] - v;
}
__global__ __launch_bounds__(1024) void post_scan_kernel(const int* __restrict__ counts, int nseg, long long cap,
                                                         int* __restrict__ seg_off, int* __restrict__ info) {
    __shared__ long long sh[1024];
    const int per = (nseg + 1023) / 1024;
    const int s0 = threadIdx.x * per, s1 = min(nseg, s0 + per);
    long long mine = 0;
    for (int s = s0; s < s1; ++s) mine += counts[s];
    long long run = block_exclusive_scan_1024(mine, sh);
    for (int s = s0; s < s1; ++s) {
        seg_off[s] = (int)(run < cap ? run : cap);         // clamped: a too-small buffer truncates, never overflows
        run += counts[s];
    }
    if (threadIdx.x == 1023) {
        const long long total = sh[1023];
        seg_off[nseg] = (int)(total < cap ? total : cap);
        info[0] = (int)(total < 0x7fffffffll ? total : 0x7fffffffll);
        info[1] = total > cap ? 1 : 0;
    }
}
__global__ __launch_bounds__(1024) void post_out_scan_kernel(const int* __restrict__ kept, int nseg, int C, int B,
                                                             int* __restrict__ out_off, int* __restrict__ img_off) {
    __shared__ long long sh[1024];
    const int per = (nseg + 1023) / 1024;
    const int s0 = threadIdx.x * per, s1 = min(nseg, s0 + per);
    long long mine = 0;
    for (int s = s0; s < s1; ++s) mine += kept[s];
    long long run = block_exclusive_scan_1024(mine, sh);
    for (int s = s0; s < s1; ++s) {
        out_off[s] = (int)run;
        if (s % C == 0) img_off[s / C] = (int)run;
        run += kept[s];
    }
    if (threadIdx.x == 1023) { out_off[nseg] = (int)sh[1023]; img_off[B] = (int)sh[1023]; }
}
// rows of segment s: det_rows[seg_off[s] .. + kept[s]) -> out_rows[out_off[s] ..): class asc, score desc per image
__global__ __launch_bounds__(64) void post_compact_kernel(const float* __restrict__ det_rows, const int* __restrict__ seg_off,
                                                          const int* __restrict__ kept, const int* __restrict__ out_off,
                                                          float* __restrict__ out_rows) {
    const int s = blockIdx.x;
    const int n = kept[s] * 7;
    const float* src = det_rows + (long long)seg_off[s] * 7;
    float* dst = out_rows + (long long)out_off[s] * 7;
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = src[i];
}

// ---- per-image cap: one block per image gives each kept row of its S segments the key (row[4] * row[5] descending, row
// position in det_rows ascending = class, then place in the segment), sorts them and flags the first max_det;
// kept2[s] = flagged rows of segment s.
__global__ __launch_bounds__(256) void post_topk_kernel(const float* __restrict__ det_rows, const int* __restrict__ seg_off,
                                                        const int* __restrict__ kept, int S, int max_det,
                                                        unsigned long long* __restrict__ tkeys, int* __restrict__ flags,
                                                        int* __restrict__ kept2) {
    __shared__ unsigned long long skeys[NMS_LDS_KEYS];
    __shared__ int cnt;
    const int s0 = blockIdx.x * S;
    const int base = seg_off[s0];
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int s = s0; s < s0 + S; ++s) {
        const int off = seg_off[s], ks = kept[s];
        for (int r = threadIdx.x; r < ks; r += 256) {
            const int pos = off + r;
            const float* row = det_rows + (long long)pos * 7;
            const int slot = atomicAdd(&cnt, 1);               // any order: the sort below fixes it (keys are distinct)
            tkeys[base + slot] = make_key(row[4] * row[5], (unsigned)pos);
            flags[pos] = 0;
        }
    }
    __syncthreads();
    const int nk = cnt;                                        // <= the image's candidates: inside its span of tkeys
    unsigned long long* k = tkeys + base;
    if (nk > max_det) {
        if (nk <= NMS_LDS_KEYS) {
            for (int i = threadIdx.x; i < nk; i += 256) skeys[i] = k[i];
            __syncthreads();
            block_bitonic_sort(skeys, nk);
            for (int i = threadIdx.x; i < max_det; i += 256) k[i] = skeys[i];
            __syncthreads();
        } else {
            block_bitonic_sort(k, nk);
        }
    }
    const int nflag = nk < max_det ? nk : max_det;
    for (int i = threadIdx.x; i < nflag; i += 256) flags[(unsigned)(k[i] & 0xffffffffull)] = 1;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int s = s0 + (threadIdx.x >> 6); s < s0 + S; s += 4) {
        const int off = seg_off[s], ks = kept[s];
        int v = 0;
        for (int r = lane; r < ks; r += 64) v += flags[off + r];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) kept2[s] = v;
    }
}
// the flagged rows of segment s, in their order -> out_rows[out_off[s] ..)
__global__ __launch_bounds__(64) void post_compact_flagged_kernel(const float* __restrict__ det_rows,
                                                                  const int* __restrict__ seg_off,
                                                                  const int* __restrict__ kept, const int* __restrict__ flags,
                                                                  const int* __restrict__ out_off,
                                                                  float* __restrict__ out_rows) {
    const int s = blockIdx.x;
    const int n = kept[s], off = seg_off[s];
    int run = out_off[s];
    for (int r0 = 0; r0 < n; r0 += 64) {
        const int r = r0 + threadIdx.x;
        const bool f = r < n && flags[off + r] != 0;
        const unsigned long long m = __ballot(f);
        if (f) {
            const float* src = det_rows + (long long)(off + r) * 7;
            float* dst = out_rows + (long long)(run + __popcll(m & ((1ull << threadIdx.x) - 1ull))) * 7;
#pragma unroll
            for (int q = 0; q < 7; ++q) dst[q] = src[q];
        }
        run += __popcll(m);
    }
}

struct PostWs { size_t keys, cursor, kbox, karea, kpos, total; };
// the Soft-NMS state of segments above the LDS bound, and the emitted (position, weight) lists, behind the hard layout
struct PostExWs { PostWs base; size_t w, ew, alive, total; };
struct TopkWs { size_t keys, flags, kept2, total; };
static PostWs post_ws(long long total, int nseg) {
    PostWs w;
    size_t o = 0;
    const size_t t = (size_t)(total > 0 ? total : 1);
    w.keys = o; o = al16(o + t * 8);
    w.cursor = o; o = al16(o + (size_t)(nseg > 0 ? nseg : 1) * 4);
    w.kbox = o; o = al16(o + t * 16);
    w.karea = o; o = al16(o + t * 4);
    w.kpos = o; o = al16(o + t * 4);
    w.total = o;
    return w;
}
static PostExWs post_ex_ws(long long total, int nseg, bool soft) {
    PostExWs w;
    w.base = post_ws(total, nseg);
    size_t o = w.base.total;
    const size_t t = soft ? (size_t)(total > 0 ? total : 1) : 0;
    w.w = o; o = al16(o + t * 4);
    w.ew = o; o = al16(o + t * 4);
    w.alive = o; o = al16(o + t);
    w.total = o;
    return w;
}
static TopkWs topk_ws(long long total, int nseg) {
    TopkWs w;
    size_t o = 0;
    const size_t t = (size_t)(total > 0 ? total : 1);
    w.keys = o; o = al16(o + t * 8);
    w.flags = o; o = al16(o + t * 4);
    w.kept2 = o; o = al16(o + (size_t)(nseg > 0 ? nseg : 1) * 4);
    w.total = o;
    return w;
}
// WBF: keys and cursors as PostWs; the gathered candidates; the cluster state of segments above WBF_LDS_CLUSTERS
struct WbfWs { size_t keys, cursor, cbox, cs, ccls, F, sum, S, cnt, cls, total; };
static WbfWs wbf_ws(long long total, int nseg) {
    WbfWs w;
    size_t o = 0;
    const size_t t = (size_t)(total > 0 ? total : 1);
    w.keys = o; o = al16(o + t * 8);
    w.cursor = o; o = al16(o + (size_t)(nseg > 0 ? nseg : 1) * 4);
    w.cbox = o; o = al16(o + t * 16);
    w.cs = o; o = al16(o + t * 4);
    w.ccls = o; o = al16(o + t * 4);
    w.F = o; o = al16(o + t * 16);
    w.sum = o; o = al16(o + t * 16);
    w.S = o; o = al16(o + t * 4);
    w.cnt = o; o = al16(o + t * 4);
    w.cls = o; o = al16(o + t * 4);
    w.total = o;
    return w;
}
static bool nms_opts_ok(const y4_nms_opts* o) {
    return (o->metric == Y4_NMS_IOU || o->metric == Y4_NMS_DIOU) &&
           (o->soft == Y4_SOFT_NONE || o->soft == Y4_SOFT_LINEAR || o->soft == Y4_SOFT_GAUSSIAN) &&
           !(o->soft == Y4_SOFT_GAUSSIAN && !(o->sigma > 0.f)) && (o->agnostic == 0 || o->agnostic == 1) && o->max_det >= 0;
}

inline int grid_for(long long total) {
    long long b = (total + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}
// the candidates' sort keys into their segments: cursors zeroed, then the LDS-tiled fill, or the row-per-thread one for wide rows
static int post_fill_keys(const float* prediction, int B, long long N, int n_classes, float conf_thre, bool agn,
                          const int* seg_offsets, int nseg, int* cursor, unsigned long long* keys, hipStream_t st) {
    if (hipMemsetAsync(cursor, 0, (size_t)nseg * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    const int pitch = (5 + n_classes) | 1;
    const size_t smem = (size_t)POST_ROWS * pitch * 4;
    if (5 + n_classes <= POST_MAX_NCH && smem <= 65536) {
        const long long ntiles = ((long long)B * N + POST_ROWS - 1) / POST_ROWS;
        auto kern = agn ? post_fill_tiled_kernel<true> : post_fill_tiled_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(ntiles < 2048 ? ntiles : 2048)), dim3(256), smem, st,
                           prediction, B, N, n_classes, conf_thre, seg_offsets, cursor, keys);
    } else {
        auto kern = agn ? post_fill_kernel<true> : post_fill_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(grid_for((long long)B * N)), dim3(256), 0, st, prediction, B, N,
                           n_classes, conf_thre, seg_offsets, cursor, keys);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
static bool fill_anchors(Anchors& a, const float* host_wh, int n) {
    if (!host_wh || n < 1 || n > 16) return false;
    for (int i = 0; i < 16; ++i) { a.w[i] = 1.f; a.h[i] = 1.f; }
    for (int i = 0; i < n; ++i) { a.w[i] = host_wh[2 * i]; a.h[i] = host_wh[2 * i + 1]; }
    return true;
}

}  // namespace

extern "C" {

int y4_bboxes_iou_f32(const float* boxes_a, long long Na, const float* boxes_b, long long Nb, int xyxy, float* iou,
                      void* stream) {
    if (Na < 0 || Nb < 0) return Y4_ERR_SHAPE;
    if (Na == 0 || Nb == 0) return Y4_OK;
    if (!boxes_a || !boxes_b || !iou) return Y4_ERR_NULL;
    long long blocks = (Na * Nb + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bboxes_iou_kernel, dim3((unsigned)blocks), dim3(256), 0, y4_stream(stream), boxes_a, Na, boxes_b, Nb,
                       xyxy, iou);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_decode_train_ex_f32(const float* logits, int ldl, float* output, float* pred,
                                int B, int F, int A, int n_classes, const float* anchors_wh_host, float scale_xy,
                                void* stream) {
    if (!logits || !output || !pred) return Y4_ERR_NULL;
    const int n_ch = 5 + n_classes;
    Anchors anc;
    if (B <= 0 || F <= 0 || A <= 0 || n_classes <= 0 || ldl < A * n_ch || !fill_anchors(anc, anchors_wh_host, A) ||
        !scale_xy_ok(scale_xy))
        return Y4_ERR_SHAPE;
    const float hxy = (scale_xy - 1.0f) * 0.5f;
    const long long npix = (long long)B * F * F;
    const int tp = decode_tp(npix);
    const long long tpi = ((long long)F * F + tp - 1) / tp;
    if (decode_tiled_ok(logits, ldl, A, n_ch, output, pred) && (long long)B * tpi < (1ll << 31)) {
        const bool sc = scale_xy != 1.0f;
        auto kern = tp == 16 ? (sc ? yolo_decode_tiled_kernel<false, 16, true> : yolo_decode_tiled_kernel<false, 16, false>)
                             : (sc ? yolo_decode_tiled_kernel<false, 32, true> : yolo_decode_tiled_kernel<false, 32, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * tpi)), dim3(256), 0, y4_stream(stream), logits,
                           (long long)ldl, output, pred, 0ll, 0ll, 1.0f, F, A, n_ch, anc, (int)tpi, scale_xy, hxy, F);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    hipLaunchKernelGGL(yolo_decode_kernel<false>, dim3((unsigned)(npix < 8192 ? npix : 8192)), dim3(256), 0,
                       y4_stream(stream), logits, (long long)ldl, output, pred, 0ll, 0ll, 1.0f, B, F, A, n_ch, anc,
                       scale_xy, hxy, F);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_decode_train_f32(const float* logits, int ldl, float* output, float* pred,
                             int B, int F, int A, int n_classes, const float* anchors_wh_host, void* stream) {
    return y4_yolo_decode_train_ex_f32(logits, ldl, output, pred, B, F, A, n_classes, anchors_wh_host, 1.0f, stream);
}

int y4_yolo_decode_eval_ex_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                               int B, int F, int A, int n_classes, const float* anchors_wh_host,
                               float stride, float scale_xy, void* stream) {
    if (!logits || !out) return Y4_ERR_NULL;
    const int n_ch = 5 + n_classes;
    Anchors anc;
    if (B <= 0 || F <= 0 || A <= 0 || n_classes <= 0 || ldl < A * n_ch || !fill_anchors(anc, anchors_wh_host, A) ||
        !scale_xy_ok(scale_xy))
        return Y4_ERR_SHAPE;
    if (box_off < 0 || box_off + (long long)A * F * F > n_total) return Y4_ERR_SHAPE;
    const float hxy = (scale_xy - 1.0f) * 0.5f;
    const long long npix = (long long)B * F * F;
    const int tp = decode_tp(npix);
    const long long tpi = ((long long)F * F + tp - 1) / tp;
    if (decode_tiled_ok(logits, ldl, A, n_ch, out, nullptr) && (long long)B * tpi < (1ll << 31)) {
        const bool sc = scale_xy != 1.0f;
        auto kern = tp == 16 ? (sc ? yolo_decode_tiled_kernel<true, 16, true> : yolo_decode_tiled_kernel<true, 16, false>)
                             : (sc ? yolo_decode_tiled_kernel<true, 32, true> : yolo_decode_tiled_kernel<true, 32, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * tpi)), dim3(256), 0, y4_stream(stream), logits,
                           (long long)ldl, out, (float*)nullptr, n_total, box_off, stride, F, A, n_ch, anc, (int)tpi,
                           scale_xy, hxy, F);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    hipLaunchKernelGGL(yolo_decode_kernel<true>, dim3((unsigned)(npix < 8192 ? npix : 8192)), dim3(256), 0,
                       y4_stream(stream), logits, (long long)ldl, out, (float*)nullptr, n_total, box_off, stride, B, F,
                       A, n_ch, anc, scale_xy, hxy, F);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_decode_eval_rect_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                                 int B, int Fh, int Fw, int A, int n_classes, const float* anchors_wh_host,
                                 float stride, float scale_xy, void* stream) {
    if (!logits || !out) return Y4_ERR_NULL;
    const int n_ch = 5 + n_classes;
    Anchors anc;
    if (B <= 0 || Fh <= 0 || Fw <= 0 || A <= 0 || n_classes <= 0 || ldl < A * n_ch || !fill_anchors(anc, anchors_wh_host, A) ||
        !scale_xy_ok(scale_xy))
        return Y4_ERR_SHAPE;
    const long long FF = (long long)Fh * Fw;
    if (FF >= (1ll << 31) || box_off < 0 || box_off + (long long)A * FF > n_total) return Y4_ERR_SHAPE;
    const float hxy = (scale_xy - 1.0f) * 0.5f;
    const long long npix = (long long)B * FF;
    const int tp = decode_tp(npix);
    const long long tpi = (FF + tp - 1) / tp;
    if (decode_tiled_ok(logits, ldl, A, n_ch, out, nullptr) && (long long)B * tpi < (1ll << 31)) {
        const bool sc = scale_xy != 1.0f;
        auto kern = tp == 16 ? (sc ? yolo_decode_tiled_kernel<true, 16, true, true> : yolo_decode_tiled_kernel<true, 16, false, true>)
                             : (sc ? yolo_decode_tiled_kernel<true, 32, true, true> : yolo_decode_tiled_kernel<true, 32, false, true>);
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * tpi)), dim3(256), 0, y4_stream(stream), logits,
                           (long long)ldl, out, (float*)nullptr, n_total, box_off, stride, Fw, A, n_ch, anc, (int)tpi,
                           scale_xy, hxy, Fh);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    hipLaunchKernelGGL((yolo_decode_kernel<true, true>), dim3((unsigned)(npix < 8192 ? npix : 8192)), dim3(256), 0,
                       y4_stream(stream), logits, (long long)ldl, out, (float*)nullptr, n_total, box_off, stride, B, Fw,
                       A, n_ch, anc, scale_xy, hxy, Fh);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_decode_eval_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                            int B, int F, int A, int n_classes, const float* anchors_wh_host,
                            float stride, void* stream) {
    return y4_yolo_decode_eval_ex_f32(logits, ldl, out, n_total, box_off, B, F, A, n_classes, anchors_wh_host, stride,
                                      1.0f, stream);
}

int y4_yolo_decode_bwd_ex_f32(const float* logits, int ldl, const float* g_output, const float* g_pred,
                              float* g_logits, int B, int F, int A, int n_classes,
                              const float* anchors_wh_host, float scale_xy, void* stream) {
    if (!logits || !g_logits) return Y4_ERR_NULL;
    const int n_ch = 5 + n_classes;
    Anchors anc;
    if (B <= 0 || F <= 0 || A <= 0 || n_classes <= 0 || ldl < A * n_ch || !fill_anchors(anc, anchors_wh_host, A) ||
        !scale_xy_ok(scale_xy))
        return Y4_ERR_SHAPE;
    const long long npix = (long long)B * F * F;
    hipLaunchKernelGGL(yolo_decode_bwd_kernel, dim3((unsigned)(npix < 8192 ? npix : 8192)), dim3(256), 0,
                       y4_stream(stream), logits, (long long)ldl, g_output, g_pred, g_logits, B, F, A, n_ch, anc, scale_xy);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_decode_bwd_f32(const float* logits, int ldl, const float* g_output, const float* g_pred,
                           float* g_logits, int B, int F, int A, int n_classes,
                           const float* anchors_wh_host, void* stream) {
    return y4_yolo_decode_bwd_ex_f32(logits, ldl, g_output, g_pred, g_logits, B, F, A, n_classes, anchors_wh_host, 1.0f,
                                     stream);
}

// the shape conditions every loss entry shares; B * R * 5 and the record slots stay inside int
static bool loss_dims_ok(int B, int F, int A, int K, int n_classes) {
    return B > 0 && F > 0 && A > 0 && K > 0 && n_classes > 0 && (long long)B * K * A < (1ll << 31);
}

size_t y4_yolo_loss_workspace_ex(int B, int F, int A, int K, int n_classes, float iou_thresh) {
    if (!loss_dims_ok(B, F, A, K, n_classes) || !loss_opts_ok(iou_thresh, 0.f)) return 0;
    return loss_ws(B, F, A, K, n_classes, loss_rec_cap(K, A, iou_thresh)).total;
}

size_t y4_yolo_loss_workspace_opts(int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts) {
    if (!loss_dims_ok(B, F, A, K, n_classes) || !opts || !loss_opts_all_ok(opts)) return 0;
    return loss_ws(B, F, A, K, n_classes, loss_rec_cap(K, A, opts->iou_thresh), opts->obj_iou_ratio > 0.f).total;
}

size_t y4_yolo_loss_workspace(int B, int F, int A, int K, int n_classes) {
    if (B <= 0 || F <= 0 || A <= 0 || K <= 0 || n_classes <= 0) return 0;
    return loss_ws(B, F, A, K, n_classes, K).total;
}

int y4_yolo_loss_fwd_opts_f32(const float* output, const float* pred, const float* labels, int K,
                              int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                              const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                              const y4_loss_opts* opts, float* obj_mask, double* loss_parts,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!output || !pred || !labels || !obj_mask || !loss_parts || !workspace || !anch_mask_host || !opts) return Y4_ERR_NULL;
    if (B <= 0 || F <= 0 || A != 3 || K <= 0 || n_classes <= 0 || (long long)A * F * F >= (1ll << 31)) return Y4_ERR_SHAPE;
    if (!loss_opts_all_ok(opts) || (long long)B * K * A >= (1ll << 31)) return Y4_ERR_SHAPE;
    const float iou_thresh = opts->iou_thresh, label_smooth = opts->label_smooth;
    const bool multi = iou_thresh < 1.f;
    Anchors all, masked;
    if (!fill_anchors(all, all_anchors_host, n_all_anchors)) return Y4_ERR_SHAPE;
    float mwh[6];
    for (int a = 0; a < 3; ++a) {
        const int id = anch_mask_host[a];
        if (id < 0 || id >= n_all_anchors) return Y4_ERR_SHAPE;
        if (multi && id % 3 != a) return Y4_ERR_SHAPE;         // the arg-max's slot (best % 3) must be its place in the mask
        mwh[2 * a] = all_anchors_host[2 * id]; mwh[2 * a + 1] = all_anchors_host[2 * id + 1];
    }
    fill_anchors(masked, mwh, 3);
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R, opts->obj_iou_ratio > 0.f);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    const float cls_lo = 0.5f * label_smooth, cls_hi = 1.0f - cls_lo;      // Darknet's rule; 0 and 1 without smoothing
    hipStream_t st = y4_stream(stream);
    if (hipMemsetAsync(w.pos_index, 0xff, (size_t)B * A * F * F * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    const int m0 = anch_mask_host[0], m1 = anch_mask_host[1], m2 = anch_mask_host[2];
    if (K <= 64) {
        if (multi)
            hipLaunchKernelGGL(yolo_assign_wave_multi_kernel, dim3(B), dim3(64), 0, st, labels, K, R, B, F, A, n_classes,
                               l.cw, stride, all, n_all_anchors, m0, m1, m2, masked, iou_thresh, w);
        else
            hipLaunchKernelGGL(yolo_assign_wave_kernel, dim3(B), dim3(64), 0, st, labels, K, B, F, A, n_classes, l.cw,
                               stride, all, n_all_anchors, m0, m1, m2, masked, w);
    } else {
        auto kern = multi ? yolo_assign_kernel<true> : yolo_assign_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((B + 63) / 64), dim3(64), 0, st, labels, K, R, B, F, A, n_classes, l.cw, stride, all,
                           n_all_anchors, m0, m1, m2, masked, iou_thresh, w);
    }
    Y4_CHECK_LAUNCH();
    if (loss_opts_any(opts)) {
        const LossOptK op = loss_opt_k(opts, workspace, l);
        hipLaunchKernelGGL((yolo_loss_dense_kernel<true, LossOptK>), dim3(l.nblocks), dim3(LOSS_BLOCK), 0, st, output, pred, B, F, A, K,
                           R, n_classes, l.cw, ignore_thresh, cls_lo, cls_hi, obj_mask, w, op);
        Y4_CHECK_LAUNCH();
        hipLaunchKernelGGL((yolo_loss_final_kernel<true, LossOptK>), dim3(1), dim3(256), 0, st, w.partials, l.nblocks,
                           loss_parts, op);
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    // the defaults: the instances in which the options do not exist
    hipLaunchKernelGGL(yolo_loss_dense_kernel<false>, dim3(l.nblocks), dim3(LOSS_BLOCK), 0, st, output, pred, B, F, A, K, R,
                       n_classes, l.cw, ignore_thresh, cls_lo, cls_hi, obj_mask, w);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(yolo_loss_final_kernel<false>, dim3(1), dim3(256), 0, st, w.partials, l.nblocks, loss_parts);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_loss_fwd_ex_f32(const float* output, const float* pred, const float* labels, int K,
                            int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                            const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                            float iou_thresh, float label_smooth, float* obj_mask, double* loss_parts,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const y4_loss_opts o = loss_opts_default(iou_thresh, label_smooth);
    return y4_yolo_loss_fwd_opts_f32(output, pred, labels, K, B, F, A, n_classes, stride, ignore_thresh, all_anchors_host,
                                     n_all_anchors, anch_mask_host, &o, obj_mask, loss_parts, workspace, workspace_bytes,
                                     stream);
}

int y4_yolo_loss_fwd_f32(const float* output, const float* pred, const float* labels, int K,
                         int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                         const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                         float* obj_mask, double* loss_parts,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_loss_fwd_ex_f32(output, pred, labels, K, B, F, A, n_classes, stride, ignore_thresh, all_anchors_host,
                                   n_all_anchors, anch_mask_host, 1.0f, 0.0f, obj_mask, loss_parts, workspace,
                                   workspace_bytes, stream);
}

int y4_yolo_loss_bwd_opts_f32(const float* output, int output_is_masked, const float* obj_mask,
                              const float* gscale, float* g_output,
                              int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts,
                              const void* workspace, size_t workspace_bytes, void* stream) {
    if (!output || !obj_mask || !g_output || !workspace || !gscale || !opts) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || !loss_opts_all_ok(opts)) return Y4_ERR_SHAPE;
    const float iou_thresh = opts->iou_thresh, label_smooth = opts->label_smooth;
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R, opts->obj_iou_ratio > 0.f);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    const float cls_lo = 0.5f * label_smooth, cls_hi = 1.0f - cls_lo;
    const long long total = (long long)B * A * F * F * (5 + n_classes);
    if (loss_opts_any(opts)) {
        hipLaunchKernelGGL((yolo_loss_bwd_kernel<true, LossOptK>), dim3(grid_for(total)), dim3(256), 0, y4_stream(stream), output,
                           output_is_masked, obj_mask, gscale, g_output, B, F, A, R, n_classes, l.cw, cls_lo, cls_hi, w,
                           loss_opt_k(opts, workspace, l));
        Y4_CHECK_LAUNCH();
        return Y4_OK;
    }
    hipLaunchKernelGGL(yolo_loss_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, y4_stream(stream), output,
                       output_is_masked, obj_mask,
                       gscale, g_output, B, F, A, R, n_classes, l.cw, cls_lo, cls_hi, w);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_loss_bwd_ex_f32(const float* output, int output_is_masked, const float* obj_mask,
                            const float* gscale, float* g_output,
                            int B, int F, int A, int K, int n_classes, float iou_thresh, float label_smooth,
                            const void* workspace, size_t workspace_bytes, void* stream) {
    const y4_loss_opts o = loss_opts_default(iou_thresh, label_smooth);
    return y4_yolo_loss_bwd_opts_f32(output, output_is_masked, obj_mask, gscale, g_output, B, F, A, K, n_classes, &o,
                                     workspace, workspace_bytes, stream);
}

int y4_yolo_loss_bwd_f32(const float* output, int output_is_masked, const float* obj_mask,
                         const float* gscale, float* g_output,
                         int B, int F, int A, int K, int n_classes,
                         const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_loss_bwd_ex_f32(output, output_is_masked, obj_mask, gscale, g_output, B, F, A, K, n_classes, 1.0f, 0.0f,
                                   workspace, workspace_bytes, stream);
}

int y4_yolo_loss_mask_output_ex_f32(float* output, const float* obj_mask, int B, int F, int A, int K,
                                    int n_classes, float iou_thresh, const void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (!output || !obj_mask || !workspace) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || !loss_opts_ok(iou_thresh, 0.f)) return Y4_ERR_SHAPE;
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    const long long total = (long long)B * A * F * F * (5 + n_classes);
    hipLaunchKernelGGL(yolo_loss_mask_output_kernel, dim3(grid_for(total)), dim3(256), 0, y4_stream(stream), output,
                       obj_mask, B, F, A, R, n_classes, w);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_yolo_loss_stats_scratch(int B, int F, int A) {
    if (B <= 0 || F <= 0 || A <= 0) return 0;
    const long long cells = (long long)B * A * F * F;
    return (size_t)((cells + LOSS_BLOCK - 1) / LOSS_BLOCK) * STATS_P * sizeof(double);
}

int y4_yolo_loss_stats_f64(const float* output, const float* pred, const float* obj_mask, int B, int F, int A, int K,
                           int n_classes, const y4_loss_opts* opts, const void* workspace, size_t workspace_bytes,
                           void* scratch, size_t scratch_bytes, double* stats_row, void* stream) {
    if (!output || !pred || !obj_mask || !opts || !workspace || !scratch || !stats_row) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || !loss_opts_all_ok(opts)) return Y4_ERR_SHAPE;
    const int R = loss_rec_cap(K, A, opts->iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R, opts->obj_iou_ratio > 0.f);
    if (workspace_bytes < l.total || scratch_bytes < y4_yolo_loss_stats_scratch(B, F, A)) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    double* partials = static_cast<double*>(scratch);
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(yolo_loss_stats_kernel, dim3(l.nblocks), dim3(LOSS_BLOCK), 0, st, output, pred, obj_mask, B, F, A, R,
                       n_classes, l.cw, w, partials);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(yolo_loss_stats_fold_kernel, dim3(1), dim3(256), 0, st, partials, l.nblocks,
                       (double)((long long)B * A * F * F), stats_row);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_loss_mask_output_f32(float* output, const float* obj_mask, int B, int F, int A, int K,
                                 int n_classes, const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_loss_mask_output_ex_f32(output, obj_mask, B, F, A, K, n_classes, 1.0f, workspace, workspace_bytes, stream);
}

int y4_yolo_loss_dense_targets_opts_f32(float* target, float* tgt_mask, float* tgt_scale,
                                        int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts,
                                        const void* workspace, size_t workspace_bytes, void* stream) {
    if (!target || !tgt_mask || !tgt_scale || !workspace || !opts) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || !loss_opts_all_ok(opts)) return Y4_ERR_SHAPE;
    const float iou_thresh = opts->iou_thresh, label_smooth = opts->label_smooth;
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R, opts->obj_iou_ratio > 0.f);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    const float cls_lo = 0.5f * label_smooth, cls_hi = 1.0f - cls_lo;
    hipStream_t st = y4_stream(stream);
    const size_t cells = (size_t)B * A * F * F;
    if (hipMemsetAsync(target, 0, cells * (5 + n_classes) * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    if (hipMemsetAsync(tgt_mask, 0, cells * (4 + n_classes) * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    if (hipMemsetAsync(tgt_scale, 0, cells * 2 * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    const long long slots = (long long)B * R;
    hipLaunchKernelGGL(yolo_dense_targets_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, target, tgt_mask,
                       tgt_scale, B, F, A, R, n_classes, l.cw, cls_lo, cls_hi, w,
                       (const float*)loss_opt_k(opts, workspace, l).pos_obj);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_loss_dense_targets_ex_f32(float* target, float* tgt_mask, float* tgt_scale,
                                      int B, int F, int A, int K, int n_classes, float iou_thresh, float label_smooth,
                                      const void* workspace, size_t workspace_bytes, void* stream) {
    const y4_loss_opts o = loss_opts_default(iou_thresh, label_smooth);
    return y4_yolo_loss_dense_targets_opts_f32(target, tgt_mask, tgt_scale, B, F, A, K, n_classes, &o, workspace,
                                               workspace_bytes, stream);
}

int y4_yolo_loss_dense_targets_f32(float* target, float* tgt_mask, float* tgt_scale,
                                   int B, int F, int A, int K, int n_classes,
                                   const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_loss_dense_targets_ex_f32(target, tgt_mask, tgt_scale, B, F, A, K, n_classes, 1.0f, 0.0f, workspace,
                                             workspace_bytes, stream);
}

static bool box_kind_ok(int kind) { return kind >= Y4_BOX_IOU && kind <= Y4_BOX_CIOU; }

int y4_yolo_box_loss_fwd_ex_f32(const float* pred, int box_kind, float gain, int B, int F, int A, int K, int n_classes,
                                float iou_thresh, double* loss_parts, const void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!pred || !loss_parts || !workspace) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || (long long)A * F * F >= (1ll << 31) || !box_kind_ok(box_kind) ||
        !loss_opts_ok(iou_thresh, 0.f)) return Y4_ERR_SHAPE;
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    hipLaunchKernelGGL(yolo_box_loss_fwd_kernel, dim3(1), dim3(BOX_BLOCK), 0, y4_stream(stream), pred, box_kind, gain,
                       B, F, A, R, w, loss_parts);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_box_loss_fwd_f32(const float* pred, int box_kind, float gain, int B, int F, int A, int K, int n_classes,
                             double* loss_parts, const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_box_loss_fwd_ex_f32(pred, box_kind, gain, B, F, A, K, n_classes, 1.0f, loss_parts, workspace,
                                       workspace_bytes, stream);
}

int y4_yolo_box_loss_bwd_ex_f32(const float* pred, int box_kind, float gain, const float* gscale, float* g_output,
                                int B, int F, int A, int K, int n_classes, float iou_thresh, float scale_xy,
                                const void* workspace, size_t workspace_bytes, void* stream) {
    if (!pred || !gscale || !g_output || !workspace) return Y4_ERR_NULL;
    if (!loss_dims_ok(B, F, A, K, n_classes) || (long long)A * F * F >= (1ll << 31) || !box_kind_ok(box_kind) ||
        !loss_opts_ok(iou_thresh, 0.f) || !scale_xy_ok(scale_xy)) return Y4_ERR_SHAPE;
    const int R = loss_rec_cap(K, A, iou_thresh);
    const LossWs l = loss_ws(B, F, A, K, n_classes, R);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    const LossPtrs w = loss_ptrs(workspace, l);
    const long long slots = (long long)B * R;
    hipLaunchKernelGGL(yolo_box_loss_bwd_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, y4_stream(stream),
                       pred, box_kind, gain, gscale, g_output, B, F, A, R, 5 + n_classes, scale_xy, w);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_box_loss_bwd_f32(const float* pred, int box_kind, float gain, const float* gscale, float* g_output,
                             int B, int F, int A, int K, int n_classes,
                             const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_box_loss_bwd_ex_f32(pred, box_kind, gain, gscale, g_output, B, F, A, K, n_classes, 1.0f, 1.0f, workspace,
                                       workspace_bytes, stream);
}

int y4_post_count_ex_f32(float* prediction, int B, long long N, int n_classes, float conf_thre,
                         int convert_xyxy, int agnostic, int* counts, void* stream) {
    if (!prediction || !counts) return Y4_ERR_NULL;
    if (B <= 0 || N <= 0 || n_classes <= 0 || (agnostic != 0 && agnostic != 1)) return Y4_ERR_SHAPE;
    if (agnostic && N * n_classes >= (1ll << 31)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    if (hipMemsetAsync(counts, 0, (size_t)B * (agnostic ? 1 : n_classes) * 4, st) != hipSuccess) return Y4_ERR_LAUNCH;
    const int pitch = (5 + n_classes) | 1;
    const size_t smem = (size_t)POST_ROWS * pitch * 4 + (size_t)2 * n_classes * 4;     // tile + the two histograms
    if (5 + n_classes <= POST_MAX_NCH && smem <= 65536) {                             // (64 KiB: the default dynamic-LDS limit)
        const long long ntiles = ((long long)B * N + POST_ROWS - 1) / POST_ROWS;
        auto kern = agnostic ? post_count_tiled_kernel<true> : post_count_tiled_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(ntiles < 2048 ? ntiles : 2048)), dim3(256), smem, st,
                           prediction, B, N, n_classes, conf_thre, convert_xyxy, counts);
    } else {
        auto kern = agnostic ? post_count_kernel<true> : post_count_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(grid_for((long long)B * N)), dim3(256), 0, st, prediction, B, N,
                           n_classes, conf_thre, convert_xyxy, counts);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_post_count_f32(float* prediction, int B, long long N, int n_classes, float conf_thre,
                      int convert_xyxy, int* counts, void* stream) {
    return y4_post_count_ex_f32(prediction, B, N, n_classes, conf_thre, convert_xyxy, 0, counts, stream);
}

int y4_post_scan_i32(const int* counts, int n_segments, long long cap, int* seg_offsets, int* info, void* stream) {
    if (!counts || !seg_offsets || !info) return Y4_ERR_NULL;
    if (n_segments <= 0 || cap <= 0 || cap >= (1ll << 31)) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(post_scan_kernel, dim3(1), dim3(1024), 0, y4_stream(stream), counts, n_segments, cap, seg_offsets, info);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_post_compact_f32(const float* det_rows, const int* seg_offsets, const int* kept, int B, int n_classes,
                        float* out_rows, int* out_offsets, int* img_offsets, void* stream) {
    if (!det_rows || !seg_offsets || !kept || !out_rows || !out_offsets || !img_offsets) return Y4_ERR_NULL;
    if (B <= 0 || n_classes <= 0) return Y4_ERR_SHAPE;
    const int nseg = B * n_classes;
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(post_out_scan_kernel, dim3(1), dim3(1024), 0, st, kept, nseg, n_classes, B, out_offsets, img_offsets);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(post_compact_kernel, dim3(nseg), dim3(64), 0, st, det_rows, seg_offsets, kept, out_offsets, out_rows);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_post_nms_workspace(long long total_candidates, int n_segments) {
    return post_ws(total_candidates, n_segments).total;
}

size_t y4_post_nms_ex_workspace(long long total_candidates, int n_segments, const y4_nms_opts* opts) {
    if (!opts || !nms_opts_ok(opts)) return 0;
    return post_ex_ws(total_candidates, n_segments, opts->soft != Y4_SOFT_NONE).total;
}

int y4_post_nms_ex_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre, float nms_thre,
                       const y4_nms_opts* opts, const int* seg_offsets, long long total_candidates,
                       float* det_rows, int* kept, void* workspace, size_t workspace_bytes, void* stream) {
    if (!prediction || !opts || !seg_offsets || !det_rows || !kept || !workspace) return Y4_ERR_NULL;
    if (B <= 0 || N <= 0 || N >= (1ll << 31) || n_classes <= 0 || total_candidates < 0 ||
        total_candidates >= (1ll << 31) || !nms_opts_ok(opts)) return Y4_ERR_SHAPE;
    const bool agn = opts->agnostic != 0, soft = opts->soft != Y4_SOFT_NONE, diou = opts->metric == Y4_NMS_DIOU;
    if (agn && N * n_classes >= (1ll << 31)) return Y4_ERR_SHAPE;
    const int nseg = agn ? B : B * n_classes;
    const PostExWs lx = post_ex_ws(total_candidates, nseg, soft);
    const PostWs& l = lx.base;
    if (workspace_bytes < lx.total) return Y4_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    int* cursor = reinterpret_cast<int*>(base + l.cursor);
    hipStream_t st = y4_stream(stream);
    if (const int rc = post_fill_keys(prediction, B, N, n_classes, conf_thre, agn, seg_offsets, nseg, cursor, keys, st)) return rc;
    float4* kbox = reinterpret_cast<float4*>(base + l.kbox);
    float* karea = reinterpret_cast<float*>(base + l.karea);
    int* kpos = reinterpret_cast<int*>(base + l.kpos);
    if (!soft) {
        auto kern = diou ? (agn ? post_nms_kernel<Y4_NMS_DIOU, true> : post_nms_kernel<Y4_NMS_DIOU, false>)
                         : (agn ? post_nms_kernel<Y4_NMS_IOU, true> : post_nms_kernel<Y4_NMS_IOU, false>);
        hipLaunchKernelGGL(kern, dim3(nseg), dim3(256), 0, st, prediction, N, n_classes, nms_thre, opts->max_det, seg_offsets,
                           keys, kbox, karea, kpos, det_rows, kept);
    } else {
        auto kern = diou ? (agn ? post_soft_nms_kernel<Y4_NMS_DIOU, true> : post_soft_nms_kernel<Y4_NMS_DIOU, false>)
                         : (agn ? post_soft_nms_kernel<Y4_NMS_IOU, true> : post_soft_nms_kernel<Y4_NMS_IOU, false>);
        hipLaunchKernelGGL(kern, dim3(nseg), dim3(256), 0, st, prediction, N, n_classes, nms_thre, opts->soft, opts->sigma,
                           conf_thre, opts->max_det, seg_offsets, keys, kbox, karea, reinterpret_cast<float*>(base + lx.w),
                           reinterpret_cast<unsigned char*>(base + lx.alive), kpos, reinterpret_cast<float*>(base + lx.ew),
                           det_rows, kept);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_post_nms_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre,
                    float nms_thre, const int* seg_offsets, long long total_candidates,
                    float* det_rows, int* kept, void* workspace, size_t workspace_bytes, void* stream) {
    y4_nms_opts opts = {};
    opts.metric = Y4_NMS_IOU; opts.soft = Y4_SOFT_NONE; opts.sigma = 0.5f;
    return y4_post_nms_ex_f32(prediction, B, N, n_classes, conf_thre, nms_thre, &opts, seg_offsets, total_candidates,
                              det_rows, kept, workspace, workspace_bytes, stream);
}

size_t y4_post_wbf_workspace(long long total_candidates, int n_segments) {
    return wbf_ws(total_candidates, n_segments).total;
}

int y4_post_wbf_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre, float iou_thre, int agnostic,
                    int n_views, const int* seg_offsets, long long total_candidates, float* det_rows, int* kept,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!prediction || !seg_offsets || !det_rows || !kept || !workspace) return Y4_ERR_NULL;
    if (B <= 0 || N <= 0 || N >= (1ll << 31) || n_classes <= 0 || total_candidates < 0 || total_candidates >= (1ll << 31) ||
        n_views < 1 || (agnostic != 0 && agnostic != 1) || !(iou_thre >= 0.f)) return Y4_ERR_SHAPE;
    const bool agn = agnostic != 0;
    if (agn && N * n_classes >= (1ll << 31)) return Y4_ERR_SHAPE;
    if (!agn && (long long)B * n_classes >= (1ll << 31)) return Y4_ERR_SHAPE;
    const int nseg = agn ? B : B * n_classes;
    const WbfWs l = wbf_ws(total_candidates, nseg);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    int* cursor = reinterpret_cast<int*>(base + l.cursor);
    hipStream_t st = y4_stream(stream);
    if (const int rc = post_fill_keys(prediction, B, N, n_classes, conf_thre, agn, seg_offsets, nseg, cursor, keys, st)) return rc;
    auto kern = agn ? post_wbf_kernel<true> : post_wbf_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(nseg), dim3(256), 0, st, prediction, N, n_classes, iou_thre, n_views, seg_offsets, keys,
                       reinterpret_cast<float4*>(base + l.cbox), reinterpret_cast<float*>(base + l.cs),
                       reinterpret_cast<int*>(base + l.ccls), reinterpret_cast<float4*>(base + l.F),
                       reinterpret_cast<float4*>(base + l.sum), reinterpret_cast<float*>(base + l.S),
                       reinterpret_cast<int*>(base + l.cnt), reinterpret_cast<int*>(base + l.cls), det_rows, kept);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_post_topk_workspace(long long total_candidates, int n_segments) {
    return topk_ws(total_candidates, n_segments).total;
}

int y4_post_topk_compact_f32(const float* det_rows, const int* seg_offsets, const int* kept, int B, int segs_per_image,
                             int max_det, long long total_candidates, float* out_rows, int* out_offsets,
                             int* img_offsets, void* workspace, size_t workspace_bytes, void* stream) {
    if (!det_rows || !seg_offsets || !kept || !out_rows || !out_offsets || !img_offsets || !workspace) return Y4_ERR_NULL;
    if (B <= 0 || segs_per_image <= 0 || max_det <= 0 || total_candidates < 0 || total_candidates >= (1ll << 31) ||
        (long long)B * segs_per_image >= (1ll << 31)) return Y4_ERR_SHAPE;
    const int nseg = B * segs_per_image;
    const TopkWs l = topk_ws(total_candidates, nseg);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    int* flags = reinterpret_cast<int*>(base + l.flags);
    int* kept2 = reinterpret_cast<int*>(base + l.kept2);
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(post_topk_kernel, dim3(B), dim3(256), 0, st, det_rows, seg_offsets, kept, segs_per_image, max_det,
                       reinterpret_cast<unsigned long long*>(base + l.keys), flags, kept2);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(post_out_scan_kernel, dim3(1), dim3(1024), 0, st, kept2, nseg, segs_per_image, B, out_offsets, img_offsets);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(post_compact_flagged_kernel, dim3(nseg), dim3(64), 0, st, det_rows, seg_offsets, kept, flags,
                       out_offsets, out_rows);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

size_t y4_nms_workspace(long long R) { return post_ws(R, 1).total; }

int y4_nms_f32(const float* boxes, const float* scores, long long R, float thresh, int limit,
               int* keep_idx, int* n_keep, void* workspace, size_t workspace_bytes, void* stream) {
    if (!boxes || !keep_idx || !n_keep || !workspace) return Y4_ERR_NULL;
    if (R <= 0 || R >= (1ll << 30)) return Y4_ERR_SHAPE;
    const PostWs l = post_ws(R, 1);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    hipStream_t st = y4_stream(stream);
    hipLaunchKernelGGL(nms_keys_kernel, dim3(grid_for(R)), dim3(256), 0, st, scores, R, keys);
    Y4_CHECK_LAUNCH();
    hipLaunchKernelGGL(nms_single_kernel, dim3(1), dim3(256), 0, st, boxes, (int)R, thresh, limit, keys,
                       reinterpret_cast<float4*>(base + l.kbox), reinterpret_cast<float*>(base + l.karea),
                       reinterpret_cast<int*>(base + l.kpos), keep_idx, n_keep);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

}  // extern "C"
