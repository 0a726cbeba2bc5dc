// YOLO head, anchor decode (training and eval, square and rectangular maps) and its gradient.  No MFMA here: HBM-bound
// sweeps.  The loss is yolo_loss.hip, the post-processing postprocess.hip.
//
// This file is compiled with -ffp-contract=off like the other two: with scale_x_y = 1 the centre is the reference's
// separate fp32 multiply / add sequence bit for bit.
#include "yolo_head_common.h"

namespace {

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

// Every forward decode: validate, fill the anchors, pick the tile height, then the tiled kernel where its conditions hold
// and the per-channel one elsewhere.  Training (EVAL = false) writes `output` and `pred` of a square map (n_total,
// box_off and stride are 0, 0, 1); eval writes rows [box_off, box_off + A * Fh * Fw) of `output` [B, n_total, n_ch] and
// has no `pred`.  RECT picks the rectangular instances: only y4_yolo_decode_eval_rect_f32 asks for them, also at Fh == Fw.
template <bool EVAL, bool RECT>
int decode_launch(const float* logits, int ldl, float* output, float* pred, long long n_total, long long box_off,
                  int B, int Fh, int Fw, int A, int n_classes, const float* anchors_wh_host, float stride, float scale_xy,
                  void* stream) {
    if (!logits || !output || (!EVAL && !pred)) return Y4_ERR_NULL;
    const int n_ch = 5 + n_classes;
    Anchors anc;
    if (B <= 0 || Fh <= 0 || Fw <= 0 || A <= 0 || n_classes <= 0 || ldl < A * n_ch || !fill_anchors(anc, anchors_wh_host, A) ||
        !scale_xy_ok(scale_xy))
        return Y4_ERR_SHAPE;
    const long long FF = (long long)Fh * Fw;
    if (RECT && FF >= (1ll << 31)) return Y4_ERR_SHAPE;
    if (EVAL && (box_off < 0 || box_off + (long long)A * FF > n_total)) return Y4_ERR_SHAPE;
    const float hxy = (scale_xy - 1.0f) * 0.5f;
    const long long npix = (long long)B * FF;
    const int tp = decode_tp(npix);
    const long long tpi = (FF + tp - 1) / tp;
    if (decode_tiled_ok(logits, ldl, A, n_ch, output, pred) && (long long)B * tpi < (1ll << 31)) {
        const bool sc = scale_xy != 1.0f;
        auto kern = tp == 16 ? (sc ? yolo_decode_tiled_kernel<EVAL, 16, true, RECT> : yolo_decode_tiled_kernel<EVAL, 16, false, RECT>)
                             : (sc ? yolo_decode_tiled_kernel<EVAL, 32, true, RECT> : yolo_decode_tiled_kernel<EVAL, 32, false, RECT>);
        hipLaunchKernelGGL(kern, dim3((unsigned)(B * tpi)), dim3(256), 0, y4_stream(stream), logits, (long long)ldl, output,
                           pred, n_total, box_off, stride, Fw, A, n_ch, anc, (int)tpi, scale_xy, hxy, Fh);
    } else {
        hipLaunchKernelGGL((yolo_decode_kernel<EVAL, RECT>), dim3((unsigned)(npix < 8192 ? npix : 8192)), dim3(256), 0,
                           y4_stream(stream), logits, (long long)ldl, output, pred, n_total, box_off, stride, B, Fw, A, n_ch,
                           anc, scale_xy, hxy, Fh);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

}  // namespace

extern "C" {

int y4_yolo_decode_train_ex_f32(const float* logits, int ldl, float* output, float* pred,
                                int B, int F, int A, int n_classes, const float* anchors_wh_host, float scale_xy,
                                void* stream) {
    return decode_launch<false, false>(logits, ldl, output, pred, 0ll, 0ll, B, F, F, A, n_classes, anchors_wh_host, 1.0f,
                                       scale_xy, stream);
}

int y4_yolo_decode_train_f32(const float* logits, int ldl, float* output, float* pred,
                             int B, int F, int A, int n_classes, const float* anchors_wh_host, void* stream) {
    return y4_yolo_decode_train_ex_f32(logits, ldl, output, pred, B, F, A, n_classes, anchors_wh_host, 1.0f, stream);
}

int y4_yolo_decode_eval_ex_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                               int B, int F, int A, int n_classes, const float* anchors_wh_host,
                               float stride, float scale_xy, void* stream) {
    return decode_launch<true, false>(logits, ldl, out, nullptr, n_total, box_off, B, F, F, A, n_classes, anchors_wh_host,
                                      stride, scale_xy, stream);
}

int y4_yolo_decode_eval_rect_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                                 int B, int Fh, int Fw, int A, int n_classes, const float* anchors_wh_host,
                                 float stride, float scale_xy, void* stream) {
    return decode_launch<true, true>(logits, ldl, out, nullptr, n_total, box_off, B, Fh, Fw, A, n_classes, anchors_wh_host,
                                     stride, scale_xy, stream);
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

}  // extern "C"
