// YOLO head, loss side: pairwise IoU, target assignment + detection loss (+ its gradient), the IoU-family box loss and
// the training statistics.  No MFMA here: HBM-bound sweeps, wavefront / block reductions.  The decode is yolo_decode.hip,
// the post-processing postprocess.hip.
//
// This file is compiled with -ffp-contract=off: IoU comparisons against thresholds must follow
// the reference's separate fp32 multiply / add / divide sequence bit for bit
// (yolo/model/yololoss.py:56-91).
#include "yolo_head_common.h"

namespace {

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
constexpr int LOSS_BLOCK = 256;
// R: records an image can hold per layer.  One positive anchor per label (iou_thresh >= 1): R = K.  Several (iou_thresh
// < 1): every label can be positive on each of the layer's A anchors, R = K * A.  With R = K the layout is unchanged.
static inline int loss_rec_cap(int K, int A, float iou_thresh) { return iou_thresh < 1.f ? K * A : K; }
static inline bool loss_opts_ok(float iou_thresh, float label_smooth) {          // false for NaN too
    return iou_thresh > 0.f && iou_thresh <= 1.f && label_smooth >= 0.f && label_smooth < 1.f;
}
// iou_obj (obj_iou_ratio > 0): pos_obj [B, R] is appended; without it offsets and total are what they were.
static LossWs loss_ws(int B, int F, int A, int K, int C, int R, bool iou_obj = false) {
    LossWs w;
    w.cw = (C + 31) / 32;
    const long long cells = (long long)B * A * F * F;
    w.nblocks = (int)((cells + LOSS_BLOCK - 1) / LOSS_BLOCK);
    Bump o;
    w.nlabel = o.take((size_t)B * 4);
    w.npos = o.take((size_t)B * 4);
    w.truth = o.take((size_t)B * K * 4 * 4);
    w.pos_cell = o.take((size_t)B * R * 4);
    w.pos_val = o.take((size_t)B * R * 5 * 4);
    w.pos_cls = o.take((size_t)B * R * w.cw * 4);
    w.pos_index = o.take((size_t)cells * 4);
    w.partials = o.take((size_t)w.nblocks * 4 * 8);
    w.pos_box = o.take((size_t)B * R * 4 * 4);                 // appended: every offset above is what it was without it
    w.pos_obj = o.take(iou_obj ? (size_t)B * R * 4 : 0);
    w.total = o.end;
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

// the shape conditions every loss entry shares; B * R * 5 and the record slots stay inside int
static bool loss_dims_ok(int B, int F, int A, int K, int n_classes) {
    return B > 0 && F > 0 && A > 0 && K > 0 && n_classes > 0 && (long long)B * K * A < (1ll << 31);
}

// What every entry that works on a filled (or to be filled) loss workspace does after its own NULL and option checks: the
// shared shape conditions, the record capacity, the layout (with pos_obj only where the entry's options have it: iou_obj),
// the size check and the pointers.  Y4_OK or the status to return.
struct LossCtx { int R; LossWs l; LossPtrs w; };
static int loss_begin(int B, int F, int A, int K, int n_classes, float iou_thresh, bool iou_obj, const void* workspace,
                      size_t workspace_bytes, LossCtx& c) {
    if (!loss_dims_ok(B, F, A, K, n_classes)) return Y4_ERR_SHAPE;
    c.R = loss_rec_cap(K, A, iou_thresh);
    c.l = loss_ws(B, F, A, K, n_classes, c.R, iou_obj);
    if (workspace_bytes < c.l.total) return Y4_ERR_WORKSPACE;
    c.w = loss_ptrs(workspace, c.l);
    return Y4_OK;
}
static int loss_begin(int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts, const void* workspace,
                      size_t workspace_bytes, LossCtx& c) {
    if (!loss_opts_all_ok(opts)) return Y4_ERR_SHAPE;
    return loss_begin(B, F, A, K, n_classes, opts->iou_thresh, opts->obj_iou_ratio > 0.f, workspace, workspace_bytes, c);
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
    // (the dims before the anchors: nothing is read through a pointer while a dimension is wrong)
    if (!loss_dims_ok(B, F, A, K, n_classes) || A != 3 || (long long)A * F * F >= (1ll << 31) || !loss_opts_all_ok(opts))
        return Y4_ERR_SHAPE;
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
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, opts, workspace, workspace_bytes, c)) return rc;
    const auto& [R, l, w] = c;
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
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, opts, workspace, workspace_bytes, c)) return rc;
    const auto& [R, l, w] = c;
    const float cls_lo = 0.5f * opts->label_smooth, cls_hi = 1.0f - cls_lo;
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
    if (!loss_opts_ok(iou_thresh, 0.f)) return Y4_ERR_SHAPE;
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, iou_thresh, false, workspace, workspace_bytes, c)) return rc;
    const long long total = (long long)B * A * F * F * (5 + n_classes);
    hipLaunchKernelGGL(yolo_loss_mask_output_kernel, dim3(grid_for(total)), dim3(256), 0, y4_stream(stream), output,
                       obj_mask, B, F, A, c.R, n_classes, c.w);
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
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, opts, workspace, workspace_bytes, c)) return rc;
    if (scratch_bytes < y4_yolo_loss_stats_scratch(B, F, A)) return Y4_ERR_WORKSPACE;
    const auto& [R, l, w] = c;
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
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, opts, workspace, workspace_bytes, c)) return rc;
    const auto& [R, l, w] = c;
    const float cls_lo = 0.5f * opts->label_smooth, cls_hi = 1.0f - cls_lo;
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

// what the two box-loss entries check beyond loss_begin(): a cell index inside int, the kind, the threshold
static bool box_loss_args_ok(int F, int A, int box_kind, float iou_thresh) {
    return (long long)A * F * F < (1ll << 31) && box_kind >= Y4_BOX_IOU && box_kind <= Y4_BOX_CIOU && loss_opts_ok(iou_thresh, 0.f);
}

int y4_yolo_box_loss_fwd_ex_f32(const float* pred, int box_kind, float gain, int B, int F, int A, int K, int n_classes,
                                float iou_thresh, double* loss_parts, const void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!pred || !loss_parts || !workspace) return Y4_ERR_NULL;
    if (!box_loss_args_ok(F, A, box_kind, iou_thresh)) return Y4_ERR_SHAPE;
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, iou_thresh, false, workspace, workspace_bytes, c)) return rc;
    hipLaunchKernelGGL(yolo_box_loss_fwd_kernel, dim3(1), dim3(BOX_BLOCK), 0, y4_stream(stream), pred, box_kind, gain,
                       B, F, A, c.R, c.w, loss_parts);
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
    if (!box_loss_args_ok(F, A, box_kind, iou_thresh) || !scale_xy_ok(scale_xy)) return Y4_ERR_SHAPE;
    LossCtx c;
    if (const int rc = loss_begin(B, F, A, K, n_classes, iou_thresh, false, workspace, workspace_bytes, c)) return rc;
    const long long slots = (long long)B * c.R;
    hipLaunchKernelGGL(yolo_box_loss_bwd_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, y4_stream(stream),
                       pred, box_kind, gain, gscale, g_output, B, F, A, c.R, 5 + n_classes, scale_xy, c.w);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

int y4_yolo_box_loss_bwd_f32(const float* pred, int box_kind, float gain, const float* gscale, float* g_output,
                             int B, int F, int A, int K, int n_classes,
                             const void* workspace, size_t workspace_bytes, void* stream) {
    return y4_yolo_box_loss_bwd_ex_f32(pred, box_kind, gain, gscale, g_output, B, F, A, K, n_classes, 1.0f, 1.0f, workspace,
                                       workspace_bytes, stream);
}
}  // extern "C"
