// COCO bbox evaluation (the COCOeval protocol the reference runs after validate(), yolo/engine/build.py:172-188) as two
// launches: a greedy match per (image, category) cell and a sorted scan per (category, area range, maxDets, IoU threshold).
// Every output is an integer count or ONE fp64 quotient of integers, so the results do not depend on block shape or order;
// the IoU is fp64 in the operation order the header states (this file is built with -ffp-contract=off).
#include "common.h"

namespace {

constexpr int kT = 10, kA = 4, kM = 3, kR = 101;
constexpr int kTA = kT * kA;          // (threshold, area range) sequences of one cell: one lane each
constexpr int kMaxDet = 100;          // detections kept per cell
constexpr int kGtChunk = 64;          // gts staged in LDS at a time
constexpr int kLdsWords = 8;          // "already matched" bits held in LDS: cells of up to 32 * 8 = 256 gts
constexpr int kMatchBlocks = 2048;    // grid of the match launch (blocks walk the cells with this stride)
constexpr int kAccThreads = 256;

// ------------------------------------------------------------------------------------------------------------ match

// One cell.  Lane l < 40 owns the sequence t = l % 10, a = l / 10 and walks the detections in rank order; for every detection
// it goes over the gts once, carrying the best counted gt (pass 1 of the header) and the best ignored gt (pass 2) side by
// side: pass 2 only counts when pass 1 found nothing, and then `best` still holds its start value.
// WS: the matched bits of this cell live in the caller's workspace (row of this block) instead of LDS.
template <bool WS>
__device__ __forceinline__ void match_cell(const double* __restrict__ gbox, const double* __restrict__ garea,
                                           const int* __restrict__ gcrowd, int g0, int ng, int nd, const double* s_d,
                                           double* s_g, double* s_ga, int* s_gc, unsigned* s_m, unsigned char* s_code,
                                           unsigned* __restrict__ ws_row, double best0, double lo, double hi) {
    const int lane = threadIdx.x;
    const bool active = lane < kTA;
    const int nw = (ng + 31) >> 5;
    auto mword = [&](int w) -> unsigned& {
        if constexpr (WS) return ws_row[(size_t)w * kTA + lane];
        else return s_m[w * kTA + lane];
    };
    auto stage = [&](int c0, int cn) {
        for (int j = lane; j < cn * 4; j += 64) s_g[j] = gbox[(size_t)(g0 + c0) * 4 + j];
        for (int j = lane; j < cn; j += 64) {
            s_ga[j] = garea[g0 + c0 + j];
            s_gc[j] = gcrowd[g0 + c0 + j];
        }
    };
    if (active)
        for (int w = 0; w < nw; ++w) mword(w) = 0u;
    const bool one = ng <= kGtChunk;
    if (one) stage(0, ng);
    __syncthreads();
    for (int d = 0; d < nd; ++d) {
        const double dx = s_d[4 * d], dy = s_d[4 * d + 1], dw = s_d[4 * d + 2], dh = s_d[4 * d + 3];
        const double dx2 = dx + dw, dy2 = dy + dh, da = dw * dh;
        double best1 = best0, best2 = best0;
        int m1 = -1, m2 = -1;
        for (int c0 = 0; c0 < ng; c0 += kGtChunk) {
            const int cn = min(kGtChunk, ng - c0);
            if (!one) {
                __syncthreads();
                stage(c0, cn);
                __syncthreads();
            }
            if (active) {
                for (int j = 0; j < cn; ++j) {
                    const int g = c0 + j;
                    const double gx = s_g[4 * j], gy = s_g[4 * j + 1], gw = s_g[4 * j + 2], gh = s_g[4 * j + 3];
                    const bool crowd = s_gc[j] != 0;
                    const double ar = s_ga[j];
                    const double gx2 = gx + gw, gy2 = gy + gh;
                    const double w = (gx2 < dx2 ? gx2 : dx2) - (gx > dx ? gx : dx);
                    const double h = (gy2 < dy2 ? gy2 : dy2) - (gy > dy ? gy : dy);
                    double v = 0.0;
                    if (!(w <= 0.0 || h <= 0.0)) {
                        const double i = w * h;
                        const double u = crowd ? da : da + gw * gh - i;
                        v = i / u;
                    }
                    const bool ign = crowd || ar < lo || ar > hi;
                    const bool taken = (mword(g >> 5) >> (g & 31)) & 1u;
                    if (!ign) {
                        if (!taken && !(v < best1)) { best1 = v; m1 = g; }
                    } else {
                        if ((!taken || crowd) && !(v < best2)) { best2 = v; m2 = g; }
                    }
                }
            }
        }
        if (active) {
            const int m = m1 >= 0 ? m1 : m2;
            unsigned code;
            if (m >= 0) {
                mword(m >> 5) |= 1u << (m & 31);
                code = m1 >= 0 ? 1u : 3u;
            } else {
                code = (da < lo || da > hi) ? 2u : 0u;
            }
            s_code[d * kTA + lane] = (unsigned char)code;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void coco_match_kernel(const double* __restrict__ dbox, const int* __restrict__ det_off,
                                                        const double* __restrict__ gbox, const double* __restrict__ garea,
                                                        const int* __restrict__ gcrowd, const int* __restrict__ gt_off,
                                                        int n_cells, int n_det, const double* __restrict__ iou_thrs,
                                                        const double* __restrict__ area_rng, unsigned* __restrict__ codes,
                                                        int* __restrict__ npig, unsigned* __restrict__ ws, int ws_words) {
    __shared__ double s_d[kMaxDet * 4];
    __shared__ double s_g[kGtChunk * 4];
    __shared__ double s_ga[kGtChunk];
    __shared__ int s_gc[kGtChunk];
    __shared__ unsigned s_m[kLdsWords * kTA];
    __shared__ unsigned char s_code[kMaxDet * kTA];
    const int lane = threadIdx.x;
    const int t = lane < kTA ? lane % kT : 0, a = lane < kTA ? lane / kT : 0;
    const double thr = iou_thrs[t];
    const double cap = 1.0 - 1e-10;
    const double best0 = cap < thr ? cap : thr;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    unsigned* ws_row = ws ? ws + (size_t)blockIdx.x * ws_words * kTA : nullptr;

    for (int cell = blockIdx.x; cell < n_cells; cell += gridDim.x) {
        const int d0 = det_off[cell], g0 = gt_off[cell];
        const int nd = min(max(det_off[cell + 1] - d0, 0), kMaxDet);
        const int ng = max(gt_off[cell + 1] - g0, 0);
        for (int j = lane; j < nd * 4; j += 64) s_d[j] = dbox[(size_t)d0 * 4 + j];
        if (lane < kTA && t == 0) {                      // non-ignored gts of (cell, a)
            int n = 0;
            for (int g = 0; g < ng; ++g) {
                const double ar = garea[g0 + g];
                n += (gcrowd[g0 + g] != 0 || ar < lo || ar > hi) ? 0 : 1;
            }
            npig[(size_t)cell * kA + a] = n;
        }
        const int nw = (ng + 31) >> 5;
        if (nw <= kLdsWords)
            match_cell<false>(gbox, garea, gcrowd, g0, ng, nd, s_d, s_g, s_ga, s_gc, s_m, s_code, nullptr, best0, lo, hi);
        else if (ws_row && nw <= ws_words)               // (the entry point has checked the workspace against the offsets)
            match_cell<true>(gbox, garea, gcrowd, g0, ng, nd, s_d, s_g, s_ga, s_gc, s_m, s_code, ws_row, best0, lo, hi);
        else
            continue;
        // ten 2-bit codes of one (area range, detection) -> one word
        for (int j = lane; j < nd * kA; j += 64) {
            const int aa = j / nd, d = j - aa * nd;
            unsigned wd = 0u;
            for (int tt = 0; tt < kT; ++tt) wd |= (unsigned)s_code[d * kTA + aa * kT + tt] << (2 * tt);
            codes[(size_t)aa * n_det + d0 + d] = wd;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------- accumulate

struct Cnt {
    int tp, fp, nf;
};

// inclusive scan over the 256 threads of (tp, fp, nf) by addition and of e by maximum; `tot`/`emax` = the block's totals
__device__ __forceinline__ void block_scan(Cnt& c, double& e, Cnt& tot, double& emax, Cnt* s_wc, double* s_we) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(c.tp, o), b = __shfl_up(c.fp, o), n = __shfl_up(c.nf, o);
        const double x = __shfl_up(e, o);
        if (lane >= o) {
            c.tp += a;
            c.fp += b;
            c.nf += n;
            e = x > e ? x : e;
        }
    }
    __syncthreads();                                     // the previous use of s_wc / s_we is over
    if (lane == 63) {
        s_wc[wv] = c;
        s_we[wv] = e;
    }
    __syncthreads();
    tot = Cnt{0, 0, 0};
    emax = -1.0;
    for (int k = 0; k < kAccThreads / 64; ++k) {
        const Cnt o = s_wc[k];
        const double x = s_we[k];
        if (k < wv) {
            c.tp += o.tp;
            c.fp += o.fp;
            c.nf += o.nf;
            e = x > e ? x : e;
        }
        tot.tp += o.tp;
        tot.fp += o.fp;
        tot.nf += o.nf;
        emax = x > emax ? x : emax;
    }
}

// One block per (k, a, m, t).  Pass 1: totals of tp / fp / listed detections over the category's segment.  Pass 2 walks the
// segment backwards in chunks of 256 (thread i takes the i-th entry from the chunk's end, so a prefix scan over threads is a
// suffix scan over entries; the carry is the sum over the chunks behind): prefix counts = totals - suffix counts, precision
// of each listed entry, its running maximum from the right, and at every entry where tp steps (or the first listed one) that
// maximum goes to the recall thresholds in (rc[i-1], rc[i]].
__global__ __launch_bounds__(kAccThreads) void coco_accumulate_kernel(
    const unsigned* __restrict__ codes, const unsigned char* __restrict__ rank, const int* __restrict__ order,
    const int* __restrict__ cat_off, const long long* __restrict__ npig_cat, const double* __restrict__ rec_thrs, int md0,
    int md1, int md2, int K, int n_det, double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ double s_q[kR];
    __shared__ Cnt s_wc[kAccThreads / 64];
    __shared__ double s_we[kAccThreads / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int t = b % kT, m = (b / kT) % kM, a = (b / (kT * kM)) % kA, k = b / (kT * kM * kA);
    const int md = m == 0 ? md0 : (m == 1 ? md1 : md2);
    const long long np = npig_cat[(size_t)k * kA + a];
    const size_t am = (size_t)a * kM + m;
    double* prow = precision + ((size_t)t * kR * K + k) * (kA * kM) + am;       // entry r at prow[r * K * 12]
    const size_t pstep = (size_t)K * (kA * kM);
    double* rout = recall + ((size_t)t * K + k) * (kA * kM) + am;
    if (np <= 0) {                                       // no counted gt (a category without a cell included): stays -1
        if (tid < kR) prow[tid * pstep] = -1.0;
        if (tid == 0) *rout = -1.0;
        return;
    }
    const int s0 = cat_off[k], s1 = cat_off[k + 1];
    const unsigned* crow = codes + (size_t)a * n_det;
    const int sh = 2 * t;
    if (tid < kR) s_q[tid] = 0.0;

    Cnt c{0, 0, 0}, tot, ctot;
    double e = -1.0, emax;
    for (int i = s0 + tid; i < s1; i += kAccThreads) {
        const int j = order[i];
        if ((int)rank[j] < md) {
            const unsigned cd = (crow[j] >> sh) & 3u;
            c.tp += cd == 1u;
            c.fp += cd == 0u;
            c.nf += 1;
        }
    }
    block_scan(c, e, tot, emax, s_wc, s_we);             // (also orders the zeroing of s_q before the writes below)

    const double dnp = (double)np;
    Cnt carry{0, 0, 0};
    double ecarry = -1.0;
    for (int hi = s1; hi > s0; hi -= kAccThreads) {
        const int i = hi - 1 - tid;
        Cnt f{0, 0, 0};
        if (i >= s0) {
            const int j = order[i];
            if ((int)rank[j] < md) {
                const unsigned cd = (crow[j] >> sh) & 3u;
                f.tp = cd == 1u;
                f.fp = cd == 0u;
                f.nf = 1;
            }
        }
        // suffix counts of the entries behind i, then the inclusive prefix counts of entry i
        Cnt sc = f;
        double pe = -1.0;
        // precision needs the prefix counts first: scan the counts, then the maximum
        block_scan(sc, pe, ctot, emax, s_wc, s_we);
        const int tp = tot.tp - (carry.tp + sc.tp - f.tp);
        const int fp = tot.fp - (carry.fp + sc.fp - f.fp);
        const int idx = tot.nf - (carry.nf + sc.nf - f.nf);                     // 1-based position in the listed detections
        double pr = -1.0;
        if (f.nf) pr = (double)tp / (((double)fp + (double)tp) + 0x1p-52);
        double env = pr;
        Cnt z{0, 0, 0}, ztot;
        double cmax;
        block_scan(z, env, ztot, cmax, s_wc, s_we);
        env = ecarry > env ? ecarry : env;
        if (f.nf && (f.tp || idx == 1)) {
            const double rc = (double)tp / dnp;
            int r = 0;
            if (idx != 1) {                              // tp stepped here: rc[i-1] = (tp - 1) / npig
                const double rp = (double)(tp - 1) / dnp;
                r = max((int)(rp * 100.0) - 1, 0);
                while (r < kR && rec_thrs[r] <= rp) ++r;
            }
            for (; r < kR && rec_thrs[r] <= rc; ++r) s_q[r] = env;
        }
        carry.tp += ctot.tp;
        carry.fp += ctot.fp;
        carry.nf += ctot.nf;
        ecarry = cmax > ecarry ? cmax : ecarry;
    }
    __syncthreads();
    if (tid < kR) prow[tid * pstep] = s_q[tid];
    if (tid == 0) *rout = tot.nf > 0 ? (double)tot.tp / dnp : 0.0;
}

// offsets as the host sees them: [0] == 0, non-decreasing, [n] == total, no segment longer than `cap` (0: any)
bool offsets_ok(const int* off, int n, long long total, int cap, int* longest) {
    if (off[0] != 0) return false;
    int mx = 0;
    for (int i = 0; i < n; ++i) {
        const long long d = (long long)off[i + 1] - off[i];
        if (d < 0 || (cap && d > cap)) return false;
        if (d > mx) mx = (int)d;
    }
    if (off[n] != total) return false;
    if (longest) *longest = mx;
    return true;
}

int ws_words_for(int max_gts) { return (max_gts + 31) / 32; }

}  // namespace

extern "C" size_t y4_coco_workspace(int n_cells, int max_gts_per_cell) {
    if (n_cells <= 0 || max_gts_per_cell <= 32 * kLdsWords) return 0;
    const size_t blocks = (size_t)(n_cells < kMatchBlocks ? n_cells : kMatchBlocks);
    return blocks * (size_t)ws_words_for(max_gts_per_cell) * kTA * sizeof(unsigned);
}

extern "C" int y4_coco_match_f64(const double* dbox, const int* det_off_dev, const int* det_off_host, int n_det,
                                 const double* gbox, const double* garea, const int* gcrowd, const int* gt_off_dev,
                                 const int* gt_off_host, int n_gt, int n_cells, const double* iou_thrs,
                                 const double* area_rng, unsigned int* codes, int* npig, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!dbox || !det_off_dev || !det_off_host || !gbox || !garea || !gcrowd || !gt_off_dev || !gt_off_host || !iou_thrs ||
        !area_rng || !codes || !npig)
        return Y4_ERR_NULL;
    if (n_det < 0 || n_gt < 0 || n_cells < 0 || n_det > (1 << 29)) return Y4_ERR_SHAPE;
    int max_gts = 0;
    if (!offsets_ok(det_off_host, n_cells, n_det, kMaxDet, nullptr) || !offsets_ok(gt_off_host, n_cells, n_gt, 0, &max_gts))
        return Y4_ERR_SHAPE;
    const size_t need = y4_coco_workspace(n_cells, max_gts);
    if (need && !workspace) return Y4_ERR_NULL;
    if (need > workspace_bytes) return Y4_ERR_WORKSPACE;
    if (n_cells == 0) return Y4_OK;
    const int blocks = n_cells < kMatchBlocks ? n_cells : kMatchBlocks;
    hipLaunchKernelGGL(coco_match_kernel, dim3(blocks), dim3(64), 0, y4_stream(stream), dbox, det_off_dev, gbox, garea, gcrowd,
                       gt_off_dev, n_cells, n_det, iou_thrs, area_rng, codes, npig, need ? (unsigned*)workspace : nullptr,
                       need ? ws_words_for(max_gts) : 0);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_coco_accumulate_f64(const unsigned int* codes, const unsigned char* rank, const int* order, int n_det,
                                      const int* cat_off_dev, const int* cat_off_host, const long long* npig_cat, int n_cat,
                                      const double* rec_thrs, const int* max_dets_host, double* precision, double* recall,
                                      void* stream) {
    if (!codes || !rank || !order || !cat_off_dev || !cat_off_host || !npig_cat || !rec_thrs || !max_dets_host || !precision ||
        !recall)
        return Y4_ERR_NULL;
    if (n_det < 0 || n_cat < 0 || n_det > (1 << 29) || n_cat > (1 << 20)) return Y4_ERR_SHAPE;
    for (int i = 0; i < kM; ++i)
        if (max_dets_host[i] < 0) return Y4_ERR_SHAPE;
    if (!offsets_ok(cat_off_host, n_cat, n_det, 0, nullptr)) return Y4_ERR_SHAPE;
    if (n_cat == 0) return Y4_OK;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)n_cat * (kT * kM * kA)), dim3(kAccThreads), 0, y4_stream(stream),
                       codes, rank, order, cat_off_dev, npig_cat, rec_thrs, max_dets_host[0], max_dets_host[1],
                       max_dets_host[2], n_cat, n_det, precision, recall);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
