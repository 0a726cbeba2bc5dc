// YOLO head, post-processing: candidate count, key fill, and one block-wide bitonic sort + bitmask NMS (or Soft-NMS, or
// weighted box fusion) per (image, class) segment, the per-image cap and the compaction; the single-list nms().  No MFMA
// here: HBM-bound sweeps, wavefront / block reductions.  The decode is yolo_decode.hip, the loss yolo_loss.hip (DESIGN.md
// section 25).
//
// This file is compiled with -ffp-contract=off: IoU comparisons against thresholds must follow
// the reference's separate fp32 multiply / add / divide sequence bit for bit (yolo/util/utils.py:64-77).
//
// Post-processing options (include/yolov4_amd.h): the overlap measure (IoU | DIoU) is a template
// parameter of the suppression kernels, segments are (image, class) or whole images (AGN), Soft-NMS (linear | Gaussian
// decay) is one block per segment with its state in LDS, a per-image cap sorts the kept rows of an image.  The measure's
// fp32 operation order is written out at nms_measure; a float32 restatement of it is bit-equal (no fma contraction here).
#include "yolo_head_common.h"

namespace {

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

// ---- workspace layouts.  The members of each are listed in their order in memory and initialised in that order (a braced
// list evaluates left to right), `total` last.  An empty candidate list or segment list still gets one element.
struct PostWs { size_t keys, cursor, kbox, karea, kpos, total; };
// the hard layout; behind it the Soft-NMS state of segments above the LDS bound and the emitted (position, weight) lists
struct PostExWs { size_t keys, cursor, kbox, karea, kpos, w, ew, alive, total; };
struct TopkWs { size_t keys, flags, kept2, total; };
// WBF: keys and cursors as PostWs; the gathered candidates; the cluster state of segments above WBF_LDS_CLUSTERS
struct WbfWs { size_t keys, cursor, cbox, cs, ccls, F, sum, S, cnt, cls, total; };
static size_t one_or(long long n) { return (size_t)(n > 0 ? n : 1); }
static PostWs post_ws(long long total, int nseg) {
    const size_t t = one_or(total), s = one_or(nseg);
    Bump b;
    return {b.take(t * 8), b.take(s * 4), b.take(t * 16), b.take(t * 4), b.take(t * 4), b.end};
}
static PostExWs post_ex_ws(long long total, int nseg, bool soft) {
    const PostWs p = post_ws(total, nseg);
    const size_t t = soft ? one_or(total) : 0;
    Bump b{p.total};
    return {p.keys, p.cursor, p.kbox, p.karea, p.kpos, b.take(t * 4), b.take(t * 4), b.take(t), b.end};
}
static TopkWs topk_ws(long long total, int nseg) {
    const size_t t = one_or(total), s = one_or(nseg);
    Bump b;
    return {b.take(t * 8), b.take(t * 4), b.take(s * 4), b.end};
}
static WbfWs wbf_ws(long long total, int nseg) {
    const size_t t = one_or(total), s = one_or(nseg);
    Bump b;
    return {b.take(t * 8), b.take(s * 4), b.take(t * 16), b.take(t * 4), b.take(t * 4), b.take(t * 16), b.take(t * 16),
            b.take(t * 4), b.take(t * 4), b.take(t * 4), b.end};
}
static bool nms_opts_ok(const y4_nms_opts* o) {
    return (o->metric == Y4_NMS_IOU || o->metric == Y4_NMS_DIOU) &&
           (o->soft == Y4_SOFT_NONE || o->soft == Y4_SOFT_LINEAR || o->soft == Y4_SOFT_GAUSSIAN) &&
           !(o->soft == Y4_SOFT_GAUSSIAN && !(o->sigma > 0.f)) && (o->agnostic == 0 || o->agnostic == 1) && o->max_det >= 0;
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

// What y4_post_nms_ex_f32 and y4_post_wbf_f32 share after their NULL checks: the shape conditions on the common arguments
// (`rest_ok`: the entry's own), the segment count, the entry's layout l = ws_of(total_candidates, nseg) with its size
// check, and the candidates' keys filled into their segments.  Y4_OK or the status to return.
template <typename Ws, typename WsOf>
int post_segments_begin(const float* prediction, int B, long long N, int n_classes, float conf_thre, int agnostic,
                        bool rest_ok, const int* seg_offsets, long long total_candidates, void* workspace,
                        size_t workspace_bytes, hipStream_t st, WsOf ws_of, Ws& l, int& nseg, unsigned long long*& keys) {
    if (B <= 0 || N <= 0 || N >= (1ll << 31) || n_classes <= 0 || total_candidates < 0 ||
        total_candidates >= (1ll << 31) || !rest_ok) return Y4_ERR_SHAPE;
    const bool agn = agnostic != 0;
    if (agn && N * n_classes >= (1ll << 31)) return Y4_ERR_SHAPE;
    nseg = agn ? B : B * n_classes;
    l = ws_of(total_candidates, nseg);
    if (workspace_bytes < l.total) return Y4_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    return post_fill_keys(prediction, B, N, n_classes, conf_thre, agn, seg_offsets, nseg,
                          reinterpret_cast<int*>(base + l.cursor), keys, st);
}

}  // namespace

extern "C" {

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
    const bool agn = opts->agnostic != 0, soft = opts->soft != Y4_SOFT_NONE, diou = opts->metric == Y4_NMS_DIOU;
    hipStream_t st = y4_stream(stream);
    PostExWs l;
    int nseg;
    unsigned long long* keys;
    if (const int rc = post_segments_begin(prediction, B, N, n_classes, conf_thre, opts->agnostic, nms_opts_ok(opts),
                                           seg_offsets, total_candidates, workspace, workspace_bytes, st,
                                           [soft](long long t, int s) { return post_ex_ws(t, s, soft); }, l, nseg, keys))
        return rc;
    char* base = static_cast<char*>(workspace);
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
                           conf_thre, opts->max_det, seg_offsets, keys, kbox, karea, reinterpret_cast<float*>(base + l.w),
                           reinterpret_cast<unsigned char*>(base + l.alive), kpos, reinterpret_cast<float*>(base + l.ew),
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
    const bool agn = agnostic != 0;
    const bool rest_ok = n_views >= 1 && (agnostic == 0 || agnostic == 1) && iou_thre >= 0.f &&
                         (agn || (long long)B * n_classes < (1ll << 31));
    hipStream_t st = y4_stream(stream);
    WbfWs l;
    int nseg;
    unsigned long long* keys;
    if (const int rc = post_segments_begin(prediction, B, N, n_classes, conf_thre, agnostic, rest_ok, seg_offsets,
                                           total_candidates, workspace, workspace_bytes, st, wbf_ws, l, nseg, keys))
        return rc;
    char* base = static_cast<char*>(workspace);
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
