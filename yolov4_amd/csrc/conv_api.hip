// The conv C ABI: the conv mode, the forward / dgrad / wgrad entries of every mode with their workspace queries, the
// prepared-filter and amax entries, the split-K slab reduce and y4_last_conv_kernel.  The entries check their arguments and
// route: mode 3 (f16x2, the default) to conv_f16x2.hip, conv_tile.hip and wgrad_tile.hip, modes 0-2 to conv_igemm.hip;
// the only kernels here are the slab reduce's.
#include <stdlib.h>
#include "common.h"
#include <cstdarg>
#include <cstdio>
#include "conv_geom.h"

namespace {

using y4::ConvGeom;
using y4::WgradGeom;

// dw[n] = sum of `splits` slabs; vector variant: a block owns VEC float4 columns; its 256/VEC thread groups each add every (256/VEC)-th slab
// (4 independent loads in flight), then the groups are combined through LDS in group order -- a fixed
// summation tree for a given split count, hence deterministic, and hundreds of slabs no longer serialise
// behind one thread's load latency.
template <int VEC>
__global__ __launch_bounds__(256) void slab_reduce_vec_kernel(const f32x4* __restrict__ slabs, f32x4* __restrict__ out,
                                                              long long nvec, int splits) {
    constexpr int SG = 256 / VEC;
    __shared__ f32x4 red[SG][VEC];
    const int v = threadIdx.x % VEC, sg = threadIdx.x / VEC;
    const long long i = (long long)blockIdx.x * VEC + v;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    if (i < nvec) {
        int k = sg;
        for (; k + 3 * SG < splits; k += 4 * SG) {
            const f32x4 a = slabs[(long long)k * nvec + i], b = slabs[(long long)(k + SG) * nvec + i];
            const f32x4 c = slabs[(long long)(k + 2 * SG) * nvec + i], d = slabs[(long long)(k + 3 * SG) * nvec + i];
            s0 += a; s1 += b; s2 += c; s3 += d;
        }
        for (; k < splits; k += SG) s0 += slabs[(long long)k * nvec + i];
    }
    red[sg][v] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sg == 0 && i < nvec) {
        f32x4 t = red[0][v];
#pragma unroll
        for (int g = 1; g < SG; ++g) t += red[g][v];
        out[i] = t;
    }
}

__global__ void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out,
                                   long long n, int splits) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += slabs[(long long)k * n + i];   // fixed order
        out[i] = s;
    }
}

void wgrad_plan(int B, int H, int W, int Cin, int Cout, int k, int stride, WgradGeom& g) {
    const int pad = (k - 1) / 2;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.k = k; g.stride = stride; g.pad = pad;
    g.Ho = (H + 2 * pad - k) / stride + 1;
    g.Wo = (W + 2 * pad - k) / stride + 1;
    g.M = B * g.Ho * g.Wo;
    g.J = k * k * Cin;
    g.tn = Cout <= 64 ? 64 : 128;
    g.tj = g.J <= 64 ? 64 : 128;
    g.ntn = (Cout + g.tn - 1) / g.tn;
    g.ntj = (g.J + g.tj - 1) / g.tj;
    const int tiles = g.ntn * g.ntj;
    const int chunks = (g.M + 31) / 32;
    // resident blocks: LDS = 2*32*(tn+tj)*4 B per block, 160 KiB per CU, <= 8 (wave slots at 4 waves/block)
    int per_cu = (160 * 1024) / (2 * 32 * (g.tn + g.tj) * 4);
    if (per_cu > 4) per_cu = 4;
    if (g.tn + g.tj == 256 && per_cu > 2) per_cu = 2;      // 128x128: 124 VGPRs + 64 KiB
    const int slots = 256 * per_cu;
    // choose the split count in [1, chunks/16] that fills whole rounds of `slots` blocks best
    int max_s = chunks / 16;
    if (max_s < 1) max_s = 1;
    if (max_s > 4096) max_s = 4096;
    int best_s = 1;
    double best_eff = -1.0;
    for (int sp = 1; sp <= max_s; ++sp) {
        const long long blocks = (long long)tiles * sp;
        const long long rounds = (blocks + slots - 1) / slots;
        double eff = (double)blocks / (double)(rounds * slots);
        if (rounds > 6) eff = 1.0;                           // enough rounds: tail is amortised
        if (eff > best_eff + 0.02) { best_eff = eff; best_s = sp; }
        if (blocks >= 2ll * slots && eff >= 0.93) break;     // good enough: fewer slabs to write and fold
        if (blocks >= 6ll * slots) break;
    }
    { static const char* fs = getenv("Y4_WGRAD_SPLITS"); if (fs) { best_s = atoi(fs); if (best_s > max_s) best_s = max_s; if (best_s < 1) best_s = 1; } }
    g.chunks_per_split = (chunks + best_s - 1) / best_s;
    // a block's pixel range (+ 2 images of slack) must fit a 32-bit buffer window; planned for pitches up to 2x the
    // channel count (channel slices of concat buffers), verified against the real pitches at call time
    const unsigned long long per_px = 8ull * (unsigned long long)((Cout + 3) / 4 * 4 > Cin * stride * stride ? (Cout + 3) / 4 * 4 : Cin * stride * stride);
    const unsigned long long slack = 2ull * g.Ho * g.Wo;
    const unsigned long long max_px = 0xf0000000ull / per_px;
    if (max_px > slack + 32 && (unsigned long long)g.chunks_per_split * 32ull + slack > max_px)
        g.chunks_per_split = (int)((max_px - slack) / 32ull);
    g.splits = (chunks + g.chunks_per_split - 1) / g.chunks_per_split;
}

int g_conv_mode = 3;          // 0: fp32 MFMA (exact fma chain), 1: split-bf16 x3 (fp32-grade, 6 bf16 MFMAs),
                              // 2: plain bf16 operands (RN), fp32 accumulate -- mixed precision, BASELINE config 5
                              // 3: split-fp16 x2 (fp32-grade, 3 fp16 MFMAs, per-tensor power-of-two scale; conv_f16x2.hip) -- default

thread_local char g_last_kernel[160] = "";          // see y4::note_kernel

// the dimension conditions every conv entry shares
bool conv_dims_ok(int B, int H, int W, int Cout, int k, int stride) {
    return B > 0 && H > 0 && W > 0 && Cout > 0 && (k == 1 || k == 3) && (stride == 1 || stride == 2);
}

// f16x2 mode: the maximum of an operand the caller gave none for, measured into `word` of the call's own workspace
int amax_or_measure(const unsigned*& amax, unsigned* word, const float* t, long long ld, long long M, int C, hipStream_t st) {
    if (amax) return Y4_OK;
    amax = word;
    return y4::amax_launch(t, ld, M, C, word, st);
}

// the end of both f16x2 forward paths: the input's maximum into hdr[1] if the caller gave none, the three amax words, the gather
int fwd_f16x2(ConvGeom& g, const unsigned* x_amax, unsigned* hdr, unsigned* y_amax, int* nparts, hipStream_t st) {
    const int rc = amax_or_measure(x_amax, hdr + 1, g.src, g.lds_, (long long)g.B * g.Hs * g.Ws, g.Cs, st);
    if (rc != Y4_OK) return rc;
    g.src_amax = x_amax; g.wt_amax = hdr; g.dst_amax = y_amax;
    return y4::f16x2_gather(g, false, st, nparts);
}

}  // namespace

namespace y4 {
void note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_kernel, sizeof(g_last_kernel), fmt, ap);
    va_end(ap);
}
int slab_reduce(const float* slabs, float* dw, long long n, int splits, hipStream_t st) {
    if ((n & 3) == 0 && !(reinterpret_cast<uintptr_t>(dw) & 15) && !(reinterpret_cast<uintptr_t>(slabs) & 15)) {
        const long long nvec = n / 4;
        if (nvec >= 64 * 1024)
            hipLaunchKernelGGL(slab_reduce_vec_kernel<64>, dim3((unsigned)((nvec + 63) / 64)), dim3(256), 0, st,
                               reinterpret_cast<const f32x4*>(slabs), reinterpret_cast<f32x4*>(dw), nvec, splits);
        else
            hipLaunchKernelGGL(slab_reduce_vec_kernel<16>, dim3((unsigned)((nvec + 15) / 16)), dim3(256), 0, st,
                               reinterpret_cast<const f32x4*>(slabs), reinterpret_cast<f32x4*>(dw), nvec, splits);
    } else {
        const int blocks = (int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(256), 0, st, slabs, dw, n, splits);
    }
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
}  // namespace y4

// ======================================================================================== C ABI
extern "C" {

int y4_set_conv_mode(int mode) {
    if (mode < 0 || mode > 3) return Y4_ERR_SHAPE;
    g_conv_mode = mode;
    return Y4_OK;
}
int y4_get_conv_mode(void) { return g_conv_mode; }

// Per-call workspace of the forward conv (modes 1-3): [64 B of amax words: [0] filter, [1] gathered tensor when the caller
// gave none][4 KiB of per-block filter maxima][filter planes].  Nothing is shared between calls, so convs may be issued
// from any number of streams / devices / threads at once.
constexpr size_t FWD_WS_HDR = 64 + 4096;

size_t y4_conv2d_fwd_workspace(int Cin, int Cout, int k) {
    if (Cin <= 0 || Cout <= 0 || k <= 0) return 0;
    return FWD_WS_HDR + (size_t)Cout * k * k * Cin * 6;
}

static int conv_fwd_impl(const float* x, int ldx, const float* w, float* y, int ldy,
                         int B, int H, int W, int Cin, int Cout, int k, int stride,
                         const float* scale, const float* shift, int act,
                         const float* residual, int ldr, float* stats, int* nparts, const unsigned* x_amax,
                         unsigned* y_amax, void* workspace, size_t workspace_bytes, void* stream,
                         void* w_prepared = nullptr, void* dgrad_filter = nullptr, size_t dgrad_filter_bytes = 0) {
    if (!x || (!w && !w_prepared) || !y) return Y4_ERR_NULL;
    if (!conv_dims_ok(B, H, W, Cout, k, stride)) return Y4_ERR_SHAPE;
    // (32: the K-tile depth of every gather kernel)
    if (Cin <= 0 || Cin % 32 != 0 || ldx < Cin || ldy < Cout || (ldx & 3) || (residual && ldr < Cout))
        return Y4_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(w) & 15)) return Y4_ERR_SHAPE;
    const int pad = (k - 1) / 2;
    ConvGeom g{};
    g.src = x; g.wt = w; g.dst = y; g.scale = scale; g.shift = shift; g.res = residual; g.stats = stats;
    g.lds_ = ldx; g.ldd = ldy; g.ldr = ldr;
    g.B = B; g.Hs = H; g.Ws = W; g.Cs = Cin; g.Cs_valid = Cin;
    g.Hd = (H + 2 * pad - k) / stride + 1;
    g.Wd = (W + 2 * pad - k) / stride + 1;
    g.N = Cout; g.k = k; g.stride = stride; g.pad = pad;
    const long long M = (long long)B * g.Hd * g.Wd;
    if (M >= (1ll << 31)) return Y4_ERR_SHAPE;
    g.M = (int)M; g.K = k * k * Cin; g.act = act;
    const int mode = g_conv_mode;
    hipStream_t st = y4_stream(stream);
    if (w_prepared) {
        // filter already split (y4_conv2d_prepare_filter_f32): [word 0: max|w| bits][word 1: scratch][.. 64 B][4 KiB][planes]
        if (mode != 3) return Y4_ERR_SHAPE;
        if (reinterpret_cast<uintptr_t>(w_prepared) & 15) return Y4_ERR_SHAPE;
        g.wt_planes = reinterpret_cast<unsigned short*>(static_cast<char*>(w_prepared) + 64 + 4096);
        return fwd_f16x2(g, x_amax, static_cast<unsigned*>(w_prepared), y_amax, nparts, st);
    }
    if (mode != 0) {
        if (!workspace) return Y4_ERR_NULL;
        if (workspace_bytes < y4_conv2d_fwd_workspace(Cin, Cout, k)) return Y4_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return Y4_ERR_SHAPE;
        unsigned* hdr = static_cast<unsigned*>(workspace);
        unsigned short* planes = reinterpret_cast<unsigned short*>(static_cast<char*>(workspace) + FWD_WS_HDR);
        g.wt_planes = planes;
        if (mode == 3) {
            int rc;
            if (dgrad_filter) {
                // the backward pass of this layer will want the transposed planes of the same filter: both in one launch,
                // into a buffer laid out as y4_conv2d_dgrad_f32's workspace (which that call then takes with w == NULL)
                if (dgrad_filter_bytes < y4_conv2d_dgrad_workspace(Cin, Cout, k)) return Y4_ERR_WORKSPACE;
                if (reinterpret_cast<uintptr_t>(dgrad_filter) & 15) return Y4_ERR_SHAPE;
                const int cp = (Cout + 31) / 32 * 32;
                unsigned* hdr_t = reinterpret_cast<unsigned*>(static_cast<char*>(dgrad_filter) + (size_t)Cin * k * k * cp * 6);
                // (the 2-D tile kernel runs dgrad in forward form: it wants the taps mirrored; same test as in y4_conv2d_dgrad_f32)
                rc = y4::f16x2_filter_planes_dual(w, planes, hdr, hdr + 16, static_cast<unsigned short*>(dgrad_filter), hdr_t, Cout, Cin,
                                                  k * k, cp, y4::tile_conv_ok(cp, Cout, Cin, k, stride, H, W), st);
            } else {
                rc = y4::f16x2_filter_planes(w, planes, Cout, g.K, hdr, hdr + 16, st);
            }
            if (rc != Y4_OK) return rc;
            return fwd_f16x2(g, x_amax, hdr, y_amax, nparts, st);      // (no producer-side maximum: one extra pass over the input)
        }
        const int rc = y4::igemm_filter(mode, w, planes, Cout, Cin, k * k, false, st);
        if (rc != Y4_OK) return rc;
    }
    return y4::igemm_gather(mode, g, false, st, nparts);
}

int y4_conv2d_fwd_f32(const float* x, int ldx, const float* w, float* y, int ldy,
                      int B, int H, int W, int Cin, int Cout, int k, int stride,
                      const float* scale, const float* shift, int act,
                      const float* residual, int ldr, const unsigned* x_amax, unsigned* y_amax,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return conv_fwd_impl(x, ldx, w, y, ldy, B, H, W, Cin, Cout, k, stride, scale, shift, act, residual, ldr, nullptr,
                         nullptr, x_amax, y_amax, workspace, workspace_bytes, stream);
}

int y4_amax_f32(const float* x, int ldx, long long M, int C, unsigned* amax_bits, void* stream) {
    if (!x || !amax_bits) return Y4_ERR_NULL;
    if (M < 0 || C <= 0 || ldx < C) return Y4_ERR_SHAPE;
    return y4::amax_launch(x, ldx, M, C, amax_bits, y4_stream(stream));
}

int y4_amax_merge_u32(unsigned* dst, const unsigned* src, void* stream) {
    if (!dst || !src) return Y4_ERR_NULL;
    return y4::amax_merge(dst, src, y4_stream(stream));
}

size_t y4_conv2d_bnstats_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    if (!conv_dims_ok(B, H, W, Cout, k, stride)) return 0;
    const int pad = (k - 1) / 2;
    const long long M = (long long)B * ((H + 2 * pad - k) / stride + 1) * ((W + 2 * pad - k) / stride + 1);
    long long rows = Cin == 3 ? (M + 255) / 256 : (M + 63) / 64;            // smallest M-tile of any variant
    const long long per_img = (long long)B * ((M / B + 127) / 128);         // the 3x3 halo kernel tiles image by image
    if (per_img > rows) rows = per_img;
    return (size_t)rows * 2 * Cout * sizeof(float);
}

int y4_conv2d_fwd_bnstats_f32(const float* x, int ldx, const float* w, float* y, int ldy,
                              int B, int H, int W, int Cin, int Cout, int k, int stride,
                              float* partials, size_t partial_bytes, long long* nparts_host, const unsigned* x_amax,
                              void* workspace, size_t workspace_bytes, void* dgrad_filter, size_t dgrad_filter_bytes,
                              void* stream) {
    if (!partials || !nparts_host) return Y4_ERR_NULL;
    if (dgrad_filter && g_conv_mode != 3) return Y4_ERR_SHAPE;
    if (partial_bytes < y4_conv2d_bnstats_workspace(B, H, W, Cin, Cout, k, stride)) return Y4_ERR_WORKSPACE;
    int np = 0;
    const int rc = conv_fwd_impl(x, ldx, w, y, ldy, B, H, W, Cin, Cout, k, stride, nullptr, nullptr, Y4_ACT_LINEAR,
                                 nullptr, 0, partials, &np, x_amax, nullptr, workspace, workspace_bytes, stream, nullptr,
                                 dgrad_filter, dgrad_filter_bytes);
    if (rc != Y4_OK) return rc;
    *nparts_host = np;
    return Y4_OK;
}

size_t y4_conv2d_dgrad_workspace(int Cin, int Cout, int k) {
    const size_t cp = (size_t)((Cout + 31) / 32) * 32;
    // fp32 transposed filter (4 B), 3 bf16 planes (6 B) or 2 fp16 planes (4 B) per element, + 64 B of amax words
    // + 4 KiB of per-block filter maxima
    return (size_t)Cin * k * k * cp * 6 + 64 + 4096;
}

int y4_conv2d_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                        int B, int H, int W, int Cin, int Cout, int k, int stride,
                        void* workspace, size_t workspace_bytes, const unsigned* dy_amax,
                        const float* residual, int ldr, void* stream) {
    const int mode = g_conv_mode;
    if (!dy || !dx || !workspace) return Y4_ERR_NULL;
    if (!w && mode != 3) return Y4_ERR_NULL;               // w == NULL: the workspace already holds the transposed planes
    if (!conv_dims_ok(B, H, W, Cout, k, stride) || Cin <= 0) return Y4_ERR_SHAPE;
    const int Cout_pad = (Cout + 31) / 32 * 32;
    // the padded channels of dy are read (multiplied by zero filter rows): they must exist
    if (lddy < Cout_pad || (lddy & 3) || lddx < Cin) return Y4_ERR_SHAPE;
    if (workspace_bytes < y4_conv2d_dgrad_workspace(Cin, Cout, k)) return Y4_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(dy) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return Y4_ERR_SHAPE;
    hipStream_t st = y4_stream(stream);
    const long long total = (long long)Cin * k * k * Cout_pad;
    unsigned* hdr = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + (size_t)total * 6);
    unsigned* wamax = hdr;                                 // the call's own words: nothing shared between calls
    if (mode == 3) {
        if (w) {
            const int rc = y4::f16x2_filter_planes_transposed(w, static_cast<unsigned short*>(workspace), Cout, Cin, k * k, Cout_pad,
                                                              wamax, hdr + 16, st, y4::tile_conv_ok(Cout_pad, Cout, Cin, k, stride, H, W));
            if (rc != Y4_OK) return rc;
        }                                                  // else: left there by y4_conv2d_fwd_bnstats_f32(..., dgrad_filter)
        Y4_CHECK_LAUNCH();
    } else {
        const int rc = y4::igemm_filter(mode, w, workspace, Cout, Cin, k * k, true, st);
        if (rc != Y4_OK) return rc;
    }
    const int pad = (k - 1) / 2;
    ConvGeom g{};
    if (residual && ldr < Cin) return Y4_ERR_SHAPE;
    g.src = dy; g.wt = static_cast<const float*>(workspace); g.dst = dx; g.scale = nullptr; g.shift = nullptr; g.res = residual;
    g.wt_planes = static_cast<const unsigned short*>(workspace);
    g.lds_ = lddy; g.ldd = lddx; g.ldr = ldr;
    g.B = B;
    g.Hs = (H + 2 * pad - k) / stride + 1;
    g.Ws = (W + 2 * pad - k) / stride + 1;
    g.Cs = Cout_pad; g.Cs_valid = Cout;
    g.Hd = H; g.Wd = W; g.N = Cin; g.k = k; g.stride = stride; g.pad = pad;
    const long long M = (long long)B * H * W;
    if (M >= (1ll << 31)) return Y4_ERR_SHAPE;
    g.M = (int)M; g.K = k * k * Cout_pad; g.act = Y4_ACT_LINEAR;
    if (mode == 3) {
        // pad channels of dy may hold anything: the maximum is taken over the valid channels only
        const int rc = amax_or_measure(dy_amax, hdr + 1, dy, lddy, (long long)B * g.Hs * g.Ws, Cout, st);
        if (rc != Y4_OK) return rc;
        g.src_amax = dy_amax; g.wt_amax = wamax;
        // few channels on a large map: the 2-D tile kernel, in forward form on the mirrored transposed planes (above)
        if (y4::tile_conv_ok(Cout_pad, Cout, Cin, k, stride, H, W)) return y4::f16x2_tile(g, st, nullptr);
        if (y4::tile_dgrad_s2_ok(Cout_pad, Cout, Cin, k, stride, g.Hs, g.Ws)) return y4::f16x2_tile_dgrad_s2(g, st);
        return y4::f16x2_gather(g, true, st, nullptr);
    }
    return y4::igemm_gather(mode, g, true, st, nullptr);
}

int y4_last_conv_kernel(char* buf, int cap) {
    if (!buf || cap <= 0) return Y4_ERR_NULL;
    snprintf(buf, (size_t)cap, "%s", g_last_kernel);
    g_last_kernel[0] = 0;
    return Y4_OK;
}

size_t y4_conv2d_prepared_bytes(int Cout, int K) {
    if (Cout <= 0 || K <= 0) return 0;
    return 64 + 4096 + (size_t)Cout * (size_t)K * 4;
}

int y4_conv2d_prepare_filter_f32(const float* w, int Cout, int K, void* prepared, size_t prepared_bytes, void* stream) {
    if (!w || !prepared) return Y4_ERR_NULL;
    if (Cout <= 0 || K <= 0 || (K & 31)) return Y4_ERR_SHAPE;
    if (prepared_bytes < y4_conv2d_prepared_bytes(Cout, K)) return Y4_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(prepared) & 15) || (reinterpret_cast<uintptr_t>(w) & 15)) return Y4_ERR_SHAPE;
    return y4::f16x2_refresh_prepared(w, prepared, Cout, K, y4_stream(stream));
}

int y4_conv2d_fwd_prepared_f32(const float* x, int ldx, void* w_prepared, float* y, int ldy,
                               int B, int H, int W, int Cin, int Cout, int k, int stride,
                               const float* scale, const float* shift, int act,
                               const float* residual, int ldr, const unsigned* x_amax, unsigned* y_amax, void* stream) {
    if (!w_prepared) return Y4_ERR_NULL;
    return conv_fwd_impl(x, ldx, nullptr, y, ldy, B, H, W, Cin, Cout, k, stride, scale, shift, act, residual, ldr, nullptr,
                         nullptr, x_amax, y_amax, nullptr, 0, stream, w_prepared);
}

size_t y4_conv2d_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    WgradGeom g{};
    wgrad_plan(B, H, W, Cin, Cout, k, stride, g);
    // slabs of the split-K partial sums + 64 B of amax words (f16x2 mode); the tile kernel (wgrad_tile.hip) writes one slab per block
    int splits = g.splits;
    if (y4::tile_wgrad_ok(Cin, Cout, k, stride, H, W, 0, 0) && y4::tile_wgrad_slabs(Cin, Cout) > splits) splits = y4::tile_wgrad_slabs(Cin, Cout);
    return (splits > 1 ? (size_t)splits * Cout * g.J * sizeof(float) : 0) + 64;
}

int y4_conv2d_wgrad_f32(const float* x, int ldx, const float* dy, int lddy, float* dw,
                        int B, int H, int W, int Cin, int Cout, int k, int stride,
                        void* workspace, size_t workspace_bytes, const unsigned* x_amax, const unsigned* dy_amax,
                        void* stream) {
    if (!x || !dy || !dw) return Y4_ERR_NULL;
    if (!conv_dims_ok(B, H, W, Cout, k, stride)) return Y4_ERR_SHAPE;
    if (Cin <= 0 || (Cin & 3) || ldx < Cin || (ldx & 3) || (lddy & 3) || lddy < ((Cout + 3) & ~3)) return Y4_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(dy) & 15)) return Y4_ERR_SHAPE;
    WgradGeom g{};
    wgrad_plan(B, H, W, Cin, Cout, k, stride, g);
    if ((long long)B * g.Ho * g.Wo >= (1ll << 31)) return Y4_ERR_SHAPE;
    g.x = x; g.dy = dy; g.ldx = ldx; g.lddy = lddy;
    {
        g.x_total_bytes = (unsigned long long)B * H * W * (unsigned long long)ldx * 4ull;
        g.dy_total_bytes = (unsigned long long)B * g.Ho * g.Wo * (unsigned long long)lddy * 4ull;
        const unsigned long long range_px = (unsigned long long)g.chunks_per_split * 32ull + 2ull * g.Ho * g.Wo;
        const unsigned long long per_px = 4ull * (unsigned long long)(lddy > ldx * stride * stride ? lddy : ldx * stride * stride);
        if (range_px * per_px >= 0xfffffff0ull) return Y4_ERR_SHAPE;      // pitch more than 2x the channel count at > 4 GiB
    }
    hipStream_t st = y4_stream(stream);
    const int mode = g_conv_mode;
    // few channels on a large map (3x3): the tile kernel -- every x pixel staged once for nine taps, one slab per block
    const bool tile = mode == 3 && y4::tile_wgrad_ok(Cin, Cout, k, stride, H, W, ldx, lddy);
    if (tile) g.splits = y4::tile_wgrad_slabs(Cin, Cout);
    const size_t slab_bytes = g.splits > 1 ? (size_t)g.splits * Cout * g.J * sizeof(float) : 0;
    if (g.splits > 1) {
        if (!workspace) return Y4_ERR_NULL;
        if (workspace_bytes < slab_bytes) return Y4_ERR_WORKSPACE;
        g.out = static_cast<float*>(workspace);
    } else {
        g.out = dw;
    }
    int rc;
    if (mode == 3) {
        if (!x_amax || !dy_amax) {
            if (!workspace || workspace_bytes < slab_bytes + 64) return Y4_ERR_WORKSPACE;
            unsigned* hdr = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + slab_bytes);
            rc = amax_or_measure(x_amax, hdr, x, ldx, (long long)B * H * W, Cin, st);
            if (rc != Y4_OK) return rc;
            rc = amax_or_measure(dy_amax, hdr + 1, dy, lddy, (long long)B * g.Ho * g.Wo, Cout, st);
            if (rc != Y4_OK) return rc;
        }
        g.x_amax = x_amax; g.dy_amax = dy_amax;
        rc = tile ? y4::f16x2_wgrad_tile(g, st) : y4::f16x2_wgrad(g, st);
    } else {
        rc = y4::igemm_wgrad(mode, g, st);
    }
    if (rc != Y4_OK || g.splits <= 1) return rc;
    return y4::slab_reduce(static_cast<const float*>(workspace), dw, (long long)Cout * g.J, g.splits, st);
}

}  // extern "C"
