// Fused optimizer steps: replace torch.optim.Adam(groups, lr, betas=(0.9, 0.999), eps=1e-8) and
// torch.optim.SGD(groups, lr, momentum, weight_decay) as built by the reference
// (yolo/optim/optimizers/adam.py:14-15, sgd.py:14-15, build.py:18-35).
//
// Adam: one sweep over (p, g, m, v): 16 B read + 12 B written per parameter, HBM-bound.  Same operation order as
// torch's single-tensor Adam:
//   m = lerp(m, g, 1-b1); v = b2*v + (1-b2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// SGD: buf = g (first step) | momentum*buf + g; p -= lr*buf, with g += wd*p first (dampening 0, no nesterov).
//
// Multi-tensor form: the host keeps a device table of chunks {p, g, m, v, n, hyper row}; ONE launch walks all
// parameters of the model (327 tensors, 64.9 M elements: ~1000 chunks of 64 Ki elements), each block taking whole
// chunks with 16-B accesses.  Per-group scalars (lr/bias corrections/weight decay) come in a small by-value table.
//
// Guarded form (not in the reference): grad_sumsq_kernel + grad_guard_kernel reduce the global gradient norm over the
// same table into a 4-double device record {total_norm, coef, applied, skipped_total} in a fixed order (no float
// atomics, no host sync); the GUARDED instance of the step kernel scales the gradients by coef (clip_grad_norm_) or
// writes nothing when the norm is not finite.  ema_kernel averages a list of tensors over the same records.
#include "common.h"

namespace {

struct Hyper { float a, b, c, d; };          // Adam: lr/bc1, 1/sqrt(bc2), wd, -   SGD: lr, momentum, wd, first(0/1)
constexpr int MAX_HYPER = 16;
struct HyperTable { Hyper h[MAX_HYPER]; };

struct Chunk {                                // 48 bytes, mirrored by the host as 6 x int64
    float* p; const float* g; float* m; float* v; long long n; long long hyper;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float lr_over_bc1, float b1, float b2,
                                          float eps, float inv_sqrt_bc2, float wd, float gscale) {
    float gi = g * gscale;
    if (wd != 0.f) gi = gi + wd * p;                          // L2 weight decay folded into the gradient
    const float mi = m + (1.0f - b1) * (gi - m);              // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = b2 * v + (1.0f - b2) * gi * gi;          // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    m = mi;
    v = vi;
    p = p - lr_over_bc1 * (mi / denom);
}

__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, float lr, float mom, float wd, bool first,
                                         float gscale) {
    float gi = g * gscale;
    if (wd != 0.f) gi = gi + wd * p;
    if (mom != 0.f) {
        const float b = first ? gi : mom * buf + gi;
        buf = b;
        gi = b;
    }
    p = p - lr * gi;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n,
                                                   float lr_over_bc1, float b1, float b2, float eps,
                                                   float inv_sqrt_bc2, float wd, float gscale) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_elem(pi, g[i], mi, vi, lr_over_bc1, b1, b2, eps, inv_sqrt_bc2, wd, gscale);
        m[i] = mi; v[i] = vi; p[i] = pi;
    }
}

// Guard record of the guarded steps (4 doubles in device memory, include/yolov4_amd.h).
enum { GUARD_NORM = 0, GUARD_COEF = 1, GUARD_APPLIED = 2, GUARD_SKIPPED = 3 };

// GUARDED: the step reads the guard record first: applied == 0 -> nothing is written; otherwise the gradient scale is
// multiplied by (float)coef (coef == 1: the same bits as the unguarded instance).
template <bool ADAM, bool GUARDED>
__global__ __launch_bounds__(256) void multi_tensor_kernel(const Chunk* __restrict__ chunks, int nchunks, const HyperTable ht,
                                                           float b1, float b2, float eps, float gscale,
                                                           const double* __restrict__ guard) {
    if (GUARDED) {
        if (guard[GUARD_APPLIED] == 0.0) return;
        gscale = gscale * (float)guard[GUARD_COEF];
    }
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        const Hyper h = ht.h[ck.hyper];
        const bool vec = ((reinterpret_cast<uintptr_t>(ck.p) | reinterpret_cast<uintptr_t>(ck.g) |
                           reinterpret_cast<uintptr_t>(ck.m) | (ADAM ? reinterpret_cast<uintptr_t>(ck.v) : 0)) & 15) == 0;
        long long i0 = 0;
        if (vec) {
            const long long n4 = ck.n >> 2;
            f32x4* p4 = reinterpret_cast<f32x4*>(ck.p);
            const f32x4* g4 = reinterpret_cast<const f32x4*>(ck.g);
            f32x4* m4 = reinterpret_cast<f32x4*>(ck.m);
            f32x4* v4 = reinterpret_cast<f32x4*>(ck.v);
            for (long long i = threadIdx.x; i < n4; i += 256) {
                f32x4 pv = p4[i], mv = m4[i], vv;
                const f32x4 gv = g4[i];
                if (ADAM) vv = v4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pv[e], me = mv[e], ve = ADAM ? vv[e] : 0.f;
                    if (ADAM) adam_elem(pe, gv[e], me, ve, h.a, b1, b2, eps, h.b, h.c, gscale);
                    else sgd_elem(pe, gv[e], me, h.a, h.b, h.c, h.d != 0.f, gscale);
                    pv[e] = pe; mv[e] = me;
                    if (ADAM) vv[e] = ve;
                }
                p4[i] = pv;
                if (ADAM || h.b != 0.f) m4[i] = mv;
                if (ADAM) v4[i] = vv;
            }
            i0 = n4 << 2;
        }
        for (long long i = i0 + threadIdx.x; i < ck.n; i += 256) {
            float pi = ck.p[i], mi = ck.m[i], vi = ADAM ? ck.v[i] : 0.f;
            if (ADAM) adam_elem(pi, ck.g[i], mi, vi, h.a, b1, b2, eps, h.b, h.c, gscale);
            else sgd_elem(pi, ck.g[i], mi, h.a, h.b, h.c, h.d != 0.f, gscale);
            ck.p[i] = pi;
            if (ADAM || h.b != 0.f) ck.m[i] = mi;
            if (ADAM) ck.v[i] = vi;
        }
    }
}

// Block sum of one double per thread in a FIXED tree (lane l takes l + 32, then + 16 ... + 1 inside each wave; thread 0
// then adds the four wave sums in wave order): the same bits in every run.  Valid in thread 0 only.
__device__ __forceinline__ double block_sum_256(double acc, double* wave_sums /* LDS, 4 doubles */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) s = ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
    __syncthreads();                                          // wave_sums is reused by the block's next chunk
    return s;
}

__device__ __forceinline__ double sq_scaled(float g, float gscale) {
    const double d = (double)(g * gscale);                    // the fp32 value the step kernels use, squared exactly
    return d * d;
}

// partials[c] = sum over chunk c of ((double)fl32(g * gscale))^2.  Thread t adds elements t, t + 256, ... (16-byte
// groups on the vector path) into one double in ascending order; inf / NaN travel through the sums by themselves.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const Chunk* __restrict__ chunks, int nchunks, float gscale,
                                                         double* __restrict__ partials) {
    __shared__ double wave_sums[4];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        double acc = 0.0;
        long long i0 = 0;
        if ((reinterpret_cast<uintptr_t>(ck.g) & 15) == 0) {
            const long long n4 = ck.n >> 2;
            const f32x4* g4 = reinterpret_cast<const f32x4*>(ck.g);
#pragma unroll 4
            for (long long i = threadIdx.x; i < n4; i += 256) {
                const f32x4 gv = g4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += sq_scaled(gv[e], gscale);
            }
            i0 = n4 << 2;
        }
#pragma unroll 4
        for (long long i = i0 + threadIdx.x; i < ck.n; i += 256) acc += sq_scaled(ck.g[i], gscale);
        const double s = block_sum_256(acc, wave_sums);
        if (threadIdx.x == 0) partials[c] = s;
    }
}

// One block: total_norm = sqrt(sum of partials) in a fixed order, then the record {total_norm, coef, applied,
// skipped_total} (coef: torch.nn.utils.clip_grad_norm_'s formula in double).
__global__ __launch_bounds__(256) void grad_guard_kernel(const double* __restrict__ partials, int nchunks, double max_norm,
                                                         double* __restrict__ guard) {
    __shared__ double wave_sums[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) acc += partials[i];
    const double s = block_sum_256(acc, wave_sums);
    if (threadIdx.x == 0) {
        const double total = sqrt(s);
        const bool applied = isfinite(total);
        double coef = 1.0;
        if (applied && max_norm > 0.0 && isfinite(max_norm)) {
            coef = max_norm / (total + 1e-6);
            if (!(coef < 1.0)) coef = 1.0;
        }
        const double skipped = guard[GUARD_SKIPPED] + (applied ? 0.0 : 1.0);
        guard[GUARD_NORM] = total;
        guard[GUARD_COEF] = coef;
        guard[GUARD_APPLIED] = applied ? 1.0 : 0.0;
        guard[GUARD_SKIPPED] = skipped;
    }
}

// e = e + (1 - decay) * (s - e) over the chunk table (p = EMA tensor e, g = live tensor s; m, v, hyper unused).
__global__ __launch_bounds__(256) void ema_kernel(const Chunk* __restrict__ chunks, int nchunks, float omd,
                                                  const double* __restrict__ guard) {
    if (guard != nullptr && guard[GUARD_APPLIED] == 0.0) return;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        long long i0 = 0;
        if (((reinterpret_cast<uintptr_t>(ck.p) | reinterpret_cast<uintptr_t>(ck.g)) & 15) == 0) {
            const long long n4 = ck.n >> 2;
            f32x4* e4 = reinterpret_cast<f32x4*>(ck.p);
            const f32x4* s4 = reinterpret_cast<const f32x4*>(ck.g);
            for (long long i = threadIdx.x; i < n4; i += 256) {
                f32x4 ev = e4[i];
                const f32x4 sv = s4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) ev[e] = ev[e] + omd * (sv[e] - ev[e]);
                e4[i] = ev;
            }
            i0 = n4 << 2;
        }
        for (long long i = i0 + threadIdx.x; i < ck.n; i += 256) {
            const float ei = ck.p[i];
            ck.p[i] = ei + omd * (ck.g[i] - ei);
        }
    }
}

}  // namespace

extern "C" int y4_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return Y4_ERR_NULL;
    if (n <= 0 || step < 1) return Y4_ERR_SHAPE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, y4_stream(stream), param, grad, exp_avg,
                       exp_avg_sq, n, (float)((double)lr / bc1), beta1, beta2, eps, (float)(1.0 / sqrt(bc2)),
                       weight_decay, grad_scale);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_adam_hyper_f32(float lr, float beta1, float beta2, float weight_decay, int step, float* out4_host) {
    if (!out4_host) return Y4_ERR_NULL;
    if (step < 1) return Y4_ERR_SHAPE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    out4_host[0] = (float)((double)lr / bc1);
    out4_host[1] = (float)(1.0 / sqrt(bc2));
    out4_host[2] = weight_decay;
    out4_host[3] = 0.f;
    return Y4_OK;
}

static inline int multi_grid(int nchunks) { return nchunks < 2048 ? nchunks : 2048; }

// guard == nullptr: the unguarded entry points (instances <ADAM, false>); `guarded` entry points require the record.
static int multi_launch(bool adam, bool guarded, const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                        float b1, float b2, float eps, float grad_scale, const double* guard, void* stream) {
    if (!chunks_dev || !hyper_host || (guarded && !guard)) return Y4_ERR_NULL;
    if (nchunks <= 0 || nhyper <= 0 || nhyper > MAX_HYPER) return Y4_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(chunks_dev) & 7) return Y4_ERR_SHAPE;
    if (guarded && (reinterpret_cast<uintptr_t>(guard) & 7)) return Y4_ERR_SHAPE;
    HyperTable ht{};
    for (int i = 0; i < nhyper; ++i)
        ht.h[i] = Hyper{hyper_host[4 * i], hyper_host[4 * i + 1], hyper_host[4 * i + 2], hyper_host[4 * i + 3]};
    const int grid = multi_grid(nchunks);
    const Chunk* ck = static_cast<const Chunk*>(chunks_dev);
    auto kernel = adam ? (guarded ? multi_tensor_kernel<true, true> : multi_tensor_kernel<true, false>)
                       : (guarded ? multi_tensor_kernel<false, true> : multi_tensor_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, y4_stream(stream), ck, nchunks, ht, b1, b2, eps, grad_scale,
                       guarded ? guard : nullptr);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_adam_multi_step_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                      float beta1, float beta2, float eps, float grad_scale, void* stream) {
    return multi_launch(true, false, chunks_dev, nchunks, hyper_host, nhyper, beta1, beta2, eps, grad_scale, nullptr, stream);
}

extern "C" int y4_sgd_multi_step_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                     float grad_scale, void* stream) {
    return multi_launch(false, false, chunks_dev, nchunks, hyper_host, nhyper, 0.f, 0.f, 0.f, grad_scale, nullptr, stream);
}

extern "C" int y4_adam_multi_step_guarded_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                              float beta1, float beta2, float eps, float grad_scale, const double* guard,
                                              void* stream) {
    return multi_launch(true, true, chunks_dev, nchunks, hyper_host, nhyper, beta1, beta2, eps, grad_scale, guard, stream);
}

extern "C" int y4_sgd_multi_step_guarded_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                             float grad_scale, const double* guard, void* stream) {
    return multi_launch(false, true, chunks_dev, nchunks, hyper_host, nhyper, 0.f, 0.f, 0.f, grad_scale, guard, stream);
}

extern "C" int y4_grad_sumsq_multi_f32(const void* chunks_dev, int nchunks, float grad_scale, double* partials,
                                       void* stream) {
    if (!chunks_dev || !partials) return Y4_ERR_NULL;
    if (nchunks <= 0) return Y4_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(chunks_dev) | reinterpret_cast<uintptr_t>(partials)) & 7) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(multi_grid(nchunks)), dim3(256), 0, y4_stream(stream),
                       static_cast<const Chunk*>(chunks_dev), nchunks, grad_scale, partials);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_grad_guard_f32(const double* partials, int nchunks, double max_norm, double* guard, void* stream) {
    if (!partials || !guard) return Y4_ERR_NULL;
    if (nchunks <= 0) return Y4_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(guard)) & 7) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(grad_guard_kernel, dim3(1), dim3(256), 0, y4_stream(stream), partials, nchunks, max_norm, guard);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}

extern "C" int y4_ema_multi_f32(const void* chunks_dev, int nchunks, float one_minus_decay, const double* guard,
                                void* stream) {
    if (!chunks_dev) return Y4_ERR_NULL;
    if (nchunks <= 0 || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return Y4_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(chunks_dev) | reinterpret_cast<uintptr_t>(guard)) & 7) return Y4_ERR_SHAPE;
    hipLaunchKernelGGL(ema_kernel, dim3(multi_grid(nchunks)), dim3(256), 0, y4_stream(stream),
                       static_cast<const Chunk*>(chunks_dev), nchunks, one_minus_decay, guard);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
