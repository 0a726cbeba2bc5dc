/*
 * yolov4_amd.h -- C ABI of libyolov4_amd.so: the MI355X (gfx950) hot path of YOLOv4.
 *
 * The reference (zjykzj/YOLOv4) has no FFI of its own: its hot path is a set of Python
 * nn.Module classes whose arithmetic runs inside PyTorch ATen.  Each entry
 * point below therefore cites the reference Python interface (file:line under /root/reference)
 * whose arithmetic it replaces; the Python classes of the same names in yolov4_amd/ bind these
 * symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - activations are NHWC fp32 with an explicit pixel pitch `ld*` (elements between two
 *     consecutive pixels, >= channel count), so a channel slice of a wider buffer is a
 *     valid operand (zero-copy concat / split);
 *   - conv filters are KRSC fp32: w[Cout][k][k][Cin], i.e. the reference's
 *     nn.Conv2d.weight [Cout,Cin,k,k] held in torch.channels_last memory format;
 *   - `stream` is a hipStream_t passed as void*; work is only enqueued, no call synchronises,
 *     allocates or frees (workspaces are caller-provided; *_workspace() return their size);
 *   - return value: Y4_OK or a Y4_ERR_* code; y4_strerror() names it.  Shapes are validated on
 *     the host before any launch.
 */
#ifndef YOLOV4_AMD_H
#define YOLOV4_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y4_OK 0
#define Y4_ERR_SHAPE 1      /* unsupported / inconsistent shape or pitch            */
#define Y4_ERR_NULL 2       /* required pointer is NULL                             */
#define Y4_ERR_LAUNCH 3     /* hipLaunch / hipMemsetAsync reported an error         */
#define Y4_ERR_WORKSPACE 4  /* workspace too small                                  */
#define Y4_ERR_NODEVICE 5   /* no gfx950 device visible                             */
#define Y4_ERR_FORMAT 6     /* malformed or truncated input data (JPEG)             */
#define Y4_ERR_UNSUPPORTED 7 /* valid input outside the supported subset (JPEG)     */

/* activation ids: darknet/darknet.py:41-51 ('relu' | 'leaky_relu' (0.1) | 'mish' | 'linear') */
#define Y4_ACT_LINEAR 0
#define Y4_ACT_LEAKY 1
#define Y4_ACT_MISH 2
#define Y4_ACT_RELU 3

const char* y4_strerror(int code);
int y4_version(void);
/* number of visible HIP devices whose arch is gfx950 (0 if none) */
int y4_device_count(void);

/* Arithmetic of the conv implicit GEMMs (process-wide):
 *   1  "bf16x3": every fp32 operand is split EXACTLY into three bf16 pieces (8+8+8
 *      mantissa bits) while its tile is staged into LDS; a product is the six leading terms
 *      a1b1+a1b2+a2b1+a1b3+a2b2+a3b1 on v_mfma_f32_32x32x16_bf16 (products exact, fp32 accumulate).
 *      Dropped terms <= 2^-23 |a*b|: measured error vs an fp64 convolution is at or below that of
 *      mode 0 (rms 1.06e-6 vs 1.19e-6 of the output range at K = 4608), at 6/16 of the MFMA cost.
 *   0  v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fp32 fma chain.
 *   2  plain bf16: operands rounded (RN) to bf16 while staged, one bf16 MFMA per product, fp32
 *      accumulate; activations / gradients / BN / loss / NMS stay fp32 (BASELINE config 5, mixed
 *      precision -- NOT fp32-grade: ~3 significant digits per product).
 *   3  "f16x2" (default): every fp32 operand is scaled by a power of two taken from its tensor's max|x| (so the
 *      maximum lands in [2^14, 2^15)) and split into two fp16 pieces hi = RN(sx), lo = RN((sx-hi) 2^11)
 *      (11 + 11 significant bits, |error| <= 2^-22 |x|); a product is THREE fp16 MFMAs
 *      (hi*hi -> acc0; hi*lo + lo*hi -> acc1; result (acc0 + 2^-11 acc1)/(s_a s_b)), fp32 accumulate.
 *      Per-product error ~2^-22, i.e. 2.4e-7 of the rms of a sum of any length: below the rounding of
 *      an fp32 fma chain and of the MFMA's own fp32 accumulation; half the MFMAs of mode 1.  Operand
 *      maxima (`*_amax` arguments: device words holding the bit pattern of max|finite element|,
 *      upper bounds are fine) come from the producing kernels (y4_bn_act_fwd_f32 / y4_bn_act_bwd_f32
 *      out_amax) or, when NULL, from one extra pass over the operand inside the call. */
int y4_set_conv_mode(int mode);
int y4_get_conv_mode(void);
/* BASELINE configs[4] ("bf16 MFMA conv, fp32 loss / NMS") as shipped: conv mode 3 with this switch on -- the layers that run on
 * the DMA-fed plane kernels (72 of the 107 BatchNorm layers, 9/10 of the conv flops) take plain bf16 operands written by the
 * BatchNorm sweeps and run one bf16 MFMA per product (y4_conv2d_*_planes_f32, y4_bn_act_fwd_f32 z_planes == 3); every other
 * layer keeps the fp32-grade f16x2 kernels of mode 3, which are HBM-bound anyway.  (Mode 2 rounds EVERY conv operand to bf16.) */
int y4_set_planes_bf16(int on);
int y4_get_planes_bf16(void);
/* 1 if EVERY plane kernel a conv layer of this geometry (x: [B][H][W][Cin]; k in {1,3}; stride 1, or 2 with k = 3 on an even
 * grid) would launch in the current mode can address its operands -- the DMA kernels use 32-bit buffer windows (an image span
 * of a 256-row tile, a wgrad block's pixel range, the whole dx of a stride-2 dgrad: each < 4 GiB) -- else 0.  dgrad_planes: the
 * layer's dgrad runs on the plane kernels too.  The host asks this before it lets a producer write its result pre-split: such
 * an operand has no fp32 form for the register-staged kernels to fall back to (yolov4_amd/darknet/darknet.py takes_planes()). */
int y4_conv_planes_fit(int B, int H, int W, int Cin, int Cout, int k, int stride, int dgrad_planes);
/* ---------------------------------------------------------------- convolution
 * Replaces nn.Conv2d inside ConvBNAct.forward, darknet/darknet.py:31-36,53-54
 * (k in {1,3}, stride in {1,2}, pad=(k-1)//2, dilation 1, groups 1).
 *
 * y[b,ho,wo,n] = act( (sum_{r,q,c} x[b,ho*s-pad+r,wo*s-pad+q,c] * w[n,r,q,c]) * scale[n] + shift[n] )
 *                + residual[b,ho,wo,n]
 * scale/shift/residual may be NULL (identity / 0).  Eval-mode BatchNorm folds into
 * scale/shift (darknet.py:55), the bias of the 3 head convs into shift (yolov4.py:237,243,249),
 * ResBlock's skip into residual (darknet.py:76-80).  Implicit GEMM on
 * v_mfma_f32_32x32x2_f32 (exact fp32).  Requires Cin % 32 == 0, or Cin == 3 (stem,
 * yolov4.py:30: direct kernel, x given with arbitrary element strides).
 * workspace: y4_conv2d_fwd_workspace() bytes of caller-owned device memory, 16-B aligned, private to the call in stream
 * order (modes 1-3: the filter's maximum and its pre-split planes; 6 B per filter element + 4160 B).  The library keeps
 * no state between calls: convs may be issued from any number of streams, devices and host threads at once.
 */
size_t y4_conv2d_fwd_workspace(int Cin, int Cout, int k);
int y4_conv2d_fwd_f32(const float* x, int ldx, const float* w, float* y, int ldy,
                      int B, int H, int W, int Cin, int Cout, int k, int stride,
                      const float* scale, const float* shift, int act,
                      const float* residual, int ldr, const unsigned* x_amax /* mode 3, nullable */,
                      unsigned* y_amax /* mode 3, nullable: max|finite y| folded in with atomicMax */,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Inference, conv mode 3: keep a KRSC filter [Cout][K = k*k*Cin] in the form the forward kernels consume -- a 64-B header
 * (word 0: bit pattern of max|w|; word 1: scratch of the conv call; words 2-5: 64-bit fingerprint, valid flag, ticket), 4 KiB of
 * fingerprint partials, then the fp16 hi/lo planes interleaved per 32-deep K tile; y4_conv2d_prepared_bytes(Cout, K) bytes in
 * all, whose first 64 bytes the caller ZEROES once after allocating.  y4_conv2d_prepare_filter_f32 is a REFRESH: it reads the
 * filter once (maximum + a 64-bit positional hash of its bit patterns; collision probability 2^-64) and re-splits it only if
 * either differs from what the buffer holds -- decided on the device, so a stale buffer cannot be used whatever wrote the weights (optimizer kernels,
 * `.data` writes, load_state_dict).  Call it before every y4_conv2d_fwd_prepared_f32: same arithmetic and results as
 * y4_conv2d_fwd_f32 at one read pass instead of two reads + one write pass over the filter.  (The reference has no
 * counterpart: nn.Conv2d re-reads its weight every call.) */
size_t y4_conv2d_prepared_bytes(int Cout, int K);
int y4_conv2d_prepare_filter_f32(const float* w, int Cout, int K, void* prepared, size_t prepared_bytes, void* stream);
int y4_conv2d_fwd_prepared_f32(const float* x, int ldx, void* w_prepared, float* y, int ldy,
                               int B, int H, int W, int Cin, int Cout, int k, int stride,
                               const float* scale, const float* shift, int act,
                               const float* residual, int ldr, const unsigned* x_amax, unsigned* y_amax, void* stream);
/* max |finite element| over the first C channels of an NHWC tensor (pitch ldx), as a bit pattern (mode 3 operand
 * maximum).  y4_amax_f32 overwrites *amax_bits; y4_amax_merge_u32 folds *src into *dst (a concat buffer's maximum is
 * the maximum of its parts).  Integer atomicMax: order independent. */
int y4_amax_f32(const float* x, int ldx, long long M, int C, unsigned* amax_bits, void* stream);
int y4_amax_merge_u32(unsigned* dst, const unsigned* src, void* stream);

/* Measurement aid (bench.py): copies the symbol of the conv kernel the calling host thread launched last, spelled as
 * rocprofv3 --stats prints it, into buf (NUL-terminated, at most cap bytes) and clears it; empty when the last launch
 * was not an f16x2-mode kernel.  No reference counterpart. */
int y4_last_conv_kernel(char* buf, int cap);

/* Training-mode variant: raw conv output + BatchNorm batch statistics fused into the epilogue.
 * partials receives one row [2][Cout] (column sums, sums of squares) per M-tile; *nparts_host
 * (HOST int64) is set to the number of rows written; feed both to y4_bn_finalize_partials_f32.
 * partial_bytes >= y4_conv2d_bnstats_workspace(). */
size_t y4_conv2d_bnstats_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride);
int y4_conv2d_fwd_bnstats_f32(const float* x, int ldx, const float* w, float* y, int ldy,
                              int B, int H, int W, int Cin, int Cout, int k, int stride,
                              float* partials, size_t partial_bytes, long long* nparts_host,
                              const unsigned* x_amax /* mode 3, nullable */,
                              void* workspace, size_t workspace_bytes /* as y4_conv2d_fwd_f32 */,
                              void* dgrad_filter /* nullable; mode 3: also receives the transposed filter planes, in the layout of
                                 y4_conv2d_dgrad_f32's workspace -- that call then takes this buffer as its workspace with
                                 w == NULL and launches no filter kernels (one split launch serves forward and backward) */,
                              size_t dgrad_filter_bytes /* >= y4_conv2d_dgrad_workspace(Cin, Cout, k) */, void* stream);

/* ---- conv mode 3 over PRE-SPLIT activations ("planes", csrc/conv_planes.hip): the input arrives as the two fp16 pieces
 * of the f16x2 split, per pixel and 32-channel K tile [64 B: 32 hi halfs | 64 B: 32 scaled-lo halfs] (4 bytes per element,
 * pitch 4 Cin bytes, Cin % 32 == 0), scaled by the power of two that *x_amax (an upper bound of max|x|) implies; that is
 * the form the BatchNorm sweeps can emit directly, and the form LDS-DMA can stage without touching the VALU.
 * y4_planes_split_f32 converts an fp32 NHWC tensor (tests, tensors produced by kernels that do not emit planes).
 * y4_conv2d_fwd_planes_f32 = y4_conv2d_fwd_bnstats_f32 on such an input (raw output + per-M-tile column sums, 256- or 128-row tiles;
 * partials may be NULL); workspace as y4_conv2d_fwd_f32.  Replaces the same nn.Conv2d, darknet/darknet.py:31-36,53-54. */
int y4_planes_split_f32(const float* x, int ldx, long long M, int C, const unsigned* amax, void* planes, void* stream);
/* The same into a CHANNEL SLICE of a wider pre-split tensor (a concat buffer whose other slices their producers write pre-split,
 * y4_bn_planes_bound_f32): `planes` points at the slice's first tile in pixel 0's row (128-B aligned; bf16 mode: byte 2 c of the
 * row for channel offset c), ld_planes = channels per pixel row of the whole tensor; *amax = the tensor's joint scale word, which
 * must dominate max|x|.  c_valid (0: C): source channels >= c_valid are PAD of x's rows (ldx >= C) and leave as zeros -- the
 * 255-channel head gradient as 256 pre-split channels.  Replaces the copy half of torch.cat, yolo/model/yolov4.py:176,183 (PANBlock). */
int y4_planes_split_into_f32(const float* x, int ldx, long long M, int C, const unsigned* amax, void* planes, int ld_planes, int c_valid,
                             void* stream);
int y4_conv2d_fwd_planes_f32(const void* x_planes, const float* w, float* y, int ldy,
                             int B, int H, int W, int Cin, int Cout, int k, int stride,
                             float* partials, size_t partial_bytes, long long* nparts_host, const unsigned* x_amax,
                             void* workspace, size_t workspace_bytes,
                             void* dgrad_filter /* nullable: as in y4_conv2d_fwd_bnstats_f32 -- stride 1: for
                                y4_conv2d_dgrad_planes_f32 (mirrored taps); stride 2: for y4_conv2d_dgrad_f32 (the register-staged
                                parity-class dgrad, taps as they are) */,
                             size_t dgrad_filter_bytes,
                             int y_bf16 /* != 0 (Cout % 32 == 0): y leaves as plain bf16 (RN) in the FIRST HALF of each fp32-sized row
                                (pitch 4 ldy bytes), the column sums are those of the rounded values; the BatchNorm sweeps read it
                                with y4_bn_act_fwd_f32 z_planes + 16 / y4_bn_act_bwd_f32 frozen_stats bit 2 */,
                             const float* bias /* nullable [Cout]: added to every result row (a conv WITHOUT BatchNorm -- the head's
                                output convs, yolo/model/yolov4.py:235-239 -- reading a pre-split input; partials NULL, y_bf16 0) */,
                             void* stream);

/* dgrad / wgrad (stride 1, and the 3x3 stride-2 layers on even maps) of a conv over planes (dy, and for wgrad also
 * x, pre-split as above; Cin % 32 == 0, Cout % 32 == 0): the same arithmetic as y4_conv2d_dgrad_f32 / y4_conv2d_wgrad_f32 in
 * conv mode 3 (conv mode 2: plain bf16 operands, 64-channel multiples, stride 1).  dgrad runs the forward DMA kernel on the
 * mirrored transposed filter (workspace: y4_conv2d_dgrad_workspace()); wgrad stages both operands pixel-major and takes its
 * fragments through the hardware transpose read (split-K slabs in y4_conv2d_wgrad_planes_workspace() bytes, fixed-order
 * reduce: deterministic); H, W are the INPUT dims.  wgrad alone also takes a Cout that is NOT whole K tiles (the head's 255): dy's
 * pixel rows then hold ceil(Cout / 32) tiles (64-channel units in the bf16 mode) whose pad channels are zero, dW has Cout rows.
 * Autograd of the same nn.Conv2d, darknet/darknet.py:31-36. */
int y4_conv2d_dgrad_planes_f32(const void* dy_planes, const float* w /* NULL: workspace prepared by the forward call */, float* dx, int lddx,
                               int B, int H, int W, int Cin, int Cout, int k,
                               int stride /* 1; or 2 (3x3, H and W even, conv mode 3 operands, no residual): four launches, one per
                                  parity class of dx over its 1 / 2 / 2 / 4 taps; the workspace then holds the UN-mirrored
                                  transposed planes (what the forward call prepares for a stride-2 layer) */,
                               void* workspace, size_t workspace_bytes, const unsigned* dy_amax,
                               const float* residual, int ldr, void* stream);
size_t y4_conv2d_wgrad_planes_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride);
int y4_conv2d_wgrad_planes_f32(const void* x_planes, const void* dy_planes, float* dw,
                               int B, int H, int W, int Cin, int Cout, int k, int stride,
                               void* workspace, size_t workspace_bytes, const unsigned* x_amax, const unsigned* dy_amax,
                               void* stream);

/* Any other ConvBNAct shape (darknet/darknet.py:25-36 takes any in_ch / out_ch / odd kernel_size / stride): direct kernels,
 * one thread per output element, plain fp32 fma chains -- written for correctness, YOLOv4 never builds such a layer.
 * Same NHWC / KRSC conventions and epilogue (scale, shift, act, residual) as y4_conv2d_fwd_f32; pad = (k - 1) / 2.
 * y4_conv2d_stem_dgrad_f32: gradient wrt the 3-channel network input (element strides as y4_conv2d_stem_fwd_f32). */
int y4_conv2d_generic_fwd_f32(const float* x, int ldx, const float* w, float* y, int ldy,
                              int B, int H, int W, int Cin, int Cout, int k, int stride,
                              const float* scale, const float* shift, int act, const float* residual, int ldr, void* stream);
int y4_conv2d_generic_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx,
                                int B, int H, int W, int Cin, int Cout, int k, int stride,
                                const float* residual, int ldr, void* stream);
int y4_conv2d_generic_wgrad_f32(const float* x, int ldx, const float* dy, int lddy, float* dw,
                                int B, int H, int W, int Cin, int Cout, int k, int stride, void* stream);
int y4_conv2d_stem_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, long long sxb, long long sxc, long long sxh,
                             long long sxw, int B, int H, int W, int Cout, void* stream);

/* Stem conv (Cin = 3): x addressed as x[b*sxb + c*sxc + h*sxh + w*sxw] so both the NCHW
 * tensor the reference feeds (yolo/engine/build.py:60) and NHWC work without a copy.
 * bnstats_partials (nullable): [ceil(B*H*W/256)][2][Cout] column sums of the output, valid when
 * scale/shift are NULL and act is linear (training-mode BatchNorm statistics). */
int y4_conv2d_stem_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw,
                           const float* w, float* y, int ldy, int B, int H, int W, int Cout,
                           const float* scale, const float* shift, int act,
                           float* bnstats_partials, void* stream);

/* dgrad: dx[B,H,W,Cin] = conv_transpose(dy[B,Ho,Wo,Cout], w) (+ residual) -- autograd of nn.Conv2d wrt input.
 * workspace: y4_conv2d_dgrad_workspace() bytes (holds the [Cin][k][k][Cout4] transposed filter).
 * residual (nullable, pitch ldr >= Cin): added in the epilogue -- the gradient arriving over a ResBlock's skip
 * connection (darknet/darknet.py:76-80: x + f(x)), so the fan-in add costs no extra pass. */
size_t y4_conv2d_dgrad_workspace(int Cin, int Cout, int k);
int y4_conv2d_dgrad_f32(const float* dy, int lddy, const float* w /* mode 3: NULL = workspace prepared by the forward call */, float* dx, int lddx,
                        int B, int H, int W, int Cin, int Cout, int k, int stride,
                        void* workspace, size_t workspace_bytes, const unsigned* dy_amax /* mode 3, nullable */,
                        const float* residual, int ldr, void* stream);

/* wgrad: dw[Cout][k][k][Cin] = sum_{b,ho,wo} dy (x) x -- autograd of nn.Conv2d wrt weight.
 * Split-K over pixels into fp32 slabs in `workspace`, reduced in a fixed order (deterministic). */
size_t y4_conv2d_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride);
int y4_conv2d_wgrad_f32(const float* x, int ldx, const float* dy, int lddy, float* dw,
                        int B, int H, int W, int Cin, int Cout, int k, int stride,
                        void* workspace, size_t workspace_bytes,
                        const unsigned* x_amax, const unsigned* dy_amax /* mode 3, nullable */, void* stream);
size_t y4_conv2d_stem_wgrad_workspace(int B, int H, int W, int Cout);
int y4_conv2d_stem_wgrad_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw,
                             const float* dy, int lddy, float* dw, int B, int H, int W, int Cout,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Stem conv + training-mode BatchNorm + activation WITHOUT the pre-BatchNorm tensor (csrc/stem_fused.hip): every pass
 * re-forms y0 = conv(x, w) in registers (the arithmetic of y4_conv2d_stem_fwd_f32 in conv modes 1-3, bit for bit), so
 * neither y0 nor its gradient is ever stored.  x as in y4_conv2d_stem_fwd_f32 (element strides), w KRSC [Cout][3][3][3].
 * y4_stem_fused_ok: 1 if the passes can address the problem in the current conv mode (modes 1-3; Cout <= 32, a multiple
 *   of 4; W >= 5; non-negative strides; the whole of x inside one 32-bit byte window) -- z and dz are windowed per 256-pixel
 *   group and may be of any size.  Otherwise 0: use the separate conv / BatchNorm calls.
 * y4_stem_bn_act_fwd_f32: batch statistics (mean, invstd and the running statistics exactly as y4_conv2d_stem_fwd_f32 +
 *   y4_bn_finalize_partials_f32 leave them; the workspace begins with the same [ceil(B*H*W/256)][2][Cout] partial rows),
 *   then z[B*H*W][ldz] = act((y0 - mean) * invstd * gamma + beta) and max|z| folded into *out_amax (nullable) as
 *   y4_bn_act_fwd_f32 does.
 * y4_stem_bn_act_bwd_f32: dgamma, dbeta as y4_bn_act_bwd_f32 (batch statistics) and dw[Cout][3][3][3] = wgrad(x, dy0) with
 *   dy0 = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), g = dz * act'(gamma * xhat + beta), kept in registers.
 * All reductions are two-stage and fixed-order (deterministic); workspaces are private to the call in stream order. */
int y4_stem_fused_ok(long long sxb, long long sxc, long long sxh, long long sxw, int B, int H, int W, int Cout);
size_t y4_stem_bn_act_fwd_workspace(int B, int H, int W, int Cout);
int y4_stem_bn_act_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                           int B, int H, int W, int Cout, const float* gamma, const float* beta, int act,
                           float* mean, float* invstd, float* running_mean, float* running_var, long long* num_batches_tracked,
                           float momentum, float eps, float* z, int ldz, unsigned* out_amax,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t y4_stem_bn_act_bwd_workspace(int B, int H, int W, int Cout);
int y4_stem_bn_act_bwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                           const float* dz, int lddz, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, int act, int B, int H, int W, int Cout,
                           float* dgamma, float* dbeta, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- BatchNorm + activation
 * Replaces nn.BatchNorm2d (training mode: batch statistics, eps 1e-5, momentum 0.1, biased
 * variance for normalisation, unbiased for running_var) + the activation,
 * darknet/darknet.py:37-51,55-56.  M = B*H*W pixels, C channels.
 *
 * y4_bn_stats_f32: mean[c], invstd[c] = 1/sqrt(var_biased+eps); running stats updated in place
 *   (running = (1-m)*running + m*batch; running_var uses var*M/(M-1)); *num_batches_tracked += 1.
 *   running_mean/running_var/num_batches_tracked may be NULL.  workspace: y4_bn_workspace(M, C)
 *   bytes (fp64 accumulators + per-block fp32 partial rows; no contended atomics).
 * y4_bn_finalize_partials_f32: same outputs from the per-M-tile column sums [nparts][2][C] that
 *   y4_conv2d_fwd_bnstats_f32 / y4_conv2d_stem_fwd_f32 leave behind (statistics fused into the conv
 *   epilogue: the conv output is not read again).  workspace: y4_bn_finalize_workspace(C) bytes.
 * All reductions are two-stage and fixed-order (fp32 partial rows -> <= 64 fp64 rows -> one), i.e. deterministic.
 */
size_t y4_bn_workspace(long long M, int C);
size_t y4_bn_finalize_workspace(int C);
int y4_bn_stats_f32(const float* y, int ldy, long long M, int C, float* mean, float* invstd,
                    float* running_mean, float* running_var, long long* num_batches_tracked,
                    float momentum, float eps, void* workspace, size_t workspace_bytes, void* stream);
int y4_bn_finalize_partials_f32(const float* partials, long long nparts, long long M, int C,
                                float* mean, float* invstd, float* running_mean, float* running_var,
                                long long* num_batches_tracked, float momentum, float eps,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The analytic bound of max|act(BatchNorm(y))| that y4_bn_act_fwd_f32 (z_planes == 2) derives by itself, as a call of its own:
 * *out = max(bound(gamma, beta, M), floor_word ? *floor_word : 0).  For SEVERAL BatchNorm layers that write channel slices of one
 * pre-split tensor (the concat in front of a CSP transition conv, darknet/darknet.py:154-163 in the reference): chain the calls
 * through floor_word, then hand the joint word to every producer's y4_bn_act_fwd_f32 with z_planes == 1, z = its slice and
 * ldz = the pitch of the whole tensor -- one scale for the whole operand, no measuring pass. */
int y4_bn_planes_bound_f32(const float* gamma, const float* beta, int C, long long M, const unsigned* floor_word, unsigned* out,
                           void* stream);
/* z = act(gamma*(y-mean)*invstd + beta) + residual   (residual may be NULL).
 * out_amax (nullable, device word): max|finite z| is folded into it with atomicMax (the caller zeroes it, or it
 * already holds the maximum of other parts of the same concat buffer) -- the operand maximum of conv mode 3.
 * z == NULL: measure only (max|z| into *out_amax, nothing stored).
 * z_planes != 0: z (C % 32 == 0; ldz == C, or z = a channel slice of a wider pre-split tensor: ldz % 32 == 0 and z 128-B aligned --
 * for z_planes == 3 the slice of channels [c, c + C) starts at byte 2 c of the row) receives the tensor PRE-SPLIT for the plane conv kernels -- per pixel and
 * 32-channel K tile [64 B: hi halfs | 64 B: scaled lo halfs], 4 bytes per element -- scaled by the power of two that
 * *out_amax implies.  z_planes == 1: *out_amax must already hold max|z| or an upper bound (e.g. a measure-only call on the
 * same arguments).  z_planes == 2: the call derives the bound itself, without a pass over the data -- |xhat| <= sqrt(M - 1)
 * for any sample of M values, |act(v)| <= |v|, so |z| <= max_c(|gamma_c| sqrt(M - 1) + |beta_c|) + max|residual|
 * (res_amax: the residual's maximum word, required with a residual) -- and leaves it in *out_amax for the consumers.  A
 * loose bound costs the split only headroom (full precision down to 2^-29 of the bound).
 * z_planes + 16: y itself holds plain bf16 values in the first half of each row (y4_conv2d_fwd_planes_f32 y_bf16).
 * z_planes == 3 (conv mode 2, bf16 MFMA conv): z receives plain bf16 values (RN), dense per pixel in the FIRST HALF of the
 * fp32-sized row (ldz == C: the row pitch stays 4 C bytes, the second half is not touched); out_amax is not used.
 * planes_twin (nullable, with z_planes != 0): z stays fp32 (pitch ldz) and planes_twin [M][C] receives the pre-split copy --
 * for a tensor that feeds both a plane-consuming conv and fp32 consumers (a fork in front of a detection head). */
int y4_bn_act_fwd_f32(const float* y, int ldy, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, int act,
                      const float* residual, int ldr, float* z, int ldz,
                      long long M, int C, unsigned* out_amax, int z_planes, const unsigned* res_amax, float* planes_twin,
                      void* stream);
/* Backward of the two ops above wrt y, gamma, beta given dz (grad wrt z; the residual branch
 * receives dz itself).  dy may alias dz.  workspace: y4_bn_workspace(M, C) bytes. */
int y4_bn_act_bwd_f32(const float* dz, int lddz, const float* y, int ldy,
                      const float* mean, const float* invstd, const float* gamma, const float* beta,
                      int act, float* dy, int lddy, float* dgamma, float* dbeta,
                      long long M, int C, void* workspace, size_t workspace_bytes,
                      unsigned* out_amax /* nullable: max|finite dy|, as above */,
                      unsigned* f16_planes /* nullable, 8 zeroed device words, conv mode 3: dy is written PRE-SPLIT for the
                         plane conv kernels (layout as y4_bn_act_fwd_f32 z_planes; lddy == C, C % 32 == 0), scaled by a
                         bound of max|dy| derived before the sweep; word [5] receives that bound and serves as dy_amax
                         of y4_conv2d_dgrad_planes_f32 / y4_conv2d_wgrad_planes_f32 */,
                      float* planes_twin /* nullable, with f16_planes: dy stays fp32 (pitch lddy) and planes_twin [M][C]
                         receives the pre-split copy -- a layer whose wgrad runs on the plane kernel and whose dgrad does
                         not (3x3 stride 2) */,
                      int frozen_stats /* bit 0: mean / invstd are constants (eval-mode BatchNorm under autograd: running
                         statistics), so dy = gamma invstd g without the two batch-statistic terms; dgamma / dbeta as usual.
                         bit 2: y holds plain bf16 values in the first half of each row (as y4_bn_act_fwd_f32 z_planes + 16).
                         bit 1 (conv mode 2): dy leaves as plain bf16 in the first half of each fp32-sized row, as
                         y4_bn_act_fwd_f32 z_planes == 3 (lddy == C, C % 32 == 0, f16_planes NULL) */,
                      void* stream);
/* The backward of conv 1x1 / stride 1 -> BatchNorm (batch statistics) -> activation in one call, conv mode 3, for the HBM-bound
 * layers on large maps ((Cout, Cin) in {(64, 64), (32, 64), (64, 128)}): y4_bn_act_bwd_f32 with the plane bound, then
 * y4_conv2d_dgrad_f32 and y4_conv2d_wgrad_f32 on its dy -- but dy is formed in registers by ONE kernel that reads dz, y, x
 * (+ res) and writes dx and the split-K slabs of dW; it is never stored (csrc/conv1x1_bwd_fused.hip).  dy is split under the
 * bound of max|dy| the reduce pass derives (bounds[5], as f16_planes above), not under a measured maximum.  Two-stage
 * fixed-order reductions throughout: deterministic.  Any other shape, frozen statistics, another conv mode or a pointer / pitch
 * that is not 16-byte aligned returns Y4_ERR_SHAPE before anything is launched or written. */
size_t y4_conv1x1_bn_act_bwd_fused_workspace(long long M, int Cin, int Cout);
int y4_conv1x1_bn_act_bwd_fused_f32(const float* dz, int lddz, const float* y, int ldy,
                                    const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                                    float* dgamma, float* dbeta, long long M /* B*H*W */, int Cin, int Cout,
                                    const float* x, int ldx, const unsigned* x_amax /* nullable: one extra pass over x */,
                                    const float* w /* [Cout][Cin]; may be NULL with w_prepared */,
                                    const void* w_prepared /* nullable: the transposed split filter as the forward call left it in
                                       its dgrad_filter buffer (y4_conv2d_fwd_bnstats_f32), maximum word included */,
                                    float* dx, int lddx, const float* res /* nullable [M][Cin]: added to dx */, int ldr,
                                    float* dw /* [Cout][Cin] */, void* workspace, size_t workspace_bytes,
                                    unsigned* bounds /* 8 zeroed device words; [5] receives the bound of max|dy| */,
                                    int frozen_stats /* must be 0 */, void* stream);
/* dbias[c] = sum_m dy[m,c]  (bias=True head convs, yolov4.py:237,243,249): two fixed-order stages, no atomics
 * (deterministic).  workspace: y4_bias_grad_workspace(M, C) bytes */
size_t y4_bias_grad_workspace(long long M, int C);
int y4_bias_grad_f32(const float* dy, int lddy, long long M, int C, float* dbias,
                     void* workspace, size_t workspace_bytes, void* stream);
/* eval-mode fold (darknet.py:55 in eval): scale = gamma/sqrt(running_var+eps),
 * shift = beta - running_mean*scale */
int y4_bn_fold_f32(const float* gamma, const float* beta, const float* running_mean,
                   const float* running_var, float eps, float* scale, float* shift, int C, void* stream);

/* ---------------------------------------------------------------- pointwise glue
 * torch.cat along channels (darknet.py:110,135; yolov4.py:71,139,146,181,186): copy src[M,C]
 * into dst[:, c_off:c_off+C]. */
int y4_copy_channels_f32(const float* src, int lds, float* dst, int ldd, long long M, int C, void* stream);
/* out[M,C] = a[M,C] + b[M,C] (gradient fan-in at forks: residual skip, CSP split, FPN/PAN taps);
 * out may alias a or b. */
int y4_add_f32(const float* a, int lda, const float* b, int ldb, float* out, int ldo,
               long long M, int C, void* stream);
/* nn.MaxPool2d(ksize, stride 1, pad ksize//2), yolov4.py:60-62,68-70.  idx (int8, per output
 * element: window offset dy*ksize+dx of the first maximum) may be NULL in inference. */
int y4_maxpool_s1_fwd_f32(const float* x, int ldx, float* y, int ldy, signed char* idx,
                          int B, int H, int W, int C, int ksize, void* stream);
int y4_maxpool_s1_bwd_f32(const float* dy, int lddy, const signed char* idx, float* dx, int lddx,
                          int accumulate, int B, int H, int W, int C, int ksize, void* stream);
/* nn.MaxPool2d(2, 2) (YOLOv4-tiny; csrc/tiny.hip): y[B, H/2, W/2, C], floor -- an odd last row / column is not read.
 * Arguments as y4_maxpool_s1_*: NHWC with pixel pitches (x may be a concat buffer or a channel slice), C % 4 == 0,
 * pitches % 4 == 0, 16-byte aligned bases.  idx (int8 per output element, dense [B*Ho*Wo][C]; NULL in inference): the code
 * 2*dy + dx of the selected element; selection is aten's (row-major scan, v > best || isnan(v): the first maximum wins a
 * tie, the last NaN keeps the code).  Backward writes EVERY element of dx exactly once (dy where the code points, 0
 * elsewhere and in a dropped odd row / column): no pre-zeroing, no accumulation.  H < 2 or W < 2: no output element;
 * forward returns Y4_OK without a launch, backward (dy, idx may then be NULL) fills dx with zeros. */
int y4_maxpool2x2_s2_fwd_f32(const float* x, int ldx, float* y, int ldy, signed char* idx, int B, int H, int W, int C,
                             void* stream);
int y4_maxpool2x2_s2_bwd_f32(const float* dy, int lddy, const signed char* idx, float* dx, int lddx, int B, int H, int W, int C,
                             void* stream);
/* Gradient fan-in of Darknet's half-channel route (route groups=2 group_id=1: a tensor read whole and as its upper half):
 * dx[M, C] = g_full[M, C] + [0 | g_hi[M, C/2]]; g_full or g_hi (not both) may be NULL and stands for zeros.  C % 8 == 0,
 * pitches % 4 == 0, 16-byte aligned bases; dx may alias g_full.  One launch, every element of dx written once. */
int y4_fork_half_bwd_f32(const float* g_full, int ldf, const float* g_hi, int ldh, float* dx, int ldx, long long M, int C,
                         void* stream);
/* Stem conv 3 -> Cout, 3x3, STRIDE 2, pad 1 (YOLOv4-tiny's first layer; csrc/tiny.hip), Cout % 4 == 0, Cout <= 64.
 * x by element strides as y4_conv2d_stem_fwd_f32, w KRSC [Cout][3][3][3], y / dy NHWC [B, Ho, Wo, Cout] with a pitch
 * (% 4, 16-byte aligned base), Ho = (H - 1) / 2 + 1.  Forward: one fp32 fma chain per output over the in-bounds taps in
 * (r, q, c) order, then scale / shift / act as y4_conv2d_generic_fwd_f32 -- the same bits as that kernel.
 * wgrad: dw[n][r][q][c] = sum over output pixels of dy x; per-block partial slabs in `workspace`
 * (y4_conv2d_stem_s2_wgrad_workspace bytes, 16-byte aligned), folded in fp64 in a fixed order (deterministic). */
int y4_conv2d_stem_s2_fwd_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* w,
                              float* y, int ldy, int B, int H, int W, int Cout, const float* scale, const float* shift, int act,
                              void* stream);
size_t y4_conv2d_stem_s2_wgrad_workspace(int B, int H, int W, int Cout);
int y4_conv2d_stem_s2_wgrad_f32(const float* x, long long sxb, long long sxc, long long sxh, long long sxw, const float* dy,
                                int lddy, float* dw, int B, int H, int W, int Cout, void* workspace, size_t workspace_bytes,
                                void* stream);
/* nearest x2 upsample, yolov4.py:77-90, and its adjoint (2x2 block sum). */
int y4_upsample2x_fwd_f32(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, void* stream);
int y4_upsample2x_bwd_f32(const float* dy, int lddy, float* dx, int lddx, int B, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------- YOLO head decode
 * Replaces YOLOLayer.forward, yolo/model/yololayer.py:88-166.  logits: head conv output
 * NHWC [B,F,F,>=A*(5+C)] pitch ldl; anchors_wh: A pairs (w,h) in grid units (host array).
 * train: output [B,A,F,F,5+C] (sigmoid on ch 0,1,4..; raw 2,3) and pred [B,A,F,F,4] (grid units).
 * eval : out[b, box_off + a*F*F + j*F + i, :] of an [B,n_total,5+C] buffer, boxes x stride. */
int y4_yolo_decode_train_f32(const float* logits, int ldl, float* output, float* pred,
                             int B, int F, int A, int n_classes, const float* anchors_wh_host, void* stream);
int y4_yolo_decode_eval_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                            int B, int F, int A, int n_classes, const float* anchors_wh_host,
                            float stride, void* stream);
/* d(logits) (NHWC, pitch ldl, pad channels zeroed) from d(output) and d(pred) (either NULL). */
int y4_yolo_decode_bwd_f32(const float* logits, int ldl, const float* g_output, const float* g_pred,
                           float* g_logits, int B, int F, int A, int n_classes,
                           const float* anchors_wh_host, void* stream);
/* The same three with the YOLOv4 grid-sensitivity factor scale_x_y (Darknet's [yolo] scale_x_y: 1.2 / 1.1 / 1.05 per
 * layer, 2.0 in the scaled models).  s = scale_xy as fp32, h = (s - 1) * 0.5f in fp32, sigma = the fp32 sigmoid:
 *   train: pred[..., 0] = ((sigma_x * s) - h) + i, pred[..., 1] = ((sigma_y * s) - h) + j; output[..., 0:2] stays sigma.
 *   eval : the same centre, times stride.  With s != 1 the eval centre is evaluated in fp64 from the logit and rounded to fp32
 *          once: sigma * s - h cancels in the first column / row, where an fp32 sigmoid would be arbitrarily far off relative
 *          to the result.  In training the tiled kernel evaluates sigma * s + (i - h): other roundings, the same value to a
 *          few ulp of its largest addend.
 *   bwd  : the g_pred contribution on channels 0 and 1 is s * g_pred.
 * w, h, objectness and classes are untouched.  scale_xy = 1 gives the bits of the entries above (sigma * 1 and x - 0 are
 * exact), which forward here.  scale_xy outside [1, 2], NaN included: Y4_ERR_SHAPE before any launch. */
int y4_yolo_decode_train_ex_f32(const float* logits, int ldl, float* output, float* pred,
                                int B, int F, int A, int n_classes, const float* anchors_wh_host, float scale_xy,
                                void* stream);
int y4_yolo_decode_eval_ex_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                               int B, int F, int A, int n_classes, const float* anchors_wh_host,
                               float stride, float scale_xy, void* stream);
int y4_yolo_decode_bwd_ex_f32(const float* logits, int ldl, const float* g_output, const float* g_pred,
                              float* g_logits, int B, int F, int A, int n_classes,
                              const float* anchors_wh_host, float scale_xy, void* stream);
/* The eval decode on a rectangular map (letterboxed inference): logits NHWC [B,Fh,Fw,>=A*(5+C)];
 * out[b, box_off + a*Fh*Fw + j*Fw + i, :], x from the column i < Fw, y from the row j < Fh.  Same kernels, dispatch rule and
 * arithmetic as y4_yolo_decode_eval_ex_f32, whose bits it gives when Fh == Fw.  box_off + A*Fh*Fw > n_total: Y4_ERR_SHAPE. */
int y4_yolo_decode_eval_rect_f32(const float* logits, int ldl, float* out, long long n_total, long long box_off,
                                 int B, int Fh, int Fw, int A, int n_classes, const float* anchors_wh_host,
                                 float stride, float scale_xy, void* stream);

/* ---------------------------------------------------------------- detection loss
 * Replaces YOLOLoss.build_target + YOLOLoss.forward for one layer,
 * yolo/model/yololoss.py:118-371,385-432.  labels: [B,K,5] fp32 rows (xc,yc,w,h,cls) in input
 * pixels.  all_anchors_host: 9 (w,h) pairs in grid units of this layer; anch_mask_host: the A
 * indices of this layer.  Outputs (all device):
 *   obj_mask [B,A,F,F] fp32, pos_index [B,A,F,F] int32 (-1 or index into pos_rec),
 *   pos_rec [B,K,8+ceil(C/32)] (x,y,w,h targets, scale, cell, class bitmask), npos [B],
 *   loss_parts[4] doubles (xy, wh, obj, cls), deterministic two-stage reduction.
 * workspace: y4_yolo_loss_workspace() bytes.  Its last array, pos_box [B,K,4], holds per record the truth box
 * (xc,yc,w,h) = label / stride of the last label that hit the cell, for y4_yolo_box_loss_*_f32 below.
 */
size_t y4_yolo_loss_workspace(int B, int F, int A, int K, int n_classes);
int y4_yolo_loss_fwd_f32(const float* output, const float* pred, const float* labels, int K,
                         int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                         const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                         float* obj_mask, double* loss_parts,
                         void* workspace, size_t workspace_bytes, void* stream);
/* grad wrt `output` (dense [B,A,F,F,5+C]) scaled by *gscale (DEVICE scalar: the upstream grad of
 * the loss, so no host sync is needed); uses the workspace filled by fwd.  output_is_masked = 1
 * when y4_yolo_loss_mask_output_f32 has already been applied to `output` (the reference's
 * in-place side effect): the w/h channels then hold o*scale. */
int y4_yolo_loss_bwd_f32(const float* output, int output_is_masked, const float* obj_mask,
                         const float* gscale, float* g_output,
                         int B, int F, int A, int K, int n_classes,
                         const void* workspace, size_t workspace_bytes, void* stream);
/* the reference's in-place side effect on outputs[*]['output'] (yololoss.py:402-407) */
int y4_yolo_loss_mask_output_f32(float* output, const float* obj_mask, int B, int F, int A, int K,
                                 int n_classes, const void* workspace, size_t workspace_bytes, void* stream);
/* dense views of the sparse targets for API parity / tests (yololoss.py:173-187 tensors) */
int y4_yolo_loss_dense_targets_f32(float* target, float* tgt_mask, float* tgt_scale,
                                   int B, int F, int A, int K, int n_classes,
                                   const void* workspace, size_t workspace_bytes, void* stream);

/* IoU-family box regression on the positive records of the workspace that y4_yolo_loss_fwd_f32 filled (call it first,
 * same B, F, A, K, n_classes).  box_kind: Y4_BOX_IOU | Y4_BOX_GIOU | Y4_BOX_DIOU | Y4_BOX_CIOU.  Per record, in grid
 * units: p = pred[b,a,j,i,:] (xc,yc,w,h), t = label / stride of the LAST label that hit the cell (stored by the assign
 * kernels beside the record); eps = 1e-7f; X = IoU, GIoU, DIoU or CIoU of (p, t) (CIoU's alpha = v / (1 - iou + v + eps)
 * is a constant in the backward).  A NaN anywhere in p makes the record's loss and gradient NaN.
 *   fwd: loss_parts[0] = gain * sum over records of (1 - X), loss_parts[1] = 0; parts 2 and 3 are left as they are.
 *        One block, fixed summation order: two calls give the same bits.
 *   bwd: overwrites channels 0..3 of every positive cell of g_output (dense [B,A,F,F,5+C], already filled by
 *        y4_yolo_loss_bwd_f32) with (*gscale) * gain * (dL/dpx, dL/dpy, dL/dpw * pw, dL/dph * ph): the gradient wrt the
 *        train-mode `output`, whose w / h channels are the raw logits.  The box is read from `pred`, never from `output`
 *        (which y4_yolo_loss_mask_output_f32 may have scaled).  Nothing else of g_output is touched.
 * Errors before any launch: NULL pointer Y4_ERR_NULL; B, F, A, K, n_classes out of range or an unknown box_kind
 * Y4_ERR_SHAPE; workspace_bytes < y4_yolo_loss_workspace() Y4_ERR_WORKSPACE. */
#define Y4_BOX_IOU 1
#define Y4_BOX_GIOU 2
#define Y4_BOX_DIOU 3
#define Y4_BOX_CIOU 4
int y4_yolo_box_loss_fwd_f32(const float* pred, int box_kind, float gain, int B, int F, int A, int K, int n_classes,
                             double* loss_parts, const void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_box_loss_bwd_f32(const float* pred, int box_kind, float gain, const float* gscale, float* g_output,
                             int B, int F, int A, int K, int n_classes,
                             const void* workspace, size_t workspace_bytes, void* stream);

/* YOLOv4 head options of the loss (Darknet's [yolo] iou_thresh and label_smooth_eps; scale_x_y for the box gradient).
 * Every entry above has an _ex form below that takes the options it depends on; the entries above forward to them with
 * iou_thresh = 1, label_smooth = 0, scale_xy = 1 and give the bits they always gave.  The options are not stored in the
 * workspace: pass to every later call the SAME iou_thresh and label_smooth that y4_yolo_loss_fwd_ex_f32 got.
 *
 * iou_thresh in (0, 1]; 1 = off.  Below 1, the positive anchors of a label are its arg-max anchor and every anchor k
 *   whose shape IoU (the fp32 value the arg-max is taken over) is > iou_thresh -- strict; a NaN IoU never is.  In the
 *   layer whose mask holds k the record's anchor slot is the place of k in the mask (anch_mask_host[a] % 3 == a is
 *   required below 1).  The (label, slot) pairs of a layer go through the steps of the single pair -- skip outside the
 *   map, find or create the cell's record, write the targets and the truth box (last writer wins), OR the class bit -- in
 *   the order of the label index t, then of the slot a; records are numbered by first hit in that order, which fixes the
 *   summation order of the box loss.  Record capacity per image: K with iou_thresh = 1 (the layout of
 *   y4_yolo_loss_workspace), K * A below 1: pos_cell, pos_val, pos_cls and pos_box grow, y4_yolo_loss_workspace_ex says
 *   by how much (it returns 0 for arguments out of range).
 * label_smooth in [0, 1): class BCE targets are 1 - 0.5 * label_smooth where the class bit is set and 0.5 * label_smooth
 *   where it is not (both fp32), in the loss forward, its backward and the dense targets (target[..., 5:] of positive
 *   cells; 0 elsewhere).  Objectness is not smoothed.
 * scale_xy in [1, 2] (box-loss backward only): channels 0 and 1 become (*gscale) * gain * scale_xy * dL/dp{x,y}, since
 *   d pred / d output = scale_xy there.  The forward needs nothing: it reads the scaled centres from `pred`.
 * Errors before any launch: NULL pointer Y4_ERR_NULL; an option or a shape out of range (NaN included) Y4_ERR_SHAPE;
 * workspace_bytes < y4_yolo_loss_workspace_ex(.., iou_thresh) Y4_ERR_WORKSPACE. */
size_t y4_yolo_loss_workspace_ex(int B, int F, int A, int K, int n_classes, float iou_thresh);
int y4_yolo_loss_fwd_ex_f32(const float* output, const float* pred, const float* labels, int K,
                            int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                            const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                            float iou_thresh, float label_smooth, float* obj_mask, double* loss_parts,
                            void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_loss_bwd_ex_f32(const float* output, int output_is_masked, const float* obj_mask,
                            const float* gscale, float* g_output,
                            int B, int F, int A, int K, int n_classes, float iou_thresh, float label_smooth,
                            const void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_loss_mask_output_ex_f32(float* output, const float* obj_mask, int B, int F, int A, int K,
                                    int n_classes, float iou_thresh, const void* workspace, size_t workspace_bytes,
                                    void* stream);
int y4_yolo_loss_dense_targets_ex_f32(float* target, float* tgt_mask, float* tgt_scale,
                                      int B, int F, int A, int K, int n_classes, float iou_thresh, float label_smooth,
                                      const void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_box_loss_fwd_ex_f32(const float* pred, int box_kind, float gain, int B, int F, int A, int K, int n_classes,
                                float iou_thresh, double* loss_parts, const void* workspace, size_t workspace_bytes,
                                void* stream);
int y4_yolo_box_loss_bwd_ex_f32(const float* pred, int box_kind, float gain, const float* gscale, float* g_output,
                                int B, int F, int A, int K, int n_classes, float iou_thresh, float scale_xy,
                                const void* workspace, size_t workspace_bytes, void* stream);

/* Focal loss, IoU-aware objectness and objectness / class gains of the loss.  The four entries below are the _ex entries
 * with every option of the dense loss in one plain struct; the entries above forward to them with the defaults
 *   iou_thresh 1, label_smooth 0, focal_gamma 0, focal_alpha 0.25, focal_terms 3, obj_iou_ratio 0,
 *   obj_iou_kind Y4_BOX_CIOU, obj_gain 1, cls_gain 1
 * and give the bits they always gave: with focal_gamma = 0, obj_iou_ratio = 0 and both gains 1 the kernels that run
 * are the ones in which the options do not exist.  Nothing is stored in the workspace about the options: pass every
 * later call the same opts the forward got.  y4_yolo_loss_mask_output*_f32 and y4_yolo_box_loss_*_f32 do not depend
 * on them; they accept the larger workspace.
 *
 * With o the value in `output` (the decode's fp32 sigmoid), t the element's target, bce / bce_grad the terms of the
 * entries above (logs clamped at -100, denominator guarded by 1e-12), all in fp32:
 * focal_gamma 0 (off) or in [0.5, 5]; focal_alpha 0 (no class balance) or in (0, 1); focal_terms bit 0: objectness,
 *   bit 1: classes (alpha and terms are not looked at with gamma = 0).  The soft-target focal term of YOLOv5:
 *     p_t = t o + (1 - t)(1 - o), q = 1 - p_t, a = alpha > 0 ? t alpha + (1 - t)(1 - alpha) : 1,
 *     FL = (bce a) q^gamma,   dFL/do = a (bce_grad q^gamma - ((bce gamma) q^(gamma - 1)) (2 t - 1)),
 *   the exact derivative; both are 0 at q = 0.  Objectness: every cell with obj_mask != 0; classes: every class element
 *   of a positive record, against the smoothed targets.
 * obj_iou_ratio r in [0, 1]; above 0, the objectness target of a cell with a record is (1 - r) + r max(X, 0), X =
 *   1 - (the box loss of kind obj_iou_kind on that record), on the operands and with the bits of y4_yolo_box_loss_fwd.
 *   A NaN X (a NaN in the cell's pred) makes the target, the cell's objectness loss and gradient and loss_parts[2] NaN.
 *   X is a constant in the backward.  The targets are kept in pos_obj [B, R] floats, appended to the workspace after
 *   pos_box (y4_yolo_loss_workspace_opts; with r = 0 the size is y4_yolo_loss_workspace_ex's and nothing touches the
 *   array); target[..., 4] of the dense targets holds them.
 * obj_gain, cls_gain finite and > 0: loss_parts[2] and [3] are multiplied once, in fp64, after the reduction; the
 *   gradient is ((g gain) *gscale) on channel 4 / the class channels.
 * Errors before any launch: NULL pointer (opts included) Y4_ERR_NULL; an option out of range (NaN included)
 * Y4_ERR_SHAPE, 0 from the size query. */
typedef struct y4_loss_opts {
    float iou_thresh, label_smooth;
    float focal_gamma, focal_alpha;
    int   focal_terms;       /* bit 0: obj, bit 1: cls */
    float obj_iou_ratio;
    int   obj_iou_kind;      /* Y4_BOX_IOU .. Y4_BOX_CIOU */
    float obj_gain, cls_gain;
} y4_loss_opts;      /* 36 bytes */
size_t y4_yolo_loss_workspace_opts(int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts /* host */);
int y4_yolo_loss_fwd_opts_f32(const float* output, const float* pred, const float* labels, int K,
                              int B, int F, int A, int n_classes, float stride, float ignore_thresh,
                              const float* all_anchors_host, int n_all_anchors, const int* anch_mask_host,
                              const y4_loss_opts* opts, float* obj_mask, double* loss_parts,
                              void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_loss_bwd_opts_f32(const float* output, int output_is_masked, const float* obj_mask,
                              const float* gscale, float* g_output,
                              int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts,
                              const void* workspace, size_t workspace_bytes, void* stream);
int y4_yolo_loss_dense_targets_opts_f32(float* target, float* tgt_mask, float* tgt_scale,
                                        int B, int F, int A, int K, int n_classes, const y4_loss_opts* opts,
                                        const void* workspace, size_t workspace_bytes, void* stream);

/* Per-layer training statistics of the loss (Darknet's "Avg IOU, .5R, .75R, Class, Obj, No Obj, count" line), read from
 * `output`, `pred`, `obj_mask` and the workspace that y4_yolo_loss_fwd_opts_f32 has just filled with the same opts.  Call
 * it after that forward and BEFORE y4_yolo_loss_mask_output*_f32 multiplies the masks into `output`.  Two launches, no
 * host synchronisation; twelve doubles are ADDED to stats_row (device memory, caller-owned, zeroed by the caller):
 *    0 n_cells      B A F F
 *    1 n_pos        cells with a record (pos_index >= 0); one record per cell, class bits OR-ed, box of the last writer
 *    2 n_ign        cells with obj_mask == 0
 *    3 sum_iou      sum over positive cells of X = 1 - (box loss of kind Y4_BOX_IOU on the record), the operands and bits
 *                   of y4_yolo_box_loss_fwd with that kind, whatever box loss is configured; a NaN pred makes it NaN
 *    4 n_iou50      positive cells with X > 0.5 (a NaN X counts as no)      5 n_iou75: X > 0.75
 *    6 sum_obj_pos  sum of output[..., 4] over positive cells
 *    7 sum_obj_bg   sum of output[..., 4] over cells without a record and obj_mask != 0;     8 n_bg: their number
 *    9 sum_cls      sum over positive cells and the set class bits c of their record of output[..., 5 + c]
 *   10 n_cls        number of those bits
 *   11 n_top1       positive cells whose arg-max class channel (lowest index on ties) has its bit set
 * Counts are exact integers; the sums are fp64 sums of the fp32 values in a fixed order (block partials, then one fold).
 * Of opts only iou_thresh (the record slots) and obj_iou_ratio (the workspace size) are looked at.  `scratch`:
 * y4_yolo_loss_stats_scratch(B, F, A) bytes of device memory, overwritten.  Errors before any launch as above. */
size_t y4_yolo_loss_stats_scratch(int B, int F, int A);
int y4_yolo_loss_stats_f64(const float* output, const float* pred, const float* obj_mask, int B, int F, int A, int K,
                           int n_classes, const y4_loss_opts* opts, const void* workspace, size_t workspace_bytes,
                           void* scratch, size_t scratch_bytes, double* stats_row, void* stream);

/* Device-side prefix sums of postprocess (no host round trip between its stages):
 * y4_post_scan_i32: seg_offsets[0..n_segments] = exclusive scan of the candidate counts, clamped to `cap` (the capacity, in
 *   candidates, of the buffers the caller allocated: a too-small capacity truncates segments, it never overflows);
 *   info[0] = true total, info[1] = 1 if it exceeds cap (the caller then repeats the call sequence with cap >= info[0]).
 * y4_post_compact_f32: out_offsets = exclusive scan of `kept`; rows of every segment copied to out_rows back to back
 *   (class ascending, score descending inside an image, utils.py:200-221); img_offsets[b] = first output row of image b,
 *   img_offsets[B] = number of detections.  One device->host copy of img_offsets (+ info) is the call's only sync. */
int y4_post_scan_i32(const int* counts, int n_segments, long long cap, int* seg_offsets, int* info, void* stream);
int y4_post_compact_f32(const float* det_rows, const int* seg_offsets, const int* kept, int B, int n_classes,
                        float* out_rows, int* out_offsets, int* img_offsets, void* stream);
/* ---------------------------------------------------------------- post-processing
 * Replaces postprocess + nms, yolo/util/utils.py:32-89,92-223.
 * Stage 1: xywh->xyxy in place on prediction [B,N,5+C] and count candidates
 *          (obj*cls >= conf) per (image, class) into counts[B*C] (int32, zeroed inside).
 * Stage 2: (host gives exclusive offsets of counts) fill candidate keys, sort inside each
 *          (image, class) segment by (score desc, box index asc), greedy NMS (IoU >= thr
 *          suppresses), write kept rows [x1,y1,x2,y2,obj,cls_conf,cls] compacted per segment
 *          and kept[B*C] counts.
 */
int y4_post_count_f32(float* prediction, int B, long long N, int n_classes, float conf_thre,
                      int convert_xyxy, int* counts, void* stream);
size_t y4_post_nms_workspace(long long total_candidates, int n_segments);
int y4_post_nms_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre,
                    float nms_thre, const int* seg_offsets /* [B*C+1] device */, long long total_candidates,
                    float* det_rows /* [total,7] */, int* kept /* [B*C] */,
                    void* workspace, size_t workspace_bytes, void* stream);
/* ---------------------------------------------------------------- post-processing with options
 * The same stages with a selectable overlap measure, Soft-NMS, class-agnostic segments and a per-image cap.  With
 * {Y4_NMS_IOU, Y4_SOFT_NONE, agnostic 0, max_det 0} the _ex entries launch the kernels of the entries above.
 *
 * Candidates: box i, class c with s0 = obj_i * cls_ic (one fp32 product) >= conf_thre.  A segment is (image, class); with
 * agnostic = 1 it is the whole image.  Sort key: score descending, then index ascending; the index is the box i, for
 * agnostic segments i * C + c (lower box, then lower class), which needs N * C < 2^31 (else Y4_ERR_SHAPE).
 * Measure of candidate a against selected box o (areas (x2 - x1) * (y2 - y1); each step one fp32 operation, in this order):
 *   tl = max(a.xy1, o.xy1), br = min(a.xy2, o.xy2), en = tl < br on both axes ? 1 : 0,
 *   inter = ((br.x - tl.x) * (br.y - tl.y)) * en, iou = inter / ((area_a + area_o) - inter)                    [Y4_NMS_IOU]
 *   dx = ((a.x1 + a.x2) - (o.x1 + o.x2)) * 0.5, dy likewise, rho2 = dx * dx + dy * dy,
 *   ew = max(a.x2, o.x2) - min(a.x1, o.x1), eh likewise, c2 = ew * ew + eh * eh,
 *   diou = iou - (c2 == 0 ? 0 : rho2 / c2)                                                                      [Y4_NMS_DIOU]
 * Hard mode (Y4_SOFT_NONE): greedy in key order; a candidate is dropped when its measure against a kept box is
 *   >= nms_thre (a NaN measure keeps it); a segment stops after max_det survivors when max_det > 0.
 * Soft mode: W_j = 1, current score s0_j * W_j.  Repeat: select the remaining j with the largest current score (ties: key
 *   order); stop when none remains or the segment has emitted max_det rows (max_det > 0); emit it; for every remaining j
 *   ov = measure(j, selected) > 0 ? measure : 0;  Y4_SOFT_LINEAR: w = ov >= nms_thre ? 1 - ov : 1;
 *   Y4_SOFT_GAUSSIAN: w = expf(-(ov * ov) / sigma);  W_j = W_j * w;  j is removed when s0_j * W_j < conf_thre.
 *   Emitted rows are (x1, y1, x2, y2, obj, cls_conf * W, cls): row[4] * row[5] is the decayed score.
 * Not supported: the beta exponent of Darknet's DIoU-NMS (powf would give up the bit-exact restatement).
 *
 * y4_post_count_ex_f32: as y4_post_count_f32; agnostic = 1 counts per image into counts[B].
 * y4_post_nms_ex_f32: as y4_post_nms_f32 on B * C (agnostic: B) segments; one 256-thread block per segment, Soft-NMS state
 *   in LDS up to 2048 candidates and in the workspace above.  kept[] has one entry per segment.
 * y4_post_topk_compact_f32: y4_post_compact_f32 behind a per-image cap: of the kept rows of an image's segs_per_image
 *   segments the max_det (>= 1) with the highest row[4] * row[5] (fp32) stay (ties: lower class, then earlier place in the
 *   segment), in the usual output order.  total_candidates = the capacity the segment offsets were clamped to.
 * Errors before any launch: NULL pointer Y4_ERR_NULL; an unknown metric / soft kind, sigma <= 0 with Y4_SOFT_GAUSSIAN,
 * agnostic outside {0, 1}, max_det < 0 (top-k: < 1) or a bad shape Y4_ERR_SHAPE (workspace query: 0); workspace too small
 * Y4_ERR_WORKSPACE. */
#define Y4_NMS_IOU 0
#define Y4_NMS_DIOU 1
#define Y4_SOFT_NONE 0
#define Y4_SOFT_LINEAR 1
#define Y4_SOFT_GAUSSIAN 2
typedef struct y4_nms_opts {
    int metric;      /* Y4_NMS_*  */
    int soft;        /* Y4_SOFT_* */
    float sigma;     /* Gaussian decay; > 0 */
    int agnostic;    /* 0 | 1 */
    int max_det;     /* 0 = no cap */
    int reserved[3]; /* 0 */
} y4_nms_opts;       /* 32 bytes */
int y4_post_count_ex_f32(float* prediction, int B, long long N, int n_classes, float conf_thre,
                         int convert_xyxy, int agnostic, int* counts, void* stream);
size_t y4_post_nms_ex_workspace(long long total_candidates, int n_segments, const y4_nms_opts* opts);
int y4_post_nms_ex_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre, float nms_thre,
                       const y4_nms_opts* opts /* host */, const int* seg_offsets /* [segments+1] device */,
                       long long total_candidates, float* det_rows /* [total,7] */, int* kept /* [segments] */,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t y4_post_topk_workspace(long long total_candidates, int n_segments);
int y4_post_topk_compact_f32(const float* det_rows, const int* seg_offsets, const int* kept, int B, int segs_per_image,
                             int max_det, long long total_candidates, float* out_rows, int* out_offsets,
                             int* img_offsets, void* workspace, size_t workspace_bytes, void* stream);
/* ---------------------------------------------------------------- weighted box fusion
 * Solovyev et al.'s merge rule in place of suppression, on the same stages: y4_post_count_ex_f32, y4_post_scan_i32 before it,
 * y4_post_compact_f32 or y4_post_topk_compact_f32 behind it, the contract of y4_post_nms_ex_f32 (segments, keys, capacity).
 * One 256-thread block per segment walks its candidates in key order j = 0 .. n-1.  Candidate: score s_j = obj * cls (one
 * fp32 product), xyxy box x_j.  Cluster t: fused box F_t, sums Sx1 Sy1 Sx2 Sy2 S, count n_t, class.  For candidate j
 *   m_t = the Y4_NMS_IOU measure above with a = x_j and o = F_t (areas from the boxes) for every cluster;
 *   it matches t when m_t > iou_thre (strict; a NaN never matches); the cluster with the largest m_t takes it (ties: lowest t):
 *     Sx1 = Sx1 + s_j * x1_j (one product, one add; the other corners likewise), S = S + s_j, n_t += 1,
 *     F_t = (Sx1 / S, Sy1 / S, Sx2 / S, Sy2 / S);
 *   without a match it opens a cluster: sums from the same products, S = s_j, n_t = 1, F = x_j itself, class = its class
 *   (agnostic = 1: clusters of a whole image, whatever the classes of their later members).
 * Rows, in creation order: (F.x1, F.y1, F.x2, F.y2, 1.0, score, class) with mean = S / float(n_t),
 * f = float(min(n_t, n_views)) / float(n_views), score = mean * f: row[4] * row[5] is the fused score.
 * Scores do not decay, so a segment takes n sequential steps (an image-sized agnostic segment is slow); max_det acts only
 * through y4_post_topk_compact_f32.  Cluster state lives in LDS up to 1024 candidates per segment, in the workspace above.
 * Errors before any launch: NULL pointer Y4_ERR_NULL; n_views < 1, agnostic outside {0, 1}, an iou_thre that is not >= 0
 * (NaN included) or a bad shape Y4_ERR_SHAPE; workspace too small Y4_ERR_WORKSPACE. */
size_t y4_post_wbf_workspace(long long total_candidates, int n_segments);
int y4_post_wbf_f32(const float* prediction, int B, long long N, int n_classes, float conf_thre, float iou_thre, int agnostic,
                    int n_views, const int* seg_offsets /* [segments+1] device */, long long total_candidates,
                    float* det_rows /* [total,7] */, int* kept /* [segments] */, void* workspace, size_t workspace_bytes,
                    void* stream);
/* plain greedy NMS on one list (nms(), utils.py:32): boxes [R,4] xyxy, order given by
 * score desc / index asc; writes keep flags in sorted order and the sorted index list. */
size_t y4_nms_workspace(long long R);
int y4_nms_f32(const float* boxes, const float* scores /* may be NULL */, long long R, float thresh,
               int limit, int* keep_idx /* [R] */, int* n_keep /* [1] */,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- stand-alone forms of fused pieces
 * bboxes_iou (yolo/model/yololoss.py:16-91): pairwise IoU [Na,4] x [Nb,4] -> iou[Na*Nb] row-major; xyxy != 0:
 * corner boxes, else (xc, yc, w, h).  Same fp32 operation sequence as the reference (bit-exact on the CPU fixtures);
 * the target-assignment / ignore-mask kernels carry their own inlined copies. */
int y4_bboxes_iou_f32(const float* boxes_a, long long Na, const float* boxes_b, long long Nb, int xyxy, float* iou,
                      void* stream);
/* Mish.forward (darknet/darknet.py:14-20) and the other activations of ConvBNAct as a flat elementwise sweep over a
 * dense tensor of n floats (act = Y4_ACT_*); backward: dx = dy * act'(x).  Mish here keeps the denormal values of e^x
 * (x < -87.3), which the fused forms flush to zero; mish'(x) is exactly 1 for x > 20 (+inf included), NaN for NaN. */
int y4_act_fwd_f32(const float* x, float* y, long long n, int act, void* stream);
int y4_act_bwd_f32(const float* x, const float* dy, float* dx, long long n, int act, void* stream);
/* Upsample.forward (yolo/model/yolov4.py:82-90) for any target size, NHWC with pitches.  integer_factor = 0: the
 * train branch, F.interpolate(size=(Ho,Wo), mode='nearest'): src = min(floor(dst * (float)in/out), in-1);
 * integer_factor = 1: the eval branch (view/expand by Ho/H, Wo/W; Y4_ERR_SHAPE unless Ho % H == Wo % W == 0).
 * Backward sums each source pixel's destination block in a fixed order. */
int y4_upsample_nearest_fwd_f32(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int Ho, int Wo, int C,
                                int integer_factor, void* stream);
int y4_upsample_nearest_bwd_f32(const float* dy, int lddy, float* dx, int lddx, int B, int H, int W, int Ho, int Wo, int C,
                                int integer_factor, void* stream);

/* ---------------------------------------------------------------- optimizer ("next" row 1)
 * Fused Adam step over one dense parameter block; replaces torch.optim.Adam as the reference builds
 * it (yolo/optim/optimizers/adam.py:14-15: betas (0.9, 0.999), eps 1e-8; both param groups of
 * build.py:18-35 have weight_decay 0).  grad is multiplied by grad_scale first (1/accumulation). */
int y4_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     float grad_scale, void* stream);
/* Multi-tensor form: ONE launch steps every parameter of the model.  chunks_dev is a device table of 48-byte
 * records {float* p; const float* g; float* m; float* v; int64 n; int64 hyper_row} (Adam: m = exp_avg,
 * v = exp_avg_sq; SGD: m = momentum_buffer, v unused); a chunk is a contiguous run of one tensor (the host cuts
 * tensors into runs of 64 Ki elements).  hyper_host holds nhyper (<= 16) rows of 4 floats, one per distinct
 * (param group, step count): Adam {lr/bc1, 1/sqrt(bc2), weight_decay, 0} as y4_adam_hyper_f32 computes them in
 * double (the same values y4_adam_step_f32 uses, so both forms are bit-identical); SGD {lr, momentum,
 * weight_decay, first_step(0/1)} with torch.optim.SGD semantics (sgd.py:14-15: dampening 0, no nesterov). */
int y4_adam_hyper_f32(float lr, float beta1, float beta2, float weight_decay, int step, float* out4_host);
int y4_adam_multi_step_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                           float beta1, float beta2, float eps, float grad_scale, void* stream);
int y4_sgd_multi_step_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                          float grad_scale, void* stream);
/* Guarded steps: global grad-norm clipping (torch.nn.utils.clip_grad_norm_) and the skip of a step whose gradients
 * are not finite, decided on the device (no host sync; fixed-order sums, no float atomics: bit-identical run to run).
 * Guard record: 4 doubles in device memory {total_norm, coef, applied (1.0 / 0.0), skipped_total}; the caller zeroes
 * it once, skipped_total counts on.  Sequence per step, over the SAME chunk table as the step:
 *   y4_grad_sumsq_multi_f32: partials[c] = sum_i ((double)fl32(g_i * grad_scale))^2 for every chunk c (the value
 *     squared is the fp32 value the step kernels use; 16-byte loads when the chunk's g is 16-byte aligned, scalar
 *     otherwise; inf / NaN travel through the sums);
 *   y4_grad_guard_f32: total_norm = sqrt(sum of partials[0..nchunks)), applied = isfinite(total_norm),
 *     coef = (max_norm > 0 and finite) ? min(1, max_norm / (total_norm + 1e-6)) : 1, in double; coef = 1 when not
 *     applied; skipped_total += !applied;
 *   y4_{adam,sgd}_multi_step_guarded_f32: the multi-tensor step with grad_scale * (float)coef; writes nothing when
 *     applied == 0; with coef == 1 bit-identical to the unguarded entry points.  guard is required.
 * Errors before any launch: Y4_ERR_NULL for a NULL pointer, Y4_ERR_SHAPE for nchunks <= 0 or a table / partials /
 * guard pointer that is not 8-byte aligned. */
int y4_grad_sumsq_multi_f32(const void* chunks_dev, int nchunks, float grad_scale, double* partials /* [nchunks] */,
                            void* stream);
int y4_grad_guard_f32(const double* partials, int nchunks, double max_norm, double* guard, void* stream);
int y4_adam_multi_step_guarded_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                   float beta1, float beta2, float eps, float grad_scale, const double* guard,
                                   void* stream);
int y4_sgd_multi_step_guarded_f32(const void* chunks_dev, int nchunks, const float* hyper_host, int nhyper,
                                  float grad_scale, const double* guard, void* stream);
/* Exponential moving average of a list of tensors in one launch: e = e + one_minus_decay * (s - e) over the same
 * 48-byte records with p = EMA tensor e, g = live tensor s (m, v, hyper_row unused: 0).  With a guard record whose
 * applied == 0 nothing is written (the step it followed was skipped).  one_minus_decay outside [0, 1]: Y4_ERR_SHAPE. */
int y4_ema_multi_f32(const void* chunks_dev, int nchunks, float one_minus_decay, const double* guard /* nullable */,
                     void* stream);

/* ---------------------------------------------------------------- eval input pipeline ("next" row 4)
 * One image: src is uint8 HWC (3 channels, row pitch in bytes), as cv2.imread hands it to the reference.
 * Resizes to SxS with the arithmetic of cv2.resize INTER_LINEAR on 8-bit data (yolo/data/transform.py:173-174),
 * swaps B and R when swap_rb (transform.py:437), divides by 255 in fp32 and writes channel-planar
 * (transform.py:461): dst[c*dst_sc + y*dst_sh + x*dst_sw], strides in elements (NCHW or NHWC slot of a batch). */
int y4_preprocess_u8_f32(const void* src, int src_h, int src_w, long long src_pitch_bytes, int swap_rb,
                         float* dst, long long dst_sc, long long dst_sh, long long dst_sw, int S, void* stream);

/* Letterbox (aspect-preserving resize onto a padded canvas) for a whole batch in ONE launch.  One record per image: */
typedef struct y4_letterbox_src {
    const void* src;                /* device pointer, uint8 HWC, 3 channels */
    int h, w;                       /* 1 .. 65535 */
    long long pitch;                /* bytes, >= 3 * w */
    int swap_rb;                    /* 1: the source is BGR, the output RGB */
    int nh, nw;                     /* size the image is resized to, >= 1 */
    int top, left;                  /* where the resized image lies in the canvas: [top, top + nh) x [left, left + nw) */
    int reserved;                   /* 48 bytes */
} y4_letterbox_src;
/* The table is passed twice, as y4_aug_src is: *_dev is what the kernel reads, *_host the same bytes in host memory, checked
 * before anything is launched (the caller copies host -> device on the same stream; no synchronisation).
 * dst[b*dst_sb + c*dst_sc + oy*dst_sh + ox*dst_sw] (strides in elements) for oy < Hc, ox < Wc:
 *   inside the image's rectangle: what cv2.resize(src, (nw, nh)) gives at (oy - top, ox - left) -- the 8-bit INTER_LINEAR
 *     arithmetic of y4_preprocess_u8_f32 with scale_x = 1 / (nw / w), scale_y = 1 / (nh / h) formed in double, and the 2x2
 *     box average when w == 2 nw and h == 2 nh;
 *   outside: fill;
 *   then the B/R swap when swap_rb, and value / 255 in fp32 (the stored fill is (float)fill / 255.0f).
 * With nh = nw = Hc = Wc = S and top = left = 0 this is y4_preprocess_u8_f32, bit for bit.
 * Errors before any launch: Y4_ERR_NULL for a NULL pointer (a record's src included); Y4_ERR_SHAPE for B outside [1, 65535],
 * Hc or Wc outside [1, 65535], h or w outside [1, 65535], pitch < 3w, nh or nw < 1, a placement that does not fit the canvas
 * (top < 0, top + nh > Hc, the same in x), fill outside [0, 255]. */
int y4_letterbox_batch_u8_f32(const y4_letterbox_src* table_dev, const y4_letterbox_src* table_host, int B,
                              float* dst, long long dst_sb, long long dst_sc, long long dst_sh, long long dst_sw,
                              int Hc, int Wc, int fill, void* stream);

/* ---------------------------------------------------------------- training input pipeline
 * The reference's per-sample CPU augmentation (yolo/data/transform.py:385-427 _get_train_item: crop-and-pad with a mean
 * fill, flip, resize to SxS, HSV "colour dithering", 4-image mosaic) as two launches per BATCH.  The random draws are made
 * on the host; both entry points are deterministic functions of a descriptor table.
 *
 * One record per source image (uint8 HWC, 3 channels, row pitch in bytes; 1 <= h, w <= 65535): */
typedef struct y4_aug_src {
    const void* src;                /* device pointer */
    int h, w;
    long long pitch;                /* bytes, >= 3 * w */
    int swap_rb;                    /* 1: the source is BGR, the output RGB (transform.py:402) */
    int crop_left, crop_top;        /* origin of the crop rectangle in the source; negative = pad (mean fill) */
    int crop_w, crop_h;             /* >= 1; w - crop_left - crop_right, h - crop_top - crop_bottom */
    int flip;                       /* mirror the crop image in x */
    int color;                      /* apply the HSV step (when dhue, dsat, dexp are not the identity) */
    float dhue, dsat, dexp;         /* h += 179 * dhue, s *= dsat, v *= dexp; |dhue| <= 4, all finite */
    int win_x, win_y;               /* origin, in the resized SxS image, of the window the tile shows */
} y4_aug_src;
/* One record per output sample: n_src = 1 (the single source covers the output, cuts unused but still checked) or 4 (tiles
 * 0..3 = top-left, top-right, bottom-left, bottom-right of the cut point); its sources are table[first .. first + n_src). */
typedef struct y4_aug_sample {
    int cut_x, cut_y, n_src, first;
} y4_aug_sample;
/* Both tables are passed twice: *_dev is what the kernels read, *_host the same bytes in host memory, which the entry point
 * checks before it launches anything (the caller copies host -> device on the same stream; no synchronisation is needed).
 *
 * y4_augment_means_u8: sums_dev[i][k] = exact integer sum of channel k (memory order) of source i, by integer adds and
 *   integer atomics only (independent of the grid); < 2^40 for any accepted image.  sums_dev is zeroed by the call.
 * y4_augment_mosaic_u8_f32: dst[b*dst_sb + c*dst_sc + oy*dst_sh + ox*dst_sw] (strides in elements), per output pixel:
 *   1. tile q = (oy >= cut_y) * 2 + (ox >= cut_x) (0 when n_src == 1); position in that tile's resized image
 *      (ry, rx) = (oy - tile_y0 + win_y, ox - tile_x0 + win_x);
 *   2. bilinear taps in the crop image as OpenCV's floating linear resize takes them: f = (float)((r + 0.5) * scale - 0.5),
 *      scale = 1.0 / ((double)S / (double)crop_n); s = floor(f), fraction f - s in fp32; in x the fraction is zeroed and s
 *      clamped where s < 0 or s >= crop_w - 1; in y both rows are clamped and the fraction kept; fp32 weights 1 - f and f,
 *      horizontal pass first.  No fixed-point path, no rounding to 8 bits (the reference resizes a float64 image);
 *   3. each tap: cx = crop_w - 1 - sx when flip; source position (cy + crop_top, cx + crop_left); inside the source the
 *      uint8 channel (after the B/R swap), outside the channel's mean sum / (h * w), formed in double, not rounded to 8 bits;
 *   4. when color && (dsat != 1 || dexp != 1 || dhue != 0), on the 0..255 scale (OpenCV's float RGB2HSV / HSV2RGB):
 *      v = max, d = v - min, s = d / (|v| + FLT_EPSILON), k = 60 / (d + FLT_EPSILON); h = (g-b)k if v == r, else
 *      (b-r)k + 120 if v == g, else (r-g)k + 240; h += 360 if h < 0; then h += 179*dhue, s *= dsat (not clamped),
 *      v *= dexp; back: s == 0 -> r = g = b = v, else h /= 60 wrapped into [0, 6) by repeated +-6, i = floor(h), f = h - i,
 *      candidates v, v(1-s), v(1-sf), v(1-s(1-f)) in the usual sector order; result clipped to [0, 255].  Without the HSV
 *      step there is no clip;
 *   5. value / 255 in fp32.
 * Errors before any launch: Y4_ERR_NULL for a NULL pointer (a record's src included); Y4_ERR_SHAPE for B < 1, S < 1,
 * S or B > 65535, n_src not 1 or 4, first outside the table, h or w outside [1, 65535], pitch < 3w, crop_w or crop_h < 1,
 * crop offsets or sizes beyond 2^24, cuts outside [0, S], a window that does not fit (win + tile extent > S, win < 0),
 * |dhue| > 4 or a non-finite colour parameter. */
int y4_augment_means_u8(const y4_aug_src* table_dev, const y4_aug_src* table_host, int n_src,
                        unsigned long long* sums_dev /* [n_src][3] */, void* stream);
int y4_augment_mosaic_u8_f32(const y4_aug_src* table_dev, const y4_aug_src* table_host, int n_table,
                             const y4_aug_sample* samples_dev, const y4_aug_sample* samples_host, int B,
                             const unsigned long long* sums_dev, float* dst, long long dst_sb, long long dst_sc,
                             long long dst_sh, long long dst_sw, int S, void* stream);

/* ---------------------------------------------------------------- ImageNet classifier (backbone pre-training)
 * The four operations behind the backbone in CSPDarknet53 (darknet/darknet.py:164-193) and its training script
 * (darknet/main_amp.py:184 CrossEntropyLoss(label_smoothing=0.1), :549-562 accuracy).  fp32 throughout; outputs are
 * overwritten, never accumulated; every floating-point reduction runs in a fixed order (bit-identical run to run, no float
 * atomics); element k of a row lies at row * ld + k and columns >= the logical width are never written.
 *
 * nn.AdaptiveAvgPool2d((1, 1)): x is [B][HW] pixel rows of pitch ldx >= C, y is [B] rows of pitch ldy >= C;
 * y[b][c] = (sum_p x[b][p][c]) / HW; backward dx[b][p][c] = dy[b][c] / HW.  B <= 65535 in the forward call (a grid dimension). */
int y4_avgpool_global_fwd_f32(const float* x, int ldx, float* y, int ldy, int B, int HW, int C, void* stream);
int y4_avgpool_global_bwd_f32(const float* dy, int lddy, float* dx, int lddx, int B, int HW, int C, void* stream);
/* nn.Linear: y[m][n] = sum_k x[m][k] w[n][k] + bias[n]; w is dense [N][K] (the layout of nn.Linear.weight), bias may be
 * NULL.  fp32 products, fp32 accumulation in k order (no reduced-precision split).  Backward: dx = dy w [M][K] (pitch lddx),
 * dw = dy^T x [N][K] dense, dbias = sum_m dy; each output is skipped when NULL (all three NULL: Y4_ERR_NULL), x is only read
 * for dw and w only for dx.  No output is split over its reduction index, so there is nothing to combine.  M, K, N <= 65535 * 64. */
int y4_linear_fwd_f32(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int M, int K, int N,
                      void* stream);
int y4_linear_bwd_f32(const float* x, int ldx, const float* w, const float* dy, int lddy, float* dx, int lddx, float* dw,
                      float* dbias, int M, int K, int N, void* stream);
/* torch.nn.CrossEntropyLoss(label_smoothing = smoothing), ignore_index -100, mean reduction, on logits [B][N] (pitch ldl)
 * and int64 labels target[B]:  row_loss[b] = lse_b - (1 - smoothing) z_t - smoothing mean_j z_j  with a max-subtracted lse;
 * rows labelled -100 give 0 and are not counted.  loss_out (2 doubles) = {sum of the counted rows / their number, that
 * number}, reduced in double; the mean is NaN when nothing is counted, as in torch.  A label is only ever compared with the
 * column index, never used in an address: a label outside [0, N) other than -100 reads nothing out of bounds and makes its
 * row, and with it the mean, NaN.
 * Backward: dlogits[b][j] = gscale[0] / counted * (softmax_j - (1 - smoothing) [j == t] - smoothing / N), exactly 0 in
 * ignored rows; gscale is a device float (the upstream gradient), loss_out is what the forward call wrote (only the count
 * is read); the row statistics are recomputed from the logits. */
int y4_ce_smooth_fwd_f32(const float* logits, int ldl, const long long* target, int B, int N, double smoothing,
                         float* row_loss /* [B] */, double* loss_out /* [2] */, void* stream);
int y4_ce_smooth_bwd_f32(const float* logits, int ldl, const long long* target, const double* loss_out, const float* gscale,
                         float* dlogits, int lddl, int B, int N, double smoothing, void* stream);
/* accuracy(): rank_b = #{j: z_j > z_t} + #{j < t: z_j == z_t} (ties go to the lower index; torch leaves their order open),
 * rank_b = N for a row that holds a NaN or whose label is outside [0, N) (-100 included);
 * correct[i] = #{b: rank_b < ks_host[i]} for the nk (1..8) values of k (k > N is allowed); rank (int32 [B]) may be NULL. */
int y4_topk_correct_f32(const float* logits, int ldl, const long long* target, int B, int N, const int* ks_host, int nk,
                        int* correct /* [nk] */, int* rank /* [B] or NULL */, void* stream);

/* ---------------------------------------------------------------- COCO bbox evaluation
 * The COCOeval protocol the reference runs on the records of validate() (yolo/engine/build.py:172-188: evaluate,
 * accumulate; the summary is twelve means the caller takes on the host), as two launches.  T = 10 IoU thresholds, R = 101
 * recall thresholds, A = 4 area ranges, M = 3 maxDets; the threshold tables are the CALLER's fp64 arrays (device memory),
 * never recomputed here.  A cell is an (image, category) pair with at least one gt or one detection; cells are numbered
 * category-major, then by image.  Both calls read CSR offsets twice: *_dev is what the kernels read, *_host the same ints
 * in host memory, checked before anything is launched.
 *
 * y4_coco_match_f64: per cell, its detections (dbox rows [x, y, w, h], det_off[cell] .. det_off[cell + 1], already sorted by
 *   score descending and cut to the first 100: a row's position in its cell is its rank) against its gts (gbox rows, garea =
 *   the annotation's area field, gcrowd = iscrowd, in annotation order).  IoU in fp64 in this order, no fused multiply-add:
 *     w = min(dx+dw, gx+gw) - max(dx, gx); h likewise; w <= 0 or h <= 0 -> 0; i = w*h;
 *     u = crowd ? dw*dh : dw*dh + gw*gh - i; iou = i/u.
 *   For every threshold t and area range a (area_rng[a] = {lo, hi}; a gt is ignored when crowd or garea < lo or > hi) the
 *   detections are visited in rank order, each starting from best = min(iou_thrs[t], 1 - 1e-10): first the gts that are not
 *   ignored and not yet matched at (t, a), in order, taking a gt unless iou < best (ties go to the later gt); only if that
 *   found nothing, the ignored gts the same way, where a crowd gt may be taken any number of times.
 *   codes[a][d] (d = row of dbox, n_det words per a) holds ten 2-bit codes, threshold t in bits 2t, 2t+1:
 *     0 unmatched (false positive), 1 matched to a counted gt, 2 unmatched with dw*dh outside area_rng[a] (ignored),
 *     3 matched to an ignored gt (ignored).
 *   npig[cell][a] = number of gts of the cell that are not ignored in a.  A cell of more than 256 gts keeps its "matched"
 *   bits in `workspace` (y4_coco_workspace(n_cells, longest gt segment) bytes; 0 and NULL allowed below that).
 *   Errors before any launch: a NULL pointer Y4_ERR_NULL; n_det, n_gt or n_cells < 0, offsets that do not start at 0, decrease,
 *   end elsewhere than n_det / n_gt, or a cell of more than 100 detections Y4_ERR_SHAPE; workspace too small Y4_ERR_WORKSPACE.
 *
 * y4_coco_accumulate_f64: order[cat_off[k] .. cat_off[k + 1]) lists category k's rows of dbox by score descending (ties: by
 *   row), rank[d] is row d's rank in its cell, npig_cat[k][a] the sum of npig over k's cells.  For every (k, a, m, t), over
 *   the listed rows with rank < max_dets[m], with integer running counts tp (code 1) and fp (code 0):
 *     rc[i] = tp[i] / npig, pr[i] = tp[i] / (fp[i] + tp[i] + 2^-52), pr made non-increasing from the right,
 *     precision[t][r][k][a][m] = pr[first i with rc[i] >= rec_thrs[r]] or 0, recall[t][k][a][m] = rc[last] or 0 without rows;
 *   npig_cat[k][a] == 0 gives -1 everywhere.  Every entry of both arrays is written; each is one fp64 quotient of integers,
 *   so nothing depends on the grid.  No floating-point atomics.
 *   Errors before any launch: NULL pointer Y4_ERR_NULL; n_det or n_cat < 0, a negative max_dets entry, offsets as above
 *   Y4_ERR_SHAPE. */
size_t y4_coco_workspace(int n_cells, int max_gts_per_cell);
int y4_coco_match_f64(const double* dbox /* [n_det][4] */, const int* det_off_dev, const int* det_off_host /* [n_cells+1] */,
                      int n_det, const double* gbox /* [n_gt][4] */, const double* garea, const int* gcrowd,
                      const int* gt_off_dev, const int* gt_off_host /* [n_cells+1] */, int n_gt, int n_cells,
                      const double* iou_thrs /* [10] */, const double* area_rng /* [4][2] */,
                      unsigned int* codes /* [4][n_det] */, int* npig /* [n_cells][4] */, void* workspace,
                      size_t workspace_bytes, void* stream);
int y4_coco_accumulate_f64(const unsigned int* codes, const unsigned char* rank /* [n_det] */, const int* order /* [n_det] */,
                           int n_det, const int* cat_off_dev, const int* cat_off_host /* [n_cat+1] */,
                           const long long* npig_cat /* [n_cat][4] */, int n_cat, const double* rec_thrs /* [101] */,
                           const int* max_dets_host /* [3] */, double* precision /* [10][101][n_cat][4][3] */,
                           double* recall /* [10][n_cat][4][3] */, void* stream);

/* ---------------------------------------------------------------- JPEG decoding (what cv2.imread does for the reference's
 * yolo/data/cocodataset.py:97), split in two: the serial Huffman stage on the host, everything per pixel on the device.
 *
 * Supported: Huffman sequential JPEG (SOF0 / SOF1), 8-bit, ONE interleaved scan, 1 component or 3 YCbCr components at 4:4:4,
 * 4:2:2 (h2v1) or 4:2:0 (h2v2); any number of DQT / DHT segments, 8- or 16-bit quantisation tables, DRI / RSTn; APPn and COM
 * are skipped, 0xFF fill bytes before markers accepted.  Y4_ERR_UNSUPPORTED: a valid JPEG outside that subset (progressive,
 * arithmetic, lossless, 12-bit, 4 components, other sampling, several scans, RGB-coded components).  Y4_ERR_FORMAT: truncated
 * data, a segment length past the end, missing tables, a Huffman code that is not in its table, a zero run past coefficient
 * 63, a coefficient outside int16, a zero dimension, a wrong RSTn sequence.
 *
 * Host stage (no GPU, no threads, no global state; every read checked against nbytes, every write against coef_cap): */
typedef struct y4_jpeg_info {
    int width, height;              /* as stored, before the orientation is applied */
    int ncomp;                      /* 1 or 3 */
    int hs[3], vs[3];               /* sampling factors (one component: 1, 1; absent components: 0) */
    int mcus_x, mcus_y;             /* MCU grid: ceil(width / (8 hs[0])) x ceil(height / (8 vs[0])) */
    int blocks_w[3], blocks_h[3];   /* padded block grid of each component: mcus_x * hs[c], mcus_y * vs[c] */
    int restart_interval;           /* MCUs between RSTn markers, 0: none */
    int orientation;                /* EXIF tag 0x0112, 1..8; 1 when absent or unreadable */
    int reserved;
    long long coef_count;           /* int16 elements of the coefficient buffer: 64 * sum_c blocks_w[c] * blocks_h[c] */
} y4_jpeg_info;
/* y4_jpeg_parse_host fills the record.  y4_jpeg_entropy_host writes the QUANTISED coefficients (not dequantised), in natural
 * (row-major, de-zigzagged) order, 64 int16 per block, component after component, each component's blocks in raster order
 * over its padded grid; and qt_host[c] = component c's quantisation table in natural order (zeros for absent components).
 * Y4_ERR_WORKSPACE when coef_cap < info->coef_count, Y4_ERR_SHAPE when the record does not belong to the data. */
int y4_jpeg_parse_host(const void* data_host, size_t nbytes, y4_jpeg_info* info_host);
int y4_jpeg_entropy_host(const void* data_host, size_t nbytes, const y4_jpeg_info* info_host, short* coef_host,
                         long long coef_cap, unsigned short* qt_host /* [3][64] */);

/* Device stage: one call per BATCH, two launches over all jobs (IDCT into the component planes; upsample, colour-convert,
 * store).  One record per image: */
typedef struct y4_jpeg_job {
    const short* coef;              /* device, 16-byte aligned, info.coef_count elements as the host stage wrote them */
    void* out;                      /* device, uint8 HWC, 3 channels */
    long long out_pitch;            /* bytes per output row, >= 3 * output width */
    long long ws_offset;            /* bytes, multiple of 16: this job's info.coef_count bytes of the workspace (the planes) */
    y4_jpeg_info info;
    int apply_orientation;          /* 1: store through the EXIF index map; output is height x width swapped for 5..8 */
    int swap_rb;                    /* 0: B, G, R in memory (cv2.imread); 1: R, G, B */
    unsigned short qt[3][64];
} y4_jpeg_job;
/* The table is passed twice, like the augmentation tables: jobs_dev is what the kernels read, jobs_host the same bytes in
 * host memory, checked before anything is launched (the caller copies host -> device on the same stream).
 * y4_jpeg_workspace: bytes of planes for these images, packed in order with each job rounded up to 16 bytes.
 *
 * The arithmetic is libjpeg-turbo's default decompression path, bit for bit:
 *   1. dequantise (coefficient * table entry, int32) and the "islow" integer IDCT of jidctint: CONST_BITS 13, PASS1_BITS 2,
 *      constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172; columns first, descaled by 11, then rows,
 *      descaled by 18 (descale by n: add 1 << (n-1), arithmetic shift right by n); add 128, clamp to 0..255;
 *      sums and products wrap modulo 2^32 (a forged file can make them; libjpeg gives arbitrary pixels there too);
 *   2. a chroma plane has dw x dh = ceil(width hs[c] / hs[0]) x ceil(height vs[c] / vs[0]) samples; indices beyond it take
 *      the last real sample, never the IDCT padding;
 *      h2v1 "fancy": out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2;
 *      h2v2 "fancy": cs[j] = 3 row[j] + neighbour[j], the neighbour being the row above for the upper output row and the row
 *      below for the lower one; out[2j] = (3 cs[j] + cs[j-1] + 8) >> 4, out[2j+1] = (3 cs[j] + cs[j+1] + 7) >> 4
 *      (with the edge replication this gives the copies / the 4 cs forms at the first and last output);
 *      dw <= 2: plain replication in both directions instead;
 *   3. cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *      G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), each clamped to 0..255; one component: R = G = B = Y;
 *   4. the pixel of stored position (x, y) goes to (x', y') of the output: orientation 1 (x, y), 2 (W-1-x, y),
 *      3 (W-1-x, H-1-y), 4 (x, H-1-y), 5 (y, x), 6 (H-1-y, x), 7 (H-1-y, W-1-x), 8 (y, W-1-x); without apply_orientation
 *      always (x, y).  Bytes between 3 * output width and out_pitch are never written.
 * Errors before any launch: NULL pointer (a job's coef or out included) Y4_ERR_NULL; n_jobs outside [1, 65535], a record
 * whose geometry is not what y4_jpeg_parse_host gives for its width, height and sampling, a misaligned coef or ws_offset, a
 * pitch below 3 * output width or an orientation outside 1..8 Y4_ERR_SHAPE; ws_offset + coef_count beyond workspace_bytes
 * Y4_ERR_WORKSPACE. */
size_t y4_jpeg_workspace(const y4_jpeg_info* infos_host, int n);
int y4_jpeg_decode_u8(const y4_jpeg_job* jobs_dev, const y4_jpeg_job* jobs_host, int n_jobs, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- JPEG encoding (what cv2.imwrite does for the reference's
 * detect.py), the decoder's mirror image: everything per pixel on the device, the serial Huffman stage on the host.
 * Baseline (SOF0), 8-bit, one interleaved scan, 1 component or YCbCr at 4:4:4 / 4:2:2 (h2v1) / 4:2:0, the standard Annex K
 * Huffman tables, JFIF APP0; no optimised tables, restart markers, progression or EXIF.
 *
 * y4_jpeg_encode_setup (host): the record y4_jpeg_parse_host would give for such a file (orientation 1, no restarts) and
 * qt_host[c] = component c's table in natural order at `quality` 1..100 (zeros for absent components): the Annex K base
 * tables scaled by s = 5000 / quality below 50, else 200 - 2 quality; entry = clamp((base s + 50) / 100, 1, 255).
 * Y4_ERR_SHAPE: a size outside 1..65535, ncomp not 1 or 3, sampling not 1x1 / 2x1 / 2x2 (gray: 1x1), quality outside 1..100. */
int y4_jpeg_encode_setup(int width, int height, int ncomp, int hs, int vs, int quality, y4_jpeg_info* info_host,
                         unsigned short* qt_host /* [3][64] */);

/* Device stage: one call per BATCH, ONE launch over all jobs, images of any sizes and samplings mixed.  One record per image: */
typedef struct y4_jpeg_enc_job {
    const void* pixels;             /* device, uint8: HWC with 3 channels (info.ncomp 3) or HW (info.ncomp 1) */
    short* coef;                    /* device, 16-byte aligned, info.coef_count elements */
    long long pitch;                /* bytes per pixel row, >= 3 * width (1 * width for one component) */
    y4_jpeg_info info;
    int swap_rb;                    /* 0: B, G, R in memory (what y4_jpeg_decode_u8 writes); 1: R, G, B */
    int reserved[3];
    unsigned short qt[3][64];       /* natural order, entries 1..255, qt[1] == qt[2] */
} y4_jpeg_enc_job;
/* Writes the QUANTISED coefficients in exactly the layout y4_jpeg_entropy_host writes.  Dummy blocks -- grid positions of a
 * component beyond ceil(ceil(width hs[c] / hs[0]) / 8) columns or ceil(ceil(height vs[c] / vs[0]) / 8) rows, inside the last
 * MCU column or row (the luma of subsampled images) -- are never written.  The table is passed twice like the decoder's.
 *
 * The arithmetic is libjpeg-turbo's default compression path, bit for bit, all in int32:
 *   1. Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *      Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16; one component: the byte itself;
 *   2. pixel rows are replicated to a multiple of vs[0], pixel columns to the width of the component's real blocks; then
 *      h2v2: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along the output row; h2v1: (a + b + bias) >> 1 with bias
 *      0, 1, 0, 1, ...; then the last DOWNSAMPLED row is replicated down to the MCU height (not the same as replicating
 *      pixel rows further: an even height averages its last two rows);
 *   3. subtract 128; the "islow" integer FDCT of jfdctint (CONST_BITS 13, PASS1_BITS 2, the IDCT's twelve constants): rows
 *      first (outputs 0 and 4 shifted left by 2, the others descaled by 11), then columns (0 and 4 descaled by 2, the others
 *      by 15);
 *   4. d = 8 * table entry, a = |c| + (d >> 1): the result is a / d when a >= d, else 0, with the sign of c.
 * Errors before any launch: NULL pointer (a job's pixels or coef included) Y4_ERR_NULL; n_jobs outside [1, 65535], a record
 * that is not what y4_jpeg_encode_setup gives, a table entry outside 1..255 or differing chroma tables, a misaligned coef or
 * table, a pitch below the row Y4_ERR_SHAPE. */
int y4_jpeg_encode_u8(const y4_jpeg_enc_job* jobs_dev, const y4_jpeg_enc_job* jobs_host, int n_jobs, void* stream);

/* Host stage (no GPU, no threads, no global state; every write checked against out_cap).  y4_jpeg_encode_host writes the file:
 * SOI; APP0 "JFIF" 1.1, no units, density 1 x 1; one DQT per table (ids 0, 1; 8-bit; zigzag); SOF0 with components 1 / 2 / 3,
 * luma hs * 16 + vs on table 0, chroma 0x11 on table 1; DHT DC0, AC0, DC1, AC1 (the Annex K tables); SOS; the MCU-interleaved
 * scan (DC differences per component, ZRL, EOB, FF stuffed with 00, the last byte padded with one-bits); EOI.  One component:
 * one DQT, two DHT.  A dummy block is coded as (DC of the block coded just before it in the same MCU, AC zero) and the
 * buffer is never read there.  y4_jpeg_encode_bound: a size that always suffices, 1024 + 416 per block (0 for a bad record).
 * Y4_ERR_WORKSPACE when the file does not fit out_cap (out_bytes is then 0), Y4_ERR_SHAPE for a bad record or table,
 * Y4_ERR_FORMAT for a coefficient the standard tables cannot code (a DC difference beyond 11 bits, an AC value beyond 10;
 * the device stage never makes one). */
size_t y4_jpeg_encode_bound(const y4_jpeg_info* info_host);
int y4_jpeg_encode_host(const short* coef_host, const y4_jpeg_info* info_host, const unsigned short* qt_host /* [3][64] */,
                        void* out_host, size_t out_cap, size_t* out_bytes);

/* ---------------------------------------------------------------- Box overlay (what detect.py's vis_bbox does with cv2):
 * frames, label plates and label text drawn in place on uint8 HWC images, ONE launch per batch.  A gather: every pixel walks
 * its image's records in order and takes the colour of the LAST record that covers it (painter's order), so overlapping
 * boxes are deterministic, nothing races and clipping to the image is free.  The host prepares the records in integer pixels: */
typedef struct y4_draw_box {
    int x1, y1, x2, y2;             /* frame rectangle (inclusive corners) */
    int half;                       /* line_width / 2: the frame is [x1-half, x2+half] x [y1-half, y2+half] without the
                                       pixels that satisfy x1+half < x < x2-half and y1+half < y < y2-half */
    int px1, py1, px2, py2;         /* label plate, inclusive corners, filled in the box colour; px2 < px1: none */
    int tx, ty;                     /* top-left pixel of the first glyph cell */
    int scale;                      /* glyph scale >= 1: a cell is 6 scale x 8 scale pixels, the glyph its top-left 5 x 7 */
    int text_off, text_len;         /* this label's glyph indices in the job's text array */
    unsigned char color[4];         /* B, G, R in memory order, then padding; the text is white */
    int reserved;
} y4_draw_box;
typedef struct y4_draw_job {
    void* image;                    /* device, uint8 HWC, 3 channels */
    long long pitch;                /* bytes per row, >= 3 * width; bytes beyond 3 * width are never touched */
    int width, height;
    const y4_draw_box* boxes;       /* device, n_boxes records */
    const y4_draw_box* boxes_host;  /* the same records in host memory: checked before the launch, not read by the kernel */
    const unsigned char* text;      /* device, text_bytes glyph indices */
    const unsigned char* glyphs;    /* device, n_glyphs x 8 bytes: rows 0..6 of a glyph, bit 4 the leftmost pixel */
    int n_boxes, text_bytes, n_glyphs, reserved;
} y4_draw_job;
/* A glyph index >= n_glyphs renders as a solid cell.  Errors before the launch: NULL pointer Y4_ERR_NULL (boxes, boxes_host
 * only when n_boxes > 0; text only when text_bytes > 0; glyphs only when n_glyphs > 0); n_images outside [1, 65535], a size
 * below 1, a pitch below 3 * width, a negative count, half < 0, scale < 1 or a text range outside [0, text_bytes] Y4_ERR_SHAPE. */
int y4_draw_boxes_u8(const y4_draw_job* jobs_dev, const y4_draw_job* jobs_host, int n_images, void* stream);

/* ---------------------------------------------------------------- ImageNet input pipeline (what torchvision and Pillow do for
 * the reference's darknet/main_amp.py:205-332): per sample crop -> Pillow's antialiased bilinear resample of the crop to
 * res_h x res_w -> an S x S window of that image -> horizontal flip -> CutMix paste -> (float(u8) - mean[c]) / std[c] into
 * fp32 planes, ONE gather launch per batch behind one small launch that builds the coefficient tables.  No crop image, no
 * resized image and no uint8 batch exists anywhere.  One record per output sample (96 bytes): */
typedef struct y4_rcrop_job {
    const void* src;                /* device, uint8 [src_h, src_w, 3] (what y4_jpeg_decode_u8 writes) */
    long long src_pitch;            /* bytes per source row, >= 3 * src_w; any alignment */
    int src_h, src_w;
    int swap_rb;                    /* 0: output channel c is memory channel c; 1: memory channel 2 - c (BGR source -> RGB) */
    int crop_x, crop_y, crop_w, crop_h;   /* the crop, inside the source; taps never leave it */
    int res_w, res_h;               /* size the crop is resampled to */
    int win_x, win_y;               /* origin of the S x S window in the resampled image */
    int flip;                       /* 1: output column ox shows window column S - 1 - ox */
    int paste_from;                 /* -1, or the sample of this batch whose pixels fill the rectangle below */
    int paste_x0, paste_y0, paste_x1, paste_y1;   /* output coordinates, x0 <= x < x1, y0 <= y < y1; may be empty */
    long long ws_offset;            /* bytes, multiple of 16: this job's tables in the workspace (4 bytes of padding before) */
} y4_rcrop_job;
/* The arithmetic is Pillow's Image.crop(box).resize((res_w, res_h), Image.BILINEAR) for 8-bit RGB, bit for bit.  Per axis,
 * with `in` the crop's size and `out` the resampled size, in IEEE double without fused multiply-add:
 *   scale = (double)in / out; fs = max(scale, 1.0); support = fs; ksize = (int)ceil(support) * 2 + 1; ss = 1.0 / fs;
 *   for resampled index xx: center = (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0);
 *   n = min((int)(center + support + 0.5), in) - xmin (both casts truncate);
 *   w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|) for x < n, summed in index order into ww, each divided by ww when
 *   ww != 0; k[x] = (int)(0.5 + w[x] * 4194304.0).
 * The horizontal pass runs first over the crop's rows: clip((2^21 + sum px * k) >> 22, 0, 255) in int32, kept as 8 bits; the
 * vertical pass applies the same formula to those values.  An axis whose size does not change has taps {2^22, 0}: the
 * identity, as Pillow's skipped pass.  The last step is the correctly rounded fp32 (float(u8) - mean[c]) / std[c] with c the
 * OUTPUT channel (no reciprocal).
 * CutMix: a pixel (oy, ox) with paste_from >= 0 inside the rectangle is computed from job paste_from's record and tables at
 * the same (oy, ox) -- with that job's flip, without that job's own paste -- so the result is plain[paste_from][:, oy, ox],
 * plain being the batch without pastes.
 *
 * Workspace: per job, at ws_offset, two int32 tables, the x axis first: bounds[S][2] = (xmin, n) of window index i (resampled
 * index win + i), then k[S][ksize] with the taps beyond n zero; ksize by the formula above from (crop_w, res_w) or (crop_h,
 * res_h).  A job takes 4 * (S * (2 + ksize_x) + S * (2 + ksize_y)) bytes rounded up to 16; y4_rcrop_workspace is the sum over
 * the jobs in order (0 for a NULL table, n < 1, S outside [1, 65535] or a crop / resampled size below 1 or a crop above 65535).
 * y4_rcrop_coeffs_i32 fills the tables only; y4_rcrop_u8_f32 fills them and gathers (two launches).  Device pointers, no
 * allocation, no synchronisation; the table is passed twice like the augmentation tables (jobs_dev is what the kernels read,
 * jobs_host the same bytes in host memory).  dst is addressed as b * dst_sb + c * dst_sc + y * dst_sh + x * dst_sw (elements):
 * every element of the [n, 3, S, S] destination is overwritten, nothing else is written.
 * Errors before any launch: NULL pointer (a job's src included) Y4_ERR_NULL; n outside [1, 65535], S outside [1, 65535], a
 * source side outside [1, 65535], a pitch below 3 * src_w, an empty crop or one outside the source, res_w or res_h outside
 * [1, 65535], a window outside the resampled image, paste_from outside [-1, n), with paste_from >= 0 a rectangle that is not
 * 0 <= x0 <= x1 <= S and 0 <= y0 <= y1 <= S, a negative or misaligned ws_offset, a std[c] that is zero or a mean / std that
 * is not finite Y4_ERR_SHAPE; ws_offset + the job's bytes beyond ws_bytes Y4_ERR_WORKSPACE. */
size_t y4_rcrop_workspace(const y4_rcrop_job* jobs_host, int n, int S);
int y4_rcrop_coeffs_i32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, void* workspace,
                        size_t ws_bytes, void* stream);
int y4_rcrop_u8_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, const float* mean3_host,
                    const float* std3_host, float* dst, long long dst_sb, long long dst_sc, long long dst_sh, long long dst_sw,
                    void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- RandAugment (what torchvision's RandAugment(num_ops,
 * magnitude, num_magnitude_bins, interpolation=NEAREST, fill=None) asks of Pillow in the reference's darknet/main_amp.py:
 * 221-227), on the uint8 RGB S x S crops between the gather above and its normalisation.  The host draws the operations and
 * turns each magnitude into integers and one float; the device sees only those.  One record per sample and round (40 bytes): */
#define Y4_RA_IDENTITY 0
#define Y4_RA_SHEAR_X 1         /* codes 1..5 are one operation on the device: the gather through a[0..5] */
#define Y4_RA_SHEAR_Y 2
#define Y4_RA_TRANSLATE_X 3
#define Y4_RA_TRANSLATE_Y 4
#define Y4_RA_ROTATE 5
#define Y4_RA_BRIGHTNESS 6
#define Y4_RA_COLOR 7
#define Y4_RA_CONTRAST 8
#define Y4_RA_SHARPNESS 9
#define Y4_RA_POSTERIZE 10
#define Y4_RA_SOLARIZE 11
#define Y4_RA_AUTOCONTRAST 12
#define Y4_RA_EQUALIZE 13
typedef struct y4_randaug_op {
    int op;                         /* Y4_RA_* */
    int a[6];                       /* codes 1..5: the inverse affine matrix in 16.16 fixed point, see below */
    float factor;                   /* codes 6..9: ImageEnhance's factor 1 + m, rounded to fp32 */
    int bits;                       /* Y4_RA_POSTERIZE: bits kept, 0..8 */
    int threshold;                  /* Y4_RA_SOLARIZE: ceil of Pillow's threshold; pixels >= it are inverted */
} y4_randaug_op;
/* The arithmetic is Pillow 12's for 8-bit RGB, bit for bit.  px is a channel of the pixel, P = S * S.
 *   codes 1..5  libImaging's affine_fixed: output (x, y) shows input ((a[2] + a[1] y + a[0] x) >> 16, (a[5] + a[4] y + a[3] x)
 *               >> 16) where that lies inside the image and black elsewhere (sums in 64 bits).  The host forms the inverse
 *               matrix m0..m5 in double (torchvision's _get_inverse_affine_matrix for the shears and translations, Image.rotate's
 *               for the rotation) and a[i] = FIX(m[i]) for i = 0, 1, 3, 4, a[2] = FIX(m2 + m0 / 2 + m1 / 2), a[5] = FIX(m5 +
 *               m3 / 2 + m4 / 2), FIX(v) = v * 65536 + 0.5 truncated, floored when negative.
 *   codes 6..9  ImagingBlend in fp32 without fused multiply-add: t = deg + factor * (px - deg); 0 <= factor <= 1: (uint8)t;
 *               else t <= 0 -> 0, t >= 255 -> 255, else (uint8)t.  deg is 0 (Brightness); L = (19595 R + 38470 G + 7471 B +
 *               32768) >> 16 of the pixel (Color); (int)(sum of L over the image / P + 0.5), the sum exact, the division in
 *               double (Contrast); ImageFilter.SMOOTH of the image (Sharpness): on the one-pixel frame the pixel itself, inside
 *               ss = 0.5 + row(y + 1) + row(y) + row(y - 1) added in that order, row(r) = (px[r][x - 1] k + px[r][x] c) +
 *               px[r][x + 1] k with k = 1.0f / 13.0f and c = 5.0f / 13.0f on row y, k elsewhere, clipped like t.
 *   code 10     px & ~(2^(8 - bits) - 1).        code 11: px < threshold ? px : 255 - px.
 *   code 12     per channel, lo / hi the first / last occupied histogram bin: the identity when hi <= lo, else scale = 255.0 /
 *               (hi - lo), offset = -lo * scale, lut[i] = clip((int)(i * scale + offset), 0, 255) in unfused double.
 *   code 13     per channel with histogram h: the identity when at most one bin is occupied or step = (P - h[hi]) / 255 is 0
 *               (integer division), else lut[i] = min((step / 2 + h[0] + .. + h[i - 1]) / step, 255).
 *
 * y4_rcrop_randaug_u8_f32 is y4_rcrop_u8_f32 with the operations in between.  With plain[b] the uint8 RGB S x S image the
 * gather produces for job b (window, channel order, flip; no paste) and aug[b] that image after ops[b][0], .., ops[b][n_ops - 1]
 * in order, output pixel (b, oy, ox) is aug[paste_from] inside job b's paste rectangle and aug[b] outside it, normalised and
 * stored exactly as y4_rcrop_u8_f32 does.  The table ops[n][n_ops] is passed twice like the job table.  n_ops = 0: the two
 * launches and the bits of y4_rcrop_u8_f32; the op table and the second workspace are not looked at and may be NULL.
 * Otherwise: the coefficient launch; the gather, into a uint8 batch [n][S][S][3]; per round at most two launches over the
 * whole batch -- per-sample 3 x 256 histograms and the sum of L by integer atomics (order independent; only in a round where
 * the host sees a code 8, 12 or 13), then the operation, from one uint8 batch into the other (never in place: codes 1..5 and
 * 9 read neighbours).  The last round evaluates "the operation of sample j at pixel p" for j = b or j = paste_from and writes
 * the normalised fp32 result; no final uint8 batch exists.  2 + 2 n_ops launches at most, no allocation, no synchronisation.
 * workspace2 (16-byte aligned) holds the two uint8 batches, each n * S * S * 3 bytes rounded up to 256, and the statistics,
 * n * n_ops * 772 int32 (3 x 256 counts, the sum of L, three words of padding): y4_randaug_workspace, 0 for n outside
 * [1, 65535], S outside [1, 4096] or n_ops outside [1, 8].
 * Errors before any launch: everything y4_rcrop_u8_f32 reports; n_ops outside [0, 8] Y4_ERR_SHAPE; with n_ops > 0: a NULL op
 * table or workspace2 Y4_ERR_NULL, S > 4096 (above it 16.16 coordinates and the 32-bit sum of L, at most 255 * 4096^2, leave
 * their range), a workspace2 that is not 16-byte aligned, a code outside 0..13, bits outside [0, 8] in a code 10 record or a
 * factor that is not finite Y4_ERR_SHAPE; ws2_bytes < y4_randaug_workspace(n, S, n_ops) Y4_ERR_WORKSPACE. */
size_t y4_randaug_workspace(int n, int S, int n_ops);
int y4_rcrop_randaug_u8_f32(const y4_rcrop_job* jobs_dev, const y4_rcrop_job* jobs_host, int n, int S, const float* mean3_host,
                            const float* std3_host, float* dst, long long dst_sb, long long dst_sc, long long dst_sh,
                            long long dst_sw, void* workspace, size_t ws_bytes, const y4_randaug_op* ops_dev,
                            const y4_randaug_op* ops_host, int n_ops, void* workspace2, size_t ws2_bytes, void* stream);

/* ---- anchor fitting on label shapes (csrc/anchors.hip) ------------------------------------------
 * The shape IoU of a label shape (tw, th) and an anchor (aw, ah) is the loss's (y4_yolo_loss_fwd_ex_f32's assignment), in
 * fp32, unfused, with IEEE division:
 *     brx = fminf(tw, aw); bry = fminf(th, ah); ai = brx * bry; iou = ai / ((tw * th + aw * ah) - ai)
 * The best anchor of a shape is the arg-max over the A anchors, lowest index on ties.  Shapes and anchors are finite with
 * 0 < w, h < 65536 (the caller's duty: device data is not looked at on the host, and there is no NaN branch).
 * Every sum is an int64 sum of fixed-point values: qw = rint(double(w) * 2^16), qh likewise, qiou = rint(double(iou) * 2^30);
 * the results are the same bytes for every grid and on every run.
 *
 * y4_anchor_assign_f32: one Lloyd assignment pass of wh [N][2] against anchors [A][2] (both on the device).
 *   assign [N] (may be NULL) the best anchor; best_iou [N] (may be NULL) its IoU; acc [A][5] is zeroed by the call and
 *   receives per anchor: the number of shapes it is best for, their sum of qw, of qh, of qiou (of the best IoU), and `hits`,
 *   the number of shapes for which the anchor is the best one or has iou > iou_thresh (strict): the positives the loss's
 *   iou_thresh rule creates.  With iou_thresh = 1, hits == count.
 * y4_anchor_fitness_f32: G candidate anchor sets cand [G][A][2] scored against the same shapes in one launch.  out [G][2]
 *   is zeroed by the call and receives per candidate: the sum over the shapes of the best anchor's qiou, and the number of
 *   shapes whose best IoU is > thr (strict).
 * One memset node and one launch each, no allocation, no synchronisation.
 * Errors before any launch (nothing is written): a NULL wh, anchors / cand or acc / out Y4_ERR_NULL; N outside [1, 2^24],
 * A outside [1, 32], G outside [1, 65535], or one of those three pointers not 8-byte aligned Y4_ERR_SHAPE. */
int y4_anchor_assign_f32(const float* wh, int N, const float* anchors, int A, float iou_thresh, unsigned char* assign,
                         float* best_iou, long long* acc, void* stream);
int y4_anchor_fitness_f32(const float* wh, int N, const float* cand, int G, int A, float thr, long long* out, void* stream);

/* ---- test-time augmentation (csrc/tta.hip) -----------------------------------------------------
 * y4_tta_view_f32: one rescaled, optionally mirrored view out [B][C][Hv][Wv] of an fp32 batch in [B][C][H][W] in one launch;
 *   both tensors by their strides in elements (b, c, y, x).  With xs = flip ? Wv - 1 - x : x:
 *     y >= ch or xs >= cw: out(b, c, y, x) = fill (the padding up to the stride multiple);
 *     else a bilinear sample with half-pixel centres and no antialiasing, each step one fp32 operation in this order:
 *       sy = (float(y) + 0.5f) * ry - 0.5f, clamped to [0, H - 1]; y0 = floorf(sy), fy = sy - y0, y1 = min(y0 + 1, H - 1);
 *       the same for sx from xs with rx; with a, b = in(y0, x0), in(y0, x1) and c, d = in(y1, x0), in(y1, x1):
 *       top = a + (b - a) * fx, bot = c + (d - c) * fx, out = top + (bot - top) * fy.
 *   The host chooses ch = max(1, int(H * r)), Hv = ch rounded up to the model's largest stride, ry = float(H) / float(ch)
 *   (and the same in x).  Errors before any launch: NULL Y4_ERR_NULL; a size outside [1, 65535], ch > Hv, cw > Wv, flip
 *   outside {0, 1} or a ratio that is not > 0 Y4_ERR_SHAPE.
 * y4_tta_merge_f32: one view's eval prediction pred [B][N][n_ch] (centre-xywh boxes in the view's pixels) into rows
 *   [row_off, row_off + N) of every image of out [B][n_total][n_ch], the boxes mapped to base-canvas pixels:
 *     cx' = (flip ? view_w - cx : cx) * inv_sx, cy' = cy * inv_sy, w' = w * inv_sx, h' = h * inv_sy (one fp32 operation per
 *   step); columns 4.. are copied.  With flip = 0 and both factors 1.0 the box columns are copied too, not multiplied.
 *   The host computes inv_sx = float(W) / float(cw).  Errors before any launch: NULL Y4_ERR_NULL; row_off + N > n_total,
 *   n_ch < 5, N * n_ch >= 2^31, B outside [1, 65535], flip outside {0, 1} or a non-positive size Y4_ERR_SHAPE. */
int y4_tta_view_f32(const float* in, int B, int C, int H, int W, long long in_sb, long long in_sc, long long in_sy,
                    long long in_sx, float* out, int Hv, int Wv, long long out_sb, long long out_sc, long long out_sy,
                    long long out_sx, int ch, int cw, float ry, float rx, int flip, float fill, void* stream);
int y4_tta_merge_f32(const float* pred, int B, long long N, int n_ch, float* out, long long n_total, long long row_off,
                     float view_w, int flip, float inv_sx, float inv_sy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLOV4_AMD_H */
