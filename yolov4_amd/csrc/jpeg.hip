// JPEG decoding: the host stage (jpeg_host.h: markers, Huffman) behind the C ABI, and the device stage as two launches per
// BATCH: (1) dequantise + libjpeg "islow" integer IDCT of every 8x8 block of every image into its component planes,
// (2) chroma upsampling ("fancy" triangle filters), YCbCr -> RGB, EXIF orientation and the HWC store.  The arithmetic is
// libjpeg-turbo's default path bit for bit; include/yolov4_amd.h states it.
// Integer byte work: no MFMA.  Kernel 1 moves 16 B per lane in, 8 B per lane out, and transposes each block twice through
// padded LDS (row loads -> column pass -> row pass -> row stores); kernel 2 makes 4 pixels per lane and stores them as three
// dwords where the output is aligned and unrotated.
#include "common.h"
#include "jpeg_host.h"

namespace {

constexpr int kBlocksPerGroup = 32;     // 8x8 blocks per 256-thread workgroup: 8 lanes per block, 8 blocks per wave64
constexpr int kLdsBlock = 72;           // dwords per block in LDS: 8 rows of pitch 9 (rows and columns both conflict-free)

// sums and products run in unsigned arithmetic (the same bits as int where int does not overflow, and defined where a hostile
// file's coefficients make it wrap); only the descaling shift is signed
__device__ __forceinline__ int descale(int x, int n) { return (int)((unsigned)x + (1u << (n - 1))) >> n; }

// one 1-D pass of jidctint's jpeg_idct_islow (CONST_BITS 13); the caller descales
__device__ __forceinline__ void idct_islow_1d(const int (&in)[8], int (&out)[8]) {
    typedef unsigned U;
    U z2 = (U)in[2], z3 = (U)in[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 - z3 * 15137u;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)in[0];
    z3 = (U)in[4];
    U tmp0 = (z2 + z3) * 8192u;
    U tmp1 = (z2 - z3) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)in[7];
    tmp1 = (U)in[5];
    tmp2 = (U)in[3];
    tmp3 = (U)in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 = 0u - z1 * 7373u;
    z2 = 0u - z2 * 20995u;
    z3 = z5 - z3 * 16069u;
    z4 = z5 - z4 * 3196u;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = (int)(tmp10 + tmp3);
    out[7] = (int)(tmp10 - tmp3);
    out[1] = (int)(tmp11 + tmp2);
    out[6] = (int)(tmp11 - tmp2);
    out[2] = (int)(tmp12 + tmp1);
    out[5] = (int)(tmp12 - tmp1);
    out[3] = (int)(tmp13 + tmp0);
    out[4] = (int)(tmp13 - tmp0);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// grid (ceil(max blocks of a job / 32), n_jobs); lane r of a block's 8 lanes owns row r on the way in and out, column r between
__global__ void __launch_bounds__(256)
jpeg_idct_kernel(const y4_jpeg_job* __restrict__ jobs, unsigned char* __restrict__ ws) {
    __shared__ int lds[kBlocksPerGroup * kLdsBlock];
    const y4_jpeg_job& job = jobs[blockIdx.y];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int g = blockIdx.x * kBlocksPerGroup + lb;
    const int nb0 = job.info.blocks_w[0] * job.info.blocks_h[0];
    const int nb1 = job.info.blocks_w[1] * job.info.blocks_h[1];
    const int nb2 = job.info.blocks_w[2] * job.info.blocks_h[2];
    const bool valid = g < nb0 + nb1 + nb2;
    const int comp = g < nb0 ? 0 : (g < nb0 + nb1 ? 1 : 2);
    const int gl = g - (comp == 0 ? 0 : (comp == 1 ? nb0 : nb0 + nb1));
    int* mine = lds + lb * kLdsBlock;

    int v[8], o[8];
    if (valid) {
        // blocks lie in the coefficient buffer in the order of g: one 16-byte load per lane, 1 KiB contiguous per wave
        const uint4 c4 = *reinterpret_cast<const uint4*>(job.coef + ((long long)g * 64 + r * 8));
        const uint4 q4 = *reinterpret_cast<const uint4*>(&job.qt[comp][r * 8]);
        const unsigned cw[4] = {c4.x, c4.y, c4.z, c4.w}, qw[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = (int)(short)(cw[j] & 0xffffu) * (int)(qw[j] & 0xffffu);
            v[2 * j + 1] = ((int)cw[j] >> 16) * (int)(qw[j] >> 16);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) mine[r * 9 + j] = v[j];
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = mine[k * 9 + r];
        idct_islow_1d(v, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = descale(o[k], 11);
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) mine[k * 9 + r] = o[k];
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = mine[r * 9 + j];
        idct_islow_1d(v, o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= (unsigned)clamp255(descale(o[j], 18) + 128) << (8 * j);
            hi |= (unsigned)clamp255(descale(o[j + 4], 18) + 128) << (8 * j);
        }
        const int bw = job.info.blocks_w[comp];
        const int by = gl / bw, bx = gl - by * bw;
        // the planes follow each other like the coefficients: component c starts at 64 * (blocks before it) bytes
        const long long plane = job.ws_offset + 64ll * (g - gl);
        unsigned char* dst = ws + plane + ((long long)(by * 8 + r) * bw + bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

struct Planes {
    const unsigned char* p;     // plane of one component
    int pitch;                  // bytes per row (8 * blocks_w)
};

// The four upsampled chroma samples for output columns x0 .. x0+3 (x0 % 4 == 0) of output row y, one per byte.  mode: 0 = 1x1 (no
// upsampling), 1 = h2v1, 2 = h2v2.  Index clamping to the real dw x dh samples reproduces libjpeg's special first / last
// columns: (3a + a + 1) >> 2 = a, (3a + a + 2) >> 2 = a, (3cs + cs + 8) >> 4 = (4cs + 8) >> 4, ... + 7 likewise.
__device__ __forceinline__ unsigned chroma4(const Planes pl, int mode, int dw, int dh, int x0, int y) {
    if (mode == 0) return *reinterpret_cast<const unsigned*>(pl.p + (long long)y * pl.pitch + x0);   // padded to 8: in range
    const int i0 = x0 >> 1;
    const int j = mode == 2 ? (y >> 1) : y;
    const unsigned char* row = pl.p + (long long)j * pl.pitch;
    const int last = dw - 1;
    const int k1 = i0 < last ? i0 : last, k2 = i0 + 1 < last ? i0 + 1 : last;      // i0 <= last already: x0 < W
    const int k0 = i0 > 0 ? i0 - 1 : 0, k3 = i0 + 2 < last ? i0 + 2 : last;
    if (dw <= 2) {                                      // libjpeg-turbo: no fancy filter on planes this narrow
        const unsigned a = row[k1], b = row[k2];
        return a | (a << 8) | (b << 16) | (b << 24);
    }
    int a0 = row[k0], a1 = row[k1], a2 = row[k2], a3 = row[k3];
    int o0, o1, o2, o3;
    if (mode == 1) {
        o0 = (3 * a1 + a0 + 1) >> 2;
        o1 = (3 * a1 + a2 + 2) >> 2;
        o2 = (3 * a2 + a1 + 1) >> 2;
        o3 = (3 * a2 + a3 + 2) >> 2;
    } else {
        int jn = (y & 1) ? j + 1 : j - 1;
        jn = jn < 0 ? 0 : (jn > dh - 1 ? dh - 1 : jn);
        const unsigned char* nrow = pl.p + (long long)jn * pl.pitch;
        a0 = 3 * a0 + nrow[k0];
        a1 = 3 * a1 + nrow[k1];
        a2 = 3 * a2 + nrow[k2];
        a3 = 3 * a3 + nrow[k3];
        o0 = (3 * a1 + a0 + 8) >> 4;
        o1 = (3 * a1 + a2 + 7) >> 4;
        o2 = (3 * a2 + a1 + 8) >> 4;
        o3 = (3 * a2 + a3 + 7) >> 4;
    }
    return (unsigned)o0 | ((unsigned)o1 << 8) | ((unsigned)o2 << 16) | ((unsigned)o3 << 24);
}

// grid (ceil(ceil(max W / 4) / 64), ceil(max H / 4), n_jobs), block (64, 4): a lane makes pixels x0 .. x0+3 of row y
__global__ void __launch_bounds__(256)
jpeg_color_kernel(const y4_jpeg_job* __restrict__ jobs, const unsigned char* __restrict__ ws) {
    const y4_jpeg_job& job = jobs[blockIdx.z];
    const int W = job.info.width, H = job.info.height;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= W || y >= H) return;
    const unsigned char* base = ws + job.ws_offset;
    const int pitch0 = job.info.blocks_w[0] * 8;
    const unsigned yw = *reinterpret_cast<const unsigned*>(base + (long long)y * pitch0 + x0);
    int px[4][3];                                       // [pixel][R, G, B], then in memory order
    if (job.info.ncomp == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i][0] = px[i][1] = px[i][2] = (yw >> (8 * i)) & 255u;
    } else {
        const int hs = job.info.hs[0], vs = job.info.vs[0];
        const int mode = hs == 1 ? 0 : (vs == 1 ? 1 : 2);
        const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
        const long long n0 = 64ll * job.info.blocks_w[0] * job.info.blocks_h[0];
        const long long n1 = 64ll * job.info.blocks_w[1] * job.info.blocks_h[1];
        const int pitch1 = job.info.blocks_w[1] * 8;
        const unsigned cbw = chroma4(Planes{base + n0, pitch1}, mode, dw, dh, x0, y);
        const unsigned crw = chroma4(Planes{base + n0 + n1, pitch1}, mode, dw, dh, x0, y);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int Y = (yw >> (8 * i)) & 255u, b = (int)((cbw >> (8 * i)) & 255u) - 128, r = (int)((crw >> (8 * i)) & 255u) - 128;
            px[i][0] = clamp255(Y + ((91881 * r + 32768) >> 16));
            px[i][1] = clamp255(Y + ((-22554 * b - 46802 * r + 32768) >> 16));
            px[i][2] = clamp255(Y + ((116130 * b + 32768) >> 16));
        }
    }
    if (!job.swap_rb) {                                 // memory order: B G R; R G B with swap_rb (selects, not indexed: no scratch)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = px[i][0];
            px[i][0] = px[i][2];
            px[i][2] = t;
        }
    }
    const int orient = job.apply_orientation ? job.info.orientation : 1;
    unsigned char* out = (unsigned char*)job.out;
    if (orient == 1 && x0 + 4 <= W && (((unsigned long long)out | (unsigned long long)job.out_pitch) & 3ull) == 0) {
        // 12 bytes at a multiple of 12 from an aligned row: three dwords
        const unsigned p0 = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16), p1 = px[1][0] | (px[1][1] << 8) | (px[1][2] << 16);
        const unsigned p2 = px[2][0] | (px[2][1] << 8) | (px[2][2] << 16), p3 = px[3][0] | (px[3][1] << 8) | (px[3][2] << 16);
        unsigned* o = reinterpret_cast<unsigned*>(out + (long long)y * job.out_pitch + 3ll * x0);
        o[0] = p0 | (p1 << 24);
        o[1] = (p1 >> 8) | (p2 << 16);
        o[2] = (p2 >> 16) | (p3 << 8);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = x0 + i;
        int ox, oy;
        switch (orient) {
            case 2: ox = W - 1 - x; oy = y; break;
            case 3: ox = W - 1 - x; oy = H - 1 - y; break;
            case 4: ox = x; oy = H - 1 - y; break;
            case 5: ox = y; oy = x; break;
            case 6: ox = H - 1 - y; oy = x; break;
            case 7: ox = H - 1 - y; oy = W - 1 - x; break;
            case 8: ox = y; oy = W - 1 - x; break;
            default: ox = x; oy = y; break;
        }
        if (x < W) {
            unsigned char* o = out + (long long)oy * job.out_pitch + 3ll * ox;
            o[0] = (unsigned char)px[i][0];
            o[1] = (unsigned char)px[i][1];
            o[2] = (unsigned char)px[i][2];
        }
    }
}

// the geometry y4_jpeg_parse_host gives for (width, height, ncomp, hs[0], vs[0]); false when the record differs from it
bool info_ok(const y4_jpeg_info& f) {
    if (f.width < 1 || f.width > 65535 || f.height < 1 || f.height > 65535) return false;
    if (f.ncomp != 1 && f.ncomp != 3) return false;
    const int hv = f.hs[0] * 16 + f.vs[0];
    if (f.ncomp == 1 ? hv != 0x11 : (hv != 0x11 && hv != 0x21 && hv != 0x22)) return false;
    const int mx = (f.width + 8 * f.hs[0] - 1) / (8 * f.hs[0]), my = (f.height + 8 * f.vs[0] - 1) / (8 * f.vs[0]);
    if (f.mcus_x != mx || f.mcus_y != my) return false;
    long long count = 0;
    for (int c = 0; c < 3; ++c) {
        const int hs = c < f.ncomp ? (c == 0 ? f.hs[0] : 1) : 0, vs = c < f.ncomp ? (c == 0 ? f.vs[0] : 1) : 0;
        if (f.hs[c] != hs || f.vs[c] != vs || f.blocks_w[c] != mx * hs || f.blocks_h[c] != my * vs) return false;
        count += 64ll * f.blocks_w[c] * f.blocks_h[c];
    }
    return f.coef_count == count && f.orientation >= 1 && f.orientation <= 8;
}

size_t round16(long long v) { return ((size_t)v + 15) & ~(size_t)15; }

}  // namespace

extern "C" int y4_jpeg_parse_host(const void* data_host, size_t nbytes, y4_jpeg_info* info_host) {
    return y4jpeg::parse((const uint8_t*)data_host, nbytes, info_host);
}

extern "C" int y4_jpeg_entropy_host(const void* data_host, size_t nbytes, const y4_jpeg_info* info_host, short* coef_host,
                                    long long coef_cap, unsigned short* qt_host) {
    return y4jpeg::entropy((const uint8_t*)data_host, nbytes, info_host, coef_host, coef_cap, qt_host);
}

extern "C" size_t y4_jpeg_workspace(const y4_jpeg_info* infos_host, int n) {
    size_t total = 0;
    if (!infos_host) return 0;
    for (int i = 0; i < n; ++i)
        if (infos_host[i].coef_count > 0) total += round16(infos_host[i].coef_count);
    return total;
}

extern "C" int y4_jpeg_decode_u8(const y4_jpeg_job* jobs_dev, const y4_jpeg_job* jobs_host, int n_jobs, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!jobs_dev || !jobs_host || !workspace) return Y4_ERR_NULL;
    if (n_jobs < 1 || n_jobs > 65535) return Y4_ERR_SHAPE;
    if (((unsigned long long)jobs_dev & 15ull) || ((unsigned long long)workspace & 15ull)) return Y4_ERR_SHAPE;
    long long max_blocks = 0;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const y4_jpeg_job& j = jobs_host[i];
        if (!j.coef || !j.out) return Y4_ERR_NULL;
        if (!info_ok(j.info)) return Y4_ERR_SHAPE;
        if (((unsigned long long)j.coef & 15ull) || j.ws_offset < 0 || (j.ws_offset & 15)) return Y4_ERR_SHAPE;
        const bool turned = j.apply_orientation && j.info.orientation >= 5;
        if (j.out_pitch < 3ll * (turned ? j.info.height : j.info.width)) return Y4_ERR_SHAPE;
        if ((unsigned long long)j.ws_offset + (unsigned long long)j.info.coef_count > workspace_bytes) return Y4_ERR_WORKSPACE;
        const long long blocks = j.info.coef_count / 64;
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        max_w = j.info.width > max_w ? j.info.width : max_w;
        max_h = j.info.height > max_h ? j.info.height : max_h;
    }
    // 65535 x 65535 at 4:4:4 is 2.0e8 blocks: the grid's x fits an int, the kernel's block index too
    const dim3 grid1((unsigned)((max_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)n_jobs);
    hipLaunchKernelGGL(jpeg_idct_kernel, grid1, dim3(256), 0, y4_stream(stream), jobs_dev, (unsigned char*)workspace);
    Y4_CHECK_LAUNCH();
    const dim3 grid2((unsigned)(((max_w + 3) / 4 + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)n_jobs);
    hipLaunchKernelGGL(jpeg_color_kernel, grid2, dim3(64, 4), 0, y4_stream(stream), jobs_dev,
                       (const unsigned char*)workspace);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
