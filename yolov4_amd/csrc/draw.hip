// Box overlay: frames, label plates and label text on uint8 HWC images, one launch per batch (include/yolov4_amd.h states the
// semantics).  A gather: one lane per pixel walks its image's box records in order and keeps the colour of the last record that
// covers it, then stores three bytes if any did.  The records are read at wave-uniform addresses (one image per workgroup), so
// the walk costs scalar loads and a handful of integer compares per record; only a pixel inside a label's text rectangle
// touches the text and glyph arrays.
#include "common.h"

namespace {

// grid (ceil(max width / 64), ceil(max height / 4), n_images), block (64, 4)
__global__ void __launch_bounds__(256)
draw_boxes_kernel(const y4_draw_job* __restrict__ jobs) {
    const y4_draw_job& job = jobs[blockIdx.z];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= job.width || y >= job.height) return;
    bool hit = false;
    unsigned c0 = 0, c1 = 0, c2 = 0;
    const int n = job.n_boxes;
    for (int i = 0; i < n; ++i) {
        const y4_draw_box& b = job.boxes[i];
        const int half = b.half;
        bool on = x >= b.x1 - half && x <= b.x2 + half && y >= b.y1 - half && y <= b.y2 + half &&
                  !(x > b.x1 + half && x < b.x2 - half && y > b.y1 + half && y < b.y2 - half);
        on = on || (x >= b.px1 && x <= b.px2 && y >= b.py1 && y <= b.py2);
        bool white = false;
        const int dx = x - b.tx, dy = y - b.ty, cell = 6 * b.scale;
        if (dx >= 0 && dy >= 0 && dy < 8 * b.scale && dx < cell * b.text_len) {
            const int ci = dx / cell;
            const int gx = (dx - ci * cell) / b.scale, gy = dy / b.scale;
            const int glyph = job.text[b.text_off + ci];
            if (glyph >= job.n_glyphs) white = true;
            else white = gx < 5 && gy < 7 && ((job.glyphs[glyph * 8 + gy] >> (4 - gx)) & 1);
        }
        if (white) {
            hit = true;
            c0 = c1 = c2 = 255u;
        } else if (on) {
            hit = true;
            c0 = b.color[0];
            c1 = b.color[1];
            c2 = b.color[2];
        }
    }
    if (hit) {
        unsigned char* p = (unsigned char*)job.image + (long long)y * job.pitch + 3ll * x;
        p[0] = (unsigned char)c0;
        p[1] = (unsigned char)c1;
        p[2] = (unsigned char)c2;
    }
}

}  // namespace

extern "C" int y4_draw_boxes_u8(const y4_draw_job* jobs_dev, const y4_draw_job* jobs_host, int n_images, void* stream) {
    if (!jobs_dev || !jobs_host) return Y4_ERR_NULL;
    if (n_images < 1 || n_images > 65535) return Y4_ERR_SHAPE;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n_images; ++i) {
        const y4_draw_job& j = jobs_host[i];
        if (!j.image) return Y4_ERR_NULL;
        if (j.width < 1 || j.width > 65535 || j.height < 1 || j.height > 65535 || j.pitch < 3ll * j.width) return Y4_ERR_SHAPE;
        if (j.n_boxes < 0 || j.text_bytes < 0 || j.n_glyphs < 0) return Y4_ERR_SHAPE;
        if (j.n_boxes > 0 && (!j.boxes || !j.boxes_host)) return Y4_ERR_NULL;
        if ((j.text_bytes > 0 && !j.text) || (j.n_glyphs > 0 && !j.glyphs)) return Y4_ERR_NULL;
        for (int k = 0; k < j.n_boxes; ++k) {
            const y4_draw_box& b = j.boxes_host[k];
            if (b.half < 0 || b.half > 4096 || b.scale < 1 || b.scale > 4096) return Y4_ERR_SHAPE;
            if (b.text_off < 0 || b.text_len < 0 || b.text_len > 4096 || (long long)b.text_off + b.text_len > j.text_bytes)
                return Y4_ERR_SHAPE;
            // coordinates far outside any image would overflow the kernel's int arithmetic (x1 - half, 6 scale text_len)
            const int lim = 1 << 24;
            const int v[10] = {b.x1, b.y1, b.x2, b.y2, b.px1, b.py1, b.px2, b.py2, b.tx, b.ty};
            for (int e = 0; e < 10; ++e)
                if (v[e] < -lim || v[e] > lim) return Y4_ERR_SHAPE;
        }
        max_w = j.width > max_w ? j.width : max_w;
        max_h = j.height > max_h ? j.height : max_h;
    }
    const dim3 grid((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)n_images);
    hipLaunchKernelGGL(draw_boxes_kernel, grid, dim3(64, 4), 0, y4_stream(stream), jobs_dev);
    Y4_CHECK_LAUNCH();
    return Y4_OK;
}
