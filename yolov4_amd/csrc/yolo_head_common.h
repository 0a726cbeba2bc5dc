// What more than one of yolo_decode.hip, yolo_loss.hip and postprocess.hip uses, and nothing else.
// Internal linkage like the rest of those files: the anonymous namespace is each including file's own.
#pragma once
#include "common.h"

namespace {

struct Anchors { float w[16]; float h[16]; };

bool fill_anchors(Anchors& a, const float* host_wh, int n) {
    if (!host_wh || n < 1 || n > 16) return false;
    for (int i = 0; i < 16; ++i) { a.w[i] = 1.f; a.h[i] = 1.f; }
    for (int i = 0; i < n; ++i) { a.w[i] = host_wh[2 * i]; a.h[i] = host_wh[2 * i + 1]; }
    return true;
}

inline bool scale_xy_ok(float s) { return s >= 1.f && s <= 2.f; }

// A workspace layout: take() hands out the offset of the next block and moves on to the next multiple of 16 bytes; `end`
// is the size so far.
struct Bump {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end = (end + bytes + 15) & ~(size_t)15;
        return at;
    }
};

inline int grid_for(long long total) {
    long long b = (total + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace
