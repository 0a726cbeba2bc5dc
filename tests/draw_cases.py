# -*- coding: utf-8 -*-
"""A numpy painter's-algorithm oracle of `draw_detections` (yolov4_amd/yolo/util/vis.py, csrc/draw.hip), written from the
semantics include/yolov4_amd.h states: boxes painted in order, each one frame, then plate, then white text.  It takes the
package's glyph table as INPUT (the font is data, not behaviour) and shares no code with the package otherwise."""
import numpy as np


def _fill(img, x1, y1, x2, y2, color):
    """inclusive rectangle, clipped to the image"""
    h, w = img.shape[:2]
    xa, ya, xb, yb = max(x1, 0), max(y1, 0), min(x2, w - 1), min(y2, h - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = color


def draw(img, boxes, labels, colors, line_width, glyphs, chars):
    """img [h, w, 3] uint8; boxes [(x1, y1, x2, y2)] numbers (truncated); labels [str or None]; colors [(c0, c1, c2)];
    glyphs uint8 [n][8] rows with bit 4 leftmost; chars: the string whose i-th character glyph i draws -> a new image"""
    out = img.copy()
    h, w = out.shape[:2]
    half = line_width // 2
    scale = max(1, line_width - 1)
    for box, label, color in zip(boxes, labels, colors):
        x1, y1, x2, y2 = (int(v) for v in box)
        color = np.asarray(color, dtype=np.uint8)
        # frame: the outer rectangle without the open inner one
        layer = np.zeros((h, w), dtype=bool)
        ys, xs = np.mgrid[0:h, 0:w]
        outer = (xs >= x1 - half) & (xs <= x2 + half) & (ys >= y1 - half) & (ys <= y2 + half)
        inner = (xs > x1 + half) & (xs < x2 - half) & (ys > y1 + half) & (ys < y2 - half)
        layer = outer & ~inner
        out[layer] = color
        if not label:
            continue
        th, tw = 8 * scale, 6 * scale * len(label)
        top = y1 - th if y1 - th >= 3 else y1
        _fill(out, x1, top, x1 + tw - 1, top + th - 1, color)
        for k, ch in enumerate(label):
            cx = x1 + 6 * scale * k
            g = chars.find(ch)
            for gy in range(8):
                for gx in range(6):
                    if g < 0:
                        on = True                                   # no glyph: a solid cell
                    else:
                        on = gx < 5 and gy < 7 and (int(glyphs[g][gy]) >> (4 - gx)) & 1
                    if on:
                        _fill(out, cx + gx * scale, top + gy * scale, cx + (gx + 1) * scale - 1, top + (gy + 1) * scale - 1,
                              (255, 255, 255))
    return out
