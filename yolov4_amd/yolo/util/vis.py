# -*- coding: utf-8 -*-
"""Drawing detections on device images: what the reference's `vis_bbox` (yolo/util/vis_bbox.py) does with cv2 on the host.

`draw_detections` prepares one record per box on the host (integer pixels: frame, label plate, text origin, glyph scale) and
draws the whole batch in place with ONE launch of y4_draw_boxes_u8 (csrc/draw.hip): every pixel takes the colour of the last
record that covers it.  The look is this package's own: square-cornered frames, a 5 x 7 bitmap font (glyphs.py); cv2's
anti-aliased lines and Hershey font are not reproduced.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from ..._lib import DrawBox, DrawJob, Y4Error, lib
from . import glyphs as G

_JOB, _BOX = ctypes.sizeof(DrawJob), ctypes.sizeof(DrawBox)
_LIMIT = 1 << 20          # coordinates are clamped here: far outside any image, far inside the kernel's int range


def _round16(v):
    return (int(v) + 15) & ~15


def class_colors(n, seed=0):
    """[n, 3] uint8, one colour per class: a fixed palette (the reference draws new random colours on every run)"""
    return np.random.RandomState(seed).randint(128, 255, (n, 3)).astype(np.uint8)


def box_layout(x1, y1, x2, y2, n_chars, line_width):
    """Arrays (or scalars) of box corners and label lengths -> int32 [n, 12]: the fields x1 .. scale of y4_draw_box in order.
    The label plate is as wide as the text (6 scale pixels per character, 8 scale high, scale = max(1, line_width - 1)) and
    sits above the box when it fits (y1 - plate height >= 3, the reference's `outside` rule), else just below the top edge;
    the text starts at its top-left corner.  Without characters there is no plate (px2 < px1)."""
    c = lambda v: np.clip(np.nan_to_num(np.asarray(v, dtype=np.float64).reshape(-1)), -_LIMIT, _LIMIT).astype(np.int64)
    x1, y1, x2, y2 = c(x1), c(y1), c(x2), c(y2)           # astype truncates towards zero, like int()
    n_chars = np.asarray(n_chars, dtype=np.int64).reshape(-1)
    scale = max(1, int(line_width) - 1)
    tw, th = 6 * scale * n_chars, 8 * scale
    top = np.where(y1 - th >= 3, y1 - th, y1)
    has = n_chars > 0
    out = np.zeros((len(x1), 12), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = x1, y1, x2, y2, int(line_width) // 2
    out[:, 5], out[:, 6] = np.where(has, x1, 0), np.where(has, top, 0)
    out[:, 7], out[:, 8] = np.where(has, x1 + tw - 1, -1), np.where(has, top + th - 1, -1)
    out[:, 9], out[:, 10], out[:, 11] = np.where(has, x1, 0), np.where(has, top, 0), scale
    return out


_GLYPH_OF_BYTE = np.full(256, G.UNKNOWN, dtype=np.uint8)
for _c, _i in G.INDEX.items():
    _GLYPH_OF_BYTE[ord(_c)] = _i


class DrawPlan(object):
    """A batch ready to draw: the pinned table (jobs, box records, label glyph indices, glyph rows) and its device twin."""

    def __init__(self, n, host, dev):
        self.n, self.host, self.dev = n, host, dev


def plan_draw(images, boxes_per_image, labels_per_image=None, colors_per_image=None, line_width=3):
    """The host work of `draw_detections`: checks, one record per box, one table for the batch.  Touches no image."""
    images = list(images)
    n = len(images)
    if n < 1:
        raise ValueError('an empty batch')
    if int(line_width) < 1 or int(line_width) > 64:
        raise ValueError('line_width is 1..64')
    device = images[0].device
    if device.type != 'cuda':
        raise Y4Error('draw_detections runs on the GPU only: there is no CPU path')
    records, texts, first, n_text = [], [], [0], 0
    for i, t in enumerate(images):
        if not (t.dtype == torch.uint8 and t.device == device and t.dim() == 3 and t.shape[2] == 3 and t.numel() > 0 and
                t.stride(2) == 1 and (t.stride(1) == 3 or t.shape[1] == 1) and
                (t.shape[0] == 1 or t.stride(0) >= 3 * t.shape[1])):
            raise Y4Error('image %d of the batch: expected a uint8 [h, w, 3] tensor on %s with dense pixels' % (i, device))
        boxes = np.asarray(boxes_per_image[i], dtype=np.float64).reshape(-1, 4)
        m = len(boxes)
        labels = list(labels_per_image[i]) if labels_per_image is not None else [None] * m
        colors = (np.asarray(colors_per_image[i], dtype=np.uint8).reshape(-1, 3) if colors_per_image is not None
                  else np.full((m, 3), 255, dtype=np.uint8))
        if len(labels) != m or len(colors) != m:
            raise ValueError('image %d: %d boxes, %d labels, %d colours' % (i, m, len(labels), len(colors)))
        # a character outside Latin-1 becomes '?', which has no glyph either: a solid cell
        coded = [(s or '').encode('latin-1', 'replace') for s in labels]
        lengths = np.array([len(b) for b in coded], dtype=np.int64).reshape(-1)
        rec = np.zeros((m, 16), dtype=np.int32)
        rec[:, :12] = box_layout(boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3], lengths, line_width)
        rec[:, 12] = n_text + np.cumsum(lengths) - lengths
        rec[:, 13] = lengths
        rec[:, 14:15].view(np.uint8)[:, :3] = colors
        records.append(rec)
        texts.append(_GLYPH_OF_BYTE[np.frombuffer(b''.join(coded), dtype=np.uint8)])
        n_text += int(lengths.sum())
        first.append(first[-1] + m)
    at_boxes = _round16(n * _JOB)
    at_text = at_boxes + first[-1] * _BOX
    at_glyphs = _round16(at_text + n_text)
    total = at_glyphs + G.GLYPHS.size
    with torch.cuda.device(device):
        host = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
        dev = torch.empty(total, dtype=torch.uint8, device=device)
    raw = host.numpy()
    raw[at_boxes:at_text] = np.concatenate(records).view(np.uint8).reshape(-1)
    raw[at_text:at_text + n_text] = np.concatenate(texts)
    raw[at_glyphs:] = G.GLYPHS.reshape(-1)
    jobs = (DrawJob * n).from_buffer(raw, 0)
    for i, t in enumerate(images):
        j = jobs[i]
        j.image = t.data_ptr()
        j.pitch = int(t.stride(0)) if t.shape[0] > 1 else 3 * int(t.shape[1])
        j.width, j.height = int(t.shape[1]), int(t.shape[0])
        j.n_boxes = first[i + 1] - first[i]
        j.boxes = dev.data_ptr() + at_boxes + first[i] * _BOX
        j.boxes_host = host.data_ptr() + at_boxes + first[i] * _BOX
        j.text = dev.data_ptr() + at_text
        j.text_bytes = n_text
        j.glyphs = dev.data_ptr() + at_glyphs
        j.n_glyphs = len(G.GLYPHS)
    return DrawPlan(n, host, dev)


def run_draw(plan):
    """One host -> device copy of the table and one launch on the current stream; nothing synchronises."""
    L = lib()
    with torch.cuda.device(plan.dev.device):
        plan.dev.copy_(plan.host, non_blocking=True)
        rc = L.y4_draw_boxes_u8(plan.dev.data_ptr(), plan.host.data_ptr(), plan.n, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            torch.cuda.current_stream().synchronize()
            raise Y4Error('y4_draw_boxes_u8: %s (code %d)' % (L.y4_strerror(rc).decode(), rc))


def draw_detections(images, boxes_per_image, labels_per_image=None, colors_per_image=None, line_width=3):
    """Draws in place.  images: list of [h, w, 3] uint8 device tensors (stride(1) == 3, stride(2) == 1, any row pitch).
    boxes_per_image[i]: array-like [n_i, 4] of (x1, y1, x2, y2) pixels, truncated to integers; labels_per_image[i]: n_i
    strings (None or '': no label); colors_per_image[i]: [n_i, 3] uint8 in the image's memory order (default: white).
    Boxes are painted in order, a later one over an earlier one.  One host -> device copy and one launch for the batch; nothing
    synchronises.  Returns images."""
    images = list(images)
    run_draw(plan_draw(images, boxes_per_image, labels_per_image, colors_per_image, line_width))
    return images
