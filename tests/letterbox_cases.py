# -*- coding: utf-8 -*-
"""NumPy restatements and case tables for letterboxed / rectangular-batch inference (tests/test_letterbox_cases.py checks
them on the CPU, tests/test_gpu_letterbox.py feeds them to the kernels).  Plain module, no fixtures."""
import numpy as np

import head_cases as HC
import headopt_cases as HO
from oracle.preprocess import _coeffs

F32 = np.float32

# (h, w, S) -> (nh, nw), the 'rect' canvas at G = 32 and the offsets (top, left)
GEOMETRY = [
    ((480, 640, 608), (456, 608), (480, 608), (12, 0)),
    ((640, 480, 608), (608, 456), (608, 480), (0, 12)),
    ((37, 29, 64), (64, 50), (64, 64), (0, 7)),
    ((1, 300, 64), (1, 64), (32, 64), (15, 0)),
    ((96, 128, 64), (48, 64), (64, 64), (8, 0)),           # both axes exactly 2x: the box-average path
    ((1, 1, 64), (64, 64), (64, 64), (0, 0)),
]


# ------------------------------------------------------------------------------------------ preprocess
def resize_linear_u8(img, nh, nw):
    """img uint8 [H,W,3] -> uint8 [nh,nw,3]: cv2.resize(img, (nw, nh)), 8-bit INTER_LINEAR; oracle.preprocess.resize_linear_u8
    with its own size per axis (the 2x2 box average needs BOTH axes at exactly 2x, OpenCV's condition)."""
    h, w = img.shape[:2]
    a = img.astype(np.int64)
    if w == 2 * nw and h == 2 * nh:
        return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _coeffs(nw, w, True)
    sy, b0, b1 = _coeffs(nh, h, False)
    sx1 = np.minimum(sx + 1, w - 1)
    hrow = a[:, sx, :] * a0[None, :, None] + a[:, sx1, :] * a1[None, :, None]
    y0 = np.clip(sy, 0, h - 1)
    y1 = np.clip(sy + 1, 0, h - 1)
    v = (((b0[:, None, None] * (hrow[y0] >> 4)) >> 16) + ((b1[:, None, None] * (hrow[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def letterbox_ref(img, nh, nw, top, left, Hc, Wc, fill=114, swap_rb=True):
    """-> fp32 [3, Hc, Wc]: the image resized to (nh, nw) at (top, left) of a canvas of `fill`, channels reversed when
    swap_rb, / 255 in fp32."""
    assert 0 <= top and top + nh <= Hc and 0 <= left and left + nw <= Wc
    canvas = np.full((Hc, Wc, 3), fill, dtype=np.uint8)
    canvas[top:top + nh, left:left + nw] = resize_linear_u8(img, nh, nw)
    if swap_rb:
        canvas = canvas[:, :, ::-1]
    return np.ascontiguousarray(canvas.transpose(2, 0, 1)).astype(F32) / F32(255)


def bilinear_float(img, nh, nw):
    """float64 bilinear sampling at OpenCV's sample positions (half-pixel centres, clamped taps): what the fixed-point
    arithmetic approximates"""
    h, w = img.shape[:2]
    a = img.astype(np.float64)
    fx = (np.arange(nw) + 0.5) * (w / nw) - 0.5
    fy = (np.arange(nh) + 0.5) * (h / nh) - 0.5
    x0 = np.floor(fx).astype(np.int64)
    y0 = np.floor(fy).astype(np.int64)
    wx = fx - x0
    wy = fy - y0
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    rows = a[:, xa] * (1 - wx)[None, :, None] + a[:, xb] * wx[None, :, None]
    return rows[ya] * (1 - wy)[:, None, None] + rows[yb] * wy[:, None, None]


def image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# the GPU batch: (h, w, nh, nw, top, left, swap_rb) on a 64 x 96 canvas.  Placements flush to each edge, a 1-pixel-high
# image, the 2x area path, sizes that enlarge and sizes that shrink.
CANVAS = (64, 96)
BATCH = [
    (37, 29, 64, 50, 0, 0, 1),          # full height, flush top, bottom and left
    (29, 37, 50, 64, 14, 32, 0),        # flush bottom and right
    (1, 300, 1, 64, 31, 16, 1),         # one row high, shrunk 4.7x in x
    (300, 9, 64, 2, 0, 94, 0),          # two columns wide, flush right; left = 94 is not a multiple of 4
    (96, 128, 48, 64, 8, 5, 1),         # both axes exactly 2x: box average; odd left
    (1, 1, 64, 64, 0, 17, 0),           # one source pixel
    (13, 21, 40, 64, 23, 31, 1),
    (13, 21, 64, 96, 0, 0, 0),          # covers the canvas: no padding at all
]


# ------------------------------------------------------------------------------------------ box mapping
def forward_box(box_xyxy, info):
    """source-pixel (x1, y1, x2, y2) -> canvas pixels: * nw / w + left, * nh / h + top (what the loader does to labels)"""
    h, w, nh, nw, top, left = info
    x1, y1, x2, y2 = box_xyxy
    return [x1 * nw / w + left, y1 * nh / h + top, x2 * nw / w + left, y2 * nh / h + top]


# ------------------------------------------------------------------------------------------ rect decode
# (C, A, Fh, Fw, B, ldl)
RECT_DECODE_CASES = [
    (80, 3, 15, 19, 2, 256),        # 285 pixels: 17 tiles plus a ragged one of 13
    (80, 3, 19, 15, 2, 256),        # the transpose: catches swapped i / j
    (1, 3, 1, 16, 3, 20),           # one row
    (1, 3, 16, 1, 3, 20),           # one column
    (20, 3, 3, 5, 2, 75),           # dense pitch: per-channel kernel
    (59, 4, 2, 3, 2, 256),          # nt = 256: the whole LDS row, A = 4
    (1, 3, 250, 400, 1, 20),        # 100000 pixels: the 32-pixel tile
]
SCALES = (1.0, 1.2)


def rect_tile(B, Fh, Fw):
    return 32 if B * Fh * Fw >= 100000 else 16


def make_logits_rect(B, Fh, Fw, A, C, ldl, seed):
    """head_cases.make_logits for B * Fh * Fw pixel rows: the same planting rule over npix = B * Fh * Fw."""
    n_ch = 5 + C
    nt = A * n_ch
    npix = B * Fh * Fw
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((npix, nt)) * 2.0).astype(F32)
    for a in range(A):
        for ch in HC.roles(C):
            for k, mag in enumerate(HC.PLANT):
                for s, sign in enumerate((1.0, -1.0)):
                    x[(7 * (2 * k + s) + 3 * a + ch) % npix, a * n_ch + ch] = sign * mag
    m = 0
    for mag in HC.PLANT_FEW:
        for sign in (1.0, -1.0):
            for ch in (0, 2, 4, 4 + C):
                p, col = (11 + 5 * m) % npix, (m % A) * n_ch + ch
                for _ in range(npix):
                    if abs(x[p, col]) < 12.0:
                        break
                    p = (p + 1) % npix
                x[p, col] = sign * mag
                m += 1
    full = np.full((npix, ldl), np.nan, dtype=F32)
    full[:, :nt] = x
    return full


def logit_view_rect(logits_nhwc, ldl, B, Fh, Fw, A, C):
    """[B, A, Fh, Fw, 5 + C] view of the pixel rows"""
    n_ch = 5 + C
    lg = np.asarray(logits_nhwc, dtype=F32).reshape(B, Fh, Fw, ldl)[..., :A * n_ch]
    return lg.reshape(B, Fh, Fw, A, n_ch).transpose(0, 3, 1, 2, 4)


def decode_ref64_rect(logits_nhwc, ldl, B, Fh, Fw, A, C, anchors_wh, stride, scale_xy=1.0):
    """head_cases.decode_ref64 (eval) on an Fh x Fw map in float64, with headopt_cases' centre ((sigma * s) - h) + cell:
    x from arange(Fw), y from arange(Fh); rows [B, A*Fh*Fw, 5+C] in input pixels, box index a*Fh*Fw + j*Fw + i."""
    n_ch = 5 + C
    s, h = HO.s_h(scale_xy)
    v = logit_view_rect(logits_nhwc, ldl, B, Fh, Fw, A, C).astype(np.float64)
    anc = np.asarray(anchors_wh, dtype=np.float64).reshape(A, 2)
    out = v.copy()
    sig = np.r_[0:2, 4:n_ch]
    out[..., sig] = HC._sig64(v[..., sig])
    pred = out.copy()
    if scale_xy == 1.0:
        pred[..., 0] += np.arange(Fw, dtype=np.float64).reshape(1, 1, 1, Fw)
        pred[..., 1] += np.arange(Fh, dtype=np.float64).reshape(1, 1, Fh, 1)
    else:
        pred[..., 0] = (out[..., 0] * s - h) + np.arange(Fw, dtype=np.float64).reshape(1, 1, 1, Fw)
        pred[..., 1] = (out[..., 1] * s - h) + np.arange(Fh, dtype=np.float64).reshape(1, 1, Fh, 1)
    with np.errstate(over='ignore'):
        pred[..., 2] = np.exp(v[..., 2]) * anc[:, 0].reshape(1, A, 1, 1)
        pred[..., 3] = np.exp(v[..., 3]) * anc[:, 1].reshape(1, A, 1, 1)
    pred[..., :4] *= float(stride)
    return pred.reshape(B, A * Fh * Fw, n_ch)
