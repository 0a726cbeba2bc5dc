# -*- coding: utf-8 -*-
"""References, acceptance criterion and case list for the training augmentation kernels (csrc/augment.hip); numpy only.

`render(case, F64)` is the fp64 reference of y4_augment_mosaic_u8_f32, written from the statement in
include/yolov4_amd.h: per output pixel the tile, the position in the tile's resized image, OpenCV's floating linear
coordinates (position and fraction rounded to fp32 exactly where OpenCV rounds them, weights 1 - f and f in fp32), the
un-flipped, crop-shifted taps with the source's fractional mean behind every tap outside the source, the float HSV round
trip with its jitter and clip, / 255.  Everything that is not a coordinate or a weight is fp64.  `render(case, F32)`
evaluates the same formulas with every intermediate rounded to fp32: the arithmetic a kernel without contraction and in
this summation order performs.  `channel_sums` is the reference of y4_augment_means_u8 (exact integers).

Acceptance for pixel values on the [0, 1] scale:  |got - ref| <= K * 2^-24.
K = 4 x (max |fp32 emulation - fp64 reference| over every case of CASES, in units of 2^-24), rounded up to a power of
two; the factor covers FMA contraction and another summation order in the kernel, neither of which is a defect.
Measured: MEASURED_UNITS (below; tests/test_augment_cases.py re-measures it and requires it to stay <= K / 4), hence K.
Bit-exact: the integer sums; the pixels of the cases marked `exact` (colour off, no pad taps, integer sample positions:
the output is u8 / 255 in fp32); guard words and everything around the destination slot.

Case list (smallest shapes at which each branch is reachable; tests/test_augment_cases.py asserts the reach):
  sources 2x3, 17x23, 37x53, 64x64; S = 32, 40, 64; crops all-negative (pad ring), all-positive, mixed; a 1x1 crop;
  64x64 -> 32 exact 2x; flip on / off; mosaic cuts at both ends of the sampler's range, at S / 2, and at 0 and S (the
  ends the entry point accepts: empty tiles); shifts hitting each of the four clamps; n_src 1 and 4; B = 3 mixing both
  with different source sizes; pitch > 3w; swap_rb 0 and 1; dst as a strided slot of a wider buffer and channels-last;
  colour: identity parameters (HSV skipped), grey, hue wrapped below 0 and above 360, v over 255, s over 1, black.
REJECTS: every argument set the entry points refuse."""
import copy

import numpy as np

F32, F64 = np.float32, np.float64
SENT = 0x7FC5A5A5                       # a NaN bit pattern no kernel produces
UNIT = 2.0 ** -24
MEASURED_UNITS = 11.5                   # max |fp32 emulation - fp64 reference| / 2^-24 over CASES
K = 64                                  # 4 x MEASURED_UNITS rounded up to a power of two
FLT_EPS = float(np.finfo(F32).eps)


# ---------------------------------------------------------------------------------------------- records

def src(img, left=0, right=0, top=0, bottom=0, flip=0, color=0, dhue=0.0, dsat=1.0, dexp=1.0, swap_rb=1, pitch_extra=0):
    """one y4_aug_src as a dict; the crop is given by the reference's four offsets"""
    h, w = img.shape[:2]
    return dict(img=np.ascontiguousarray(img, dtype=np.uint8), h=h, w=w, pitch_extra=pitch_extra, swap_rb=swap_rb,
                crop_left=left, crop_right=right, crop_top=top, crop_bottom=bottom, crop_w=w - left - right,
                crop_h=h - top - bottom, flip=flip, color=color, dhue=float(F32(dhue)), dsat=float(F32(dsat)),
                dexp=float(F32(dexp)), win_x=0, win_y=0)


def raw_shifts(s, S):
    """the four shifts before the clamps of blend_mosaic (already cut-limited): see shifts()"""
    cl, cr = (s['crop_right'], s['crop_left']) if s['flip'] else (s['crop_left'], s['crop_right'])
    return (max(0, -cl * S / s['crop_w']), max(0, -s['crop_top'] * S / s['crop_h']),
            max(0, -cr * S / s['crop_w']), max(0, -s['crop_bottom'] * S / s['crop_h']))


def shifts(s, cut_x, cut_y, S):
    """(left, top, right, bottom, clamped flags): int(min(cut, raw)) then left <= S - cut_x, top <= S - cut_y,
    right <= cut_x, bottom <= cut_y"""
    rl, rt, rr, rb = raw_shifts(s, S)
    first = (int(min(cut_x, rl)), int(min(cut_y, rt)), int(min(S - cut_x, rr)), int(min(S - cut_y, rb)))
    caps = (S - cut_x, S - cut_y, cut_x, cut_y)
    out = tuple(min(a, c) for a, c in zip(first, caps))
    return out + (tuple(a > c for a, c in zip(first, caps)),)


def tile_rect(q, cut_x, cut_y, S):
    """(x0, y0, extent_x, extent_y) of tile q in the output"""
    x0, y0 = (cut_x if q & 1 else 0), (cut_y if q & 2 else 0)
    return x0, y0, (S - cut_x if q & 1 else cut_x), (S - cut_y if q & 2 else cut_y)


def sample(S, srcs, cut=None):
    """one output sample: a single source, or four with the windows blend_mosaic slices out of their resized images"""
    srcs = [dict(s) for s in srcs]
    if len(srcs) == 1:
        return dict(cut_x=0, cut_y=0, srcs=srcs)
    cut_x, cut_y = cut
    for q, s in enumerate(srcs):
        left, top, right, bottom, _ = shifts(s, cut_x, cut_y, S)
        s['win_x'] = cut_x - right if q & 1 else left
        s['win_y'] = cut_y - bottom if q & 2 else top
    return dict(cut_x=cut_x, cut_y=cut_y, srcs=srcs)


def case(name, S, samples, layout='nchw', exact=False):
    return dict(name=name, S=S, samples=samples, layout=layout, exact=exact)


# ---------------------------------------------------------------------------------------------- references

def channel_sums(s):
    """exact sums per channel in memory order (python ints)"""
    return [int(s['img'][:, :, k].astype(np.uint64).sum()) for k in range(3)]


def _coords(r, S, n):
    """OpenCV's floating linear resize: source index and fp32 fraction of output index r in n samples"""
    scale = 1.0 / (float(S) / float(n))
    f = ((r.astype(F64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f)
    return s.astype(np.int64), (f - s).astype(F32)


def hsv_jitter(rgb, dhue, dsat, dexp, T, stats=None):
    """OpenCV's float RGB -> HSV, the jitter, HSV -> RGB, clip to [0, 255]; rgb [..., 3] of dtype T on the 0..255 scale"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    eps = T(FLT_EPS)
    v = np.maximum(r, np.maximum(g, b))
    d = (v - np.minimum(r, np.minimum(g, b))).astype(T)
    s = (d / (np.abs(v) + eps).astype(T)).astype(T)
    k = (T(60) / (d + eps).astype(T)).astype(T)
    h = np.where(v == r, ((g - b).astype(T) * k).astype(T),
                 np.where(v == g, (((b - r).astype(T) * k).astype(T) + T(120)).astype(T),
                          (((r - g).astype(T) * k).astype(T) + T(240)).astype(T)))
    h = np.where(h < 0, (h + T(360)).astype(T), h)
    h = (h + T(T(179) * T(dhue))).astype(T)
    s = (s * T(dsat)).astype(T)
    v = (v * T(dexp)).astype(T)
    h = (h / T(60)).astype(T)
    below, above = h < 0, h >= 6
    while (h < 0).any():
        h = np.where(h < 0, (h + T(6)).astype(T), h)
    while (h >= 6).any():
        h = np.where(h >= 6, (h - T(6)).astype(T), h)
    i = np.floor(h)
    f = (h - i).astype(T)
    i = i.astype(np.int64)
    one = T(1)
    c0 = v
    c1 = (v * (one - s).astype(T)).astype(T)
    c2 = (v * (one - (s * f).astype(T)).astype(T)).astype(T)
    c3 = (v * (one - (s * (one - f).astype(T)).astype(T)).astype(T)).astype(T)
    cand = np.stack([c0, c1, c2, c3], -1)
    order = np.array([[0, 3, 1], [2, 0, 1], [1, 0, 3], [1, 2, 0], [3, 1, 0], [0, 1, 2]])     # sector -> (r, g, b)
    out = np.take_along_axis(cand, order[i], -1)
    grey = s == 0
    out = np.where(grey[..., None], v[..., None], out).astype(T)
    clipped = np.clip(out, T(0), T(255)).astype(T)
    if stats is not None:
        live = ~grey
        stats['hsv'] += int(h.size)
        stats['grey'] += int(grey.sum())
        stats['black'] += int((v == 0).sum())
        stats['wrap_below'] += int((below & live).sum())
        stats['wrap_above'] += int((above & live).sum())
        stats['clip_high'] += int((out > 255).sum())
        stats['clip_low'] += int((out < 0).sum())
        stats['s_over_1'] += int((s > 1).sum())
    return clipped


def resized(s, S, ry, rx, T, stats=None):
    """values [len(ry), len(rx), 3] on the 0..255 scale (output channel order) of the source's resized S x S image at rows
    ry, columns rx: steps 2-4"""
    sx, fx = _coords(rx, S, s['crop_w'])
    low, high = sx < 0, sx >= s['crop_w'] - 1
    fx = np.where(low | high, F32(0), fx)
    sx = np.where(low, 0, np.where(high, s['crop_w'] - 1, sx))
    sx1 = np.minimum(sx + 1, s['crop_w'] - 1)
    sy, fy = _coords(ry, S, s['crop_h'])
    y0 = np.clip(sy, 0, s['crop_h'] - 1)
    y1 = np.clip(sy + 1, 0, s['crop_h'] - 1)
    wx0, wx1 = (F32(1) - fx).astype(F32).astype(T), fx.astype(T)
    wy0, wy1 = (F32(1) - fy).astype(F32).astype(T), fy.astype(T)
    img = s['img'][:, :, ::-1] if s['swap_rb'] else s['img']
    mean = (img.reshape(-1, 3).astype(np.uint64).sum(0).astype(F64) / float(s['h'] * s['w'])).astype(T)

    def tap(cy, cx):
        ux = (s['crop_w'] - 1 - cx if s['flip'] else cx) + s['crop_left']
        uy = cy + s['crop_top']
        inside = ((uy >= 0) & (uy < s['h']))[:, None] & ((ux >= 0) & (ux < s['w']))[None, :]
        val = img[np.clip(uy, 0, s['h'] - 1)[:, None], np.clip(ux, 0, s['w'] - 1)[None, :]].astype(T)
        if stats is not None:
            stats['pad_taps'] += int((~inside).sum())
        return np.where(inside[..., None], val, mean[None, None, :]).astype(T)

    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    h0 = ((tap(y0, sx) * wx0).astype(T) + (tap(y0, sx1) * wx1).astype(T)).astype(T)
    h1 = ((tap(y1, sx) * wx0).astype(T) + (tap(y1, sx1) * wx1).astype(T)).astype(T)
    val = ((h0 * wy0).astype(T) + (h1 * wy1).astype(T)).astype(T)
    if stats is not None:
        stats['fractional'] += int((fx != 0).sum()) + int((fy != 0).sum())
    if s['color'] and (s['dsat'] != 1 or s['dexp'] != 1 or s['dhue'] != 0) and val.size:
        val = hsv_jitter(val, s['dhue'], s['dsat'], s['dexp'], T, stats)
    return val


def new_stats():
    return dict(pad_taps=0, fractional=0, hsv=0, grey=0, black=0, wrap_below=0, wrap_above=0, clip_high=0, clip_low=0,
                s_over_1=0)


def render(c, T=F64, stats=None):
    """[B, 3, S, S] of dtype T on the [0, 1] scale"""
    S = c['S']
    out = np.zeros((len(c['samples']), 3, S, S), dtype=T)
    for b, sm in enumerate(c['samples']):
        for q, s in enumerate(sm['srcs']):
            x0, y0, ex, ey = (0, 0, S, S) if len(sm['srcs']) == 1 else tile_rect(q, sm['cut_x'], sm['cut_y'], S)
            ry = np.arange(ey, dtype=np.int64) + s['win_y']
            rx = np.arange(ex, dtype=np.int64) + s['win_x']
            val = resized(s, S, ry, rx, T, stats)
            out[b, :, y0:y0 + ey, x0:x0 + ex] = (val / T(255)).astype(T).transpose(2, 0, 1)
    return out


def emulation_error_units(c):
    """max |fp32 emulation - fp64 reference| of one case in units of 2^-24"""
    return float(np.abs(render(c, F32).astype(F64) - render(c, F64)).max() / UNIT)


# ---------------------------------------------------------------------------------------------- destination layouts

def dst_layout(kind, B, S):
    """(total words, offset of element [0,0,0,0], strides (sb, sc, sh, sw) in elements)"""
    if kind == 'nchw':
        return B * 3 * S * S, 0, (3 * S * S, S * S, S, 1)
    if kind == 'slot':                     # [B, 3, S + 2, S + 3][:, :, 1:1 + S, 2:2 + S]
        H, W = S + 2, S + 3
        return B * 3 * H * W, W + 2, (3 * H * W, H * W, W, 1)
    if kind == 'nhwc4':                    # [B, S, S, 4][..., 1:4] viewed as [B, 3, S, S]
        return B * S * S * 4, 1, (S * S * 4, 1, S * 4, 4)
    raise KeyError(kind)


def dst_index(kind, B, S):
    """flat word index of every element of the [B, 3, S, S] view"""
    _, off, (sb, sc, sh, sw) = dst_layout(kind, B, S)
    b, ch, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(S), np.arange(S), indexing='ij')
    return off + b * sb + ch * sc + y * sh + x * sw


# ---------------------------------------------------------------------------------------------- cases

def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _colour_img(h, w, seed):
    """random pixels plus rows of grey, black, saturated reds either side of hue 0 and near-white pixels"""
    im = _img(h, w, seed)
    g = np.random.RandomState(seed + 1).randint(1, 256, size=w).astype(np.uint8)
    im[0] = g[:, None]                                   # grey: s == 0
    im[1] = 0                                            # black: v == 0
    im[2] = np.array([20, 3, 250], np.uint8)             # BGR: red, hue just above 0 ...
    im[3] = np.array([3, 20, 250], np.uint8)
    im[4] = np.array([40, 0, 255], np.uint8)             # ... and just below 360
    im[5] = np.array([250, 252, 255], np.uint8)          # bright: v * dexp > 255
    return im


def _mosaic_srcs(flip=(0, 1, 0, 1), pitch_extra=0, **kw):
    return [src(_img(17, 23, 11), -5, -3, -4, -6, flip=flip[0], pitch_extra=pitch_extra, **kw),
            src(_img(37, 53, 12), 6, -9, 5, -7, flip=flip[1], pitch_extra=pitch_extra, **kw),
            src(_img(2, 3, 13), -1, 0, 0, -1, flip=flip[2], pitch_extra=pitch_extra, **kw),
            src(_img(64, 64, 14), -12, 10, -11, 9, flip=flip[3], pitch_extra=pitch_extra, **kw)]


def _clamp_srcs():
    """big negative offsets on every side: every raw shift is large"""
    return [src(_img(17, 23, 21 + i), -20, -20, -15, -15, flip=i & 1) for i in range(4)]


def _build():
    cs = []
    a, b, c64, tiny = _img(17, 23, 1), _img(37, 53, 2), _img(64, 64, 3), _img(2, 3, 4)
    cs.append(case('pad_ring', 32, [sample(32, [src(a, -3, -4, -2, -5)])]))
    cs.append(case('pad_ring_flip_noswap', 40, [sample(40, [src(a, -3, -4, -2, -5, flip=1, swap_rb=0)])]))
    cs.append(case('pure_crop', 40, [sample(40, [src(b, 5, 7, 3, 4)])]))
    cs.append(case('pure_crop_flip', 32, [sample(32, [src(b, 5, 7, 3, 4, flip=1, pitch_extra=5)])]))
    cs.append(case('mixed_signs', 64, [sample(64, [src(b, -6, 9, 4, -7)])], layout='slot'))
    cs.append(case('mixed_signs_flip', 64, [sample(64, [src(b, -6, 9, 4, -7, flip=1)])]))
    cs.append(case('tiny_source', 32, [sample(32, [src(tiny, -1, 0, 0, -1)])]))
    cs.append(case('crop_1x1', 32, [sample(32, [src(tiny, 1, 1, 1, 0)])]))
    cs.append(case('exact_2x', 32, [sample(32, [src(c64)])]))
    cs.append(case('identity_64', 64, [sample(64, [src(c64)])], exact=True))
    cs.append(case('identity_64_noswap', 64, [sample(64, [src(c64, swap_rb=0, pitch_extra=7)])], layout='nhwc4', exact=True))
    cs.append(case('crop_to_32_flip', 32, [sample(32, [src(b, 10, 11, 2, 3, flip=1)])], exact=True))
    for S in (40, 64):
        lo, hi = int(S * 0.2), int(S * (1 - 0.2))
        for name, cut in (('lo_lo', (lo, lo)), ('hi_hi', (hi, hi)), ('lo_hi', (lo, hi)), ('half', (S // 2, S // 2)),
                          ('abi_0_S', (0, S)), ('abi_S_0', (S, 0))):
            if S == 64 and name not in ('hi_hi', 'half'):
                continue
            cs.append(case('mosaic_%d_%s' % (S, name), S, [sample(S, _mosaic_srcs(), cut)]))
    cs.append(case('mosaic_clamp_left_top', 40, [sample(40, _clamp_srcs(), (32, 32))]))
    cs.append(case('mosaic_clamp_right_bottom', 40, [sample(40, _clamp_srcs(), (8, 8))]))
    cs.append(case('batch3_mixed', 32, [sample(32, [src(a, -3, 2, 1, -2, pitch_extra=3)]),
                                        sample(32, _mosaic_srcs(flip=(1, 0, 1, 0), pitch_extra=2), (13, 20)),
                                        sample(32, [src(c64, 4, -5, -6, 7, flip=1, swap_rb=0)])], layout='slot'))
    col = _colour_img(17, 23, 31)
    cs.append(case('colour_identity', 32, [sample(32, [src(col, -2, 1, 1, -2, color=1)])]))
    cs.append(case('colour_hue_down', 32, [sample(32, [src(col, 0, 0, 0, 0, color=1, dhue=-0.1, dsat=1 / 1.3, dexp=1 / 1.2)])]))
    cs.append(case('colour_hue_up', 32, [sample(32, [src(col, -2, 1, 1, -2, color=1, dhue=0.1, dsat=1.5, dexp=1.5)])]))
    cs.append(case('colour_sat_only', 40, [sample(40, [src(b, 5, 7, 3, 4, flip=1, color=1, dsat=1.5)])]))
    cs.append(case('colour_mosaic', 40, [sample(40, _mosaic_srcs(color=1, dhue=0.07, dsat=1.4, dexp=1 / 1.4), (17, 25))]))
    return cs


CASES = _build()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------- refused argument sets

Y4_ERR_SHAPE, Y4_ERR_NULL = 1, 2
# (name, where, index, field, value, code): one change to the valid case batch3_mixed.  where: 'src' / 'sample' = a field
# of that table's record `index`; 'arg' = an argument of y4_augment_mosaic_u8_f32 (a pointer named here becomes NULL)
REJECTS = [
    ('null_table_dev', 'arg', 0, 'table_dev', None, Y4_ERR_NULL),
    ('null_table_host', 'arg', 0, 'table_host', None, Y4_ERR_NULL),
    ('null_samples_dev', 'arg', 0, 'samples_dev', None, Y4_ERR_NULL),
    ('null_samples_host', 'arg', 0, 'samples_host', None, Y4_ERR_NULL),
    ('null_sums', 'arg', 0, 'sums_dev', None, Y4_ERR_NULL),
    ('null_dst', 'arg', 0, 'dst', None, Y4_ERR_NULL),
    ('null_source', 'src', 2, 'src', None, Y4_ERR_NULL),
    ('B_0', 'arg', 0, 'B', 0, Y4_ERR_SHAPE),
    ('S_0', 'arg', 0, 'S', 0, Y4_ERR_SHAPE),
    ('S_65536', 'arg', 0, 'S', 65536, Y4_ERR_SHAPE),
    ('n_src_2', 'sample', 1, 'n_src', 2, Y4_ERR_SHAPE),
    ('n_src_0', 'sample', 0, 'n_src', 0, Y4_ERR_SHAPE),
    ('first_past_table', 'sample', 1, 'first', 3, Y4_ERR_SHAPE),
    ('crop_w_0', 'src', 1, 'crop_w', 0, Y4_ERR_SHAPE),
    ('crop_h_negative', 'src', 5, 'crop_h', -1, Y4_ERR_SHAPE),
    ('pitch_short', 'src', 3, 'pitch', 3 * 3 - 1, Y4_ERR_SHAPE),
    ('h_0', 'src', 0, 'h', 0, Y4_ERR_SHAPE),
    ('cut_x_negative', 'sample', 1, 'cut_x', -1, Y4_ERR_SHAPE),
    ('cut_y_over_S', 'sample', 1, 'cut_y', 33, Y4_ERR_SHAPE),
    ('window_x_past', 'src', 2, 'win_x', 32, Y4_ERR_SHAPE),
    ('window_y_negative', 'src', 4, 'win_y', -1, Y4_ERR_SHAPE),
    ('window_single_moved', 'src', 0, 'win_x', 1, Y4_ERR_SHAPE),
    ('dhue_nan', 'src', 1, 'dhue', float('nan'), Y4_ERR_SHAPE),
]
# y4_augment_means_u8 on the same table
REJECTS_MEANS = [
    ('null_table_dev', 'arg', 0, 'table_dev', None, Y4_ERR_NULL),
    ('null_table_host', 'arg', 0, 'table_host', None, Y4_ERR_NULL),
    ('null_sums', 'arg', 0, 'sums_dev', None, Y4_ERR_NULL),
    ('n_src_0', 'arg', 0, 'n_src', 0, Y4_ERR_SHAPE),
    ('null_source', 'src', 2, 'src', None, Y4_ERR_NULL),
    ('pitch_short', 'src', 3, 'pitch', 3 * 3 - 1, Y4_ERR_SHAPE),
    ('w_0', 'src', 0, 'w', 0, Y4_ERR_SHAPE),
]


def flat_sources(c):
    """the case's source records in table order, and per sample (cut_x, cut_y, n_src, first)"""
    table, samples = [], []
    for sm in c['samples']:
        samples.append((sm['cut_x'], sm['cut_y'], len(sm['srcs']), len(table)))
        table.extend(sm['srcs'])
    return table, samples


def clone(c):
    return copy.deepcopy(c)
