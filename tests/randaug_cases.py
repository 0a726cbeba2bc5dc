# -*- coding: utf-8 -*-
"""RandAugment's fourteen operations in numpy, and the cases the kernels of csrc/randaug.hip are tested on.

`apply_op` restates, for an 8-bit RGB S x S image, what torchvision's RandAugment(interpolation=NEAREST, fill=None) asks of
Pillow: Image.transform(AFFINE) through libImaging's 16.16 fixed-point path for the five geometric operations,
ImageEnhance's blend with the degenerate image for Brightness / Color / Contrast / Sharpness, and ImageOps' posterize,
solarize, autocontrast and equalize -- as include/yolov4_amd.h states them.  `record` is the parameter mapping (magnitude ->
the integers and the factor the device sees), written here a second time, independent of yolov4_amd/darknet/data.py.
`batch` restates the whole entry point on top of tests/resample_cases.py: plain -> operations -> paste -> normalise.
tests/golden/randaug.npz (tests/golden/make_golden_randaug.py) holds Pillow's pixels for every case;
tests/test_randaug_cases.py pins this file to it and shows that every case reaches the branch it exists for.
"""
import math

import numpy as np

import resample_cases as R

OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness',
       'Posterize', 'Solarize', 'AutoContrast', 'Equalize')
CODE = {name: i for i, name in enumerate(OPS)}
SIGNED = ('ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness')
GEOMETRIC = ('ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate')
ENHANCERS = ('Brightness', 'Color', 'Contrast', 'Sharpness')
NEED_STATS = ('Contrast', 'AutoContrast', 'Equalize')
NBINS = 31


# ------------------------------------------------------------------------------------------------ magnitudes

def bins(name, S, nbins=NBINS):
    """the magnitude table of one operation (None: the operation takes no magnitude)"""
    if name in ('ShearX', 'ShearY'):
        return np.linspace(0.0, 0.3, nbins)
    if name in ('TranslateX', 'TranslateY'):
        return np.linspace(0.0, 150.0 / 331.0 * S, nbins)
    if name == 'Rotate':
        return np.linspace(0.0, 30.0, nbins)
    if name in ENHANCERS:
        return np.linspace(0.0, 0.9, nbins)
    if name == 'Posterize':
        return np.array([8 - int(round(i / ((nbins - 1) / 4.0))) for i in range(nbins)], dtype=np.float64)
    if name == 'Solarize':
        return np.linspace(255.0, 0.0, nbins)
    return None


def magnitude(name, bin_, S, neg=False, nbins=NBINS):
    table = bins(name, S, nbins)
    if table is None:
        return 0.0
    m = float(table[bin_])
    return -m if (neg and name in SIGNED) else m


# ------------------------------------------------------------------------------------------------ parameter mapping

def fix(v):
    t = v * 65536.0 + 0.5
    return int(math.floor(t)) if t < 0.0 else int(t)


def fixed_matrix(a):
    return (fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5))


def inverse_affine(center, translate, shear_deg):
    """torchvision's _get_inverse_affine_matrix(center, 0, translate, 1, shear)"""
    sx, sy = math.radians(shear_deg[0]), math.radians(shear_deg[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(-sy) / math.cos(sy)
    b = -math.cos(-sy) * math.tan(sx) / math.cos(sy)
    c = math.sin(-sy) / math.cos(sy)
    d = -math.sin(-sy) * math.tan(sx) / math.cos(sy) + 1.0
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle, S):
    """Pillow's Image.rotate(angle) for an S x S image"""
    t = -math.radians(angle % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx = cy = S / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def matrix(name, m, S):
    if name == 'ShearX':
        return inverse_affine((0.0, 0.0), (0, 0), (math.degrees(math.atan(m)), 0.0))
    if name == 'ShearY':
        return inverse_affine((0.0, 0.0), (0, 0), (0.0, math.degrees(math.atan(m))))
    if name == 'TranslateX':
        return inverse_affine((S * 0.5, S * 0.5), (int(m), 0), (0.0, 0.0))
    if name == 'TranslateY':
        return inverse_affine((S * 0.5, S * 0.5), (0, int(m)), (0.0, 0.0))
    assert name == 'Rotate'
    return rotate_matrix(m, S)


def record(name, m, S):
    """-> (code, six int32, factor (float32), posterize bits, solarize threshold): what one y4_randaug_op holds"""
    A, factor, bits, thr = (0,) * 6, 0.0, 0, 0
    if name in GEOMETRIC:
        A = fixed_matrix(matrix(name, m, S))
    elif name in ENHANCERS:
        factor = float(np.float32(1.0 + m))
    elif name == 'Posterize':
        bits = int(m)
    elif name == 'Solarize':
        thr = int(math.ceil(m))
    return CODE[name], tuple(A), factor, bits, thr


# ------------------------------------------------------------------------------------------------ the operations

def luma(img):
    w = img.astype(np.int64)
    return (19595 * w[..., 0] + 38470 * w[..., 1] + 7471 * w[..., 2] + 32768) >> 16


def affine_fixed(img, A):
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    sx = (A[2] + A[1] * y + A[0] * x) >> 16
    sy = (A[5] + A[4] * y + A[3] * x) >> 16
    assert max(np.abs(A[2] + A[1] * y + A[0] * x).max(), np.abs(A[5] + A[4] * y + A[3] * x).max()) < 2 ** 31
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.zeros_like(img)
    out[ok] = img[sy[ok], sx[ok]]
    return out


def blend(deg, img, factor):
    """Pillow's ImagingBlend(deg, img, factor) for 8-bit pixels: float32 throughout"""
    a = np.float32(factor)
    d = deg.astype(np.float32)
    t = d + a * (img.astype(np.float32) - d)
    assert t.dtype == np.float32
    if not (np.float32(0.0) <= a <= np.float32(1.0)):
        t = np.where(t <= 0.0, np.float32(0.0), np.where(t >= 255.0, np.float32(255.0), t))
    return t.astype(np.uint8)


def smooth(img):
    """Pillow's ImageFilter.SMOOTH: (1, 1, 1, 1, 5, 1, 1, 1, 1) / 13 in float32; each row of three summed first, the rows
    added from the one below to the one above, starting from 0.5; the one-pixel frame copied"""
    out = img.copy()
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return out
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    f = img.astype(np.float32)

    def row(r, c):
        return (r[:, :-2] * k1 + r[:, 1:-1] * c) + r[:, 2:] * k1

    ss = np.float32(0.5) + row(f[2:], k1)
    ss = ss + row(f[1:-1], k5)
    ss = ss + row(f[:-2], k1)
    assert ss.dtype == np.float32
    ss = np.where(ss <= 0.0, np.float32(0.0), np.where(ss >= 255.0, np.float32(255.0), ss))
    out[1:-1, 1:-1] = ss.astype(np.uint8)
    return out


def contrast_mean(img):
    return int(float(int(luma(img).sum())) / float(img.shape[0] * img.shape[1]) + 0.5)


def autocontrast_lut(h):
    """h: 256 counts of one channel -> its lookup table"""
    occupied = np.flatnonzero(h)
    lo, hi = int(occupied[0]), int(occupied[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], dtype=np.uint8)


def equalize_raw_lut(h):
    """the table before its clip at 255 (None: the identity)"""
    occupied = np.flatnonzero(h)
    if len(occupied) <= 1:
        return None
    step = (int(h.sum()) - int(h[occupied[-1]])) // 255
    if step == 0:
        return None
    lut, n = [], step // 2
    for i in range(256):
        lut.append(n // step)
        n += int(h[i])
    return np.array(lut, dtype=np.int64)


def equalize_lut(h):
    raw = equalize_raw_lut(h)
    return np.arange(256, dtype=np.uint8) if raw is None else np.minimum(raw, 255).astype(np.uint8)


def histogram(img):
    return [np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)]


def apply_op(img, name, m):
    """img [S, S, 3] uint8 RGB -> the same after one operation of magnitude m (signed)"""
    S = img.shape[0]
    code, A, factor, bits, thr = record(name, m, S)
    if name == 'Identity':
        return img.copy()
    if name in GEOMETRIC:
        return affine_fixed(img, A)
    if name == 'Brightness':
        return blend(np.zeros_like(img), img, factor)
    if name == 'Color':
        return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, factor)
    if name == 'Contrast':
        return blend(np.full_like(img, contrast_mean(img)), img, factor)
    if name == 'Sharpness':
        return blend(smooth(img), img, factor)
    if name == 'Posterize':
        return img & np.uint8(~(2 ** (8 - bits) - 1) & 255)
    if name == 'Solarize':
        return np.where(img < thr, img, 255 - img).astype(np.uint8)
    luts = [autocontrast_lut(h) if name == 'AutoContrast' else equalize_lut(h) for h in histogram(img)]
    assert name in ('AutoContrast', 'Equalize')
    return np.stack([luts[c][img[..., c]] for c in range(3)], axis=-1)


def apply_ops(img, ops):
    for name, m in ops:
        img = apply_op(img, name, m)
    return img


# ------------------------------------------------------------------------------------------------ the entry point

def plain_u8(src, s, S):
    """the uint8 RGB S x S image the gather produces for one sample: window, channel order, flip; no paste"""
    cx, cy, cw, ch = s['crop']
    win = R.resample(src[cy:cy + ch, cx:cx + cw], s['res'][0], s['res'][1], s['win'][0], s['win'][1], S, S)
    if s['swap_rb']:
        win = win[:, :, ::-1]
    if s['flip']:
        win = win[:, ::-1]
    return np.ascontiguousarray(win)


def sample_ops(s, S):
    return [(name, magnitude(name, bin_, S, neg)) for name, bin_, neg in s['ops']]


def batch(sources, samples, S, mean=R.MEAN, std=R.STD):
    """-> (aug [B, S, S, 3] uint8 without pastes, out [B, 3, S, S] float32 with them)"""
    aug = [apply_ops(plain_u8(sources[s['src']], s, S), sample_ops(s, S)) for s in samples]
    mixed = [a.copy() for a in aug]
    for b, s in enumerate(samples):
        if s['paste_from'] >= 0:
            x0, y0, x1, y1 = s['paste']
            mixed[b][y0:y1, x0:x1] = aug[s['paste_from']][y0:y1, x0:x1]
    out = np.stack([R.normalise(np.ascontiguousarray(m.transpose(2, 0, 1)), mean, std) for m in mixed])
    return np.stack(aug), out


# ------------------------------------------------------------------------------------------------ sources

# name -> (kind, h, w, seed)
SOURCES = {
    'rand_1': ('random', 1, 1, 21), 'rand_2': ('random', 2, 2, 22), 'rand_3': ('random', 3, 3, 23),
    'two_8': ('twogrey', 8, 8, 24), 'rand_20': ('random', 20, 20, 25), 'flat_16': ('flat', 16, 16, 26),
    'narrow_16': ('narrow', 16, 16, 27), 'rand_37': ('random', 37, 37, 28), 'rand_37b': ('random', 37, 37, 29),
    'smooth_37': ('ramp', 37, 37, 30), 'rand_96': ('random', 96, 96, 31), 'ramp_96': ('ramp', 96, 96, 32),
    'rand_53x37': ('random', 53, 37, 1),
}


def make_source(kind, h, w, seed):
    """[h, w, 3] uint8.  twogrey: two grey levels; flat: one colour; narrow: values in [100, 110]; ramp: a diagonal ramp
    with a little noise, different per channel (its smoothed image differs from it nearly everywhere)"""
    rs = np.random.RandomState(seed)
    if kind == 'random':
        return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == 'twogrey':
        return np.repeat(np.where(rs.randint(0, 2, size=(h, w, 1)) > 0, 200, 40), 3, axis=2).astype(np.uint8)
    if kind == 'flat':
        return np.tile(np.array([90, 17, 201], np.uint8), (h, w, 1))
    if kind == 'narrow':
        return rs.randint(100, 111, size=(h, w, 3)).astype(np.uint8)
    assert kind == 'ramp'
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(2 * yy + xx) % 256, (yy + 3 * xx + 50) % 256, (255 - yy - xx) % 256], axis=-1)
    return np.clip(base + rs.randint(-9, 10, size=(h, w, 3)), 0, 255).astype(np.uint8)


def make_sources():
    return {name: make_source(*spec) for name, spec in SOURCES.items()}


# ------------------------------------------------------------------------------------------------ cases

def _s(src, ops=(), crop=None, res=None, win=(0, 0), flip=0, swap_rb=0, pitch_extra=0, offset=0, paste_from=-1,
       paste=(0, 0, 0, 0)):
    _, h, w, _ = SOURCES[src]
    return dict(src=src, ops=[tuple(o) + (False,) * (3 - len(o)) for o in ops], crop=tuple(crop) if crop else (0, 0, w, h),
                res=res, win=tuple(win), flip=flip, swap_rb=swap_rb, pitch_extra=pitch_extra, offset=offset,
                paste_from=paste_from, paste=tuple(paste))


def _case(S, samples, layout='nchw'):
    n_ops = len(samples[0]['ops'])
    for s in samples:
        assert len(s['ops']) == n_ops
        if s['res'] is None:
            s['res'] = (S, S)
    return dict(S=S, layout=layout, samples=samples, n_ops=n_ops)


def every_op():
    """every operation at bins 0, 9 and 30, both signs where signed: (name, bin, negative)"""
    out = []
    for name in OPS:
        if bins(name, 20) is None:
            out.append((name, 0, False))
            continue
        for b in (0, 9, 30):
            out.append((name, b, False))
            if name in SIGNED and b > 0:
                out.append((name, b, True))
    return out


SMALL_OPS = [('Sharpness', 9), ('Sharpness', 30, True), ('Rotate', 9), ('ShearX', 30), ('TranslateY', 9, True), ('Equalize', 0),
             ('AutoContrast', 0), ('Contrast', 9), ('Color', 30), ('Brightness', 30), ('Solarize', 9), ('Posterize', 30)]
LEVEL_OPS = [('Equalize', 0), ('AutoContrast', 0), ('Contrast', 9), ('Contrast', 30), ('Contrast', 30, True), ('Color', 9),
             ('Sharpness', 30), ('Sharpness', 30, True), ('Brightness', 9, True)]

# name -> case.  ops = [(name, magnitude bin, negative)] per sample; the rest as in resample_cases.CASES.
CASES = {
    # each operation alone, 54 samples of one batch: 400 pixels, two blocks of 256
    'every_op_s20': _case(20, [_s('rand_20', [o]) for o in every_op()]),
    # the 3 x 3 filter's frame with zero, zero and one interior pixel; histograms of 1, 4 and 9 pixels
    's1': _case(1, [_s('rand_1', [o]) for o in SMALL_OPS]),
    's2': _case(2, [_s('rand_2', [o]) for o in SMALL_OPS], layout='nhwc'),
    's3': _case(3, [_s('rand_3', [o]) for o in SMALL_OPS], layout='gaps'),
    # two grey levels in 64 pixels: Equalize's step is 0
    'two_grey_s8': _case(8, [_s('two_8', [o]) for o in LEVEL_OPS]),
    # one colour: AutoContrast's hi <= lo, Equalize's single bin, a smoothed image equal to the image
    'flat_s16': _case(16, [_s('flat_16', [o]) for o in LEVEL_OPS]),
    'narrow_s16': _case(16, [_s('narrow_16', [o]) for o in LEVEL_OPS], layout='nhwc'),
    # chains of two, S odd and no multiple of anything: geometric then Equalize (the black corners enter the histogram),
    # Contrast then Rotate, Equalize then AutoContrast, Sharpness twice (the second reads the first's neighbours); one flipped
    'chains_s37': _case(37, [
        _s('rand_37', [('Rotate', 30), ('Equalize', 0)]),
        _s('smooth_37', [('Contrast', 30), ('Rotate', 9, True)], flip=1),
        _s('narrow_16', [('Equalize', 0), ('AutoContrast', 0)], res=(37, 37)),
        _s('smooth_37', [('Sharpness', 30), ('Sharpness', 30)]),
        _s('rand_37b', [('ShearY', 30, True), ('Sharpness', 9, True)], swap_rb=1, pitch_extra=3, offset=1),
    ], layout='gaps'),
    'three_s37': _case(37, [
        _s('rand_37', [('ShearX', 9), ('Color', 9, True), ('Posterize', 9)]),
        _s('smooth_37', [('Equalize', 0), ('Sharpness', 30), ('TranslateY', 30)], flip=1),
    ]),
    'zero_s37': _case(37, [_s('rand_37'), _s('smooth_37', flip=1, paste_from=0, paste=(5, 7, 30, 20))]),
    # CutMix: every partner has other operations than its receiver; a fixed point would hide nothing, so there is none
    'cutmix_s37': _case(37, [
        _s('rand_37', [('Equalize', 0), ('TranslateX', 9)], paste_from=1, paste=(20, 0, 37, 13)),
        _s('smooth_37', [('Sharpness', 30), ('Contrast', 9, True)], flip=1, paste_from=2, paste=(3, 5, 30, 21)),
        _s('rand_37b', [('Rotate', 9), ('AutoContrast', 0)], swap_rb=1, paste_from=0, paste=(1, 2, 19, 36)),
    ], layout='nhwc'),
    # 96: more than one 64-column tile, 36 blocks of 256 pixels per sample
    'two_s96': _case(96, [
        _s('ramp_96', [('Sharpness', 9), ('Rotate', 9)]),
        _s('rand_96', [('Equalize', 0), ('ShearY', 9)], flip=1, paste_from=0, paste=(60, 10, 96, 70)),
    ]),
    # a crop and a downscale in front, a BGR source: Color must see the OUTPUT channel order
    'crop_s16': _case(16, [_s('rand_53x37', [('Color', 30, True), ('Rotate', 9)], crop=(5, 3, 30, 24), flip=1, swap_rb=1)]),
}

PARAM_FIELDS = R.PARAM_FIELDS


def case_params(c):
    return R.case_params(c)


def case_ops(c):
    """[B, n_ops, 3] int32 (code, bin, negative): what the fixture records of a case's operations"""
    return np.array([[(CODE[n], b, int(neg)) for n, b, neg in s['ops']] for s in c['samples']], dtype=np.int32).reshape(
        len(c['samples']), c['n_ops'], 3)
