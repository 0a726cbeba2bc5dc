# -*- coding: utf-8 -*-
"""The ImageNet input pipeline's arithmetic in numpy, and the cases the kernels of csrc/resample.hip are tested on.

`coeffs` / `resample` restate Pillow's Image.crop(box).resize((res_w, res_h), Image.BILINEAR) for 8-bit RGB as
include/yolov4_amd.h states it (libImaging's precompute_coeffs, normalize_coeffs_8bpc and the two 8-bit passes); Python floats
are IEEE doubles and Python never fuses a multiply-add, so the tables are Pillow's bit for bit.  `plain_batch` / `batch`
restate crop -> window -> flip -> paste -> normalise.  Written from the header's statement, independent of the kernels.
tests/golden/resample.npz (tests/golden/make_golden_resample.py) holds the synthetic sources and Pillow's pixels for every
case; tests/test_resample_cases.py pins this file to it and shows that every case reaches the branch it exists for.
"""
import math

import numpy as np

PREC = 22
SENT = 0x7FC5A5A5                   # a NaN bit pattern no kernel produces
MEAN = np.array([0.485 * 255, 0.456 * 255, 0.406 * 255], dtype=np.float32)
STD = np.array([0.229 * 255, 0.224 * 255, 0.225 * 255], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the arithmetic

def ksize(n_in, n_out):
    scale = float(n_in) / float(n_out)
    return int(math.ceil(max(scale, 1.0))) * 2 + 1


def coeffs(n_in, n_out, win, count):
    """-> (bounds [count, 2] int32 = (xmin, n), k [count, ksize] int32) for resampled indices win .. win + count - 1"""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((count, 2), dtype=np.int32)
    k = np.zeros((count, ks), dtype=np.int32)
    for i in range(count):
        center = (win + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, n)
        k[i, :n] = [int(0.5 + v * 4194304.0) for v in w]
    return bounds, k


def _pass(img, bounds, k):
    """one 8-bit pass along axis 1 of img [rows, n_in, 3] -> [rows, count, 3] uint8"""
    out = np.empty((img.shape[0], len(bounds), 3), dtype=np.uint8)
    wide = img.astype(np.int64)
    for i, (xmin, n) in enumerate(bounds):
        acc = (wide[:, xmin:xmin + n, :] * k[i, :n].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PREC - 1))
        assert np.abs(acc).max() < 2 ** 31, 'the kernels accumulate in int32'
        out[:, i, :] = np.clip(acc >> PREC, 0, 255)
    return out


def resample(crop, res_w, res_h, win_x=0, win_y=0, out_w=None, out_h=None):
    """crop [h, w, 3] uint8 -> the out_h x out_w window at (win_y, win_x) of the crop resampled to res_h x res_w"""
    out_w = res_w if out_w is None else out_w
    out_h = res_h if out_h is None else out_h
    h, w = crop.shape[:2]
    bx, kx = coeffs(w, res_w, win_x, out_w)
    by, ky = coeffs(h, res_h, win_y, out_h)
    hor = _pass(crop, bx, kx)                                           # [h, out_w, 3]
    return _pass(hor.transpose(1, 0, 2), by, ky).transpose(1, 0, 2)      # [out_h, out_w, 3]


def normalise(u8_chw, mean=MEAN, std=STD):
    return (u8_chw.astype(np.float32) - mean[:, None, None]) / std[:, None, None]


def plain_sample(src, s, S, mean=MEAN, std=STD):
    """one sample without its paste: src [h, w, 3] uint8 in memory order -> [3, S, S] float32"""
    cx, cy, cw, ch = s['crop']
    win = resample(src[cy:cy + ch, cx:cx + cw], s['res'][0], s['res'][1], s['win'][0], s['win'][1], S, S)
    if s['swap_rb']:
        win = win[:, :, ::-1]
    if s['flip']:
        win = win[:, ::-1]
    return normalise(np.ascontiguousarray(win.transpose(2, 0, 1)), mean, std)


def plain_batch(sources, samples, S, mean=MEAN, std=STD):
    return np.stack([plain_sample(sources[s['src']], s, S, mean, std) for s in samples])


def batch(sources, samples, S, mean=MEAN, std=STD):
    plain = plain_batch(sources, samples, S, mean, std)
    out = plain.copy()
    for b, s in enumerate(samples):
        if s['paste_from'] >= 0:
            x0, y0, x1, y1 = s['paste']
            out[b, :, y0:y1, x0:x1] = plain[s['paste_from'], :, y0:y1, x0:x1]
    return plain, out


# ------------------------------------------------------------------------------------------------ sources

# name -> (kind, h, w, seed)
SOURCES = {
    'rand_53x37': ('random', 53, 37, 1),
    'bin_53x37': ('binary', 53, 37, 2),
    'chk_53x37': ('checker', 53, 37, 0),
    'rand_7x9': ('random', 7, 9, 3),
    'bin_7x9': ('binary', 7, 9, 4),
    'rand_17x300': ('random', 17, 300, 5),
    'bin_17x300': ('binary', 17, 300, 6),
    'rand_4x5': ('random', 4, 5, 7),
    'rand_23x16': ('random', 23, 16, 8),
    'rand_19x20': ('random', 19, 20, 9),
    'chk_41x50': ('checker', 41, 50, 0),
    'rand_33x40': ('random', 33, 40, 10),
    'bin_33x40': ('binary', 33, 40, 11),
    'rand_300x17': ('random', 300, 17, 12),
}


def make_source(kind, h, w, seed):
    """[h, w, 3] uint8.  binary: only 0 and 255 (the largest intermediate swings); checker: a 1-pixel checkerboard whose
    phase differs per channel (every 2-tap average is a rounding tie)"""
    if kind == 'random':
        return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == 'binary':
        return (np.random.RandomState(seed).randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    assert kind == 'checker'
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((yy + xx + c) % 2) * 255 for c in range(3)], axis=-1).astype(np.uint8)


def make_sources():
    return {name: make_source(*spec) for name, spec in SOURCES.items()}


# ------------------------------------------------------------------------------------------------ cases

def _s(src, crop=None, res=None, win=(0, 0), flip=0, swap_rb=0, pitch_extra=0, offset=0, paste_from=-1, paste=(0, 0, 0, 0)):
    _, h, w, _ = SOURCES[src]
    return dict(src=src, crop=tuple(crop) if crop else (0, 0, w, h), res=res, win=tuple(win), flip=flip, swap_rb=swap_rb,
                pitch_extra=pitch_extra, offset=offset, paste_from=paste_from, paste=tuple(paste))


def _case(S, samples, layout='nchw'):
    for s in samples:
        if s['res'] is None:
            s['res'] = (S, S)
    return dict(S=S, layout=layout, samples=samples)


# name -> case.  crop = (x, y, w, h); res = (res_w, res_h); win = (win_x, win_y); paste = (x0, y0, x1, y1).
CASES = {
    # 37 wide, 53 high -> 16: downscale 2.3 / 3.3, ksize 7 / 9
    'down_whole': _case(16, [_s('rand_53x37')]),
    'down_whole_swap': _case(16, [_s('rand_53x37', swap_rb=1)]),
    'down_whole_binary': _case(16, [_s('bin_53x37', swap_rb=1)]),
    'down_whole_checker': _case(16, [_s('chk_53x37')]),
    # Pillow box (5, 3, 35, 27)
    'down_crop': _case(16, [_s('rand_53x37', crop=(5, 3, 30, 24))]),
    'down_crop_flip': _case(16, [_s('rand_53x37', crop=(5, 3, 30, 24), flip=1, swap_rb=1)]),
    'down_crop_pitch': _case(16, [_s('bin_53x37', crop=(5, 3, 30, 24), pitch_extra=5, offset=1)], layout='gaps'),
    # 9 x 7 -> 16: upscale, fs = 1, 3 taps, edge taps clamped to n < ksize
    'up': _case(16, [_s('rand_7x9')]),
    'up_binary_flip': _case(16, [_s('bin_7x9', flip=1, pitch_extra=1)], layout='nhwc'),
    # 290 x 13 crop of a 300 x 17 source -> 8: ksize 75 on x
    'long_taps': _case(8, [_s('rand_17x300', crop=(4, 2, 290, 13))]),
    'long_taps_binary': _case(8, [_s('bin_17x300', crop=(4, 2, 290, 13), swap_rb=1, offset=3)], layout='gaps'),
    # ... and the same on y: one tile of 8 output rows walks all 290 source rows
    'long_taps_y': _case(8, [_s('rand_300x17', crop=(2, 4, 13, 290), flip=1)]),
    'one_pixel': _case(8, [_s('rand_4x5', crop=(2, 1, 1, 1))]),
    # the identity pass: on x only (16 x 23 -> 16), and on both axes (16 x 16 crop -> 16)
    'identity_x': _case(16, [_s('rand_23x16')]),
    'identity_both': _case(16, [_s('rand_19x20', crop=(3, 2, 16, 16), flip=1)]),
    # S = 33: neither a tile nor a wave
    'odd_size': _case(33, [_s('chk_41x50', swap_rb=1)], layout='nhwc'),
    # the validation geometry: 40 x 33 -> 48 x 39, the central 32 x 32 window
    'val_window': _case(32, [_s('rand_33x40', res=(48, 39), win=(8, 4), swap_rb=1)]),
    'val_window_binary': _case(32, [_s('bin_33x40', res=(48, 39), win=(8, 4), pitch_extra=2)], layout='nhwc'),
    # five samples of mixed sizes; the partners are the permutation (2, 1, 4, 0, 3): a fixed point (1 <- 1), a rectangle on two
    # borders (0), an empty one (3), a flipped partner under an unflipped receiver (2 <- 4); every partner has a paste of its
    # own, which the receiver must not see
    'cutmix': _case(33, [
        _s('rand_53x37', paste_from=2, paste=(20, 0, 33, 13)),
        _s('bin_7x9', flip=1, paste_from=1, paste=(3, 5, 30, 21)),
        _s('rand_17x300', crop=(4, 2, 290, 13), swap_rb=1, paste_from=4, paste=(1, 2, 19, 32)),
        _s('chk_41x50', paste_from=0, paste=(7, 9, 7, 30)),
        _s('rand_33x40', res=(48, 39), win=(9, 3), flip=1, swap_rb=1, pitch_extra=3, offset=1, paste_from=3,
           paste=(15, 16, 33, 33)),
    ], layout='gaps'),
    'cutmix_nhwc': _case(16, [
        _s('rand_53x37', crop=(5, 3, 30, 24), paste_from=1, paste=(0, 0, 16, 16)),
        _s('rand_23x16', flip=1),
        _s('bin_53x37', swap_rb=1, paste_from=0, paste=(4, 0, 12, 16)),
    ], layout='nhwc'),
}
SINGLE = sorted(n for n, c in CASES.items() if len(c['samples']) == 1)
BATCHES = sorted(n for n, c in CASES.items() if len(c['samples']) > 1)

PARAM_FIELDS = ('crop_x', 'crop_y', 'crop_w', 'crop_h', 'res_w', 'res_h', 'win_x', 'win_y', 'flip', 'swap_rb', 'pitch_extra',
                'offset', 'paste_from', 'paste_x0', 'paste_y0', 'paste_x1', 'paste_y1', 'S')


def case_params(c):
    """[B, 18] int32: what the fixture records of a case"""
    return np.array([list(s['crop']) + list(s['res']) + list(s['win']) + [s['flip'], s['swap_rb'], s['pitch_extra'], s['offset'],
                                                                          s['paste_from']] + list(s['paste']) + [c['S']]
                     for s in c['samples']], dtype=np.int32)


def dst_layout(layout, B, S):
    """-> (elements of the buffer, offset of element [0, 0, 0, 0], (sb, sc, sh, sw)) in fp32 elements"""
    if layout == 'nchw':
        return 3 * B * S * S, 0, (3 * S * S, S * S, S, 1)
    if layout == 'nhwc':
        return 3 * B * S * S, 0, (3 * S * S, 1, 3 * S, 3)
    assert layout == 'gaps'                # gaps between pixels, rows, planes and samples, and a margin on both ends
    sw = 2
    sh = sw * S + 3
    sc = sh * S + 5
    sb = 3 * sc + 7
    return 11 + B * sb + 13, 11, (sb, sc, sh, sw)


def dst_index(layout, B, S):
    """[B, 3, S, S] int64: the buffer element every output element goes to"""
    _, off, (sb, sc, sh, sw) = dst_layout(layout, B, S)
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(S), np.arange(S), indexing='ij')
    return off + b * sb + c * sc + y * sh + x * sw


def job_bytes(s, S):
    """bytes of one job's tables in the workspace"""
    words = S * (2 + ksize(s['crop'][2], s['res'][0])) + S * (2 + ksize(s['crop'][3], s['res'][1]))
    return (4 * words + 15) & ~15


def job_tables(s, S):
    """the int32 words of one job's tables, as the workspace holds them (without the padding to 16 bytes)"""
    bx, kx = coeffs(s['crop'][2], s['res'][0], s['win'][0], S)
    by, ky = coeffs(s['crop'][3], s['res'][1], s['win'][1], S)
    return np.concatenate([bx.ravel(), kx.ravel(), by.ravel(), ky.ravel()]).astype(np.int32)
