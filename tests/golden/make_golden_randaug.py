# -*- coding: utf-8 -*-
"""Writes tests/golden/randaug.npz: the synthetic sources of tests/randaug_cases.py, Pillow's pixels for every sample of
every case after its RandAugment operations, and the case parameters.

    python tests/golden/make_golden_randaug.py

Needs Pillow and numpy only.  `pillow_op` is what torchvision's RandAugment._apply_op asks of Pillow for one operation
(interpolation NEAREST, fill None).  Keys: src_<source>, pil_<case>_<sample> ([S, S, 3] uint8 RGB: crop -> resize -> window ->
channel order -> flip -> operations, all by Pillow), par_<case> ([B, 18] int32, resample_cases.PARAM_FIELDS), ops_<case>
([B, n_ops, 3] int32: code, magnitude bin, negative), pillow_version."""
import math
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import randaug_cases as RA  # noqa: E402


def _affine(im, center, translate, shear_deg):
    return im.transform(im.size, Image.AFFINE, RA.inverse_affine(center, translate, shear_deg), Image.NEAREST)


def pillow_op(im, name, m):
    """one operation of torchvision.transforms.RandAugment on a PIL RGB image (torchvision's affine matrix is restated in
    randaug_cases.inverse_affine; everything after the matrix is Pillow's)"""
    w, h = im.size
    if name == 'Identity':
        return im
    if name == 'ShearX':
        return _affine(im, (0.0, 0.0), (0, 0), (math.degrees(math.atan(m)), 0.0))
    if name == 'ShearY':
        return _affine(im, (0.0, 0.0), (0, 0), (0.0, math.degrees(math.atan(m))))
    if name == 'TranslateX':
        return _affine(im, (w * 0.5, h * 0.5), (int(m), 0), (0.0, 0.0))
    if name == 'TranslateY':
        return _affine(im, (w * 0.5, h * 0.5), (0, int(m)), (0.0, 0.0))
    if name == 'Rotate':
        return im.rotate(m, Image.NEAREST)
    if name == 'Brightness':
        return ImageEnhance.Brightness(im).enhance(1.0 + m)
    if name == 'Color':
        return ImageEnhance.Color(im).enhance(1.0 + m)
    if name == 'Contrast':
        return ImageEnhance.Contrast(im).enhance(1.0 + m)
    if name == 'Sharpness':
        return ImageEnhance.Sharpness(im).enhance(1.0 + m)
    if name == 'Posterize':
        return ImageOps.posterize(im, int(m))
    if name == 'Solarize':
        return ImageOps.solarize(im, m)
    if name == 'AutoContrast':
        return ImageOps.autocontrast(im)
    assert name == 'Equalize'
    return ImageOps.equalize(im)


def pillow_ops(rgb, ops):
    im = Image.fromarray(np.ascontiguousarray(rgb), 'RGB')
    for name, m in ops:
        im = pillow_op(im, name, m)
    return np.asarray(im, dtype=np.uint8)


def pillow_sample(src, s, S):
    cx, cy, cw, ch = s['crop']
    mem = src[:, :, ::-1] if s['swap_rb'] else src
    im = Image.fromarray(np.ascontiguousarray(mem), 'RGB').crop((cx, cy, cx + cw, cy + ch)).resize(tuple(s['res']), Image.BILINEAR)
    wx, wy = s['win']
    im = im.crop((wx, wy, wx + S, wy + S))
    if s['flip']:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return pillow_ops(np.asarray(im), RA.sample_ops(s, S))


def main():
    sources = RA.make_sources()
    out = {'src_' + k: v for k, v in sources.items()}
    for name, c in RA.CASES.items():
        out['par_' + name] = RA.case_params(c)
        out['ops_' + name] = RA.case_ops(c)
        for b, s in enumerate(c['samples']):
            out['pil_%s_%d' % (name, b)] = pillow_sample(sources[s['src']], s, c['S'])
    out['pillow_version'] = np.array([int(v) for v in PIL.__version__.split('.')[:3]], dtype=np.int32)
    path = os.path.join(HERE, 'randaug.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes, Pillow', PIL.__version__)


if __name__ == '__main__':
    main()
