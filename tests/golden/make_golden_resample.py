# -*- coding: utf-8 -*-
"""Writes tests/golden/resample.npz: the synthetic sources of tests/resample_cases.py, Pillow's
Image.crop(box).resize((res_w, res_h), Image.BILINEAR) pixels for every sample of every case, and the case parameters.

    python tests/golden/make_golden_resample.py

Needs Pillow and numpy only.  Keys: src_<source>, pil_<case>_<sample> ([res_h, res_w, 3] uint8, the WHOLE resampled crop in
the source's channel order), par_<case> ([B, 18] int32, resample_cases.PARAM_FIELDS), pillow_version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_cases as R  # noqa: E402


def pillow_resized(src, s):
    cx, cy, cw, ch = s['crop']
    im = Image.fromarray(src, 'RGB').crop((cx, cy, cx + cw, cy + ch)).resize(tuple(s['res']), Image.BILINEAR)
    return np.asarray(im, dtype=np.uint8)


def main():
    sources = R.make_sources()
    out = {'src_' + k: v for k, v in sources.items()}
    for name, c in R.CASES.items():
        out['par_' + name] = R.case_params(c)
        for b, s in enumerate(c['samples']):
            out['pil_%s_%d' % (name, b)] = pillow_resized(sources[s['src']], s)
    out['pillow_version'] = np.array([int(v) for v in PIL.__version__.split('.')[:3]], dtype=np.int32)
    path = os.path.join(HERE, 'resample.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes, Pillow', PIL.__version__)


if __name__ == '__main__':
    main()
