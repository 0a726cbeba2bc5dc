# -*- coding: utf-8 -*-
"""Writes the JPEG encoder fixtures: tests/golden/jpegenc.npz, synthetic pixel arrays and the bytes Pillow's `save` gives for
them (`<name>__px`: RGB HWC uint8, or HW for gray; `<name>__jpg`: the file as a uint8 vector).

    python tests/golden/make_golden_jpegenc.py

Needs Pillow built on libjpeg-turbo (the encoder whose arithmetic include/yolov4_amd.h restates).  Reads nothing but its own
synthetic images.  tests/jpegenc_cases.py lists the cases (CASES) and what each is for.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_jpeg import picture          # noqa: E402  (the same generator as the decoder's fixtures)
from jpegenc_cases import CASES               # noqa: E402

SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def saturated(w, h, seed):
    """pure 0 / 255 primaries in 8x8 checker cells: the largest coefficients the colour transform can give"""
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 2, (-(-h // 8), -(-w // 8), 3)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(cells, 8, axis=0), 8, axis=1)[:h, :w])


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures pin libjpeg-turbo arithmetic'
    out = {}
    total = 0
    for i, (name, c) in enumerate(sorted(CASES.items())):
        w, h = c['width'], c['height']
        px = saturated(w, h, 1000 + i) if c['kind'] == 'saturated' else picture(w, h, 1000 + i)
        buf = io.BytesIO()
        if c['sampling'] is None:
            px = np.ascontiguousarray(px[..., 1])
            Image.fromarray(px).save(buf, format='JPEG', quality=c['quality'])
        else:
            Image.fromarray(px).save(buf, format='JPEG', quality=c['quality'], subsampling=SUBSAMPLING[c['sampling']])
        out[name + '__px'] = px
        out[name + '__jpg'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
        total += len(buf.getvalue())
    np.savez_compressed(os.path.join(HERE, 'jpegenc.npz'), **out)
    print('%d cases, %d JPEG bytes' % (len(CASES), total))


if __name__ == '__main__':
    main()
