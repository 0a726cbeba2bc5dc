# -*- coding: utf-8 -*-
"""Writes the JPEG fixtures: tests/golden/jpeg/*.jpg and tests/golden/jpeg.npz (PIL's decoded pixels, RGB, HWC uint8).

    python tests/golden/make_golden_jpeg.py

Needs Pillow built on libjpeg-turbo (the decoder whose arithmetic include/yolov4_amd.h restates).  Reads nothing but its own
synthetic images.  What each fixture is for is stated in tests/jpeg_cases.py (FIXTURES), which the tests check by parsing.

The 16-bit DQT case: Pillow clamps quality-scaled tables to 8 bits (force_baseline), so no quality setting emits one; custom
`qtables` with entries above 255 do (the file then carries SOF1), and that is how `q16_*` is made.
"""
import io
import os

import numpy as np
from PIL import Image, ImageOps, features

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'jpeg')

SIZES = [(1, 1), (8, 8), (16, 2), (9, 3), (9, 4), (9, 5), (2, 9), (17, 33), (29, 37), (48, 40)]      # (w, h)
SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def picture(w, h, seed):
    """smooth colour gradients, a hard edge and mild noise: every coefficient band is exercised, the files stay small"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 170 * x / max(w - 1, 1), 220 - 180 * y / max(h - 1, 1), 128 + 100 * np.sin(x / 3.0 + y / 5.0)], axis=2)
    img[(x + 2 * y) % 11 < 2] = (250, 10, 30)
    img[h // 2:, : w // 3] = img[h // 2:, : w // 3][..., ::-1]
    img += rng.randn(h, w, 3) * 6
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(arr, mode='RGB', **kw):
    if mode == 'L':
        im = Image.fromarray(arr[..., 1])
    elif mode == 'CMYK':
        im = Image.fromarray(arr).convert('CMYK')
    else:
        im = Image.fromarray(arr)
    buf = io.BytesIO()
    im.save(buf, format='JPEG', **kw)
    return buf.getvalue()


def main():
    assert features.check_feature('libjpeg_turbo'), 'the fixtures pin libjpeg-turbo arithmetic'
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for i, (w, h) in enumerate(SIZES):
        for name, ss in SUBSAMPLING.items():
            files['s%dx%d_%s' % (w, h, name)] = encode(picture(w, h, 100 + i), quality=75, subsampling=ss)
    for i, (w, h) in enumerate([(1, 1), (9, 5), (29, 37), (48, 40)]):
        files['gray_%dx%d' % (w, h)] = encode(picture(w, h, 200 + i), 'L', quality=75)
    for q in (30, 95, 100):
        files['q%d_29x37_420' % q] = encode(picture(29, 37, 300 + q), quality=q, subsampling=2)
    files['opt_48x40_420'] = encode(picture(48, 40, 400), quality=75, subsampling=2, optimize=True)
    files['rst_48x40_420'] = encode(picture(48, 40, 500), quality=75, subsampling=2, restart_marker_blocks=3)
    files['rst_48x40_444'] = encode(picture(48, 40, 501), quality=75, subsampling=0, restart_marker_blocks=3)
    files['rst_gray_48x40'] = encode(picture(48, 40, 502), 'L', quality=75, restart_marker_blocks=3)
    ramp = [min(12 + 9 * k, 600) for k in range(64)]
    files['q16_29x37_420'] = encode(picture(29, 37, 600), qtables=[ramp, ramp], subsampling=2)
    files['narrow_4x6_420'] = encode(picture(4, 6, 650), quality=75, subsampling=2)
    files['narrow_3x5_422'] = encode(picture(3, 5, 651), quality=75, subsampling=1)
    files['wide_300x9_420'] = encode(picture(300, 9, 660), quality=50, subsampling=2)
    base = picture(13, 21, 700)
    for o in range(1, 9):
        exif = Image.Exif()
        exif[0x0112] = o
        files['orient%d_13x21' % o] = encode(base, quality=90, subsampling=2, exif=exif)
    files['progressive_17x33'] = encode(picture(17, 33, 800), quality=75, progressive=True)
    files['cmyk_9x5'] = encode(picture(9, 5, 900), 'CMYK', quality=75)

    pixels = {}
    for name, data in sorted(files.items()):
        with open(os.path.join(OUT, name + '.jpg'), 'wb') as f:
            f.write(data)
        if name.startswith('cmyk'):
            continue
        im = Image.open(io.BytesIO(data))
        pixels[name] = np.asarray(im.convert('RGB'))
        if name.startswith('orient'):
            pixels[name + '__raw'] = pixels[name]
            pixels[name] = np.asarray(ImageOps.exif_transpose(im).convert('RGB'))
    np.savez_compressed(os.path.join(HERE, 'jpeg.npz'), **pixels)
    print('%d files, %d bytes (largest %d); %d arrays' % (len(files), sum(map(len, files.values())),
                                                           max(map(len, files.values())), len(pixels)))


if __name__ == '__main__':
    main()
