# -*- coding: utf-8 -*-
"""The JPEG encoder fixtures (tests/golden/jpegenc.npz; written by tests/golden/make_golden_jpegenc.py), what each exists
for, and a numpy restatement of the compression arithmetic as include/yolov4_amd.h states it: quality-scaled tables, RGB ->
YCbCr, edge replication and chroma downsampling, the "islow" integer FDCT, quantisation, and the rule for dummy blocks.
Written from ITU-T T.81 and the arithmetic in the header, independent of csrc/jpeg_enc_host.h and csrc/jpeg_enc.hip.

Pixels here are RGB (as the npz); the library reads BGR unless swap_rb is set.
"""
import numpy as np

SIZES = [(1, 1), (8, 8), (16, 16), (9, 5), (17, 33), (29, 37), (33, 17), (48, 40), (50, 9), (300, 9)]      # (w, h)
SAMPLING = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}


def _case(w, h, sampling, quality, kind='picture'):
    return dict(width=w, height=h, sampling=sampling, quality=quality, kind=kind)


# name -> what the case is: sampling None is gray (one component)
CASES = {}
for _w, _h in SIZES:
    for _s in SAMPLING:
        CASES['e%dx%d_%s' % (_w, _h, _s)] = _case(_w, _h, _s, 75)
for _q in (1, 30, 95, 100):
    CASES['eq%d_29x37_420' % _q] = _case(29, 37, '420', _q)
for _w, _h in [(1, 1), (9, 5), (29, 37)]:
    CASES['egray_%dx%d' % (_w, _h)] = _case(_w, _h, None, 75)
CASES['esat_40x24_420'] = _case(40, 24, '420', 100, 'saturated')       # FF stuffing and the largest magnitudes
NAMES = sorted(CASES)
# the conditions some cases exist for
RIGHT_DUMMY = ['e17x33_420', 'e17x33_422', 'e33x17_420']       # luma width_in_blocks odd: a dummy block column
BOTTOM_DUMMY = ['e48x40_420', 'e17x33_420', 'e33x17_420']      # luma height_in_blocks odd at 4:2:0: a dummy block row

# ITU-T T.81 Annex K tables K.1 and K.2, natural (row-major) order
LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
        80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
        95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
          99, 99, 99] + [99] * 32


def quality_tables(quality):
    """-> uint16 [2][64]: luminance and chrominance tables at this quality, natural order"""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.array([[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (LUMA, CHROMA)], dtype=np.uint16)


def geometry(w, h, ncomp, hs, vs):
    """-> mcus_x, mcus_y, padded block grids [(bw, bh)] and real block grids [(width_in_blocks, height_in_blocks)]"""
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    fac = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    grids = [(mx * a, my * b) for a, b in fac]
    real = [(-(-(-(-w * a // hs)) // 8), -(-(-(-h * b // vs)) // 8)) for a, b in fac]
    return mx, my, grids, real


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_cols(p, width):
    return np.concatenate([p, np.repeat(p[:, -1:], width - p.shape[1], axis=1)], axis=1) if width > p.shape[1] else p


def _pad_rows(p, height):
    return np.concatenate([p, np.repeat(p[-1:], height - p.shape[0], axis=0)], axis=0) if height > p.shape[0] else p


def component_plane(p, h_c, v_c, hs, vs, my):
    """full-resolution plane [h, w] of one component -> the samples of its real blocks, [8 my v_c, 8 width_in_blocks]"""
    h, w = p.shape
    p = _pad_rows(p, -(-h // vs) * vs)                                           # 1. rows to a multiple of vs
    wib = -(-(-(-w * h_c // hs)) // 8)
    p = _pad_cols(p, 8 * wib * (hs // h_c))                                      # 2. columns
    fx, fy = hs // h_c, vs // v_c
    if (fx, fy) == (2, 2):                                                       # 3. downsample
        bias = np.tile(np.array([1, 2]), p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif (fx, fy) == (2, 1):
        bias = np.tile(np.array([0, 1]), p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    else:
        assert (fx, fy) == (1, 1)
    return _pad_rows(p, 8 * my * v_c)                                            # 4. the last downsampled row, down


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of the "islow" forward DCT over a list of eight int64 arrays"""
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z = (t12 + t13) * 4433
    o[2] = _descale(z + t13 * 6270, n)
    o[6] = _descale(z - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return o


def fdct_quantise(plane, qt):
    """samples [8 bh, 8 bw] -> quantised coefficients int16 [bh, bw, 64]"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128          # [bh, bw, row, col]
    rows = np.stack(_fdct_1d([d[..., k] for k in range(8)], True), axis=3)                # along each row
    cols = np.stack(_fdct_1d([rows[:, :, k, :] for k in range(8)], False), axis=2)        # along each column
    div = 8 * np.asarray(qt, dtype=np.int64).reshape(8, 8)
    a = np.abs(cols) + (div >> 1)
    q = np.where(a >= div, a // div, 0) * np.sign(cols)
    return q.reshape(bh, bw, 64).astype(np.int16)


def coefficients(px, sampling, quality, fill_dummies=True):
    """px: RGB [h, w, 3] or gray [h, w] uint8; sampling: '444' / '422' / '420' (ignored for gray)
    -> (coef int16 [coef_count] in the library's layout, real bool [coef_count], qt uint16 [3][64]).
    Dummy blocks hold the values the scan codes for them (DC of the block coded just before in the same MCU, AC zero) with
    fill_dummies, else zeros; `real` is False there."""
    gray = px.ndim == 2
    h, w = px.shape[:2]
    ncomp = 1 if gray else 3
    hs, vs = (1, 1) if gray else SAMPLING[sampling]
    mx, my, grids, real_grids = geometry(w, h, ncomp, hs, vs)
    tabs = quality_tables(quality)
    qt = np.zeros((3, 64), dtype=np.uint16)
    planes = [px.astype(np.int64)] if gray else list(rgb_to_ycc(px))
    comps, masks = [], []
    for c in range(ncomp):
        h_c, v_c = (hs, vs) if c == 0 else (1, 1)
        qt[c] = tabs[0 if c == 0 else 1]
        bw, bh = grids[c]
        rw, rh = real_grids[c]
        blocks = np.zeros((bh, bw, 64), dtype=np.int16)
        samples = component_plane(planes[c], h_c, v_c, hs, vs, my)
        blocks[:, :rw] = fdct_quantise(samples, qt[c])
        mask = np.zeros((bh, bw, 64), dtype=bool)
        mask[:rh, :rw] = True
        blocks[~mask] = 0
        if fill_dummies:
            for m_y in range(my):
                for m_x in range(mx):
                    last = 0
                    for by in range(v_c):
                        for bx in range(h_c):
                            y, x = m_y * v_c + by, m_x * h_c + bx
                            if mask[y, x, 0]:
                                last = blocks[y, x, 0]
                            else:
                                blocks[y, x, 0] = last
        comps.append(blocks.reshape(-1))
        masks.append(mask.reshape(-1))
    return np.concatenate(comps), np.concatenate(masks), qt
