# -*- coding: utf-8 -*-
"""The JPEG fixtures (tests/golden/jpeg/, tests/golden/jpeg.npz; written by tests/golden/make_golden_jpeg.py), what each
exists for, and a numpy restatement of the whole decode as include/yolov4_amd.h states it: markers, Huffman decoding,
dequantisation + the "islow" integer IDCT, fancy chroma upsampling, YCbCr -> RGB, EXIF orientation.  Written from ITU-T T.81
and the arithmetic in the header, independent of csrc/jpeg_host.h and csrc/jpeg.hip.

Pixels here are RGB (as the npz); the library's default output is BGR.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
JPEG_DIR = os.path.join(GOLDEN, 'jpeg')

SIZES = [(1, 1), (8, 8), (16, 2), (9, 3), (9, 4), (9, 5), (2, 9), (17, 33), (29, 37), (48, 40)]          # (w, h)
SAMPLING = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}


def _cond(w, h, ncomp, hv, **kw):
    d = dict(width=w, height=h, ncomp=ncomp, hs=hv[0], vs=hv[1], restart=False, orientation=1, dqt16=False, sof=0xC0)
    d.update(kw)
    return d


# name -> the conditions the fixture exists for (checked by parsing the file in test_jpeg_cases.py)
FIXTURES = {}
for _w, _h in SIZES:
    for _n, _hv in SAMPLING.items():
        FIXTURES['s%dx%d_%s' % (_w, _h, _n)] = _cond(_w, _h, 3, _hv)
for _w, _h in [(1, 1), (9, 5), (29, 37), (48, 40)]:
    FIXTURES['gray_%dx%d' % (_w, _h)] = _cond(_w, _h, 1, (1, 1))
for _q in (30, 95, 100):
    FIXTURES['q%d_29x37_420' % _q] = _cond(29, 37, 3, (2, 2))
FIXTURES['opt_48x40_420'] = _cond(48, 40, 3, (2, 2), optimized=True)
FIXTURES['rst_48x40_420'] = _cond(48, 40, 3, (2, 2), restart=True)
FIXTURES['rst_48x40_444'] = _cond(48, 40, 3, (1, 1), restart=True)
FIXTURES['rst_gray_48x40'] = _cond(48, 40, 1, (1, 1), restart=True)
FIXTURES['q16_29x37_420'] = _cond(29, 37, 3, (2, 2), dqt16=True, sof=0xC1)
FIXTURES['narrow_4x6_420'] = _cond(4, 6, 3, (2, 2))          # chroma planes exactly 2 wide: the last width without the filter
FIXTURES['narrow_3x5_422'] = _cond(3, 5, 3, (2, 1))
FIXTURES['wide_300x9_420'] = _cond(300, 9, 3, (2, 2))          # wider than one 256-pixel workgroup of the colour kernel
for _o in range(1, 9):
    FIXTURES['orient%d_13x21' % _o] = _cond(13, 21, 3, (2, 2), orientation=_o)
ORIENT = ['orient%d_13x21' % o for o in range(1, 9)]
UNSUPPORTED = ['progressive_17x33', 'cmyk_9x5']
SUPPORTED = sorted(FIXTURES)

# the edge conditions of the pixel stage and the fixtures that must meet them
NARROW_CHROMA = ['s1x1_420', 's1x1_422', 's2x9_420', 's2x9_422', 'narrow_4x6_420', 'narrow_3x5_422']   # subsampled, dw <= 2
WIDE_CHROMA_ODD = ['s9x3_420', 's9x5_422', 's17x33_420', 's29x37_422']              # dw > 2 and odd width / height
ODD = ['s9x3_444', 's9x5_420', 's17x33_422', 's29x37_420', 'gray_29x37']


def read(name):
    with open(os.path.join(JPEG_DIR, name + '.jpg'), 'rb') as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ markers

NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
           28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
           47, 55, 62, 63]


def _u16(b, o):
    return (b[o] << 8) | b[o + 1]


def _exif_orientation(seg):
    if seg[:6] != b'Exif\0\0':
        return None
    t = seg[6:]
    le = t[:2] == b'II'
    rd = lambda o, n: int.from_bytes(t[o:o + n], 'little' if le else 'big')
    ifd = rd(4, 4)
    for i in range(rd(ifd, 2)):
        e = ifd + 2 + 12 * i
        if rd(e, 2) == 0x0112:
            v = rd(e + 8, 2)
            return v if 1 <= v <= 8 else 1
    return 1


def parse(data):
    """-> dict: width, height, ncomp, comps [(id, hs, vs, tq)], qt {t: 64 natural}, dqt16, huff {(class, id): {bits: sym}},
    restart_interval, orientation, sof (marker byte), n_dht (segments), scan (td, ta per component), scan_start"""
    assert data[:2] == b'\xff\xd8'
    out = dict(qt={}, huff={}, restart_interval=0, orientation=1, dqt16=False, n_dht=0, sof=None)
    pos = 2
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        ln = _u16(data, pos)
        seg = data[pos + 2:pos + ln]
        if m in (0xC0, 0xC1, 0xC2):
            out['sof'] = m
            out['precision'], out['height'], out['width'], out['ncomp'] = seg[0], _u16(seg, 1), _u16(seg, 3), seg[5]
            out['comps'] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, t = seg[o] >> 4, seg[o] & 15
                vals = [_u16(seg, o + 1 + 2 * i) if pq else seg[o + 1 + i] for i in range(64)]
                tab = [0] * 64
                for i, v in enumerate(vals):
                    tab[NATURAL[i]] = v
                out['qt'][t] = tab
                out['dqt16'] |= bool(pq)
                o += 1 + (128 if pq else 64)
        elif m == 0xC4:
            out['n_dht'] += 1
            o = 0
            while o < len(seg):
                tc, th = seg[o] >> 4, seg[o] & 15
                counts = list(seg[o + 1:o + 17])
                syms = seg[o + 17:o + 17 + sum(counts)]
                table, code, k = {}, 0, 0
                for l in range(1, 17):
                    for _ in range(counts[l - 1]):
                        table[format(code, '0%db' % l)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                out['huff'][(tc, th)] = table
                o += 17 + sum(counts)
        elif m == 0xDD:
            out['restart_interval'] = _u16(seg, 0)
        elif m == 0xE1:
            v = _exif_orientation(seg)
            if v is not None:
                out['orientation'] = v
        elif m == 0xDA:
            ns = seg[0]
            out['scan_ncomp'] = ns
            out['scan'] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            out['scan_start'] = pos + ln
            return out
        pos += ln


def geometry(p):
    """the padded block grid of each component: [(blocks_w, blocks_h)], and the MCU grid"""
    if p['ncomp'] == 1:
        hv = [(1, 1)]
    else:
        hv = [(c[1], c[2]) for c in p['comps']]
    hmax, vmax = hv[0]
    mx, my = -(-p['width'] // (8 * hmax)), -(-p['height'] // (8 * vmax))
    return hv, mx, my, [(mx * h, my * v) for h, v in hv]


# ------------------------------------------------------------------------------------------------ entropy decoding

def _segments(data, start):
    """the entropy-coded data split at RSTn, unstuffed, as bit strings; and the RSTn numbers met"""
    segs, rst, cur, pos = [], [], bytearray(), start
    while True:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
        elif data[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
        elif 0xD0 <= data[pos + 1] <= 0xD7:
            segs.append(cur)
            rst.append(data[pos + 1] - 0xD0)
            cur = bytearray()
            pos += 2
        elif data[pos + 1] == 0xFF:
            pos += 1
        else:
            segs.append(cur)
            break
    return [''.join(format(b, '08b') for b in s) for s in segs], rst


_entropy_cache = {}


def entropy(data):
    """-> (coef int16 [coef_count] in the library's layout, qt uint16 [3][64], parse dict)"""
    key = bytes(data)
    if key in _entropy_cache:
        return _entropy_cache[key]
    p = parse(data)
    hv, mx, my, grids = geometry(p)
    ncomp = p['ncomp']
    comps = [np.zeros((bh, bw, 64), dtype=np.int16) for bw, bh in grids]
    segs, rst = _segments(data, p['scan_start'])
    ri = p['restart_interval']
    assert rst == [i % 8 for i in range(len(rst))]
    assert len(segs) == (-(-(mx * my) // ri) if ri else 1)
    dc_tabs = [p['huff'][(0, p['scan'][c][0])] for c in range(ncomp)]
    ac_tabs = [p['huff'][(1, p['scan'][c][1])] for c in range(ncomp)]

    def symbol(bits, at, table):
        for l in range(1, 17):
            s = table.get(bits[at:at + l])
            if s is not None and at + l <= len(bits):
                return s, at + l
        raise ValueError('code not in table')

    def extend(bits, at, s):
        if s == 0:
            return 0, at
        v = int(bits[at:at + s], 2)
        assert at + s <= len(bits)
        return (v if v >= 1 << (s - 1) else v - (1 << s) + 1), at + s

    done = 0
    for seg_i, bits in enumerate(segs):
        at, pred = 0, [0] * ncomp
        n_here = min(ri, mx * my - done) if ri else mx * my
        for _ in range(n_here):
            my_i, mx_i = divmod(done, mx)
            for c in range(ncomp):
                for by in range(hv[c][1]):
                    for bx in range(hv[c][0]):
                        blk = comps[c][my_i * hv[c][1] + by, mx_i * hv[c][0] + bx]
                        s, at = symbol(bits, at, dc_tabs[c])
                        v, at = extend(bits, at, s)
                        pred[c] += v
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs, at = symbol(bits, at, ac_tabs[c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            assert k <= 63
                            v, at = extend(bits, at, s)
                            blk[NATURAL[k]] = v
                            k += 1
            done += 1
        assert len(bits) - at < 8 and set(bits[at:]) <= {'1'}, 'padding of ones to the byte boundary'
    coef = np.concatenate([c.reshape(-1) for c in comps])
    qt = np.zeros((3, 64), dtype=np.uint16)
    for c in range(ncomp):
        qt[c] = p['qt'][p['comps'][c][3]]
    _entropy_cache[key] = (coef, qt, p)
    return _entropy_cache[key]


# ------------------------------------------------------------------------------------------------ pixels

def _islow_1d(x):
    """one pass of jidctint's jpeg_idct_islow over a list of eight integer arrays; the caller descales"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = x[0], x[4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_plane(coef_blocks, qt):
    """coef_blocks int16 [bh, bw, 64], qt [64] -> uint8 plane [8 bh, 8 bw]"""
    bh, bw, _ = coef_blocks.shape
    d = coef_blocks.astype(np.int64).reshape(bh, bw, 8, 8) * np.asarray(qt, dtype=np.int64).reshape(8, 8)
    cols = [_descale(v, 11) for v in _islow_1d([d[:, :, k, :] for k in range(8)])]       # [k]: row k of the workspace
    ws = np.stack(cols, axis=2)                                                           # [bh, bw, row, col]
    rows = [_descale(v, 18) for v in _islow_1d([ws[:, :, :, k] for k in range(8)])]      # [k]: column k of the output
    px = np.clip(np.stack(rows, axis=3) + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p):
    """[dh, dw] real samples -> [dh, 2 dw]"""
    p = p.astype(np.int32)
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.zeros((dh, 2 * dw), dtype=np.int32)
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def upsample_h2v2(p):
    """[dh, dw] real samples -> [2 dh, 2 dw]"""
    p = p.astype(np.int32)
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    cs = np.zeros((2 * dh, dw), dtype=np.int32)
    cs[0::2] = 3 * p + above
    cs[1::2] = 3 * p + below
    out = np.zeros((2 * dh, 2 * dw), dtype=np.int32)
    out[:, 2::2] = (3 * cs[:, 1:] + cs[:, :-1] + 8) >> 4
    out[:, 1:-1:2] = (3 * cs[:, :-1] + cs[:, 1:] + 7) >> 4
    out[:, 0] = (4 * cs[:, 0] + 8) >> 4
    out[:, -1] = (4 * cs[:, -1] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def orient(img, o):
    """EXIF orientation o applied to an HWC image"""
    if o == 2:
        return img[:, ::-1]
    if o == 3:
        return img[::-1, ::-1]
    if o == 4:
        return img[::-1]
    if o == 5:
        return img.transpose(1, 0, 2)
    if o == 6:
        return img.transpose(1, 0, 2)[:, ::-1]
    if o == 7:
        return img[::-1, ::-1].transpose(1, 0, 2)
    if o == 8:
        return img.transpose(1, 0, 2)[::-1]
    return img


def pixels_from_coefficients(coef, qt, width, height, ncomp, hs, vs, orientation=1):
    """the pixel stage on a coefficient buffer in the library's layout -> RGB HWC uint8"""
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    grids = [(mx * hs, my * vs)] + [(mx, my)] * (ncomp - 1)
    planes, at = [], 0
    for c, (bw, bh) in enumerate(grids):
        n = bw * bh * 64
        planes.append(idct_plane(np.asarray(coef[at:at + n]).reshape(bh, bw, 64), qt[c]))
        at += n
    y = planes[0][:height, :width]
    if ncomp == 1:
        rgb = np.stack([y, y, y], axis=2)
    else:
        dw, dh = -(-width // hs), -(-height // vs)
        up = {(1, 1): lambda p: p, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(hs, vs)]
        cb, cr = (up(pl[:dh, :dw])[:height, :width] for pl in planes[1:])
        rgb = ycc_to_rgb(y, cb, cr)
    return np.ascontiguousarray(orient(rgb, orientation))


def decode(data, apply_orientation=True):
    """bytes -> RGB HWC uint8"""
    coef, qt, p = entropy(data)
    hv = geometry(p)[0]
    return pixels_from_coefficients(coef, qt, p['width'], p['height'], p['ncomp'], hv[0][0], hv[0][1],
                                    p['orientation'] if apply_orientation else 1)
