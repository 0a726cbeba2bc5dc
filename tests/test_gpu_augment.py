# -*- coding: utf-8 -*-
"""The training augmentation kernels of csrc/augment.hip -- y4_augment_means_u8 and y4_augment_mosaic_u8_f32 -- driven
through the C ABI on every case of tests/augment_cases.py (references, acceptance criterion K * 2^-24 and case list are
there; tests/test_augment_cases.py shows without a GPU that every case reaches its branch), then through the public
interface (`train_batch`, `Transform`).

Every device buffer -- sources, descriptor table, sums, destination -- lies between two guards of a NaN bit pattern no
kernel produces; source pitch padding and everything around the destination slot hold the same pattern and must still
hold it afterwards.  Sums are compared bit for bit, the pixels of the `exact` cases too; every other pixel within the
bound, and each test prints the share of the bound it used.  Refused calls return their codes and write nothing.
The no-scratch check of the two kernels is compile-only and runs without a GPU.

Largest share of the bound used on an MI355X (every test prints its own): 0.180 in colour_hue_up (hue wrapped above 360 with
s > 1 and v over 255), 0.150 through train_batch, 0.113 in colour_sat_only, at most 0.032 without the HSV step; the exact
cases are bit-exact.  The whole file takes under 3 s; the slowest test, test_train_batch_equals_the_reference, 0.4 s."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import augment_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from kernel_resources import kernel_resources  # noqa: E402

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
G = 128                                  # guard bytes in front of and behind every device buffer
SENT_BYTES = np.array([A.SENT], np.uint32).view(np.uint8)
USED = {}
CFG = {'AUGMENTATION': {'JITTER': 0.3, 'RANDOM_HORIZONTAL_FLIP': True, 'COLOR_DITHERING': True, 'HUE': 0.1,
                        'SATURATION': 1.5, 'EXPOSURE': 1.5, 'IS_MOSAIC': True, 'MIN_OFFSET': 0.2},
       'DATA': {'MAX_NUM_LABELS': 60}}


def test_augment_kernels_use_no_scratch():
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'augment.hip'), ())
    names = [r['name'].split('(')[0] for r in rows]
    assert any('augment_sums_kernel' in n for n in names) and any('augment_mosaic_kernel' in n for n in names), names
    bad = [(r['name'].split('(')[0], r['scratch'], r['vgpr_spill']) for r in rows if r['scratch'] != 0 or r['vgpr_spill'] != 0]
    assert not bad, bad
    assert all(r['lds'] == 0 for r in rows), 'byte-gather work: no LDS'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import lib
    return lib(), ops._stream


def _note(group, used, what=''):
    m = float(np.max(used)) if np.size(used) else 0.0
    USED[group] = max(USED.get(group, 0.0), m)
    print('%s %s: share of the bound used %.3f; group maximum so far %.3f' % (group, what, m, USED[group]))


class Bytes(object):
    """n bytes on the device between two guards; body = the sentinel pattern unless `init` (uint8) is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        h = np.resize(SENT_BYTES, self.n + 2 * G)
        if init is not None:
            h[G:G + self.n] = np.ascontiguousarray(init, dtype=np.uint8).ravel()
        self.before = h.copy()
        self.t = torch.from_numpy(h).to(dev)

    def ptr(self, off=0):
        return self.t.data_ptr() + G + off

    def get(self):
        h = self.t.cpu().numpy()
        assert np.array_equal(h[:G], self.before[:G]) and np.array_equal(h[G + self.n:], self.before[G + self.n:]), \
            'write outside the buffer'
        return h[G:G + self.n].copy()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before)


class Launch(object):
    """device copies of one case: sources at their pitches, the descriptor table, sums and the destination"""

    def __init__(self, dev, c):
        from yolov4_amd._lib import AugSample, AugSrc
        self.c, self.S, self.B = c, c['S'], len(c['samples'])
        table, samples = A.flat_sources(c)
        self.n = len(table)
        self.imgs = []
        self.srcs = (AugSrc * self.n)()
        self.samples = (AugSample * self.B)()
        for i, s in enumerate(table):
            pitch = 3 * s['w'] + s['pitch_extra']
            rows = np.resize(SENT_BYTES, (s['h'], pitch)).copy()       # pitch padding holds the pattern too
            rows[:, :3 * s['w']] = s['img'].reshape(s['h'], 3 * s['w'])
            buf = Bytes(dev, rows.size, rows)
            self.imgs.append(buf)
            r = self.srcs[i]
            r.src, r.h, r.w, r.pitch, r.swap_rb = buf.ptr(), s['h'], s['w'], pitch, s['swap_rb']
            r.crop_left, r.crop_top, r.crop_w, r.crop_h, r.flip = s['crop_left'], s['crop_top'], s['crop_w'], s['crop_h'], s['flip']
            r.color, r.dhue, r.dsat, r.dexp, r.win_x, r.win_y = s['color'], s['dhue'], s['dsat'], s['dexp'], s['win_x'], s['win_y']
        for b, (cx, cy, n, first) in enumerate(samples):
            sm = self.samples[b]
            sm.cut_x, sm.cut_y, sm.n_src, sm.first = cx, cy, n, first
        self.dev = dev
        self.sums = Bytes(dev, 24 * self.n)
        total, self.off, self.strides = A.dst_layout(c['layout'], self.B, self.S)
        self.total = total
        self.dst = Bytes(dev, 4 * total)
        self.upload()

    def upload(self):
        """(re)build the device table from the host records"""
        self.src_bytes = ctypes.sizeof(self.srcs)
        raw = np.concatenate([np.frombuffer(self.srcs, dtype=np.uint8), np.frombuffer(self.samples, dtype=np.uint8)])
        self.table = Bytes(self.dev, raw.size, raw)

    def args_means(self):
        return dict(table_dev=self.table.ptr(), table_host=ctypes.addressof(self.srcs), n_src=self.n, sums_dev=self.sums.ptr())

    def args_mosaic(self):
        sb, sc, sh, sw = self.strides
        return dict(table_dev=self.table.ptr(), table_host=ctypes.addressof(self.srcs), n_table=self.n,
                    samples_dev=self.table.ptr(self.src_bytes), samples_host=ctypes.addressof(self.samples), B=self.B,
                    sums_dev=self.sums.ptr(), dst=self.dst.ptr(4 * self.off), dst_sb=sb, dst_sc=sc, dst_sh=sh, dst_sw=sw,
                    S=self.S)

    def means(self, **over):
        L, stream = _abi()
        a = dict(self.args_means(), **over)
        return L.y4_augment_means_u8(a['table_dev'], a['table_host'], a['n_src'], a['sums_dev'], stream())

    def mosaic(self, **over):
        L, stream = _abi()
        a = dict(self.args_mosaic(), **over)
        return L.y4_augment_mosaic_u8_f32(a['table_dev'], a['table_host'], a['n_table'], a['samples_dev'], a['samples_host'],
                                          a['B'], a['sums_dev'], a['dst'], a['dst_sb'], a['dst_sc'], a['dst_sh'], a['dst_sw'],
                                          a['S'], stream())

    def got_sums(self):
        return self.sums.get().view(np.uint64).reshape(self.n, 3)

    def got_pixels(self):
        """the [B, 3, S, S] view as fp32; every other word of the buffer still holds the sentinel"""
        words = self.dst.get().view(np.uint32)
        idx = A.dst_index(self.c['layout'], self.B, self.S)
        around = np.ones(self.total, bool)
        around[idx.ravel()] = False
        assert (words[around] == A.SENT).all(), 'write beside the destination slot'
        return words[idx].view(F32)

    def inputs_unchanged(self):
        return all(b.unchanged() for b in self.imgs) and self.table.unchanged()


def _check(L, ref):
    c = L.c
    sums = L.got_sums()
    want = np.array([A.channel_sums(s) for s in A.flat_sources(c)[0]], dtype=np.uint64)
    assert np.array_equal(sums, want), (c['name'], 'sums', sums.tolist(), want.tolist())
    got = L.got_pixels()
    assert L.inputs_unchanged(), 'a source or the table was written'
    err = np.abs(got.astype(F64) - ref)
    assert np.isfinite(got).all(), (c['name'], 'a pixel was not written')
    if c['exact']:
        same = got.view(np.uint32) == ref.astype(F32).view(np.uint32)
        assert same.all(), (c['name'], 'first differing elements', np.argwhere(~same)[:5].tolist())
    used = err.max() / (A.K * A.UNIT)
    _note('augment', used, c['name'])
    bad = np.argwhere(err > A.K * A.UNIT)[:5]
    assert used <= 1, (c['name'], [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad])


@gpu
@pytest.mark.parametrize('name', [c['name'] for c in A.CASES])
def test_case_through_the_c_abi(dev, name):
    c = A.BY_NAME[name]
    L = Launch(dev, c)
    assert L.means() == 0
    assert L.mosaic() == 0                               # no synchronisation between the two launches
    torch.cuda.synchronize()
    _check(L, A.render(c, F64))


@gpu
def test_sums_do_not_depend_on_what_was_there(dev):
    """the call zeroes the totals itself: a second call gives the same sums"""
    L = Launch(dev, A.BY_NAME['batch3_mixed'])
    assert L.means() == 0 and L.means() == 0
    torch.cuda.synchronize()
    want = np.array([A.channel_sums(s) for s in A.flat_sources(L.c)[0]], dtype=np.uint64)
    assert np.array_equal(L.got_sums(), want)


def _mutated(dev, where, idx, fld, value):
    L = Launch(dev, A.clone(A.BY_NAME['batch3_mixed']))
    over = {}
    if where == 'arg':
        over[fld] = value
    else:
        rec = (L.srcs if where == 'src' else L.samples)[idx]
        setattr(rec, fld, value)
        L.upload()
    return L, over


@gpu
@pytest.mark.parametrize('rej', A.REJECTS, ids=[r[0] for r in A.REJECTS])
def test_refused_mosaic_calls(dev, rej):
    _, where, idx, fld, value, code = rej
    L, over = _mutated(dev, where, idx, fld, value)
    assert L.mosaic(**over) == code
    torch.cuda.synchronize()
    assert L.dst.unchanged() and L.sums.unchanged(), 'a refused call wrote something'


@gpu
@pytest.mark.parametrize('rej', A.REJECTS_MEANS, ids=[r[0] for r in A.REJECTS_MEANS])
def test_refused_means_calls(dev, rej):
    _, where, idx, fld, value, code = rej
    L, over = _mutated(dev, where, idx, fld, value)
    assert L.means(**over) == code
    torch.cuda.synchronize()
    assert L.sums.unchanged() and L.dst.unchanged(), 'a refused call wrote something'


# ---------------------------------------------------------------------------------------------- public interface

def _params_of(sm):
    from yolov4_amd.yolo.data.transform import AugParams, MosaicParams
    return MosaicParams(cut_x=sm['cut_x'], cut_y=sm['cut_y'], tiles=[
        AugParams(crop_left=s['crop_left'], crop_right=s['crop_right'], crop_top=s['crop_top'], crop_bottom=s['crop_bottom'],
                  flip=bool(s['flip']), color=bool(s['color']), dhue=s['dhue'], dsat=s['dsat'], dexp=s['dexp'])
        for s in sm['srcs']])


def _public_case():
    S = 40
    a, b = A._colour_img(17, 23, 41), A._img(37, 53, 42)
    samples = [A.sample(S, [A.src(a, -3, 2, 1, -2, flip=1, color=1, dhue=-0.06, dsat=1.3, dexp=1 / 1.2)]),
               A.sample(S, A._mosaic_srcs(color=1, dhue=0.04, dsat=1 / 1.4, dexp=1.3), (29, 11)),
               A.sample(S, [A.src(b, 4, -5, -6, 7)])]
    return A.case('public', S, samples)


@gpu
def test_train_batch_equals_the_reference(dev):
    from yolov4_amd.yolo.data import transform as T
    c = _public_case()
    items, params = [], []
    for i, sm in enumerate(c['samples']):
        imgs = [s['img'] for s in sm['srcs']]
        if i == 2:
            imgs = [torch.from_numpy(imgs[0]).to(dev)]                # a tensor already on the device
        boxes = [np.array([[1.0, 2.0, s['w'] / 2, s['h'] / 2, q]]) for q, s in enumerate(sm['srcs'])]
        items.append((imgs, boxes))
        params.append(_params_of(sm))
    wide = torch.full((3, 3, c['S'] + 2, c['S'] + 3), float('nan'), device=dev)
    out = wide[:, :, 1:1 + c['S'], 2:2 + c['S']]
    x, labels = T.train_batch(items, c['S'], CFG, params=params, out=out)
    assert x.data_ptr() == out.data_ptr() and x.shape == (3, 3, c['S'], c['S']) and x.dtype == torch.float32 and x.is_cuda
    torch.cuda.synchronize()
    ref = A.render(c, F64)
    used = np.abs(x.cpu().numpy().astype(F64) - ref).max() / (A.K * A.UNIT)
    _note('train_batch', used)
    assert used <= 1
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[:, :, 1:1 + c['S'], 2:2 + c['S']] = False
    assert torch.isnan(wide[mask]).all(), 'write beside the output slot'
    assert labels.shape == (3, 60, 5) and labels.dtype == torch.float64 and not labels.is_cuda
    for i, sm in enumerate(c['samples']):
        want = T.sample_labels(items[i][1], [(s['h'], s['w']) for s in sm['srcs']], params[i], c['S'], 60)
        assert np.array_equal(labels[i].numpy(), want)
    # sample 2 by hand: crop 54 x 36 at (4, -6); the box x 1..27.5 -> 0..23.5 (cut), y 2..20.5 -> 8..26.5
    assert np.allclose(labels[2, 0].numpy(), [23.5 * 40 / 54 / 2, (8 + 26.5) * 40 / 36 / 2, 23.5 * 40 / 54, 18.5 * 40 / 36, 0],
                       rtol=0, atol=1e-12)
    assert not labels[2, 1:].any()
    # drawn parameters: shapes, range, and the labels stay inside the image
    x2, lab2 = T.train_batch(items, c['S'], CFG)
    torch.cuda.synchronize()
    assert x2.shape == x.shape and float(x2.min()) >= 0 and float(x2.max()) <= 1 and torch.isfinite(x2).all()
    assert float(lab2[..., :4].max()) <= c['S']


@gpu
def test_transform_contract(dev):
    from yolov4_amd.yolo.data import transform as T
    S = 64
    imgs = [A._img(37, 53, 50 + i) for i in range(4)]
    boxes = [np.array([[5.0, 6.0, 20.0, 15.0, 3.0], [30.0, 10.0, 15.0, 20.0, 7.0]]) for _ in range(4)]
    img, target = T.Transform(CFG, is_train=True)(imgs, boxes, S)
    torch.cuda.synchronize()
    lab = target['padded_labels']
    assert img.shape == (3, S, S) and img.dtype == torch.float32 and img.is_cuda and target['img_info'] == []
    assert float(img.min()) >= 0 and float(img.max()) <= 1 and torch.isfinite(img).all()
    assert lab.shape == (60, 5) and lab.dtype == torch.float64 and not lab.is_cuda
    valid = lab[:, 2] > 0
    assert (lab[~valid] == 0).all() and float(lab[:, :4].max()) <= S and float(lab.min()) >= 0
    single = dict(CFG, AUGMENTATION=dict(CFG['AUGMENTATION'], IS_MOSAIC=False))
    img1, t1 = T.Transform(single, is_train=True)(imgs[:1], boxes[:1], S)
    assert img1.shape == (3, S, S) and t1['padded_labels'].shape == (60, 5)
    # evaluation: the existing path, bit for bit
    img_v, tv = T.Transform(CFG, is_train=False)(imgs[:1], boxes[:1], S)
    want, info = T.val_transform(imgs[0], S)
    torch.cuda.synchronize()
    assert torch.equal(img_v, want) and tv['img_info'] == info == [37, 53, S, S]
    sx, sy = S / 53, S / 37
    assert np.allclose(tv['padded_labels'][0].numpy(), [(5 + 10) * sx, (6 + 7.5) * sy, 20 * sx, 15 * sy, 3], rtol=0, atol=1e-12)
    assert not tv['padded_labels'][2:].any()
