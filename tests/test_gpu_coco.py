# -*- coding: utf-8 -*-
"""The COCO evaluation kernels of csrc/coco_eval.hip -- y4_coco_match_f64 and y4_coco_accumulate_f64 -- through the C ABI on
every case of tests/coco_cases.py (restatement, cases and acceptance are there; tests/test_coco_cases.py shows without a
GPU that every case reaches its branch), then through `COCOEvaluator` and `validate()`.

Every device buffer lies between two guards of a sentinel byte pattern that must survive, inputs must come back unchanged,
and every output word is written.  Match codes, npig, precision, recall and the 12 statistics are compared with
`array_equal`: every entry is an integer or one IEEE fp64 quotient of integers.  Refused calls return their codes and
write nothing; a second run gives the same bytes."""
import ctypes

import numpy as np
import pytest
import torch

import coco_cases as C

gpu = pytest.mark.gpu
G = 256                                             # guard bytes in front of and behind every device buffer
SENT = 0xA5
NAMES = [c['name'] for c in C.CASES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


class Buf(object):
    """a numpy array on the device between two guards; without `init` the body holds the sentinel too"""

    def __init__(self, dev, shape, dtype, init=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        h = np.full(self.n + 2 * G, SENT, np.uint8)
        if init is not None:
            h[G:G + self.n] = np.ascontiguousarray(init, dtype=self.dtype).reshape(-1).view(np.uint8)
        self.before = h.copy()
        self.t = torch.from_numpy(h).to(dev)

    def ptr(self):
        return self.t.data_ptr() + G

    def get(self):
        h = self.t.cpu().numpy()
        assert np.array_equal(h[:G], self.before[:G]) and np.array_equal(h[G + self.n:], self.before[G + self.n:]), \
            'write outside the buffer'
        return h[G:G + self.n].copy().view(self.dtype).reshape(self.shape)

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before)


class Launch(object):
    """device copies of one case, laid out from the restatement's own cell order and the evaluator's gt packing"""

    def __init__(self, dev, c):
        from yolov4_amd._lib import lib
        from yolov4_amd.yolo.util import cocoeval as E
        self.c, self.ref = c, C.reference(c['name'])
        r = self.ref
        p = E.COCOEvaluator(c['ann']).pack(c['records'], c['image_ids'])
        self.p = p
        self.n_cells, self.K, self.n_det, self.n_gt = p['n_cells'], p['n_cat'], len(r['kept']), len(p['g_area'])
        assert np.array_equal(p['det_off'], r['det_off']) and list(zip(p['cell_cat'], p['cell_img'])) == r['cells']
        recs = c['records']
        kbox = np.array([recs[j]['bbox'] for j in r['kept']], np.float64).reshape(-1, 4)
        kscore = np.array([recs[j]['score'] for j in r['kept']], np.float64)
        cell_of = np.repeat(np.arange(self.n_cells), np.diff(r['det_off']))
        rank = (np.arange(self.n_det) - r['det_off'][:-1][cell_of]).astype(np.uint8)
        kcat = p['cell_cat'][cell_of]
        o1 = np.argsort(-kscore, kind='stable')
        order = o1[np.argsort(kcat[o1], kind='stable')].astype(np.int32)
        self.host = {'det_off': p['det_off'].copy(), 'gt_off': p['gt_off'].copy(), 'cat_off': p['cat_off'].copy(),
                     'max_dets': np.array(C.MAXDETS, np.int32)}
        self.cell_cat = p['cell_cat']
        nz = lambda n: max(int(n), 1)                                                                      # noqa: E731
        b = lambda shape, dt, init=None: Buf(dev, shape, dt, init)                                         # noqa: E731
        self.inp = {'dbox': b((nz(self.n_det), 4), np.float64, kbox if self.n_det else None),
                    'det_off': b((self.n_cells + 1,), np.int32, p['det_off']),
                    'gbox': b((nz(self.n_gt), 4), np.float64, p['g_box'] if self.n_gt else None),
                    'garea': b((nz(self.n_gt),), np.float64, p['g_area'] if self.n_gt else None),
                    'gcrowd': b((nz(self.n_gt),), np.int32, p['g_crowd'] if self.n_gt else None),
                    'gt_off': b((self.n_cells + 1,), np.int32, p['gt_off']),
                    'iou': b((10,), np.float64, E.IOU_THRS), 'area': b((4, 2), np.float64, E.AREA_RNG),
                    'rec': b((101,), np.float64, E.REC_THRS),
                    'rank': b((nz(self.n_det),), np.uint8, rank if self.n_det else None),
                    'order': b((nz(self.n_det),), np.int32, order if self.n_det else None),
                    'cat_off': b((self.K + 1,), np.int32, p['cat_off'])}
        self.codes = b((4, nz(self.n_det)), np.uint32)
        self.npig = b((nz(self.n_cells), 4), np.int32)
        longest = int(np.diff(p['gt_off']).max()) if self.n_cells else 0
        self.ws_bytes = int(lib().y4_coco_workspace(self.n_cells, longest))
        self.ws = b((nz(self.ws_bytes),), np.uint8)
        self.npig_cat = None
        self.precision = b((10, 101, self.K, 4, 3), np.float64)
        self.recall = b((10, self.K, 4, 3), np.float64)
        self.dev = dev

    def match(self, **over):
        from yolov4_amd import ops
        from yolov4_amd._lib import lib
        i, h = self.inp, self.host
        a = dict(dbox=i['dbox'].ptr(), det_off=i['det_off'].ptr(), det_off_host=h['det_off'].ctypes.data, n_det=self.n_det,
                 gbox=i['gbox'].ptr(), garea=i['garea'].ptr(), gcrowd=i['gcrowd'].ptr(), gt_off=i['gt_off'].ptr(),
                 gt_off_host=h['gt_off'].ctypes.data, n_gt=self.n_gt, n_cells=self.n_cells, iou=i['iou'].ptr(),
                 area=i['area'].ptr(), codes=self.codes.ptr(), npig=self.npig.ptr(),
                 ws=self.ws.ptr() if self.ws_bytes else None, ws_bytes=self.ws_bytes)
        a.update(over)
        return lib().y4_coco_match_f64(a['dbox'], a['det_off'], a['det_off_host'], a['n_det'], a['gbox'], a['garea'], a['gcrowd'],
                                       a['gt_off'], a['gt_off_host'], a['n_gt'], a['n_cells'], a['iou'], a['area'], a['codes'],
                                       a['npig'], a['ws'], a['ws_bytes'], ops._stream())

    def set_npig_cat(self, npig):
        s = np.zeros((self.K, 4), np.int64)
        np.add.at(s, self.cell_cat, npig.astype(np.int64))
        self.npig_cat = Buf(self.dev, (max(self.K, 1), 4), np.int64, s if self.K else None)

    def accumulate(self, **over):
        from yolov4_amd import ops
        from yolov4_amd._lib import lib
        i, h = self.inp, self.host
        a = dict(codes=self.codes.ptr(), rank=i['rank'].ptr(), order=i['order'].ptr(), n_det=self.n_det,
                 cat_off=i['cat_off'].ptr(), cat_off_host=h['cat_off'].ctypes.data, npig_cat=self.npig_cat.ptr(), n_cat=self.K,
                 rec=i['rec'].ptr(), max_dets=h['max_dets'].ctypes.data, precision=self.precision.ptr(),
                 recall=self.recall.ptr())
        a.update(over)
        return lib().y4_coco_accumulate_f64(a['codes'], a['rank'], a['order'], a['n_det'], a['cat_off'], a['cat_off_host'],
                                            a['npig_cat'], a['n_cat'], a['rec'], a['max_dets'], a['precision'], a['recall'],
                                            ops._stream())

    def inputs_unchanged(self):
        return all(b.unchanged() for b in self.inp.values())

    def got_match(self):
        return self.codes.get()[:, :self.n_det], self.npig.get()[:self.n_cells]


def _run(dev, name):
    L = Launch(dev, C.BY_NAME[name])
    assert L.match() == 0
    torch.cuda.synchronize()
    codes, npig = L.got_match()
    L.set_npig_cat(npig)
    assert L.accumulate() == 0
    torch.cuda.synchronize()
    return L, codes, npig, L.precision.get(), L.recall.get()


@gpu
@pytest.mark.parametrize('name', NAMES)
def test_case_through_the_c_abi(dev, name):
    L, codes, npig, precision, recall = _run(dev, name)
    r = L.ref
    assert L.inputs_unchanged(), 'an input was written'
    if L.ws_bytes:
        L.ws.get()                                  # guards of the workspace
    assert np.array_equal(npig, r['npig']), (name, 'npig')
    same = codes == r['codes']
    assert same.all(), (name, 'codes differ at (area, row)', np.argwhere(~same)[:5].tolist())
    assert np.array_equal(recall, r['recall']), (name, 'recall', np.argwhere(recall != r['recall'])[:5].tolist())
    assert np.array_equal(precision, r['precision']), (name, 'precision', np.argwhere(precision != r['precision'])[:5].tolist())


@gpu
@pytest.mark.parametrize('name', ['many_gts', 'long_cat', 'random_2'])
def test_second_run_gives_the_same_bytes(dev, name):
    a, b = _run(dev, name), _run(dev, name)
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


@gpu
@pytest.mark.parametrize('name', NAMES)
def test_stats_through_the_evaluator(dev, name):
    from yolov4_amd.yolo.util.cocoeval import COCOEvaluator
    c, r = C.BY_NAME[name], C.reference(name)
    ev = COCOEvaluator(c['ann'], device=dev)
    got = ev(c['records'], c['image_ids'])
    assert np.array_equal(ev.precision, r['precision']) and np.array_equal(ev.recall, r['recall'])
    assert ev.stats.dtype == np.float64 and np.array_equal(ev.stats, r['stats'])
    assert got == (float(r['stats'][0]), float(r['stats'][1]))
    assert len(ev.summary().split('\n')) == 12
    if 'bad_records' in c:
        with pytest.raises(ValueError):
            ev(c['bad_records'], c['image_ids'])


@gpu
def test_empty_records_are_evaluated(dev):
    from yolov4_amd.yolo.util.cocoeval import COCOEvaluator
    c = C.BY_NAME['perfect']
    ev = COCOEvaluator(c['ann'], device=dev)
    assert ev([], c['image_ids']) == (0.0, 0.0)
    want = C.evaluate(c['ann'], [], c['image_ids'])
    assert np.array_equal(ev.precision, want['precision']) and np.array_equal(ev.stats, want['stats'])
    assert (ev.precision == 0).any() and (ev.precision == -1).any()


REJECTS_MATCH = [('null_dbox', dict(dbox=None), 2), ('null_codes', dict(codes=None), 2), ('null_host_offsets', dict(gt_off_host=None), 2),
                 ('negative_n_det', dict(n_det=-1), 1), ('negative_cells', dict(n_cells=-1), 1), ('n_det_off_by_one', dict(n_det='+1'), 1),
                 ('n_gt_off_by_one', dict(n_gt='+1'), 1), ('decreasing', 'decreasing', 1), ('workspace_missing', dict(ws=None, ws_bytes=0), 2),
                 ('workspace_small', dict(ws_bytes='-1'), 4)]
REJECTS_ACC = [('null_codes', dict(codes=None), 2), ('null_recall', dict(recall=None), 2), ('null_max_dets', dict(max_dets=None), 2),
               ('negative_n_cat', dict(n_cat=-1), 1), ('n_det_off_by_one', dict(n_det='+1'), 1), ('negative_max_det', 'max_dets', 1)]


@gpu
@pytest.mark.parametrize('rej', REJECTS_MATCH, ids=[r[0] for r in REJECTS_MATCH])
def test_refused_match_calls(dev, rej):
    _, over, code = rej
    L = Launch(dev, C.BY_NAME['many_gts'])
    assert L.ws_bytes > 0
    if over == 'decreasing':
        bad = L.host['det_off'].copy()
        bad[0] = 1
        over = dict(det_off_host=bad.ctypes.data)
    over = {k: (getattr(L, k) + int(v) if isinstance(v, str) else v) for k, v in over.items()}
    assert L.match(**over) == code
    torch.cuda.synchronize()
    assert L.codes.unchanged() and L.npig.unchanged() and L.ws.unchanged(), 'a refused call wrote something'


@gpu
@pytest.mark.parametrize('rej', REJECTS_ACC, ids=[r[0] for r in REJECTS_ACC])
def test_refused_accumulate_calls(dev, rej):
    _, over, code = rej
    L = Launch(dev, C.BY_NAME['random_1'])
    L.set_npig_cat(L.ref['npig'])
    if over == 'max_dets':
        bad = np.array([1, -10, 100], np.int32)
        over = dict(max_dets=bad.ctypes.data)
    over = {k: (getattr(L, k) + int(v) if isinstance(v, str) else v) for k, v in over.items()}
    assert L.accumulate(**over) == code
    torch.cuda.synchronize()
    assert L.precision.unchanged() and L.recall.unchanged(), 'a refused call wrote something'


@gpu
def test_validate_reports_ap(dev):
    """validate() with a stub network: three 64 x 64 images, fixed predictions, evaluator = COCOEvaluator(ann)"""
    from yolov4_amd.yolo.engine.build import validate
    from yolov4_amd.yolo.util.cocoeval import COCOEvaluator
    from yolov4_amd.yolo.util.utils import COCO_CLASS_IDS
    S, N = 64, 6
    gts = [C.G(11, 1, [4, 4, 20, 20]), C.G(11, 2, [30, 30, 24, 20]), C.G(12, 1, [8, 10, 40, 36]), C.G(13, 3, [2, 2, 30, 30])]
    ann = C.case('validate', gts, [], [11, 12, 13], [1, 2, 3])['ann']
    pred = torch.zeros((3, N, 85))

    def put(b, n, box, cls, obj, conf):
        x, y, w, h = box
        pred[b, n, :5] = torch.tensor([x + w / 2, y + h / 2, w, h, obj])
        pred[b, n, 5 + cls] = conf
    put(0, 0, [4, 4, 20, 20], 0, .9, .9)            # hit
    put(0, 1, [31, 30, 24, 18], 1, .8, .9)          # IoU < 1
    put(0, 2, [40, 2, 10, 10], 0, .95, .9)          # miss scored above the hit
    put(1, 0, [8, 10, 40, 30], 0, .7, .8)
    put(1, 1, [50, 50, 10, 10], 1, .6, .5)          # category without a gt in this image
    put(2, 0, [2, 2, 30, 30], 1, .9, .9)            # wrong class: category 3 has a gt and no detection

    class Stub(torch.nn.Module):
        def forward(self, x):
            return pred[:x.shape[0]].clone().to(x.device)

    class DS:
        class_ids = COCO_CLASS_IDS

    class Loader(list):
        dataset = DS()
    info = torch.tensor([[S, S, S, S, 11., 0.], [S, S, S, S, 12., 0.], [S, S, S, S, 13., 0.]])
    ev = COCOEvaluator(ann, device=dev)
    got = validate(Loader([(torch.zeros(3, 3, S, S), {'img_info': info})]), Stub(), 0.1, 0.45, device=dev, evaluator=ev)
    recs = validate.records
    assert len(recs) == 6 and sorted(set(r['image_id'] for r in recs)) == [11, 12, 13]
    want = C.evaluate(ann, recs, [11, 12, 13])
    assert got == (float(want['stats'][0]), float(want['stats'][1])) and 0 < got[0] < got[1] < 1
    assert np.array_equal(ev.stats, want['stats']) and np.array_equal(ev.precision, want['precision'])
