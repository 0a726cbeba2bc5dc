# -*- coding: utf-8 -*-
"""The anchor-fitting kernels of csrc/anchors.hip -- y4_anchor_assign_f32 and y4_anchor_fitness_f32 -- through the C ABI on
every case of tests/anchor_cases.py (restatement and cases are there; tests/test_anchor_cases.py shows without a GPU that
every case reaches its branch), then `kmeans_anchors`, `evolve_anchors` and `anchor_report` of
yolov4_amd/yolo/util/anchors.py against the restatement's loops.

Every device buffer lies between two guards of a sentinel byte pattern that must survive, inputs must come back unchanged,
and every output word is written.  No tolerance appears: every compared value is an integer, an fp32 quotient NumPy
reproduces, or an fp64 quotient of integers.  Refused calls return their codes and write nothing; a second run gives the
same bytes."""
import numpy as np
import pytest
import torch

import anchor_cases as C
import recipe

gpu = pytest.mark.gpu
G = 256                                             # guard bytes in front of and behind every device buffer
SENT = 0xA5


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
    """device copies of one case"""

    def __init__(self, dev, c):
        self.c = c
        self.N, self.A = len(c['wh']), len(c['anchors'])
        self.Gn, self.Ac = c['cand'].shape[:2]
        self.wh = Buf(dev, (self.N, 2), np.float32, c['wh'])
        self.anchors = Buf(dev, (self.A, 2), np.float32, c['anchors'])
        self.cand = Buf(dev, c['cand'].shape, np.float32, c['cand'])
        self.assign = Buf(dev, (self.N,), np.uint8)
        self.best = Buf(dev, (self.N,), np.float32)
        self.acc = Buf(dev, (self.A, 5), np.int64)
        self.out = Buf(dev, (self.Gn, 2), np.int64)

    def run_assign(self, **over):
        from yolov4_amd import ops
        from yolov4_amd._lib import lib
        a = dict(wh=self.wh.ptr(), N=self.N, anchors=self.anchors.ptr(), A=self.A, thresh=self.c['iou_thresh'],
                 assign=self.assign.ptr(), best=self.best.ptr(), acc=self.acc.ptr())
        a.update(over)
        return lib().y4_anchor_assign_f32(a['wh'], a['N'], a['anchors'], a['A'], a['thresh'], a['assign'], a['best'], a['acc'],
                                          ops._stream())

    def run_fitness(self, **over):
        from yolov4_amd import ops
        from yolov4_amd._lib import lib
        a = dict(wh=self.wh.ptr(), N=self.N, cand=self.cand.ptr(), G=self.Gn, A=self.Ac, thr=self.c['thr'], out=self.out.ptr())
        a.update(over)
        return lib().y4_anchor_fitness_f32(a['wh'], a['N'], a['cand'], a['G'], a['A'], a['thr'], a['out'], ops._stream())

    def inputs_unchanged(self):
        return self.wh.unchanged() and self.anchors.unchanged() and self.cand.unchanged()

    def outputs_untouched(self):
        return self.assign.unchanged() and self.best.unchanged() and self.acc.unchanged() and self.out.unchanged()


def _run(dev, name):
    L = Launch(dev, C.BY_NAME[name])
    assert L.run_assign() == 0
    assert L.run_fitness() == 0
    torch.cuda.synchronize()
    return L, L.assign.get(), L.best.get(), L.acc.get(), L.out.get()


@gpu
@pytest.mark.parametrize('name', C.NAMES)
def test_case_through_the_c_abi(dev, name):
    L, assign, best, acc, out = _run(dev, name)
    r = C.reference(name)
    assert L.inputs_unchanged(), 'an input was written'
    assert np.array_equal(assign, r['assign']), (name, 'assign', np.argwhere(assign != r['assign'])[:5].tolist())
    bits, want = best.view(np.uint32), r['best_iou'].view(np.uint32)
    assert np.array_equal(bits, want), (name, 'best_iou', np.argwhere(bits != want)[:5].tolist())
    assert np.array_equal(acc, r['acc']), (name, 'acc', acc.tolist(), r['acc'].tolist())
    assert np.array_equal(out, r['out']), (name, 'out', np.argwhere(out != r['out'])[:5].tolist())
    # (the restatement's values differ from the sentinel, so equality also shows that every output word was written)
    sent32, sent64 = np.uint32(0xA5A5A5A5), np.array([SENT] * 8, np.uint8).view(np.int64)[0]
    assert (r['assign'] != SENT).all() and (want != sent32).all() and (r['acc'] != sent64).all() and (r['out'] != sent64).all()


@gpu
@pytest.mark.parametrize('name', ['n6151_a32_g9', 'multi_hits', 'two_rounds'])
def test_second_run_gives_the_same_bytes(dev, name):
    a, b = _run(dev, name), _run(dev, name)
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


@gpu
def test_optional_outputs_may_be_null(dev):
    L = Launch(dev, C.BY_NAME['multi_hits'])
    assert L.run_assign(assign=None, best=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(L.acc.get(), C.reference('multi_hits')['acc'])
    assert L.assign.unchanged() and L.best.unchanged()


REJECTS_ASSIGN = [('a_0', dict(A=0), 1), ('a_33', dict(A=33), 1), ('n_0', dict(N=0), 1), ('n_above', dict(N=(1 << 24) + 1), 1),
                  ('null_wh', dict(wh=None), 2), ('null_anchors', dict(anchors=None), 2), ('null_acc', dict(acc=None), 2)]
REJECTS_FITNESS = [('a_0', dict(A=0), 1), ('a_33', dict(A=33), 1), ('n_0', dict(N=0), 1), ('g_0', dict(G=0), 1),
                   ('g_65536', dict(G=65536), 1), ('null_wh', dict(wh=None), 2), ('null_cand', dict(cand=None), 2),
                   ('null_out', dict(out=None), 2)]


@gpu
@pytest.mark.parametrize('rej', REJECTS_ASSIGN, ids=[r[0] for r in REJECTS_ASSIGN])
def test_refused_assign_calls(dev, rej):
    _, over, code = rej
    L = Launch(dev, C.BY_NAME['multi_hits'])
    assert L.run_assign(**over) == code
    torch.cuda.synchronize()
    assert L.outputs_untouched() and L.inputs_unchanged(), 'a refused call wrote something'


@gpu
@pytest.mark.parametrize('rej', REJECTS_FITNESS, ids=[r[0] for r in REJECTS_FITNESS])
def test_refused_fitness_calls(dev, rej):
    _, over, code = rej
    L = Launch(dev, C.BY_NAME['multi_hits'])
    assert L.run_fitness(**over) == code
    torch.cuda.synchronize()
    assert L.outputs_untouched() and L.inputs_unchanged(), 'a refused call wrote something'


# ------------------------------------------------------------------------------------------------- the Python layer
@gpu
def test_raw_wrappers(dev):
    from yolov4_amd import ops
    c, r = C.BY_NAME['multi_hits'], C.reference('multi_hits')
    wh = torch.from_numpy(c['wh']).to(dev)
    assign, best, acc = ops.anchor_assign_raw(wh, torch.from_numpy(c['anchors']).to(dev), c['iou_thresh'])
    assert assign.dtype == torch.uint8 and np.array_equal(assign.cpu().numpy(), r['assign'])
    assert np.array_equal(best.cpu().numpy().view(np.uint32), r['best_iou'].view(np.uint32))
    assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), r['acc'])
    out = ops.anchor_fitness_raw(wh, torch.from_numpy(c['cand']).to(dev), c['thr'])
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), r['out'])


@gpu
def test_kmeans_recovers_constructed_clusters(dev):
    from yolov4_amd.yolo.util.anchors import kmeans_anchors
    from yolov4_amd import ops
    wh, lab, init = C.cluster_shapes()
    anchors, info = kmeans_anchors(wh, 6, init=init)
    want, winfo = C.kmeans(wh, 6, init=init)
    assert anchors.dtype == np.float32 and np.array_equal(anchors.view(np.uint32), want.view(np.uint32))
    assert info['iterations'] == winfo['iterations'] and info['counts'] == winfo['counts'] == [40 + 7 * i for i in range(6)]
    assert info['fitness'] == winfo['fitness'] and info['mean_best_iou'] == winfo['mean_best_iou']
    assign, _, _ = ops.anchor_assign_raw(torch.from_numpy(wh).to(dev), torch.from_numpy(anchors).to(dev), 1.0)
    assert np.array_equal(assign.cpu().numpy(), lab)      # the centres are listed by area, so sorted anchor i is cluster i
    for i in range(6):
        m = wh[lab == i]
        assert (m.min(axis=0) <= anchors[i]).all() and (anchors[i] <= m.max(axis=0)).all()


@pytest.fixture(scope='module')
def lognormal():
    wh = C.lognormal_shapes(2000, 21)
    return wh, C.kmeans(wh, 9, n_init=3, seed=4)


@gpu
def test_kmeans_starts_match_the_restatement(dev, lognormal):
    from yolov4_amd.yolo.util.anchors import kmeans_anchors
    wh, (want, winfo) = lognormal
    anchors, info = kmeans_anchors(wh, 9, n_init=3, seed=4)
    assert np.array_equal(anchors.view(np.uint32), want.view(np.uint32))
    assert {k: info[k] for k in info} == {k: winfo[k] for k in info}
    a = anchors.astype(np.float64)
    assert (np.diff(a[:, 0] * a[:, 1]) >= 0).all()


@gpu
def test_evolution_matches_the_restatement(dev, lognormal):
    from yolov4_amd.yolo.util.anchors import evolve_anchors
    wh, (start, _) = lognormal
    anchors, info = evolve_anchors(wh, start, generations=20, population=16, seed=2)
    want, track = C.evolve(wh, start, 20, 16, seed=2)
    assert info['fitness'] == track, 'parent trajectory'
    assert np.array_equal(anchors.view(np.uint32), want.view(np.uint32))
    assert track[-1] >= track[0] and all(b >= a for a, b in zip(track, track[1:]))
    assert info['accepted'] == sum(b > a for a, b in zip(track, track[1:]))
    assert info['mean_best_iou'] == track[-1] / (len(wh) * 2.0 ** 30)


def _tiny_cfg():
    from yolov4_amd.yolo.model.yolov4_tiny import default_cfg
    return default_cfg()


@gpu
@pytest.mark.parametrize('which', ['yolov4', 'tiny'])
@pytest.mark.parametrize('iou_thresh', [1.0, 0.213])
def test_report(dev, which, iou_thresh):
    from yolov4_amd.yolo.util.anchors import anchor_report, format_report
    cfg = recipe.MODEL_CFG if which == 'yolov4' else _tiny_cfg()
    wh = C.lognormal_shapes(3000, 31, median=40.0, spread=1.0)
    rep = anchor_report(wh, cfg, iou_thresh)
    want = C.report(wh, cfg, iou_thresh)
    for k, v in want.items():
        assert rep[k] == v, k
    assert len(rep['positives']) == len(cfg['ANCHOR_MASK']) and sum(rep['counts']) == len(wh)
    if which == 'tiny':
        assert rep['unassigned'] == rep['counts'][0] / len(wh) > 0
    else:
        assert rep['unassigned'] == 0
    if iou_thresh == 1.0:
        assert sum(rep['positives']) == len(wh) - round(rep['unassigned'] * len(wh)) + (rep['counts'][3] if which == 'tiny' else 0)
    else:
        assert sum(rep['positives']) > len(wh)
    assert anchor_report(wh, {'MODEL': cfg}, iou_thresh) == rep
    assert len(format_report(rep).split('\n')) == 2 + len(cfg['ANCHORS']) + len(cfg['ANCHOR_MASK']) + 1


@gpu
def test_cli_end_to_end(dev, tmp_path, capsys):
    import json
    from yolov4_amd.yolo.util.anchors import label_shapes, main
    shapes = C.lognormal_shapes(80, 41, lo=3.0, hi=300.0).astype(np.float64)
    doc = {'images': [{'id': 1, 'width': 640, 'height': 480}], 'categories': [{'id': 1}],
           'annotations': [{'id': i + 1, 'image_id': 1, 'category_id': 1, 'bbox': [0, 0, float(w), float(h)]}
                           for i, (w, h) in enumerate(shapes)]}
    (tmp_path / 'annotations').mkdir()
    (tmp_path / 'annotations' / 'instances_train2017.json').write_text(json.dumps(doc))
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps({'MODEL': _tiny_cfg(), 'CRITERION': {'IOU_THRESH': 0.213}, 'TEST': {'IMGSIZE': 416}}))
    assert main([str(tmp_path), '-c', str(cfg), '--check']) == 0
    text = capsys.readouterr().out
    wh = label_shapes(str(tmp_path / 'annotations' / 'instances_train2017.json'), 416)
    want = C.report(wh, _tiny_cfg(), 0.213)
    assert '%d labels, 6 anchors, iou_thresh 0.213' % len(wh) in text and 'ANCHORS:' not in text
    assert 'layer 0 (mask [1, 2, 3]): %d positives' % want['positives'][0] in text
    assert main([str(tmp_path), '-c', str(cfg), '--n-init', '2', '--evolve', '3', '--population', '4', '--seed', '1']) == 0
    text = capsys.readouterr().out
    anchors, _ = C.kmeans(wh, 6, n_init=2, seed=1)
    anchors, _ = C.evolve(wh, anchors, 3, 4, seed=1)
    from yolov4_amd.yolo.util.anchors import format_cfg
    assert text.rstrip().endswith(format_cfg(anchors, 2)) and 'fitted anchors' in text
