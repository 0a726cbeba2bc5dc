# -*- coding: utf-8 -*-
"""Without a GPU: the restatement of tests/coco_cases.py gives the hand values of the COCO protocol, every case reaches
the branch it is named after, the host packing of yolov4_amd/yolo/util/cocoeval.py groups gts and records into the same
cells as a brute-force grouping, the header declares the entry points, and csrc/coco_eval.hip compiles for gfx950 without
scratch or spilled registers."""
import os
import re
import sys

import numpy as np
import pytest

import coco_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from kernel_resources import kernel_resources  # noqa: E402

ONE = 1 / (1 + 2.0 ** -52)
NAMES = [c['name'] for c in C.CASES]


def close(a, b):
    return abs(a - b) <= 1e-12


def test_perfect():
    r = C.reference('perfect')
    assert all(close(v, ONE) for v in r['stats'][:6]), r['stats']
    assert all(close(v, 1.0) for v in r['stats'][6:]), r['stats']
    assert r['minus_one'] > 0                      # a category of one size leaves the other two area ranges at -1


def test_fp_above_tp():
    s = C.reference('fp_above_tp')['stats']
    assert close(s[0], 0.5) and close(s[1], 0.5)


def test_half_found():
    r = C.reference('half_found')
    assert close(r['stats'][1], 51 / 101) and close(r['stats'][0], 3 / 10 * 51 / 101)
    assert np.array_equal(r['recall'][:, 0, 0, 2], [0.5] * 3 + [0.0] * 7)


def test_empty_sides():
    r = C.reference('empty_sides')
    assert close(r['stats'][0], 0.5) and close(r['stats'][1], 0.5)
    p = r['precision'][0, 0, :, 0, 2]
    assert close(p[0], ONE) and p[1] == -1 and p[2] == 0
    assert (r['precision'][:, :, 1] == -1).all() and (r['recall'][:, 1] == -1).all()


def test_crowd():
    r = C.reference('crowd')
    assert close(r['stats'][0], ONE) and close(r['stats'][1], ONE)
    # the two detections inside the crowd box match it (IoU = intersection / detection area = 1) at every threshold and area
    assert r['crowd_matches'] == 2 * C.T * C.A
    assert ((r['codes'][0, :2] >> 0) & 3).tolist() == [3, 3] and int(r['codes'][0, 2] & 3) == 1
    assert r['npig'][0].tolist() == [1, 0, 1, 0]


def test_area():
    c, r = C.BY_NAME['area'], C.reference('area')
    gts = c['ann']['annotations']
    assert any(g['area'] != g['bbox'][2] * g['bbox'][3] for g in gts)
    # by the area field: image 1 has 1 small, 2 medium, 1 large (by w*h it would be 1, 1, 2); 32^2 and 96^2 lie in two ranges
    assert r['npig'].tolist() == [[4, 1, 2, 1], [2, 1, 2, 1]]
    codes0 = (r['codes'] & 3)
    assert (codes0 == 2).any() and (codes0 == 0).any() and (codes0 == 3).any()
    # the 10x10 miss is ignored (code 2) in medium and large, a false positive in all and small
    i = [n for n, j in enumerate(r['kept']) if c['records'][j]['bbox'][2] == 10][0]
    assert codes0[:, i].tolist() == [0, 0, 2, 2]


def test_maxdets():
    r = C.reference('maxdets')
    assert r['truncated'] == 1 and r['det_off'].tolist() == [0, 100, 102]
    assert len(r['kept']) == 102
    rc = r['recall'][0, 0, 0]
    assert 0 < rc[0] < rc[1] <= rc[2]                               # the rank filters for 1 and 10
    scores = [C.BY_NAME['maxdets']['records'][j]['score'] for j in r['kept'][:100]]
    assert scores == sorted(scores, reverse=True) and len(set(scores)) < 100        # ties, kept in record order
    tied = [(a, b) for a, b, sa, sb in zip(r['kept'][:99], r['kept'][1:100], scores, scores[1:]) if sa == sb]
    assert tied and all(a < b for a, b in tied)


def test_ties():
    c, r = C.BY_NAME['ties'], C.reference('ties')
    assert 0 in c['exact']
    # image 1: both detections are true positives at every threshold the equal IoU 90/110 reaches, because the first took
    # the LATER gt; had it taken the earlier one, the second (IoU 1 with it) would only find IoU 80/120
    first, second = r['codes'][0, 0], r['codes'][0, 1]
    assert [(int(first) >> (2 * t)) & 3 for t in range(C.T)] == [1] * 7 + [0] * 3
    assert [(int(second) >> (2 * t)) & 3 for t in range(C.T)] == [1] * 10
    for n, j in enumerate(c['exact']):             # IoU exactly iouThrs[j]: matched up to t = j, not above
        cell = r['cells'].index((0, c['image_ids'].index(2 + j)))
        code = int(r['codes'][0, r['det_off'][cell]])
        assert [(code >> (2 * t)) & 3 for t in range(C.T)] == [1] * (j + 1) + [0] * (C.T - 1 - j)
    scores = [x['score'] for x in c['records'] if x['image_id'] >= 20]
    assert len(set(scores)) <= 4 and all(s * 16 == int(s * 16) for s in scores)


def test_filters():
    c, r = C.BY_NAME['filters'], C.reference('filters')
    assert r['cells'] == [(0, 0), (0, 1), (1, 0)]                   # image 3 has nothing, image 4 and category 7 are out
    assert sorted(r['kept'].tolist()) == [0, 1, 4]
    with pytest.raises(ValueError):
        C.evaluate(c['ann'], c['bad_records'], c['image_ids'])


def test_many_gts_and_long_cat():
    r = C.reference('many_gts')
    assert len(C.BY_NAME['many_gts']['ann']['annotations']) == 300 and len(r['kept']) == 100 and len(r['cells']) == 1
    assert r['crowd_matches'] > 0 and r['ignored'] > 0 and 0 < r['stats'][0] < 1
    from yolov4_amd import _lib
    assert _lib.lib().y4_coco_workspace(1, 300) > 0 and _lib.lib().y4_coco_workspace(1, 150) == 0     # the two matched-bit paths
    r = C.reference('mid_gts')
    assert len(C.BY_NAME['mid_gts']['ann']['annotations']) == 150 > 64 and r['crowd_matches'] > 0 and r['ignored'] > 0
    r = C.reference('long_cat')
    assert len(r['kept']) >= 3000 and len(r['cells']) == 40 and 0 < r['stats'][0] < 1


@pytest.mark.parametrize('name', ['random_1', 'random_2', 'random_3'])
def test_random_mixes_reach_every_branch(name):
    r = C.reference(name)
    codes = np.stack([(r['codes'] >> (2 * t)) & 3 for t in range(C.T)])
    assert all((codes == v).any() for v in range(4))
    assert r['crowd_matches'] > 0 and r['minus_one'] >= 0 and (r['npig'] > 0).any()
    assert int(np.diff(r['det_off']).max()) > 10 and 0 < r['stats'][0] < 1


@pytest.mark.parametrize('name', NAMES)
def test_host_packing_equals_brute_force_grouping(name):
    """the test that fails before the feature exists"""
    from yolov4_amd.yolo.util.cocoeval import KEEP, COCOEvaluator
    c = C.BY_NAME[name]
    ev = COCOEvaluator(c['ann'])
    p = ev.pack(c['records'], c['image_ids'])
    brute = C.brute_cells(c)
    keys = sorted(brute)
    assert p['n_cells'] == len(keys) and p['n_cat'] == len(c['ann']['categories'])
    assert list(zip(p['cell_cat'].tolist(), p['cell_img'].tolist())) == keys
    assert p['gt_off'].dtype == np.int32 and p['det_off'].dtype == np.int32 and p['cat_off'].dtype == np.int32
    anns = c['ann']['annotations']
    for n, key in enumerate(keys):
        g, d = brute[key]
        got_g = p['g_index'][p['gt_off'][n]:p['gt_off'][n + 1]].tolist()
        assert got_g == g, (key, 'gts in annotation order')
        assert sorted(p['d_index'][p['det_cell'] == n].tolist()) == d, key
        assert p['det_off'][n + 1] - p['det_off'][n] == min(len(d), KEEP)
    assert p['gt_off'][-1] == len(p['g_area']) == sum(len(brute[k][0]) for k in keys)
    for j, gi in enumerate(p['g_index'].tolist()):
        assert p['g_box'][j].tolist() == anns[gi]['bbox'] and p['g_area'][j] == anns[gi]['area'] \
            and p['g_crowd'][j] == anns[gi]['iscrowd']
    for j, di in enumerate(p['d_index'].tolist()):
        assert p['d_box'][j].tolist() == c['records'][di]['bbox'] and p['d_score'][j] == c['records'][di]['score']
    K = p['n_cat']
    per_cat = [sum(min(len(brute[k][1]), KEEP) for k in keys if k[0] == kk) for kk in range(K)]
    assert p['cat_off'].tolist() == np.concatenate([[0], np.cumsum(per_cat)]).tolist()
    assert p['image_ids'].tolist() == sorted(set(c['image_ids']))
    if 'bad_records' in c:
        with pytest.raises(ValueError):
            ev.pack(c['bad_records'], c['image_ids'])


def test_summary_statistics_are_the_restatements():
    from yolov4_amd.yolo.util import cocoeval
    assert np.array_equal(cocoeval.IOU_THRS, C.IOU) and np.array_equal(cocoeval.REC_THRS, C.REC)
    assert cocoeval.AREA_RNG.tolist() == [[float(v) for v in r] for r in C.AREA] and list(cocoeval.MAX_DETS) == C.MAXDETS
    for name in ('half_found', 'empty_sides', 'random_2'):
        r = C.reference(name)
        assert np.array_equal(cocoeval.summarize(r['precision'], r['recall']), r['stats'])


def test_no_cpu_fallback():
    import torch
    import yolov4_amd
    from yolov4_amd.yolo.util.cocoeval import COCOEvaluator
    c = C.BY_NAME['perfect']
    with pytest.raises(yolov4_amd.Y4Error):
        COCOEvaluator(c['ann'], device='cpu')(c['records'], c['image_ids'])
    if not torch.cuda.is_available():
        with pytest.raises(yolov4_amd.Y4Error):
            COCOEvaluator(c['ann'])(c['records'], c['image_ids'])


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, 'include', 'yolov4_amd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for sym in ('y4_coco_workspace', 'y4_coco_match_f64', 'y4_coco_accumulate_f64'):
        assert re.search(r'\b' + sym + r'\s*\(', txt), sym
    from yolov4_amd import _lib
    L = _lib.lib()
    assert L.y4_coco_workspace(1000, 256) == 0
    assert L.y4_coco_workspace(1000, 257) == 1000 * 9 * 40 * 4
    assert L.y4_coco_workspace(100000, 600) == 2048 * 19 * 40 * 4
    assert L.y4_coco_workspace(0, 600) == 0


def test_refused_calls_on_the_host():
    """checked before any launch, so without a GPU too: NULL pointers 2, bad counts and offsets 1"""
    from yolov4_amd import _lib
    L = _lib.lib()
    fake = 0x1000
    off = np.array([0, 2, 3], np.int32)
    goff = np.array([0, 1, 1], np.int32)
    o, g = off.ctypes.data, goff.ctypes.data

    def match(dbox=fake, doff=o, n_det=3, goff_=g, n_gt=1, n_cells=2, codes=fake):
        return L.y4_coco_match_f64(dbox, fake, doff, n_det, fake, fake, fake, fake, goff_, n_gt, n_cells, fake, fake, codes, fake,
                                   None, 0, None)
    assert match(dbox=None) == 2 and match(codes=None) == 2 and match(doff=None) == 2
    assert match(n_det=-1) == 1 and match(n_cells=-1) == 1 and match(n_gt=-1) == 1
    assert match(n_det=4) == 1 and match(n_gt=2) == 1               # offsets end elsewhere
    bad = np.array([0, 3, 2], np.int32)
    assert match(doff=bad.ctypes.data, n_det=2) == 1                 # decreasing
    long_ = np.array([0, 101, 101], np.int32)
    assert match(doff=long_.ctypes.data, n_det=101) == 1             # a cell of more than 100 detections
    many = np.array([0, 600, 600], np.int32)
    assert match(goff_=many.ctypes.data, n_gt=600) == 2              # needs a workspace, none given
    md = (_lib.c_int * 3)(1, 10, 100)

    def acc(codes=fake, coff=o, n_det=3, n_cat=2, md_=md):
        return L.y4_coco_accumulate_f64(codes, fake, fake, n_det, fake, coff, fake, n_cat, fake, md_, fake, fake, None)
    assert acc(codes=None) == 2 and acc(coff=None) == 2 and acc(md_=None) == 2
    assert acc(n_det=-1) == 1 and acc(n_cat=-1) == 1 and acc(n_det=5) == 1 and acc(coff=bad.ctypes.data, n_det=2) == 1
    assert acc(md_=(_lib.c_int * 3)(1, -10, 100)) == 1


def test_coco_kernels_use_no_scratch():
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'coco_eval.hip'), ('-ffp-contract=off',))
    names = [r['name'].split('(')[0] for r in rows]
    assert any('coco_match_kernel' in n for n in names) and any('coco_accumulate_kernel' in n for n in names), names
    bad = [(r['name'].split('(')[0], r['scratch'], r['vgpr_spill'], r['sgpr_spill']) for r in rows
           if r['scratch'] != 0 or r['vgpr_spill'] != 0 or r['sgpr_spill'] != 0]
    assert not bad, bad
