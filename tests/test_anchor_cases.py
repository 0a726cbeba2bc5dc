# -*- coding: utf-8 -*-
"""Without a GPU: every case of tests/anchor_cases.py reaches the branch it is named for and the launch shapes it was
sized by are those of csrc/anchors.hip; `label_shapes`, `format_cfg` and the CLI's argument parsing of
yolov4_amd/yolo/util/anchors.py; the random draws of the evolution against the restatement's; and no CPU fallback."""
import json
import os
import re

import numpy as np
import pytest
import torch

import anchor_cases as C
from yolov4_amd.yolo.util import anchors as A          # the module under test: its limits are the kernels'

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_launch_shapes_are_the_sources():
    src = open(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'anchors.hip')).read()

    def const(name):
        return int(eval(re.search(r'constexpr int %s = ([0-9 <*]+);' % name, src).group(1)))
    assert const('kThreads') == C.ASSIGN_BLOCK and const('kAssignBlocks') == C.ASSIGN_GRID
    assert const('kThreads') * const('kSpt') == C.FIT_TILE and const('kGc') == C.FIT_CHUNK and const('kFitBlocks') == C.FIT_BLOCKS
    assert (const('kMaxA'), const('kMaxN'), const('kMaxG')) == (A.MAX_ANCHORS, A.MAX_SHAPES, A.MAX_CANDIDATES) == (32, 1 << 24, 65535)


def test_the_dimensions_the_cases_cover():
    ns = set(len(c['wh']) for c in C.CASES)
    assert {1, 63, 64, 65, C.ASSIGN_BLOCK - 1, C.ASSIGN_BLOCK, C.ASSIGN_BLOCK + 1, 3 * C.ASSIGN_BLOCK + 7, C.FIT_TILE - 1,
            C.FIT_TILE, C.FIT_TILE + 1, 3 * C.FIT_TILE + 7} <= ns
    assert {1, 6, 9, 32} <= set(len(c['anchors']) for c in C.CASES)
    assert {1, 6, 9, 32} <= set(c['cand'].shape[1] for c in C.CASES)
    assert {1, 2, C.FIT_CHUNK + 1, 65535} <= set(len(c['cand']) for c in C.CASES)
    assert {1.0, 0.213} <= set(c['iou_thresh'] for c in C.CASES)
    assert len(set(C.NAMES)) == len(C.NAMES)
    for c in C.CASES:
        for a in (c['wh'], c['anchors'], c['cand']):
            assert np.isfinite(a).all() and (a > 0).all() and (a < A.MAX_SIDE).all(), c['name']


@pytest.mark.parametrize('name', C.NAMES)
def test_case_reaches_its_branch(name):
    c, r = C.BY_NAME[name], C.reference(name)
    reach = c['reach']
    n, a = len(c['wh']), len(c['anchors'])
    acc, out = r['acc'], r['out']
    iou = C.iou_matrix(c['wh'], c['anchors']) if n * a < 1 << 20 else None
    assert np.isfinite(r['best_iou']).all() and (r['best_iou'] > 0).all() and (r['best_iou'] <= 1).all()
    assert acc[:, 0].sum() == n and (acc[:, 4] >= acc[:, 0]).all() and (out[:, 1] <= n).all()
    assert out.shape == (len(c['cand']), 2) and (out[:, 0] > 0).all()
    if c['iou_thresh'] == 1.0:
        assert np.array_equal(acc[:, 4], acc[:, 0])
    for key in ('n', 'a', 'g'):
        if key in reach:
            assert reach[key] == {'n': n, 'a': a, 'g': len(c['cand'])}[key]
    if 'twins' in reach:
        lo, hi = reach['twins']
        assert np.array_equal(c['anchors'][lo], c['anchors'][hi]) and acc[lo, 0] > 0 and acc[hi, 0] == 0
        assert np.array_equal(iou[:, lo], iou[:, hi])
    if 'tie_row' in reach:
        row = iou[reach['tie_row']]
        assert row[0] == row[1] == row[2] == F32(0.5) and len(set(map(tuple, c['anchors'][:3]))) == 3
        assert r['assign'][reach['tie_row']] == 0
    if reach.get('strict'):
        at = r['best_iou'] == F32(c['iou_thresh'])
        assert at.any() and c['thr'] == c['iou_thresh']
        # a shape AT the threshold is a hit of its best anchor only, and is not counted by the fitness launch
        assert (iou[at] > F32(c['iou_thresh'])).sum() == 0
        assert np.array_equal(c['cand'][0], c['anchors']) and out[0, 1] == (r['best_iou'] > F32(c['thr'])).sum() < n
    if reach.get('extremes'):
        assert c['wh'].min() == 0.5 and c['wh'].max() == 65535
        assert (r['best_iou'] == 1).any() and C.q16(c['wh']).max() == 65535 << 16
    if 'empty' in reach:
        assert acc[reach['empty'], 0] == 0 and (np.delete(acc[:, 0], reach['empty']) > 0).all()
    if reach.get('multi'):
        assert (acc[:, 4] > acc[:, 0]).any()
    if 'rounds' in reach:
        assert -(-n // (C.ASSIGN_GRID * C.ASSIGN_BLOCK)) == reach['rounds']
    if reach.get('stride'):
        tiles, chunks = -(-n // C.FIT_TILE), -(-len(c['cand']) // C.FIT_CHUNK)
        assert max(1, C.FIT_BLOCKS // chunks) < tiles


def test_restatement_on_hand_values():
    asg, bi, acc = C.assign(np.array([[4, 4], [10, 10]], F32), np.array([[2, 4], [4, 2], [10, 20]], F32), 0.4)
    assert asg.tolist() == [0, 2] and bi.tolist() == [0.5, 0.5]
    assert acc.tolist() == [[1, 4 << 16, 4 << 16, 1 << 29, 1], [0, 0, 0, 0, 1], [1, 10 << 16, 10 << 16, 1 << 29, 1]]
    out = C.fitness(np.array([[4, 4], [10, 10]], F32), np.array([[[4, 4], [10, 10]], [[2, 4], [10, 20]]], F32), 0.5)
    assert out.tolist() == [[2 << 30, 2], [1 << 30, 0]]
    assert C.sorted_order(np.array([[4, 4], [2, 8], [1, 1], [8, 2]], F32)).tolist() == [2, 1, 0, 3]


def test_constructed_clusters_are_separated():
    wh, lab, init = C.cluster_shapes()
    assert np.bincount(lab).tolist() == [40 + 7 * i for i in range(6)]
    iou = C.iou_matrix(wh, np.array(C.CLUSTER_CENTRES, F32))
    own = iou[np.arange(len(wh)), lab]
    other = iou.copy()
    other[np.arange(len(wh)), lab] = 0
    assert own.min() > 0.8 and other.max() < 0.35
    anchors, info = C.kmeans(wh, 6, init=init)
    assert np.array_equal(info['assign'], lab) and info['iterations'] <= 3


# ------------------------------------------------------------------------------------------------------ label_shapes
def _annotation_file(tmp_path, drop_width=False):
    images = [{'id': 7, 'width': 640, 'height': 480}, {'id': 9, 'width': 300, 'height': 500}]
    if drop_width:
        del images[1]['width']
    doc = {'images': images, 'categories': [{'id': 5}, {'id': 2}, {'id': 11}],
           'annotations': [{'id': 1, 'image_id': 7, 'category_id': 2, 'bbox': [1, 2, 64, 48]},
                           {'id': 2, 'image_id': 9, 'category_id': 11, 'bbox': [0, 0, 30.5, 125.25]},
                           {'id': 3, 'image_id': 7, 'category_id': 5, 'bbox': [5, 5, 1, 40]},        # w == min_size: dropped
                           {'id': 4, 'image_id': 9, 'category_id': 5, 'bbox': [5, 5, 10, 0.5]},      # h too small
                           {'id': 5, 'image_id': 9, 'category_id': 5, 'bbox': [5, 5, 7, 3]}]}
    d = tmp_path / 'annotations'
    d.mkdir()
    p = d / 'instances_train2017.json'
    p.write_text(json.dumps(doc))
    return str(p)


def test_label_shapes_filter_and_stretch(tmp_path):
    from yolov4_amd.yolo.util.anchors import annotation_path, label_shapes
    p = _annotation_file(tmp_path)
    assert annotation_path(str(tmp_path), 'train2017') == p and annotation_path(p, 'val2017') == p
    wh = label_shapes(p, 416)
    want = np.array([[64 * 416 / 640, 48 * 416 / 480], [30.5 * 416 / 300, 125.25 * 416 / 500], [7 * 416 / 300, 3 * 416 / 500]])
    assert wh.dtype == np.float32 and np.array_equal(wh, want.astype(np.float32))
    # classes are positions among the sorted category ids (2, 5, 11): num_classes = 2 drops category 11
    assert np.array_equal(label_shapes(p, 416, num_classes=2), want[[0, 2]].astype(np.float32))
    assert np.array_equal(label_shapes(p, 416, min_size=5), want[[0, 1]].astype(np.float32))
    assert label_shapes(p, 608, min_size=1000).shape == (0, 2)

    class DS:                                            # what label_shapes reads of a COCODataset
        annotation_file, num_classes = p, 2
    assert np.array_equal(label_shapes(DS(), 416), want[[0, 2]].astype(np.float32))
    from yolov4_amd.yolo.data.cocodataset import COCODataset
    ds = COCODataset(str(tmp_path), 'train2017', num_classes=3)
    assert np.array_equal(label_shapes(ds, 416), want.astype(np.float32))
    kept = sum(len(ds.get_labels(i)) for i in range(len(ds)))
    assert kept == len(want)


def test_label_shapes_errors(tmp_path):
    from yolov4_amd.yolo.util.anchors import label_shapes
    with pytest.raises(ValueError, match='width'):
        label_shapes(_annotation_file(tmp_path, drop_width=True), 416)
    big = tmp_path / 'big.json'
    big.write_text(json.dumps({'images': [{'id': 1, 'width': 2, 'height': 2}], 'categories': [{'id': 1}],
                               'annotations': [{'id': 1, 'image_id': 1, 'category_id': 1, 'bbox': [0, 0, 400, 2]}]}))
    with pytest.raises(ValueError, match='65536'):
        label_shapes(str(big), 416)                      # 400 * 416 / 2 = 83200


# --------------------------------------------------------------------------------------------------------- format_cfg
def test_format_cfg():
    from yolov4_amd.yolo.util.anchors import format_cfg
    a = [[0.2, 0.6], [2.5, 3.5], [10.49, 10.51], [20, 30], [40.5, 41.5], [100, 200]]
    text = format_cfg(np.array(a, np.float32), 2)
    assert text == ('ANCHORS: [[1, 1], [2, 4], [10, 11], [20, 30], [40, 42], [100, 200]]\n'
                    'ANCHOR_MASK: [[0, 1, 2], [3, 4, 5]]')
    lines = text.split('\n')
    masks = json.loads(lines[1].split(': ', 1)[1])
    assert all(m[i] % 3 == i for m in masks for i in range(3))
    assert json.loads(lines[0].split(': ', 1)[1])[5] == [100, 200]
    assert format_cfg(np.ones((9, 2)), 3).count('[') == 2 + 9 + 3
    for k, layers in ((6, 3), (9, 2), (5, 2), (0, 0)):
        with pytest.raises(ValueError):
            format_cfg(np.ones((k, 2)), layers)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_arguments():
    from yolov4_amd.yolo.util.anchors import build_parser
    ap = build_parser()
    a = ap.parse_args(['/data/coco', '-c', 'cfg.json'])
    assert (a.data, a.cfg, a.split, a.img_size, a.k, a.n_init, a.evolve, a.population, a.seed, a.check) == \
        ('/data/coco', 'cfg.json', 'train2017', None, None, 8, 0, 64, 0, False)
    a = ap.parse_args(['ann.json', '--cfg', 'c.yaml', '--split', 'val2017', '--img-size', '608', '--k', '6', '--n-init', '3',
                       '--evolve', '500', '--population', '32', '--seed', '4', '--check'])
    assert (a.data, a.cfg, a.split, a.img_size, a.k, a.n_init, a.evolve, a.population, a.seed, a.check) == \
        ('ann.json', 'c.yaml', 'val2017', 608, 6, 3, 500, 32, 4, True)
    with pytest.raises(SystemExit):
        ap.parse_args(['/data/coco'])                    # -c is required
    with pytest.raises(SystemExit):
        ap.parse_args(['-c', 'cfg.json'])                # and so is DATA


# ------------------------------------------------------------------------------------------------- draws, no fallback
def test_evolution_draws_are_the_restatements():
    from yolov4_amd.yolo.util.anchors import children_of, mutation_factors
    parent = np.array([[12, 16], [40, 28], [1.5, 300]], F32)
    rng, ref = (np.random.Generator(np.random.PCG64(3)) for _ in range(2))
    for _ in range(3):
        f = mutation_factors(rng, 5, 3, 0.1, 0.9)
        normal, uniform = ref.standard_normal((5, 3, 2)), ref.random((5, 3, 2))
        assert np.array_equal(f, np.clip(1.0 + 0.1 * normal * (uniform < 0.9), 0.3, 3.0))
        kids = children_of(parent, f, 2.0)
        assert kids.dtype == F32 and kids.shape == (5, 3, 2) and kids.min() == 2.0
        assert np.array_equal(kids, np.maximum(parent.astype(np.float64)[None] * f, 2.0).astype(F32))
    # mutate_prob = 0: every factor is 1 and the draw would repeat for ever; a tiny one repeats until something moves
    f = mutation_factors(np.random.Generator(np.random.PCG64(0)), 1, 1, 0.1, 0.02)
    assert (f != 1).any()
    assert children_of(np.array([[60000, 3]], F32), np.full((1, 1, 2), 3.0), 2.0).max() < 65536


def test_validation_needs_no_gpu():
    from yolov4_amd.yolo.util import anchors as A
    wh = C.lognormal_shapes(50, 1)
    for bad in (np.zeros((4, 2)), np.full((4, 2), 65536.0), np.full((4, 2), np.nan), np.ones((4, 3)), np.ones((0, 2))):
        with pytest.raises(ValueError):
            A.kmeans_anchors(bad, 2)
    for k in (0, 33):
        with pytest.raises(ValueError):
            A.kmeans_anchors(wh, k)
    with pytest.raises(ValueError):
        A.evolve_anchors(wh, wh[:3], population=0)


def test_no_cpu_fallback():
    import recipe
    from yolov4_amd import Y4Error, ops
    from yolov4_amd.yolo.util import anchors as A
    wh = C.lognormal_shapes(50, 1)
    with pytest.raises(Y4Error):
        ops.anchor_assign_raw(torch.from_numpy(wh), torch.from_numpy(wh[:3]))
    with pytest.raises(Y4Error):
        ops.anchor_fitness_raw(torch.from_numpy(wh), torch.from_numpy(wh[None, :3]), 0.2)
    if not torch.cuda.is_available():
        with pytest.raises(Y4Error):
            A.kmeans_anchors(wh, 3)
        with pytest.raises(Y4Error):
            A.evolve_anchors(wh, wh[:3], generations=1, population=2)
        with pytest.raises(Y4Error):
            A.anchor_report(wh, recipe.MODEL_CFG)


def test_refusals_happen_on_the_host():
    """NULL pointers and shapes outside the limits are refused before anything touches a device (fake pointers are never
    dereferenced on the host)"""
    from yolov4_amd._lib import lib
    L, p = lib(), 0x1000
    assert L.y4_anchor_assign_f32(None, 4, p, 3, 1.0, None, None, p, None) == 2
    assert L.y4_anchor_assign_f32(p, 4, None, 3, 1.0, None, None, p, None) == 2
    assert L.y4_anchor_assign_f32(p, 4, p, 3, 1.0, p, p, None, None) == 2
    for n, a in ((0, 3), ((1 << 24) + 1, 3), (4, 0), (4, 33), (-1, 3)):
        assert L.y4_anchor_assign_f32(p, n, p, a, 1.0, None, None, p, None) == 1
    assert L.y4_anchor_assign_f32(p + 4, 4, p, 3, 1.0, None, None, p, None) == 1      # (w, h) pairs are 8-byte words
    assert L.y4_anchor_fitness_f32(None, 4, p, 2, 3, 0.2, p, None) == 2
    assert L.y4_anchor_fitness_f32(p, 4, None, 2, 3, 0.2, p, None) == 2
    assert L.y4_anchor_fitness_f32(p, 4, p, 2, 3, 0.2, None, None) == 2
    for n, g, a in ((0, 2, 3), (4, 0, 3), (4, 65536, 3), (4, 2, 0), (4, 2, 33), ((1 << 24) + 1, 2, 3)):
        assert L.y4_anchor_fitness_f32(p, n, p, g, a, 0.2, p, None) == 1
