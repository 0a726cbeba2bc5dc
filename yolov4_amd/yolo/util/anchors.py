# -*- coding: utf-8 -*-
"""Anchor fitting on a dataset's label shapes: what Darknet's `detector calc_anchors` and the evolution stage of YOLOv5's
autoanchor do, with the metric the loss itself assigns by (the shape IoU of csrc/yolo_loss.hip's yolo_assign_kernel).

    label_shapes     (w, h) of every label, stretched to S x S, from an annotation file (no JPEG is decoded)
    kmeans_anchors   Lloyd iterations under the shape IoU, mean update
    evolve_anchors   mutation / selection on the sum of best IoUs, a whole generation per launch
    anchor_report    how a cfg's anchors fit: best IoU, labels per anchor, positives per head, labels no head trains on
    format_cfg       the ANCHORS: / ANCHOR_MASK: lines of a cfg

    python -m yolov4_amd.yolo.util.anchors DATA -c CFG [--split train2017] [--img-size S] [--k K] [--n-init 8]
                                           [--evolve GENERATIONS] [--population 64] [--seed 0] [--check]

The assignment pass and the fitness of a generation are the two kernels of csrc/anchors.hip; the host keeps the loop, the
random draws and one fp64 quotient of integers per centroid coordinate.  There is no CPU path: without an MI355X the
functions that launch raise Y4Error.  Arithmetic, fixed-point format and limits: include/yolov4_amd.h, DESIGN.md §20.
"""
import argparse
import json
import os.path
import sys

import numpy as np
import torch

from ... import ops
from ..._lib import Y4Error, lib

MAX_SIDE = 65536.0                       # shapes and anchors lie in (0, MAX_SIDE)
MAX_ANCHORS, MAX_SHAPES, MAX_CANDIDATES = 32, 1 << 24, 65535
Q_WH, Q_IOU = 2.0 ** 16, 2.0 ** 30       # fixed-point units of the device sums
_BELOW_MAX = np.nextafter(np.float32(MAX_SIDE), np.float32(0))


# ------------------------------------------------------------------------------------------------------------- labels
def label_shapes(source, img_size, min_size=1, num_classes=None):
    """float32 [N, 2]: (w * S / W, h * S / H) of every box of the annotation file, S = img_size, (W, H) the size of the box's
    image as the file's `images` list states it -- the stretch to S x S of the loader's evaluation branch and of Darknet's
    calc_anchors -- computed in fp64 and rounded once.  Boxes are kept as COCODataset keeps them: w > min_size and
    h > min_size (in file pixels), class (position of the category id among the sorted ids) in [0, num_classes).

    source: a COCODataset (its annotation_file is read; num_classes=None then means the dataset's) or the path of an
    instances_*.json (num_classes=None: every class).  Order: the file's annotation order."""
    path = getattr(source, 'annotation_file', source)
    if num_classes is None:
        num_classes = getattr(source, 'num_classes', None)
    with open(path, 'r') as f:
        doc = json.load(f)
    S = float(img_size)
    if not S > 0:
        raise ValueError('img_size must be positive')
    size = {}
    for im in doc.get('images', []):
        if im.get('width') is None or im.get('height') is None:
            raise ValueError('image %r of %s has no width / height' % (im.get('id'), path))
        if not (im['width'] > 0 and im['height'] > 0):
            raise ValueError('image %r of %s has a non-positive size' % (im.get('id'), path))
        size[im['id']] = (float(im['width']), float(im['height']))
    class_of = {}
    for k, c in enumerate(sorted(c['id'] for c in doc.get('categories', []))):
        class_of.setdefault(c, k)
    rows = []
    for a in doc.get('annotations', []):
        w, h = a['bbox'][2], a['bbox'][3]
        if not (w > min_size and h > min_size):
            continue
        cls = class_of[a['category_id']]
        if num_classes is not None and not 0 <= cls < num_classes:
            continue
        if a['image_id'] not in size:
            raise ValueError('annotation %r of %s names image %r, which the file does not list'
                             % (a.get('id'), path, a['image_id']))
        W, H = size[a['image_id']]
        rows.append((float(w) * S / W, float(h) * S / H))
    wh = np.array(rows, dtype=np.float64).reshape(-1, 2).astype(np.float32)
    if len(wh):
        _checked(wh, 'label shapes of %s' % path)
    return wh


def _checked(a, what, rows=None):
    """`a` as contiguous float32 [n, 2] with every value finite and inside (0, MAX_SIDE)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or (rows is not None and a.shape[0] != rows):
        raise ValueError('%s: expected [%s, 2], got %s' % (what, 'n' if rows is None else rows, a.shape))
    if not (np.isfinite(a).all() and (a > 0).all() and (a < MAX_SIDE).all()):
        raise ValueError('%s: every width and height has to lie in (0, %d)' % (what, int(MAX_SIDE)))
    return a


def _device():
    lib()                                                         # raises Y4Error when the library has not been built
    if not torch.cuda.is_available():
        raise Y4Error('anchor fitting runs on an MI355X only (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _shapes_on_device(wh):
    wh = _checked(wh, 'wh')
    if len(wh) > MAX_SHAPES:
        raise ValueError('at most %d shapes, got %d' % (MAX_SHAPES, len(wh)))
    return wh, torch.from_numpy(wh).to(_device())


def _sorted_order(anchors):
    """by area ascending (exact in fp64), ties by the smaller width"""
    a = anchors.astype(np.float64)
    return np.lexsort((a[:, 0], a[:, 0] * a[:, 1]))


# ------------------------------------------------------------------------------------------------------------ k-means
def _assign(wh_d, c, iou_thresh=1.0):
    """one launch, one read-back: acc int64 [k, 5] of the centroids `c`"""
    _, _, acc = ops.anchor_assign_raw(wh_d, torch.from_numpy(c).to(wh_d.device), iou_thresh, want_assign=False, want_iou=False)
    return acc.cpu().numpy()


def _mean_update(c, acc):
    """centroid = sum q / (count * 2^16) in fp64, rounded to fp32; an empty cluster keeps its centroid"""
    new = c.copy()
    filled = acc[:, 0] > 0
    cnt = acc[filled, 0].astype(np.float64) * Q_WH
    new[filled, 0] = (acc[filled, 1].astype(np.float64) / cnt).astype(np.float32)
    new[filled, 1] = (acc[filled, 2].astype(np.float64) / cnt).astype(np.float32)
    return new


def _lloyd(wh_d, c, max_iter):
    """-> (centroids, their acc table, launches of the iteration).  The assignment repeats exactly when the table of
    (count, sum qw, sum qh) repeats -- short of a collision of three 64-bit sums, after which the centroids repeat as well
    and the result is the same -- so the table that is read back anyway decides, and the assignment stays on the device."""
    prev = None
    for it in range(1, max_iter + 1):
        acc = _assign(wh_d, c)
        if prev is not None and np.array_equal(acc[:, :3], prev):
            return c, acc, it
        prev = acc[:, :3].copy()
        c = _mean_update(c, acc)
    return c, _assign(wh_d, c), max_iter


def kmeans_anchors(wh, k, init=None, n_init=8, max_iter=300, seed=0):
    """k anchors by Lloyd iterations under the shape IoU.  -> (anchors float32 [k, 2] sorted by area, info).

    init: an explicit [k, 2] start, run once.  Otherwise n_init starts, each k distinct rows of numpy.unique(wh, axis=0)
    drawn by ONE numpy.random.Generator(PCG64(seed)) with choice(len(unique), k, replace=False), start after start; the start
    whose result has the highest sum of best IoUs wins, the earlier one on ties.
    info: 'iterations' (assignment launches of the winning start), 'mean_best_iou', 'counts' (labels per anchor, in the
    order of the result), 'fitness' (the integer sum of qiou), 'start' (index of the winning start)."""
    k = int(k)
    if not 1 <= k <= MAX_ANCHORS:
        raise ValueError('k must lie in [1, %d]' % MAX_ANCHORS)
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    wh, wh_d = _shapes_on_device(wh)
    if init is not None:
        starts = [_checked(init, 'init', k).copy()]
    else:
        if n_init < 1:
            raise ValueError('n_init must be at least 1')
        uniq = np.unique(wh, axis=0)
        if len(uniq) < k:
            raise ValueError('%d anchors asked of %d distinct shapes' % (k, len(uniq)))
        rng = np.random.Generator(np.random.PCG64(seed))
        starts = [uniq[rng.choice(len(uniq), size=k, replace=False)].copy() for _ in range(int(n_init))]
    best = None
    for s, c0 in enumerate(starts):
        c, acc, it = _lloyd(wh_d, c0, int(max_iter))
        fit = int(acc[:, 3].sum())
        if best is None or fit > best[0]:
            best = (fit, c, acc, it, s)
    fit, c, acc, it, s = best
    order = _sorted_order(c)
    info = {'iterations': it, 'mean_best_iou': fit / (len(wh) * Q_IOU), 'counts': acc[order, 0].tolist(), 'fitness': fit,
            'start': s}
    return c[order], info


# ---------------------------------------------------------------------------------------------------------- evolution
def mutation_factors(rng, population, k, sigma, mutate_prob):
    """[population, k, 2] fp64 factors of one generation.  Draw order on the one stream: rng.standard_normal((G, k, 2)),
    then rng.random((G, k, 2)); factor = clip(1 + sigma * normal * (uniform < mutate_prob), 0.3, 3.0).  The pair of draws
    is repeated while every factor equals 1."""
    while True:
        normal = rng.standard_normal((population, k, 2))
        uniform = rng.random((population, k, 2))
        f = np.clip(1.0 + sigma * normal * (uniform < mutate_prob), 0.3, 3.0)
        if (f != 1.0).any():
            return f


def children_of(parent, factors, min_size):
    """max(parent * factor, min_size) in fp64, rounded once to fp32 (and kept below 65536, the kernels' limit)"""
    c = np.maximum(parent.astype(np.float64)[None] * factors, float(min_size)).astype(np.float32)
    return np.minimum(c, _BELOW_MAX)


def evolve_anchors(wh, anchors, generations=1000, population=64, sigma=0.1, mutate_prob=0.9, thr=0.213, seed=0, min_size=2.0):
    """Mutation and selection from `anchors` on fitness = sum over the labels of the best anchor's IoU (as the integer sum
    of qiou).  Per generation `population` children of the parent (mutation_factors, children_of) are scored in one launch
    and 16 * population bytes come back; the best child (lowest index on ties) replaces the parent only when strictly
    better, so fitness never decreases.  -> (anchors float32 [k, 2] sorted by area, info).

    info: 'fitness' (the parent's, before the first generation and after each one: generations + 1 integers), 'accepted'
    (generations that replaced the parent), 'mean_best_iou', 'above_thr' (share of labels whose best IoU is > thr)."""
    population, generations = int(population), int(generations)
    if not 1 <= population <= MAX_CANDIDATES:
        raise ValueError('population must lie in [1, %d]' % MAX_CANDIDATES)
    if generations < 0 or not (0 < float(min_size) < MAX_SIDE):
        raise ValueError('generations >= 0 and 0 < min_size < %d' % int(MAX_SIDE))
    parent = _checked(anchors, 'anchors').copy()
    k = len(parent)
    if k > MAX_ANCHORS:
        raise ValueError('at most %d anchors' % MAX_ANCHORS)
    wh, wh_d = _shapes_on_device(wh)
    rng = np.random.Generator(np.random.PCG64(seed))

    def score(cand):
        return ops.anchor_fitness_raw(wh_d, torch.from_numpy(np.ascontiguousarray(cand)).to(wh_d.device), thr).cpu().numpy()
    first = score(parent[None])
    fit, above = int(first[0, 0]), int(first[0, 1])
    track, accepted = [fit], 0
    for _ in range(generations):
        cand = children_of(parent, mutation_factors(rng, population, k, sigma, mutate_prob), min_size)
        out = score(cand)
        g = int(np.argmax(out[:, 0]))                       # first maximum
        if int(out[g, 0]) > fit:
            parent, fit, above = cand[g], int(out[g, 0]), int(out[g, 1])
            accepted += 1
        track.append(fit)
    info = {'fitness': track, 'accepted': accepted, 'mean_best_iou': fit / (len(wh) * Q_IOU), 'above_thr': above / len(wh)}
    return parent[_sorted_order(parent)], info


# ------------------------------------------------------------------------------------------------------------- report
def anchor_report(wh, model_cfg, iou_thresh=1.0):
    """How the anchors of a cfg (its MODEL dict, or a whole cfg with one) fit the label shapes `wh`, as a dict:

    n_labels, anchors, masks, iou_thresh
    mean_best_iou   mean over the labels of the best anchor's IoU
    above_half      share of labels whose best IoU is > 0.5
    above_thresh    ... is > iou_thresh
    counts          per anchor, the labels it is the best anchor of
    positives       per layer, the positives the loss creates: the sum over the layer's ANCHOR_MASK of the labels for which
                    the anchor is the best one or has IoU > iou_thresh (CRITERION.IOU_THRESH; 1.0: the best one only)
    unassigned      share of labels whose best anchor is in no layer's mask: they train nothing"""
    model = model_cfg.get('MODEL', model_cfg)
    anchors = _checked(model['ANCHORS'], 'ANCHORS')
    if len(anchors) > MAX_ANCHORS:
        raise ValueError('at most %d anchors' % MAX_ANCHORS)
    masks = [[int(a) for a in m] for m in model.get('ANCHOR_MASK', [[0, 1, 2], [3, 4, 5], [6, 7, 8]])]
    if any(not 0 <= a < len(anchors) for m in masks for a in m):
        raise ValueError('ANCHOR_MASK names an anchor the cfg does not have')
    wh, wh_d = _shapes_on_device(wh)
    n = len(wh)
    acc = _assign(wh_d, anchors, iou_thresh)
    one = torch.from_numpy(anchors[None]).to(wh_d.device)
    half = ops.anchor_fitness_raw(wh_d, one, 0.5).cpu().numpy()
    above = ops.anchor_fitness_raw(wh_d, one, iou_thresh).cpu().numpy()
    masked = sorted(set(a for m in masks for a in m))
    return {'n_labels': n, 'anchors': anchors.tolist(), 'masks': masks, 'iou_thresh': float(iou_thresh),
            'mean_best_iou': int(acc[:, 3].sum()) / (n * Q_IOU), 'above_half': int(half[0, 1]) / n,
            'above_thresh': int(above[0, 1]) / n, 'counts': acc[:, 0].tolist(),
            'positives': [int(acc[m, 4].sum()) for m in masks],
            'unassigned': (n - int(acc[masked, 0].sum())) / n}


def format_report(rep):
    lines = ['%d labels, %d anchors, iou_thresh %g' % (rep['n_labels'], len(rep['anchors']), rep['iou_thresh']),
             '  mean best IoU %.4f; best IoU > 0.5: %.2f %%; > iou_thresh: %.2f %%'
             % (rep['mean_best_iou'], 100 * rep['above_half'], 100 * rep['above_thresh'])]
    for a, ((w, h), c) in enumerate(zip(rep['anchors'], rep['counts'])):
        layers = [str(l) for l, m in enumerate(rep['masks']) if a in m]
        lines.append('  anchor %2d  %8.1f x %-8.1f best for %8d labels  (%s)'
                     % (a, w, h, c, 'layer ' + ', '.join(layers) if layers else 'in no mask'))
    for l, p in enumerate(rep['positives']):
        lines.append('  layer %d (mask %s): %d positives' % (l, rep['masks'][l], p))
    lines.append('  labels whose best anchor is in no mask: %.2f %%' % (100 * rep['unassigned']))
    return '\n'.join(lines)


def format_cfg(anchors, n_layers):
    """The `ANCHORS:` and `ANCHOR_MASK:` YAML lines for k = 3 * n_layers anchors (else ValueError: the loss takes masks with
    mask[a] % 3 == a only).  Values are rounded to the nearest integer (ties to even), never below 1; the masks are
    consecutive triples, the smallest anchors on layer 0."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 2)
    n_layers = int(n_layers)
    if n_layers < 1 or len(a) != 3 * n_layers:
        raise ValueError('%d layers take %d anchors, got %d' % (n_layers, 3 * n_layers, len(a)))
    r = np.maximum(np.rint(a), 1.0).astype(np.int64)
    masks = [[3 * l, 3 * l + 1, 3 * l + 2] for l in range(n_layers)]
    return 'ANCHORS: [%s]\nANCHOR_MASK: [%s]' % (', '.join('[%d, %d]' % (w, h) for w, h in r),
                                                 ', '.join('[%d, %d, %d]' % tuple(m) for m in masks))


# ---------------------------------------------------------------------------------------------------------------- CLI
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m yolov4_amd.yolo.util.anchors',
                                 description='Check a cfg\'s anchors against a dataset\'s labels and fit better ones')
    ap.add_argument('data', metavar='DATA', help='dataset root (with annotations/instances_<split>.json) or an annotation file')
    ap.add_argument('-c', '--cfg', required=True, help='cfg file (JSON, or YAML when the yaml package is there)')
    ap.add_argument('--split', default='train2017')
    ap.add_argument('--img-size', type=int, default=None, help='S of the S x S stretch (default: TRAIN.IMGSIZE, else TEST.IMGSIZE)')
    ap.add_argument('--k', type=int, default=None, help='anchors to fit (default: as many as the cfg has)')
    ap.add_argument('--n-init', type=int, default=8)
    ap.add_argument('--evolve', type=int, default=0, metavar='GENERATIONS')
    ap.add_argument('--population', type=int, default=64)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--check', action='store_true', help='report on the cfg\'s anchors only')
    return ap


def annotation_path(data, split):
    if os.path.isdir(data):
        return os.path.join(data, 'annotations', 'instances_%s.json' % split)
    return data


def main(argv=None):
    from ...detect import load_cfg
    args = build_parser().parse_args(argv)
    cfg = load_cfg(args.cfg)
    model = cfg.get('MODEL', cfg)
    S = args.img_size
    if S is None:
        S = cfg.get('TRAIN', {}).get('IMGSIZE') or cfg.get('TEST', {}).get('IMGSIZE')
        if S is None:
            raise SystemExit('the cfg names no image size: give --img-size')
    thresh = float(cfg.get('CRITERION', {}).get('IOU_THRESH', 1.0))
    wh = label_shapes(annotation_path(args.data, args.split), int(S), num_classes=model.get('N_CLASSES'))
    if len(wh) == 0:
        raise SystemExit('no labels')
    print('anchors of %s at %d x %d' % (args.cfg, S, S))
    print(format_report(anchor_report(wh, model, thresh)))
    if args.check:
        return 0
    k = args.k if args.k is not None else len(model['ANCHORS'])
    anchors, info = kmeans_anchors(wh, k, n_init=args.n_init, seed=args.seed)
    print('k-means: %d iterations, mean best IoU %.4f' % (info['iterations'], info['mean_best_iou']))
    if args.evolve > 0:
        anchors, info = evolve_anchors(wh, anchors, generations=args.evolve, population=args.population, seed=args.seed)
        print('evolution: %d of %d generations accepted, mean best IoU %.4f' % (info['accepted'], args.evolve, info['mean_best_iou']))
    if k % 3 == 0:
        n_layers = k // 3
        fitted = dict(model, ANCHORS=[[float(w), float(h)] for w, h in anchors],
                      ANCHOR_MASK=[[3 * l, 3 * l + 1, 3 * l + 2] for l in range(n_layers)])
        print('fitted anchors')
        print(format_report(anchor_report(wh, fitted, thresh)))
        print(format_cfg(anchors, n_layers))
    else:
        print('fitted anchors (k is no multiple of 3: no ANCHOR_MASK the loss accepts)')
        print(', '.join('[%.1f, %.1f]' % (w, h) for w, h in anchors))
    return 0


if __name__ == '__main__':
    sys.exit(main())
