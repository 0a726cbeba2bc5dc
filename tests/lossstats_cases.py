# -*- coding: utf-8 -*-
"""Per-layer training statistics of the detection loss (y4_yolo_loss_stats_f64), restated in
numpy, and the inputs of their tests (tests/test_lossstats_cases.py checks the restatement and the inputs without a GPU,
tests/test_gpu_lossstats.py feeds them to the kernel of csrc/yolo_loss.hip).

The restatement stands on what headopt_cases / lossopt_cases.loss_ref already restate exactly: the positive set (one
record per cell, class bits OR-ed, box of the last writer), the cells and the ignore mask.  X, the plain IoU of a
positive cell's pred and its record's box, comes from boxloss_cases through headopt_cases.box_ref, in float64 (the
reference) and in float32 (the yardstick: what plain fp32 arithmetic achieves).  The sums are math.fsum of the exact
values: fsum(X) in either precision, and fsum of the fp32 numbers in `output`.

Plain module, no fixtures."""
import functools
import math

import numpy as np

import boxloss_cases as BC
import head_cases as HC
import headopt_cases as HO
import lossopt_cases as LO
from oracle import head as H

F32 = np.float32

ROWS = ('n_cells', 'n_pos', 'n_ign', 'sum_iou', 'n_iou50', 'n_iou75', 'sum_obj_pos', 'sum_obj_bg', 'n_bg', 'sum_cls',
        'n_cls', 'n_top1')
COUNTS = (0, 1, 2, 4, 5, 8, 10, 11)
EXACT_SUMS = (6, 7, 9)                                          # fp64 sums of fp32 values: only the order differs from fsum
SUM_IOU = 3
MARGIN = 1e-4                                                   # no float64 X of a GPU input is this close to 0.5 / 0.75

# Largest kernel |sum_iou - ref64| / the fp32 yardstick's largest |sum_iou32 - sum_iou64| over the SETS cases, measured on
# an MI355X by tests/test_gpu_lossstats.py (it prints the figure before it asserts; bar BOX_FACTOR = 4)
MEASURED_SUM_IOU = 0.176


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def stats_ref(output, pred, ref, dtype=np.float64):
    """The twelve numbers of one layer from the loss restatement `ref` (lossopt_cases.loss_ref with label_smooth = 0 on
    the same output, pred and labels), X evaluated in `dtype`.  Returns (row [12] float64, extras): extras holds X, the
    number of terms and the sum of magnitudes of each exact sum (the derived fp64 summation bound), and the class rows
    of the positive cells."""
    output = np.asarray(output, F32)
    pos = ref['tgt_mask'][..., 0] > 0
    om = ref['obj_mask']
    cells = HO.record_cells(ref['info'])
    assert int(pos.sum()) == len(cells)                        # one record per positive cell
    if len(cells):
        x = dtype(1) - HO.box_ref(pred, ref['info'], 'iou', 1.0, 1.0, dtype)['per_record']
        assert x.dtype == dtype
    else:
        x = np.zeros(0, dtype)
    x64 = x.astype(np.float64)
    with np.errstate(invalid='ignore'):
        n50, n75 = int((x > dtype(0.5)).sum()), int((x > dtype(0.75)).sum())
    obj = output[..., 4].astype(np.float64)
    bg = ~pos & (om != 0)
    bits = np.asarray(ref['target'][..., 5:][pos]) > 0.5       # label_smooth = 0: the targets are the bits
    cls = output[..., 5:][pos]
    top = cls.argmax(axis=1) if len(cls) else np.zeros(0, np.int64)      # the first of equal maxima
    row = np.array([pos.size, pos.sum(), (om == 0).sum(), _fsum(x64), n50, n75, _fsum(obj[pos]), _fsum(obj[bg]), bg.sum(),
                    _fsum(cls[bits]), bits.sum(), bits[np.arange(len(top)), top].sum()], np.float64)
    terms = {6: obj[pos], 7: obj[bg], 9: cls[bits].astype(np.float64)}
    extras = dict(X=x, n={q: int(v.size) for q, v in terms.items()}, mag={q: _fsum(np.abs(v)) for q, v in terms.items()},
                  cls=cls, bits=bits, cells=cells)
    return row, extras


def sum_bound(extras, q):
    """n * 2^-52 * sum|x|: what the order of an fp64 summation of n exact terms can move it from fsum"""
    return extras['n'][q] * 2.0 ** -52 * extras['mag'][q]


def summary_ref(row):
    s = dict(zip(ROWS, row))

    def ratio(a, b):
        return a / b if b else math.nan
    return dict(count=int(s['n_pos']), avg_iou=ratio(s['sum_iou'], s['n_pos']), r50=ratio(s['n_iou50'], s['n_pos']),
                r75=ratio(s['n_iou75'], s['n_pos']), obj=ratio(s['sum_obj_pos'], s['n_pos']),
                no_obj=ratio(s['sum_obj_bg'], s['n_bg']), cls=ratio(s['sum_cls'], s['n_cls']),
                top1=ratio(s['n_top1'], s['n_pos']), ignored=int(s['n_ign']))


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests
SOURCES = ('plain', 'box')
IOU_THRESH = (1.0, 0.213)


def layers_of(C, K, source):
    """(labels, cfg, [(output, pred)] per layer) of lossopt_cases.plain_layers / box_layers"""
    return LO.plain_layers(C, K) if source == 'plain' else LO.box_layers(C, K)


@functools.lru_cache(maxsize=None)
def set_reference(C, K, source, l, iou_thresh, f32=False):
    """(row, extras) of layer l of a SETS case, computed once and shared; read-only"""
    labels, cfg, layers = layers_of(C, K, source)
    ref = LO.reference(C, K, source, l, None, iou_thresh, 0.0)
    return stats_ref(layers[l][0], layers[l][1], ref, F32 if f32 else np.float64)


@functools.lru_cache(maxsize=None)
def sum_iou_fp32_error():
    """the fp32 yardstick's largest |sum_iou32 - sum_iou64| over SETS x sources x 3 layers x both iou_thresh"""
    e = 0.0
    for C, K in LO.SETS:
        for source in SOURCES:
            for l in range(3):
                for it in IOU_THRESH:
                    a, b = set_reference(C, K, source, l, it)[0], set_reference(C, K, source, l, it, True)[0]
                    e = max(e, abs(b[SUM_IOU] - a[SUM_IOU]))
    return e


@functools.lru_cache(maxsize=None)
def x_fp32_error():
    """the fp32 yardstick's largest per-record |X32 - X64| over the same cases: the bound of an edge case's sum_iou is
    n_pos x BOX_FACTOR x this (each term held by the rule for X, summed by the triangle inequality)"""
    e = 0.0
    for C, K in LO.SETS:
        for source in SOURCES:
            for l in range(3):
                for it in IOU_THRESH:
                    a, b = set_reference(C, K, source, l, it)[1]['X'], set_reference(C, K, source, l, it, True)[1]['X']
                    if len(a):
                        e = max(e, float(np.abs(b.astype(np.float64) - a).max()))
    return e


# name: (B, F, layer, C, K, labels per image).  A is 3 in every layer of this head, so B * A * F * F = 257 (a prime) cannot
# be had: 258 = 86 * 3 * 1 * 1 is the smallest cell count above one 256-thread block, two cells into the second.
EDGES = {
    'B1-F1': (1, 1, 2, 3, 4, (2,)),
    'C1': (2, 4, 2, 1, 6, (6, 3)),
    'one-empty-image': (3, 4, 1, 5, 5, (5, 0, 2)),
    'no-labels': (2, 4, 1, 5, 5, (0, 0)),
    'cells-258': (86, 1, 2, 3, 2, tuple(q % 3 for q in range(86))),
}


@functools.lru_cache(maxsize=None)
def edge_case(name, seed=0):
    """dict(labels, cfg, l, output, pred, ref): a small layer of its own shape, decoded by the oracle from normal logits"""
    B, Fs, l, C, K, counts = EDGES[name]
    rng = np.random.RandomState(1000 + seed + sum(map(ord, name)))
    cfg = HC.cfg_with_classes(C)
    S = Fs * H.STRIDES[l]
    lg = rng.normal(0.0, 1.5, (B, 3 * (5 + C), Fs, Fs)).astype(F32)
    output, pred = H.yolo_decode(lg, l, cfg, True)
    labels = np.zeros((B, K, 5), np.float64)
    aw, ah = np.array(cfg['ANCHORS'], np.float64)[cfg['ANCHOR_MASK'][l]].T
    for b, n in enumerate(counts):
        labels[b, :n, 0:2] = rng.uniform(1.0, S - 1.0, (n, 2))
        q = rng.randint(0, 3, n)                                # sizes near the layer's anchors, so the layer gets positives
        labels[b, :n, 2] = aw[q] * rng.uniform(0.8, 1.2, n)
        labels[b, :n, 3] = ah[q] * rng.uniform(0.8, 1.2, n)
        labels[b, :n, 4] = rng.randint(0, C, n)
    with np.errstate(invalid='ignore'):                         # a box larger than a one- or four-cell map: tgt_scale is NaN, unused here
        ref = LO.loss_ref(output, pred, l, labels, cfg, 0.7, 1.0, 0.0)
    for a in (output, pred, labels):
        a.setflags(write=False)
    row, extras = stats_ref(output, pred, ref)
    return dict(labels=labels, cfg=cfg, l=l, output=output, pred=pred, ref=ref, row=row, extras=extras, C=C)


def gpu_inputs():
    """(tag, row, extras) of every input the GPU tests count on"""
    for C, K in LO.SETS:
        for source in SOURCES:
            for l in range(3):
                for it in IOU_THRESH:
                    yield ('C%d-K%d-%s-l%d-iou%g' % (C, K, source, l, it),) + set_reference(C, K, source, l, it)
    for name in EDGES:
        e = edge_case(name)
        yield name, e['row'], e['extras']


def flip_margin(x64):
    """smallest distance of a float64 X from 0.5 / 0.75 (inf without records)"""
    x = np.asarray(x64, np.float64)
    x = x[np.isfinite(x)]
    return float(min(np.abs(x - 0.5).min(), np.abs(x - 0.75).min())) if len(x) else math.inf


def max_ties(cls):
    """positive cells with two class channels equal at the maximum"""
    cls = np.asarray(cls)
    if not len(cls) or cls.shape[1] < 2:
        return 0
    return int(((cls == cls.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
