# -*- coding: utf-8 -*-
"""The IoU-family box losses (IoU / GIoU / DIoU / CIoU) restated in numpy, and the seeded inputs of their tests
(tests/test_boxloss_cases.py checks the restatement and the inputs without a GPU, tests/test_gpu_boxloss.py feeds the
inputs to the kernels of csrc/yolo_loss.hip).

`box_eval` is written once and evaluated in the dtype of its inputs: in float64 it is the reference, in float32 (every
operation rounded, absolute grid coordinates) it is the yardstick of the tolerance: a kernel may be BOX_FACTOR times as
far from the float64 result as this plain float32 evaluation of the same formulas is.

Plain module, no fixtures."""
import functools

import numpy as np

import head_cases as HC
from oracle import head as H

F32 = np.float32
KINDS = ('iou', 'giou', 'diou', 'ciou')
KIND_IDS = {'iou': 1, 'giou': 2, 'diou': 3, 'ciou': 4}           # Y4_BOX_* of include/yolov4_amd.h
EPS = float(F32(1e-7))                                           # the fp32 value: both evaluations see the same number

BOX_C = (1, 33)
BOX_K = (1, 64, 65)
GAINS = (1.0, 0.05)

# A kernel result may be BOX_FACTOR x the plain-fp32 evaluation's own error away from float64: room for another, equally
# valid operation order and for a device atanf / division a few ulp off the host's.  Measured on an MI355X over
# BOX_C x BOX_K x 3 layers x GAINS (kernel error / fp32-restatement error, worst case per kind): MEASURED below -- the
# kernels work relative to the cell origin, which keeps the grid offset out of the corner differences.
BOX_FACTOR = 4.0
MEASURED = {'iou': (0.101, 0.110), 'giou': (0.146, 0.487), 'diou': (0.185, 0.203), 'ciou': (0.203, 0.200)}   # (loss, gradient)

PLANTS = ('equal', 'disjoint', 'pred_in_truth', 'truth_in_pred', 'aspect_1_40', 'aspect_40_1', 'touching', 'thin', 'generic')
TIE_PLANTS = ('equal', 'touching')                               # exact ties of min / max: judged on the loss only


# ------------------------------------------------------------------------------------------ the formulas
def box_eval(p, t, kind):
    """p, t: [N, 4] boxes (xc, yc, w, h) of one dtype (float64 or float32), grid units.  Returns (loss [N], grad [N, 4]):
    loss = 1 - X with X the IoU / GIoU / DIoU / CIoU of the pair, grad = d loss / d(px, py, log pw, log ph) in closed
    form -- (dL/dpx, dL/dpy, dL/dpw * pw, dL/dph * ph), the gradient wrt the train-mode `output` of the decode.  alpha
    of CIoU is a constant in the gradient.  Ties: a corner of p is the selected operand of min / max only under a
    strict inequality; the clamp of the intersection extent passes a gradient only where the raw extent is > 0."""
    if kind not in KINDS:
        raise KeyError(kind)
    p = np.asarray(p)
    t = np.asarray(t)
    dt = p.dtype.type
    assert p.dtype == t.dtype and dt in (np.float64, np.float32)
    eps, two, half, one, zero = dt(EPS), dt(2), dt(0.5), dt(1), dt(0)
    px, py, pw, ph = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    tx, ty, tw, th = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    pl, pr, pt, pb = px - pw / two, px + pw / two, py - ph / two, py + ph / two
    tl, tr, tt, tb = tx - tw / two, tx + tw / two, ty - th / two, ty + th / two
    iwr = np.minimum(pr, tr) - np.maximum(pl, tl)
    ihr = np.minimum(pb, tb) - np.maximum(pt, tt)
    iw, ih = np.maximum(zero, iwr), np.maximum(zero, ihr)
    inter = iw * ih
    uni = ((pw * ph + tw * th) - inter) + eps
    iou = inter / uni
    f = lambda m: m.astype(p.dtype)
    ar, al = f((pr < tr) & (iwr > 0)), f((pl > tl) & (iwr > 0))
    ab, at = f((pb < tb) & (ihr > 0)), f((pt > tt) & (ihr > 0))
    dI = [ih * (ar - al), iw * (ab - at), ih * ((ar + al) / two), iw * ((ab + at) / two)]
    dU = [-dI[0], -dI[1], ph - dI[2], pw - dI[3]]
    d = [(dI[k] - iou * dU[k]) / uni for k in range(4)]
    x = iou
    if kind != 'iou':
        cw = np.maximum(pr, tr) - np.minimum(pl, tl)
        ch = np.maximum(pb, tb) - np.minimum(pt, tt)
        cr, cl, cb, ct = f(pr > tr), f(pl < tl), f(pb > tb), f(pt < tt)
        dcw = [cr - cl, None, (cr + cl) / two, None]
        dch = [None, cb - ct, None, (cb + ct) / two]
        if kind == 'giou':
            ca = cw * ch + eps
            x = iou - (ca - uni) / ca
            ca2 = ca * ca
            d[0] = (d[0] + dU[0] / ca) - uni * (ch * dcw[0]) / ca2
            d[1] = (d[1] + dU[1] / ca) - uni * (cw * dch[1]) / ca2
            d[2] = (d[2] + dU[2] / ca) - uni * (ch * dcw[2]) / ca2
            d[3] = (d[3] + dU[3] / ca) - uni * (cw * dch[3]) / ca2
        else:
            c2 = (cw * cw + ch * ch) + eps
            ex, ey = px - tx, py - ty
            rho2 = ex * ex + ey * ey
            x = iou - rho2 / c2
            c4 = c2 * c2
            d[0] = d[0] - ((two * ex) * c2 - rho2 * ((two * cw) * dcw[0])) / c4
            d[1] = d[1] - ((two * ey) * c2 - rho2 * ((two * ch) * dch[1])) / c4
            d[2] = d[2] + (rho2 * ((two * cw) * dcw[2])) / c4
            d[3] = d[3] + (rho2 * ((two * ch) * dch[3])) / c4
            if kind == 'ciou':
                phe = ph + eps
                da = np.arctan(tw / (th + eps)) - np.arctan(pw / phe)
                v = (dt(4.0 / np.pi ** 2) * da) * da
                alpha = v / (((one - iou) + v) + eps)
                x = x - alpha * v
                den = phe * phe + pw * pw
                k = dt(8.0 / np.pi ** 2) * da
                d[2] = d[2] + alpha * ((k * phe) / den)
                d[3] = d[3] - alpha * ((k * pw) / den)
    loss = one - x
    grad = np.stack([-d[0], -d[1], -(d[2] * pw), -(d[3] * ph)], 1)
    assert loss.dtype == p.dtype and grad.dtype == p.dtype
    return loss, grad


def box_quantities(p, t):
    """(iou, giou, diou, ciou) [N] each of float64 boxes: what the range checks look at."""
    return tuple(1.0 - box_eval(np.asarray(p, np.float64), np.asarray(t, np.float64), k)[0] for k in KINDS)


def exact_ties(p, t):
    """[N] bool: a pair of corners compared by min / max is equal, or an intersection extent is exactly 0."""
    p = np.asarray(p, np.float64)
    t = np.asarray(t, np.float64)
    tie = np.zeros(len(p), bool)
    for c, s in ((0, 2), (1, 3)):
        plo, phi = p[:, c] - p[:, s] / 2, p[:, c] + p[:, s] / 2
        tlo, thi = t[:, c] - t[:, s] / 2, t[:, c] + t[:, s] / 2
        tie |= (plo == tlo) | (phi == thi) | (np.minimum(phi, thi) - np.maximum(plo, tlo) == 0)
    return tie


# ------------------------------------------------------------------------------------------ a layer
def positives(output, pred, labels, cfg, layer_no):
    """The positive cells of a layer and their last-writer truth boxes, from oracle.head.build_target plus the labels:
    (cells [N, 4] int (b, a, j, i) in (image, record) order as np.argwhere gives them, truth [N, 4] fp32 = label / stride,
    label_idx [N]).  The record of a cell is written by every label that hits it; its regression targets -- and so its
    truth box -- are those of the LAST one, found here as the last label of the image whose targets are the cell's."""
    output = np.asarray(output, F32)
    target, _, tgt_mask, _ = H.build_target(output, np.asarray(pred, F32), layer_no, labels, cfg, 0.7)
    lab = np.asarray(labels).astype(F32)
    st = F32(H.STRIDES[layer_no])
    manc = H.masked_anchors(cfg, layer_no)
    n = (lab.sum(axis=2, dtype=F32) > 0).sum(axis=1)
    box = (lab[:, :, :4] / st).astype(F32)
    cells = np.argwhere(tgt_mask[..., 0] > 0)
    truth = np.zeros((len(cells), 4), F32)
    idx = np.zeros(len(cells), np.int64)
    for q, (b, a, j, i) in enumerate(cells):
        want = target[b, a, j, i, :4]
        hit = -1
        for u in range(int(n[b])):
            tx, ty, tw, th = box[b, u]
            with np.errstate(divide='ignore'):
                mine = np.array([tx - F32(np.int16(tx)), ty - F32(np.int16(ty)), np.log(tw / manc[a, 0] + F32(1e-16)),
                                 np.log(th / manc[a, 1] + F32(1e-16))], F32)
            if int(np.int16(tx)) == i and int(np.int16(ty)) == j and np.array_equal(mine, want):
                hit = u
        assert hit >= 0, (layer_no, b, a, j, i)
        truth[q] = box[b, hit]
        idx[q] = hit
    return cells, truth, idx


def layer_box_loss(output, pred, labels, cfg, kind, gain, layer_no, dtype=np.float64, pos=None):
    """The box loss of one layer restated: loss = gain * sum over the positive cells of (1 - X), per-record gradient
    wrt output[..., 0:4] times gain.  `output` only fixes the shape (the box is read from pred).  dtype float32: the
    plain fp32 evaluation on the same fp32 inputs (records summed in float64, like the kernel).  pos: what `positives`
    returned for these inputs, when the caller has it already."""
    cells, truth, idx = pos if pos is not None else positives(output, pred, labels, cfg, layer_no)
    pred = np.asarray(pred, F32)
    p = np.stack([pred[b, a, j, i] for b, a, j, i in cells]).astype(dtype) if len(cells) else np.zeros((0, 4), dtype)
    t = truth.astype(dtype)
    loss, grad = box_eval(p, t, kind) if len(cells) else (np.zeros(0, dtype), np.zeros((0, 4), dtype))
    g = dtype(gain) if dtype is F32 else float(F32(gain))
    return dict(loss=float(loss.astype(np.float64).sum()) * float(F32(gain)), per_record=loss, grad=grad * g,
                cells=cells, p=p, t=t, label_idx=idx, ties=exact_ties(p, t))


# ------------------------------------------------------------------------------------------ inputs
def plant(kind, t, a):
    """A predicted box of the geometric class `kind` for the truth t = (tx, ty, tw, th) (fp32), `a` in [0, 1)."""
    tx, ty, tw, th = [float(v) for v in t]
    s = float(np.sqrt(max(tw * th, 1e-4) / 40.0))
    return {
        'equal': (tx, ty, tw, th),
        'disjoint': (tx + tw + 1.0 + a, ty - 0.3 * th, 0.5 * tw + 0.01, 0.8 * th + 0.01),
        'pred_in_truth': (tx + 0.1 * tw, ty - 0.05 * th, 0.5 * tw, 0.6 * th),
        'truth_in_pred': (tx - 0.1 * tw, ty + 0.05 * th, 1.7 * tw + 0.01, 1.5 * th + 0.01),
        'aspect_1_40': (tx + 0.2 * a, ty - 0.1, s, 40.0 * s),
        'aspect_40_1': (tx - 0.1, ty + 0.2 * a, 40.0 * s, s),
        # the left edge of p on the right edge of t, up to the rounding of tx + tw
        'touching': (float(F32(F32(tx) + F32(tw))), ty + 0.25 * th, tw, th),
        'thin': (tx + 0.1 * tw * a, ty + 0.1 * th, 1e-3, 0.9 * th + 0.01),
    }[kind]


@functools.lru_cache(maxsize=None)
def make_case(C, K):
    """Three images at 128 px, the three layers F = (16, 8, 4): per layer a dict with `output`, `pred` [3, 3, F, F, .] fp32
    (oracle decode of head_cases.make_loss_logits, pred then planted at the positive cells, class q % 9 of PLANTS for
    the q-th positive of the case counted over the three layers), `labels` [3, K, 5], `plants` [N] names in the cell
    order of `positives`.  Arrays are read-only: the tests share them."""
    cfg = HC.cfg_with_classes(C)
    labels = HC.make_labels(K, C, 100 + K)[0]
    logits = HC.make_loss_logits(C, 900)[0]
    layers = []
    q = 0
    for l, lg in enumerate(logits):
        out, pred = H.yolo_decode(lg, l, cfg, True)
        cells, truth, idx = positives(out, pred, labels, cfg, l)
        names = []
        for (b, a, j, i), t in zip(cells, truth):
            name = PLANTS[q % len(PLANTS)]
            if name != 'generic':
                pred[b, a, j, i] = np.array(plant(name, t, (q * 0.37) % 1.0), F32)
            names.append(name)
            q += 1
        for arr in (out, pred, lg):
            arr.setflags(write=False)
        layers.append(dict(logits=lg, output=out, pred=pred, plants=names, n_pos=len(cells), pos=(cells, truth, idx)))
    labels.setflags(write=False)
    return dict(cfg=cfg, labels=labels, layers=layers, C=C, K=K)


def plant_counts(case):
    n = {k: 0 for k in PLANTS}
    for lay in case['layers']:
        for k in lay['plants']:
            n[k] += 1
    return n


def judged_rows(ref, plants):
    """[N] bool: records whose gradient is compared (no exact tie of min / max in either box pair)."""
    return ~(ref['ties'] | np.array([k in TIE_PLANTS for k in plants], bool))


def row_rel_err(got, ref_grad):
    """per record: max |got - ref| over its four components / its largest |ref| component"""
    ref_grad = np.asarray(ref_grad, np.float64)
    if len(ref_grad) == 0:
        return np.zeros(0)
    scale = np.abs(ref_grad).max(axis=1)
    err = np.abs(np.asarray(got, np.float64) - ref_grad).max(axis=1)
    return err / np.maximum(scale, HC.TINY)


@functools.lru_cache(maxsize=None)
def references(C, K, kind, gain):
    """Per layer (ref64, ref32) of layer_box_loss on make_case(C, K)."""
    case = make_case(C, K)
    out = []
    for l, lay in enumerate(case['layers']):
        a = (lay['output'], lay['pred'], case['labels'], case['cfg'], kind, gain, l)
        out.append((layer_box_loss(*a, pos=lay['pos']), layer_box_loss(*a, dtype=F32, pos=lay['pos'])))
    return out


@functools.lru_cache(maxsize=None)
def fp32_errors(kind, gain):
    """The plain-fp32 evaluation's own error over the whole case set BOX_C x BOX_K x 3 layers at one kind and gain:
    (largest |loss32 - loss64| of a layer, largest row-relative gradient error of a judged record)."""
    e_loss = e_grad = 0.0
    for C in BOX_C:
        for K in BOX_K:
            case = make_case(C, K)
            for (r64, r32), lay in zip(references(C, K, kind, gain), case['layers']):
                e_loss = max(e_loss, abs(r32['loss'] - r64['loss']))
                rows = judged_rows(r64, lay['plants'])
                if rows.any():
                    e_grad = max(e_grad, float(row_rel_err(r32['grad'][rows], r64['grad'][rows]).max()))
    return e_loss, e_grad


def bounds(kind, gain):
    """(loss bound, row-relative gradient bound) of a kernel result at this kind and gain."""
    e_loss, e_grad = fp32_errors(kind, gain)
    return BOX_FACTOR * e_loss, BOX_FACTOR * e_grad
