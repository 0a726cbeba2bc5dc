# -*- coding: utf-8 -*-
"""The YOLOv4 head options -- scale_x_y, several positive anchors per label (iou_thresh), class label smoothing --
restated in numpy, and the seeded inputs of their tests (tests/test_headopt_cases.py checks the restatement and the
inputs without a GPU, tests/test_gpu_headopt.py feeds the inputs to the kernels of csrc/yolo_decode.hip and csrc/yolo_loss.hip).

The rules (include/yolov4_amd.h):
  scale_x_y   s fp32 in [1, 2], h = (s - 1) * 0.5f in fp32: pred centre = ((sigma * s) - h) + cell, `output` keeps sigma;
              d pred / d output = s on channels 0 and 1.
  iou_thresh  the positive anchors of a label are its arg-max anchor and every anchor whose fp32 shape IoU is > iou_thresh;
              (label, anchor slot) pairs in the order of t, then of the slot; records numbered by first hit.
  label_smooth  class BCE targets 1 - 0.5 eps where the class bit is set, 0.5 eps where it is not (fp32 values).

`loss_ref` is written once and evaluated in a dtype, like boxloss_cases.box_eval: the positive set, the cells and the
ignore mask are always float32 in the kernel's operation order (so they are exact); the targets and the per-element loss
terms are float64 on the fp32 inputs (the reference of the GPU tests) or float32 in oracle.head's order (which, with
the options off, must reproduce oracle.head exactly: test_headopt_cases.py).  Sums are float64 either way.

Plain module, no fixtures."""
import functools

import numpy as np

import boxloss_cases as BC
import head_cases as HC
from oracle import head as H

F32 = np.float32

SCALES = (1.0, (1.2, 1.1, 1.05), 2.0)
EPS = (0.0, 0.1)
IOU_THRESH = (1.0, 0.213)
HEAD_C = (1, 33)
HEAD_K = (1, 64, 65, 100)

# decode: head_cases.DEC_CONST / BWD_CONST plus the roundings the option adds -- the product sigma * s and the subtraction
# of h in the forward (2), the product s * g_pred in the backward (1).  Derived, not measured.
DEC_CONST = HC.DEC_CONST + 2.0          # measured on an MI355X over DECODE_CASES, s in (1.2, 2.0): 0.93 is the largest needed
BWD_CONST = HC.BWD_CONST + 1.0          # measured likewise: 1.97 is the largest constant needed
MEASURED_DECODE = {'train': 0.93, 'eval': 0.93, 'backward': 1.97}
# kernel error / fp32-restatement error of the box loss with several anchors and s != 1, measured on an MI355X over
# BOX_SETS x 3 layers x boxloss_cases.GAINS, worst case per kind (loss, gradient), as boxloss_cases.MEASURED
MEASURED_BOX = {'iou': (0.181, 0.132), 'giou': (0.375, 0.828), 'diou': (0.087, 0.115), 'ciou': (0.318, 0.117)}


def scale_of(scale, layer_no):
    return float(scale[layer_no]) if isinstance(scale, (tuple, list)) else float(scale)


def s_h(scale_xy):
    """(s, h) as the fp32 values the kernels use, returned as Python floats"""
    s = F32(scale_xy)
    h = (s - F32(1)) * F32(0.5)
    return float(s), float(h)


def smooth_targets(eps):
    """(lo, hi) = (0.5 eps, 1 - 0.5 eps) evaluated in fp32, as Python floats"""
    lo = F32(0.5) * F32(eps)
    hi = F32(1) - lo
    return float(lo), float(hi)


# ------------------------------------------------------------------------------------------ decode
def decode_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, stride, train, scale_xy=1.0):
    """head_cases.decode_ref64 with the centre ((sigma * s) - h) + cell; also returns S [.., 2], the sum of the absolute
    addends sigma * s + h + cell (times stride in eval) of the two centre channels, in the result's layout:
    train -> (output, pred, S [B,A,F,F,2]); eval -> (rows [B, A*F*F, 5+C], S [B, A*F*F, 2])."""
    s, h = s_h(scale_xy)
    out, pred = HC.decode_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, stride, True)
    gx = np.arange(F, dtype=np.float64).reshape(1, 1, 1, F)
    gy = np.arange(F, dtype=np.float64).reshape(1, 1, F, 1)
    pred = pred.copy()
    pred[..., 0] = (out[..., 0] * s - h) + gx
    pred[..., 1] = (out[..., 1] * s - h) + gy
    S = np.stack([out[..., 0] * s + h + gx, out[..., 1] * s + h + gy], -1)
    if train:
        return out, pred, S
    rows = HC.decode_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, stride, False).copy()
    rows[..., 0:2] = (pred[..., 0:2] * float(stride)).reshape(B, A * F * F, 2)
    return rows, (S * float(stride)).reshape(B, A * F * F, 2)


def decode_xy_accept(got, ref64, v, S, const=DEC_CONST):
    """Per-element acceptance of a decoded centre: |got - ref| <= (|v| + const) * 2^-23 * S, or <= 2^-126.  S, not |ref|:
    sigma * s - h cancels near a cell's lower border.  NaN never passes."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - np.asarray(ref64, np.float64))
    ok = err <= (np.abs(np.asarray(v, np.float64)) + const) * 2.0 ** -23 * np.asarray(S, np.float64)
    ok |= err <= HC.TINY
    return ok & ~np.isnan(got)


def decode_xy_needed(got, ref64, v, S):
    """the constant decode_xy_accept would need"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64))
    need = err / (2.0 ** -23 * np.asarray(S, np.float64)) - np.abs(np.asarray(v, np.float64))
    need = need[err > HC.TINY]
    return float(need.max()) if need.size else 0.0


def decode_bwd_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, g_output, g_pred, scale_xy=1.0):
    """head_cases.decode_bwd_ref64 with d pred / d output = s on channels 0 and 1: the addend is |s * g_pred|."""
    s, _ = s_h(scale_xy)
    if g_pred is not None:
        g_pred = np.array(g_pred, dtype=np.float64)
        g_pred[..., 0:2] *= s
    return HC.decode_bwd_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, g_output, g_pred)


def decode32(logits, layer_no, cfg, scale_xy):
    """oracle.head.yolo_decode (train) with the centre re-evaluated in fp32 as ((sigma * s) - h) + cell: (output, pred)"""
    out, pred = H.yolo_decode(logits, layer_no, cfg, True)
    s, h = s_h(scale_xy)
    Fs = out.shape[2]
    pred = pred.copy()
    pred[..., 0] = (out[..., 0] * F32(s) - F32(h)) + np.arange(Fs, dtype=F32).reshape(1, 1, 1, Fs)
    pred[..., 1] = (out[..., 1] * F32(s) - F32(h)) + np.arange(Fs, dtype=F32).reshape(1, 1, Fs, 1)
    return out, pred


# ------------------------------------------------------------------------------------------ assignment
def shape_iou32(tw, th, anchors):
    """fp32 shape IoU [n, n_all] of labels (tw, th) [n] against anchors [n_all, 2], in yolo_assign_kernel's operation
    order: brx = min(tw, aw), bry = min(th, ah), ai = (brx * bry) * en, iou = ai / ((tw * th + aw * ah) - ai)."""
    tw = np.asarray(tw, F32).reshape(-1, 1)
    th = np.asarray(th, F32).reshape(-1, 1)
    aw = np.asarray(anchors, F32)[:, 0].reshape(1, -1)
    ah = np.asarray(anchors, F32)[:, 1].reshape(1, -1)
    brx, bry = np.minimum(tw, aw), np.minimum(th, ah)
    en = ((F32(0) < brx) & (F32(0) < bry)).astype(F32)
    ai = (brx * bry) * en
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = ai / ((tw * th + aw * ah) - ai)
    assert iou.dtype == F32
    return iou


def assign(labels, layer_no, cfg, Fs, iou_thresh=1.0):
    """The (label, anchor slot) pairs of a layer in the order the kernels take them, per image:
    dict(n [B], pairs: list per image of (t, a, j, i, extra), iou [B] arrays [n, n_all], best [B] arrays [n]).
    extra: the pair is positive through iou_thresh only (not the arg-max).  Pairs outside the map are skipped."""
    lab = np.asarray(labels).astype(F32)
    st = F32(H.STRIDES[layer_no])
    mask = list(cfg['ANCHOR_MASK'][layer_no])
    anc = H.all_anchors(cfg, layer_no)
    thr = F32(iou_thresh)
    multi = thr < F32(1)
    n = (lab.sum(axis=2, dtype=F32) > 0).sum(axis=1)
    pairs, ious, bests = [], [], []
    for b in range(lab.shape[0]):
        nb = int(n[b])
        tx, ty = lab[b, :nb, 0] / st, lab[b, :nb, 1] / st
        iou = shape_iou32(lab[b, :nb, 2] / st, lab[b, :nb, 3] / st, anc)
        best = np.argmax(iou, axis=1) if nb else np.zeros(0, np.int64)         # NaN counts as maximal, first one wins
        ti, tj = tx.astype(np.int16), ty.astype(np.int16)
        out = []
        for t in range(nb):
            i, j = int(ti[t]), int(tj[t])
            if i < 0 or i >= Fs or j < 0 or j >= Fs:
                continue
            for a, k in enumerate(mask):
                is_best = int(best[t]) == k
                with np.errstate(invalid='ignore'):
                    extra = bool(multi and not is_best and iou[t, k] > thr)
                if is_best or extra:
                    out.append((t, a, j, i, extra))
        pairs.append(out)
        ious.append(iou)
        bests.append(best)
    return dict(n=[int(v) for v in n], pairs=pairs, iou=ious, best=bests)


def records_of(pairs):
    """cells (a, j, i) of one image in record order (first hit)"""
    recs = []
    for t, a, j, i, _ in pairs:
        if (a, j, i) not in recs:
            recs.append((a, j, i))
    return recs


def assign_props(labels, cfg, iou_thresh):
    """Per layer: most records of one image, extra pairs, pairs that hit a cell an earlier pair of the image made a record
    of, labels positive on all three anchors of the layer."""
    props = []
    for l, Fs in enumerate(HC.LOSS_F):
        asg = assign(labels, l, cfg, Fs, iou_thresh)
        rec = [len(records_of(p)) for p in asg['pairs']]
        extra = sum(sum(1 for q in p if q[4]) for p in asg['pairs'])
        coll = sum(len(p) - r for p, r in zip(asg['pairs'], rec))
        all3 = 0
        for p in asg['pairs']:
            per_t = {}
            for t, a, _, _, _ in p:
                per_t.setdefault(t, set()).add(a)
            all3 += sum(1 for v in per_t.values() if len(v) == 3)
        props.append(dict(max_records=max(rec), records=rec, extra=extra, collisions=coll, all_three=all3))
    return props


def closest_to_thresh(labels, cfg, iou_thresh):
    """smallest |iou - iou_thresh| over the labels and the anchors of their own layer's mask, all layers"""
    d = np.inf
    for l, Fs in enumerate(HC.LOSS_F):
        asg = assign(labels, l, cfg, Fs, iou_thresh)
        for iou in asg['iou']:
            if len(iou):
                d = min(d, float(np.abs(iou[:, list(cfg['ANCHOR_MASK'][l])].astype(np.float64) - float(F32(iou_thresh))).min()))
    return d


def planted_tie(labels, cfg, layer_no=1):
    """(thresh, b, t, a): the fp32 shape IoU of a label of image 0 against a non-arg-max anchor of the layer's mask, as a
    threshold.  At exactly this threshold the pair is not positive (strict >); at np.nextafter(thresh, 0) it is."""
    asg = assign(labels, layer_no, cfg, HC.LOSS_F[layer_no], 1.0)
    mask = list(cfg['ANCHOR_MASK'][layer_no])
    iou, best = asg['iou'][0], asg['best'][0]
    for t in range(len(best)):
        for a, k in enumerate(mask):
            if int(best[t]) != k and int(best[t]) in mask and 0.05 < iou[t, k] < 0.9:
                return float(iou[t, k]), 0, t, a
    raise AssertionError('no label with a non-arg-max anchor in this layer')


# ------------------------------------------------------------------------------------------ loss
def _bce_terms(o, t, dt):
    with np.errstate(divide='ignore'):
        lo = np.maximum(np.log(o), dt(-100))
        l1 = np.maximum(np.log(dt(1) - o), dt(-100))
    return -(t * lo + (dt(1) - t) * l1)


def _bce_grad(o, t, dt):
    return (o - t) / np.maximum((dt(1) - o) * o, dt(1e-12))


def build_target(output, pred, layer_no, labels, cfg, ignore_thresh=0.7, iou_thresh=1.0, label_smooth=0.0,
                 dtype=np.float64):
    """(target, obj_mask, tgt_mask, tgt_scale, info): the dense targets of oracle.head.build_target under the options.
    target and tgt_scale are of `dtype`; info holds per image the record cells in record order, the truth box of every
    record (fp32, last writer wins) and whether the record's first pair was an extra one."""
    dt = dtype
    output = np.asarray(output, F32)
    pred = np.asarray(pred, F32)
    B, A, Fs = output.shape[:3]
    C = cfg['N_CLASSES']
    lab = np.asarray(labels).astype(F32)
    st = F32(H.STRIDES[layer_no])
    manc = H.masked_anchors(cfg, layer_no)
    lo, hi = smooth_targets(label_smooth)
    asg = assign(labels, layer_no, cfg, Fs, iou_thresh)
    target = np.zeros((B, A, Fs, Fs, 5 + C), dt)
    tgt_mask = np.zeros((B, A, Fs, Fs, 4 + C), F32)
    tgt_scale = np.zeros((B, A, Fs, Fs, 2), dt)
    obj_mask = np.ones((B, A, Fs, Fs), F32)
    bits = np.zeros((B, A, Fs, Fs, C), bool)
    info = []
    for b in range(B):
        n = asg['n'][b]
        recs, truth, first_extra = [], {}, {}
        if n:
            box = (lab[b, :n, :4] / st).astype(F32)                            # exact: the strides are powers of two
            piou = H.bboxes_iou(pred[b].reshape(-1, 4), box, xyxy=False)        # the ignore mask, fp32 as the kernel
            has_nan = np.isnan(piou).any(axis=1)
            with np.errstate(invalid='ignore'):
                best = np.where(has_nan, F32(np.nan), np.nanmax(np.where(np.isnan(piou), -np.inf, piou), axis=1))
                ign = best > F32(ignore_thresh)
            obj_mask[b] = (~ign).reshape(A, Fs, Fs).astype(F32)
            for t, a, j, i, extra in asg['pairs'][b]:
                if (a, j, i) not in truth:
                    recs.append((a, j, i))
                    first_extra[(a, j, i)] = extra
                truth[(a, j, i)] = box[t]
                tx, ty, tw, th = [box[t, q].astype(dt) for q in range(4)]
                obj_mask[b, a, j, i] = 1
                tgt_mask[b, a, j, i, :] = 1
                tgt_scale[b, a, j, i, :] = np.sqrt(dt(2) - tw * th / dt(Fs) / dt(Fs))
                target[b, a, j, i, 0] = tx - dt(i)
                target[b, a, j, i, 1] = ty - dt(j)
                with np.errstate(divide='ignore'):
                    target[b, a, j, i, 2] = np.log(tw / manc[a, 0].astype(dt) + dt(1e-16))
                    target[b, a, j, i, 3] = np.log(th / manc[a, 1].astype(dt) + dt(1e-16))
                target[b, a, j, i, 4] = 1
                cls = int(lab[b, t, 4].astype(np.int16))
                if 0 <= cls < C:
                    bits[b, a, j, i, cls] = True
        info.append(dict(records=recs, truth=np.array([truth[r] for r in recs], F32).reshape(-1, 4),
                         first_extra=[first_extra[r] for r in recs]))
    pos = tgt_mask[..., 0] > 0
    target[..., 5:][pos] = np.where(bits[pos], dt(hi), dt(lo))
    return target, obj_mask, tgt_mask, tgt_scale, info


def loss_ref(output, pred, layer_no, labels, cfg, ignore_thresh=0.7, iou_thresh=1.0, label_smooth=0.0, dtype=np.float64):
    """oracle.head.yolo_loss_layer under the options: the same dict, plus `info` of build_target.  Per-element terms in
    `dtype` on the fp32 inputs, BCE logs clamped at -100, sums in float64."""
    dt = dtype
    target, obj_mask, tgt_mask, tgt_scale, info = build_target(output, pred, layer_no, labels, cfg, ignore_thresh,
                                                               iou_thresh, label_smooth, dt)
    out = np.asarray(output, F32).astype(dt)
    n_ch = out.shape[-1]
    rest = np.r_[0:4, 5:n_ch]
    om, tm = obj_mask.astype(dt), tgt_mask.astype(dt)
    mo, mt = out.copy(), target.copy()
    for m in (mo, mt):
        m[..., 4] *= om
        m[..., rest] *= tm
        m[..., 2:4] *= tgt_scale
    w = tgt_scale * tgt_scale
    l_xy = (w * _bce_terms(mo[..., :2], mt[..., :2], dt)).sum(dtype=np.float64)
    l_wh = ((mo[..., 2:4] - mt[..., 2:4]) ** 2).sum(dtype=np.float64) / 2
    l_obj = _bce_terms(mo[..., 4], mt[..., 4], dt).sum(dtype=np.float64)
    l_cls = _bce_terms(mo[..., 5:], mt[..., 5:], dt).sum(dtype=np.float64)
    g = np.zeros_like(out)
    g[..., :2] = w * _bce_grad(mo[..., :2], mt[..., :2], dt) * tm[..., :2]
    g[..., 2:4] = (mo[..., 2:4] - mt[..., 2:4]) * tgt_scale * tm[..., 2:4]
    g[..., 4] = _bce_grad(mo[..., 4], mt[..., 4], dt) * om
    g[..., 5:] = _bce_grad(mo[..., 5:], mt[..., 5:], dt) * tm[..., 4:]
    return dict(loss=l_xy + l_wh + l_obj + l_cls, xy=l_xy, wh=l_wh, obj=l_obj, cls=l_cls, grad_output=g, target=target,
                obj_mask=obj_mask, tgt_mask=tgt_mask, tgt_scale=tgt_scale, mutated_output=mo, info=info)


# ------------------------------------------------------------------------------------------ box loss on the records
def record_cells(info):
    """[N, 4] int (b, a, j, i) in (image, record) order: the summation order of the box-loss kernel"""
    cells = [(b, a, j, i) for b, d in enumerate(info) for (a, j, i) in d['records']]
    return np.array(cells, np.int64).reshape(-1, 4)


def box_ref(pred, info, kind, gain, scale_xy=1.0, dtype=np.float64):
    """The box loss of a layer over the records of `info` through boxloss_cases.box_eval: loss = gain * sum(1 - X),
    grad [N, 4] = gain * d loss / d output[..., 0:4] -- channels 0 and 1 times s, d pred / d output."""
    cells = record_cells(info)
    truth = np.concatenate([d['truth'] for d in info], 0) if len(cells) else np.zeros((0, 4), F32)
    pred = np.asarray(pred, F32)
    p = np.stack([pred[b, a, j, i] for b, a, j, i in cells]).astype(dtype) if len(cells) else np.zeros((0, 4), dtype)
    t = truth.astype(dtype)
    loss, grad = BC.box_eval(p, t, kind) if len(cells) else (np.zeros(0, dtype), np.zeros((0, 4), dtype))
    s, _ = s_h(scale_xy)
    g = grad * (dtype(gain) if dtype is F32 else float(F32(gain)))
    g[:, 0:2] = g[:, 0:2] * dtype(s)
    extra = np.array([e for d in info for e in d['first_extra']], bool)
    return dict(loss=float(loss.astype(np.float64).sum()) * float(F32(gain)), per_record=loss, grad=g, cells=cells, p=p,
                t=t, ties=BC.exact_ties(p, t), extra=extra)


# ------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def loss_inputs(C, K, saturate=False):
    """Three images at 128 px on the three layers: labels [3, K, 5] and per layer (logits, output, pred) of the oracle's
    decode of head_cases.make_loss_logits.  Read-only arrays: the tests share them."""
    cfg = HC.cfg_with_classes(C)
    labels = HC.make_labels(K, C, 100 + K)[0]
    lgs, props = HC.make_loss_logits(C, 900, labels if saturate else None, saturate=saturate)
    layers = []
    for l, lg in enumerate(lgs):
        out, pred = H.yolo_decode(lg, l, cfg, True)
        for a in (lg, out, pred):
            a.setflags(write=False)
        layers.append((lg, out, pred))
    labels.setflags(write=False)
    return dict(cfg=cfg, labels=labels, layers=layers, props=props, C=C, K=K)


@functools.lru_cache(maxsize=None)
def box_case(C, K, scale=(1.2, 1.1, 1.05), iou_thresh=0.213):
    """The box-loss inputs with several anchors and s != 1: pred decoded in fp32 with the layer's scale, then planted at
    the record cells like boxloss_cases.make_case (class q % 9 of BC.PLANTS for the q-th record of the case).  Per layer
    dict(output, pred, plants [N], info)."""
    base = loss_inputs(C, K)
    layers = []
    q = 0
    for l, (lg, _, _) in enumerate(base['layers']):
        out, pred = decode32(lg, l, base['cfg'], scale_of(scale, l))
        info = build_target(out, pred, l, base['labels'], base['cfg'], 0.7, iou_thresh)[4]
        names = []
        for b, d in enumerate(info):
            for (a, j, i), t in zip(d['records'], d['truth']):
                name = BC.PLANTS[q % len(BC.PLANTS)]
                if name != 'generic':
                    pred[b, a, j, i] = np.array(BC.plant(name, t, (q * 0.37) % 1.0), F32)
                names.append(name)
                q += 1
        for a in (out, pred):
            a.setflags(write=False)
        layers.append(dict(output=out, pred=pred, plants=names, info=info))
    return dict(cfg=base['cfg'], labels=base['labels'], layers=layers, scale=scale, iou_thresh=iou_thresh)


BOX_SETS = ((33, 64), (1, 65), (33, 100))                      # (C, K): the wave assign form, the one-thread form, K * A > 255


@functools.lru_cache(maxsize=None)
def box_references(C, K, kind, gain):
    """Per layer (ref64, ref32) of box_ref on box_case(C, K) with the layer's scale."""
    case = box_case(C, K)
    out = []
    for l, lay in enumerate(case['layers']):
        s = scale_of(case['scale'], l)
        out.append((box_ref(lay['pred'], lay['info'], kind, gain, s), box_ref(lay['pred'], lay['info'], kind, gain, s, F32)))
    return out


@functools.lru_cache(maxsize=None)
def box_fp32_errors(kind, gain):
    """boxloss_cases.fp32_errors over BOX_SETS x 3 layers: the plain-fp32 evaluation's own (loss, row-relative gradient)
    error, the yardstick of boxloss_cases' rule."""
    e_loss = e_grad = 0.0
    for C, K in BOX_SETS:
        case = box_case(C, K)
        for (r64, r32), lay in zip(box_references(C, K, kind, gain), case['layers']):
            e_loss = max(e_loss, abs(r32['loss'] - r64['loss']))
            rows = BC.judged_rows(r64, lay['plants'])
            if rows.any():
                e_grad = max(e_grad, float(BC.row_rel_err(r32['grad'][rows], r64['grad'][rows]).max()))
    return e_loss, e_grad


def box_bounds(kind, gain):
    e_loss, e_grad = box_fp32_errors(kind, gain)
    return BC.BOX_FACTOR * e_loss, BC.BOX_FACTOR * e_grad
