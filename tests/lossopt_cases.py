# -*- coding: utf-8 -*-
"""Focal loss, IoU-aware objectness and the objectness / class gains of the detection loss, restated in numpy, and the
option sets and inputs of their tests (tests/test_lossopt_cases.py checks the restatement and the inputs without a GPU,
tests/test_gpu_lossopt.py feeds them to the kernels of csrc/yolo_loss.hip).

The rules (include/yolov4_amd.h, y4_loss_opts), with o the value in `output`, t the element's
target, bce / bce_grad the terms of headopt_cases:
  focal      p_t = t o + (1 - t)(1 - o), q = 1 - p_t, a = alpha > 0 ? t alpha + (1 - t)(1 - alpha) : 1,
             FL = (bce a) q^gamma, dFL/do = a (bce_grad q^gamma - ((bce gamma) q^(gamma - 1)) (2 t - 1)); 0 at q = 0.
             Objectness: every cell with obj_mask != 0.  Classes: every class element of a positive record.
  IoU-aware  t_obj = (1 - r) + r max(X, 0) at a cell with a record, X = 1 - (box loss of the record); NaN X is carried.
  gains      parts[2] *= obj_gain, parts[3] *= cls_gain in fp64; the gradients are g * gain.

`loss_ref` extends headopt_cases.loss_ref the way that one is written: the positive set, cells and ignore mask are exact
fp32; the per-element terms are evaluated in `dtype` on the fp32 inputs -- float64 is the reference of the GPU tests,
float32 the yardstick (what plain fp32 arithmetic achieves) --; sums are float64.  With every option off it is
headopt_cases.loss_ref bit for bit.  Option values enter as the fp32 numbers the kernels get.

Plain module, no fixtures."""
import functools

import numpy as np

import boxloss_cases as BC
import head_cases as HC
import headopt_cases as HO

F32 = np.float32

DEFAULTS = dict(focal_gamma=0.0, focal_alpha=0.25, focal_terms='obj+cls', obj_iou_ratio=0.0, obj_iou_kind='ciou',
                obj_gain=1.0, cls_gain=1.0)
TERM_BITS = {'obj': 1, 'cls': 2, 'obj+cls': 3}

SETS = HO.BOX_SETS + ((33, 1),)                                # (C, K): both assign forms, K * A > 255, one label
FOCAL_SETS = tuple(dict(focal_gamma=g, focal_alpha=a) for g in (2.0, 1.5, 0.5) for a in (0.25, 0.0)) + \
    (dict(focal_gamma=2.0, focal_terms='obj'), dict(focal_gamma=2.0, focal_terms='cls'))
IOU_SETS = tuple(dict(obj_iou_ratio=r, obj_iou_kind=k) for r in (0.5, 1.0) for k in BC.KINDS)
GAIN_SETS = (dict(obj_gain=0.4, cls_gain=2.5), dict(obj_gain=(4.0, 1.0, 0.4)))
ALL_ON = dict(focal_gamma=2.0, focal_alpha=0.25, focal_terms='obj+cls', obj_iou_ratio=0.5, obj_iou_kind='ciou',
              obj_gain=(4.0, 1.0, 0.4), cls_gain=2.5)
ALL_ON_HEAD = dict(iou_thresh=0.213, label_smooth=0.1, scale=(1.2, 1.1, 1.05))

# Largest figures measured on an MI355X by tests/test_gpu_lossopt.py (it prints them before it asserts):
#   parts: |got - ref64| / |ref64| over all option sets (bar 1e-4)
#   grad: the largest of |got - ref64| / (1e-5 + 1e-4 |ref64|) over the unsaturated sets (bar 1)
#   t_obj: kernel error / the fp32 yardstick's largest t_obj error, per kind (bar BOX_FACTOR = 4)
MEASURED_PARTS = 1.43e-7
MEASURED_GRAD = 0.034                    # the saturated set against the scaled bar: 0.032
MEASURED_T_OBJ = {'iou': 0.095, 'giou': 0.276, 'diou': 0.095, 'ciou': 0.095}


def opt_id(o):
    return '-'.join('%s=%s' % (k.replace('focal_', '').replace('obj_iou_', ''), v) for k, v in o.items()).replace(' ', '')


def options(opt=None, layer_no=0):
    """DEFAULTS overlaid with `opt`; a per-layer obj_gain is resolved to the layer's; numbers become the fp32 values the
    kernels get, as Python floats."""
    o = dict(DEFAULTS)
    o.update(opt or {})
    g = o['obj_gain']
    o['obj_gain'] = g[layer_no] if isinstance(g, (tuple, list)) else g
    for k in ('focal_gamma', 'focal_alpha', 'obj_iou_ratio', 'obj_gain', 'cls_gain'):
        o[k] = float(F32(o[k]))
    return o


def any_on(o):
    return o['focal_gamma'] > 0 or o['obj_iou_ratio'] > 0 or o['obj_gain'] != 1 or o['cls_gain'] != 1


# ------------------------------------------------------------------------------------------ the focal term
def focal(o, t, gamma, alpha, dt):
    """(FL, dFL/do) elementwise in dtype dt, in the operation order of the header's formulas"""
    o = np.asarray(o, dt)
    t = np.asarray(t, dt)
    one = dt(1)
    bce, bg = HO._bce_terms(o, t, dt), HO._bce_grad(o, t, dt)
    q = one - (t * o + (one - t) * (one - o))
    a = t * dt(alpha) + (one - t) * (one - dt(alpha)) if alpha > 0 else np.ones_like(o)
    with np.errstate(invalid='ignore'):
        pos = q > 0                                           # False for NaN: the NaN of bce then decides
    qs = np.where(pos, q, one)
    m = np.where(pos, np.power(qs, dt(gamma)), dt(0))
    m1 = np.where(pos, np.power(qs, dt(gamma) - one), dt(0))
    with np.errstate(invalid='ignore'):
        fl = (bce * a) * m
        dfl = a * (bg * m - ((bce * dt(gamma)) * m1) * (dt(2) * t - one))
    assert fl.dtype == dt and dfl.dtype == dt
    return fl, dfl


def focal_torch64(o, t, gamma, alpha):
    """(FL, dFL/do) of the composed expression a * bce * (1 - p_t)^gamma through torch float64 autograd, t a constant"""
    import torch
    o = torch.tensor(np.asarray(o, np.float64), requires_grad=True)
    t = torch.tensor(np.asarray(t, np.float64))
    bce = -(t * torch.log(o) + (1 - t) * torch.log(1 - o))
    p_t = t * o + (1 - t) * (1 - o)
    a = t * alpha + (1 - t) * (1 - alpha) if alpha > 0 else torch.ones_like(o)
    fl = a * bce * (1 - p_t) ** gamma
    fl.sum().backward()
    return fl.detach().numpy(), o.grad.numpy()


# ------------------------------------------------------------------------------------------ the loss
def obj_targets(pred, info, o, dt):
    """(cells [N, 4], t_obj [N], X [N]) of the records in record order; t_obj is 1 without the IoU-aware option"""
    cells = HO.record_cells(info)
    if o['obj_iou_ratio'] <= 0 or not len(cells):
        return cells, np.ones(len(cells), dt), np.full(len(cells), np.nan, dt)
    loss = HO.box_ref(pred, info, o['obj_iou_kind'], 1.0, 1.0, dt)['per_record']
    assert loss.dtype == dt
    x = dt(1) - loss
    r = dt(o['obj_iou_ratio'])
    with np.errstate(invalid='ignore'):
        t = (dt(1) - r) + r * np.maximum(x, dt(0))           # np.maximum carries NaN
    return cells, t, x


def loss_ref(output, pred, layer_no, labels, cfg, ignore_thresh=0.7, iou_thresh=1.0, label_smooth=0.0, opt=None,
             dtype=np.float64):
    """headopt_cases.loss_ref under the options of `opt` (DEFAULTS' keys): the same dict with obj, cls, loss, target and
    grad_output re-evaluated, plus t_obj / X per record and `cells`.  The box parts and channels are the base's."""
    dt = dtype
    o = options(opt, layer_no)
    base = HO.loss_ref(output, pred, layer_no, labels, cfg, ignore_thresh, iou_thresh, label_smooth, dt)
    out = np.asarray(output, F32).astype(dt)
    om, tm = base['obj_mask'].astype(dt), base['tgt_mask'].astype(dt)
    target = base['target'].copy()
    cells, t_obj, x = obj_targets(pred, base['info'], o, dt)
    if len(cells):
        target[tuple(cells.T) + (4,)] = t_obj
    focal_on = o['focal_gamma'] > 0
    bits = TERM_BITS[o['focal_terms']] if focal_on else 0
    g = base['grad_output'].copy()
    # objectness: masked output against masked target, as the base
    mo4, mt4 = out[..., 4] * om, target[..., 4] * om
    with np.errstate(invalid='ignore'):
        if bits & 1:
            l4, g4 = focal(mo4, mt4, o['focal_gamma'], o['focal_alpha'], dt)
        else:
            l4, g4 = HO._bce_terms(mo4, mt4, dt), HO._bce_grad(mo4, mt4, dt)
        l_obj = l4.sum(dtype=np.float64) * o['obj_gain']
        g[..., 4] = (g4 * om) * dt(o['obj_gain'])
        moc, mtc = out[..., 5:] * tm[..., 4:], target[..., 5:] * tm[..., 4:]
        if bits & 2:
            lc, gc = focal(moc, mtc, o['focal_gamma'], o['focal_alpha'], dt)
        else:
            lc, gc = HO._bce_terms(moc, mtc, dt), HO._bce_grad(moc, mtc, dt)
        l_cls = lc.sum(dtype=np.float64) * o['cls_gain']
        g[..., 5:] = (gc * tm[..., 4:]) * dt(o['cls_gain'])
    ref = dict(base)
    ref.update(loss=base['xy'] + base['wh'] + l_obj + l_cls, obj=l_obj, cls=l_cls, grad_output=g, target=target,
               cells=cells, t_obj=t_obj, X=x, opt=o)
    return ref


def build_target(output, pred, layer_no, labels, cfg, ignore_thresh=0.7, iou_thresh=1.0, label_smooth=0.0, opt=None,
                 dtype=np.float64):
    """(target, obj_mask, tgt_mask, tgt_scale, info) of headopt_cases.build_target with target[..., 4] = t_obj"""
    target, obj_mask, tgt_mask, tgt_scale, info = HO.build_target(output, pred, layer_no, labels, cfg, ignore_thresh,
                                                                  iou_thresh, label_smooth, dtype)
    cells, t_obj, _ = obj_targets(pred, info, options(opt, layer_no), dtype)
    if len(cells):
        target[tuple(cells.T) + (4,)] = t_obj
    return target, obj_mask, tgt_mask, tgt_scale, info


# ------------------------------------------------------------------------------------------ inputs and shared references
def plain_layers(C, K, saturate=False):
    """per layer (output, pred) of headopt_cases.loss_inputs, with its labels and cfg: (labels, cfg, layers)"""
    d = HO.loss_inputs(C, K, saturate)
    return d['labels'], d['cfg'], [(out, pred) for _, out, pred in d['layers']]


def box_layers(C, K):
    """per layer (output, pred) of headopt_cases.box_case -- scales (1.2, 1.1, 1.05), records of iou_thresh 0.213, planted
    boxes -- with its labels and cfg"""
    d = HO.box_case(C, K)
    return d['labels'], d['cfg'], [(lay['output'], lay['pred']) for lay in d['layers']]


def _freeze(opt):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in (opt or {}).items()))


@functools.lru_cache(maxsize=None)
def _reference(C, K, source, l, iou_thresh, label_smooth, fopt, f32):
    labels, cfg, layers = {'plain': plain_layers(C, K), 'sat': plain_layers(C, K, True) if source == 'sat' else None,
                           'box': box_layers(C, K) if source == 'box' else None}[source]
    out, pred = layers[l]
    return loss_ref(out, pred, l, labels, cfg, 0.7, iou_thresh, label_smooth, dict(fopt), F32 if f32 else np.float64)


def reference(C, K, source, l, opt=None, iou_thresh=1.0, label_smooth=0.0, f32=False):
    """loss_ref on layer l of the inputs `source` in ('plain', 'sat', 'box'), computed once and shared; read-only"""
    return _reference(C, K, source, l, iou_thresh, label_smooth, _freeze(opt), f32)


@functools.lru_cache(maxsize=None)
def t_obj_fp32_error(kind):
    """the fp32 yardstick's largest |t_obj32 - t_obj64| over SETS x 3 layers x r in (0.5, 1) on box_case"""
    e = 0.0
    for C, K in SETS:
        for l in range(3):
            for r in (0.5, 1.0):
                o = dict(obj_iou_ratio=r, obj_iou_kind=kind)
                a = reference(C, K, 'box', l, o, 0.213, 0.0)
                b = reference(C, K, 'box', l, o, 0.213, 0.0, True)
                if len(a['t_obj']):
                    e = max(e, float(np.abs(b['t_obj'].astype(np.float64) - a['t_obj']).max()))
    return e


def grad_ratio(got, ref64, atol=1e-5, rtol=1e-4):
    """largest |got - ref| / (atol + rtol |ref|): head_cases.close(..., scale=False) passes iff this is <= 1"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    with np.errstate(invalid='ignore'):
        return float((np.abs(got - ref64) / (atol + rtol * np.abs(ref64))).max())
