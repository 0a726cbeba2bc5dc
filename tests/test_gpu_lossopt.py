# -*- coding: utf-8 -*-
"""Focal loss, IoU-aware objectness and the objectness / class gains of csrc/yolo_loss.hip through the C ABI (the *_opts
entries) against the float64 restatement of tests/lossopt_cases.py, then through YOLOLayer + YOLOLoss.

With the defaults the new entries must give the bits -- workspace bytes included -- of the entries they generalise.
tests/test_lossopt_cases.py shows without a GPU that the restatement is the closed form of the composed expression, that
the inputs hold what they are named for and that plain fp32 arithmetic meets the gradient bar used here with a factor 2
to spare.  Every measured ratio is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import boxloss_cases as BC
import head_cases as HC
import headopt_cases as HO
import lossopt_cases as LO
from oracle import head as H

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import check, float_array, int_array, lib
    return lib(), ops._ptr, ops._stream, check, float_array, int_array


def _up(a, dev, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(dev)        # a copy: the shared inputs are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _struct(opt, l, iou, eps):
    from yolov4_amd._lib import FOCAL_TERMS, LossOpts
    o = LO.options(opt, l)
    return LossOpts(iou, eps, o['focal_gamma'], o['focal_alpha'], FOCAL_TERMS[o['focal_terms']], o['obj_iou_ratio'],
                    BC.KIND_IDS[o['obj_iou_kind']], o['obj_gain'], o['cls_gain'])


KEYS = ('obj_mask', 'parts', 'target', 'tgt_mask', 'tgt_scale', 'grad', 'mutated', 'grad_masked')


def _run(dev, output, pred, labels, l, C, opt=None, iou=1.0, eps=0.0, entry='opts'):
    """The loss entries on one layer: the *_opts forms with the options `opt` (lossopt_cases.DEFAULTS' keys), the _ex
    forms (entry='ex') or the first entries (entry='old', iou = 1 and eps = 0 only).  Everything comes back as numpy,
    the workspace (filled with 0xAB beforehand) included."""
    L, ptr, stream, check, farr, iarr = _abi()
    cfg = HC.cfg_with_classes(C)
    B, A, F, _, n_ch = output.shape
    K = labels.shape[1]
    od, pd, lab = _up(output, dev), _up(pred, dev), _up(labels, dev)
    st = _struct(opt, l, iou, eps)
    if entry == 'opts':
        nbytes = L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(st))
    elif entry == 'ex':
        nbytes = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, iou)
    else:
        nbytes = L.y4_yolo_loss_workspace(B, F, A, K, C)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    obj = torch.full((B, A, F, F), float('nan'), device=dev)
    parts = torch.full((4,), float('nan'), dtype=torch.float64, device=dev)
    anchors = H.all_anchors(cfg, l)
    head = (ptr(od), ptr(pd), ptr(lab), K, B, F, A, C, float(H.STRIDES[l]), float(np.float32(0.7)), farr(anchors.ravel()),
            len(anchors), iarr(cfg['ANCHOR_MASK'][l]))
    tail = (ptr(obj), ptr(parts), ptr(ws), nbytes, stream())
    target = torch.full((B, A, F, F, n_ch), float('nan'), device=dev)
    tgt_mask = torch.full((B, A, F, F, 4 + C), float('nan'), device=dev)
    tgt_scale = torch.full((B, A, F, F, 2), float('nan'), device=dev)
    one = torch.ones(1, device=dev)
    g, g2, mo = torch.full_like(od, float('nan')), torch.full_like(od, float('nan')), od.clone()
    dims = (B, F, A, K, C)
    dense = (ptr(target), ptr(tgt_mask), ptr(tgt_scale))
    if entry == 'opts':
        o = ctypes.byref(st)
        check(L.y4_yolo_loss_fwd_opts_f32(*head, o, *tail), 'loss_fwd_opts')
        check(L.y4_yolo_loss_dense_targets_opts_f32(*dense, *dims, o, ptr(ws), nbytes, stream()), 'dense_targets_opts')
        check(L.y4_yolo_loss_bwd_opts_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), *dims, o, ptr(ws), nbytes, stream()), 'bwd_opts')
        check(L.y4_yolo_loss_mask_output_ex_f32(ptr(mo), ptr(obj), *dims, iou, ptr(ws), nbytes, stream()), 'mask_output_ex')
        check(L.y4_yolo_loss_bwd_opts_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), *dims, o, ptr(ws), nbytes, stream()), 'bwd_opts')
    elif entry == 'ex':
        check(L.y4_yolo_loss_fwd_ex_f32(*head, iou, eps, *tail), 'loss_fwd_ex')
        check(L.y4_yolo_loss_dense_targets_ex_f32(*dense, *dims, iou, eps, ptr(ws), nbytes, stream()), 'dense_targets_ex')
        check(L.y4_yolo_loss_bwd_ex_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), *dims, iou, eps, ptr(ws), nbytes, stream()), 'bwd_ex')
        check(L.y4_yolo_loss_mask_output_ex_f32(ptr(mo), ptr(obj), *dims, iou, ptr(ws), nbytes, stream()), 'mask_output_ex')
        check(L.y4_yolo_loss_bwd_ex_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), *dims, iou, eps, ptr(ws), nbytes, stream()), 'bwd_ex')
    else:
        assert iou == 1.0 and eps == 0.0
        check(L.y4_yolo_loss_fwd_f32(*head, *tail), 'loss_fwd')
        check(L.y4_yolo_loss_dense_targets_f32(*dense, *dims, ptr(ws), nbytes, stream()), 'dense_targets')
        check(L.y4_yolo_loss_bwd_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), *dims, ptr(ws), nbytes, stream()), 'bwd')
        check(L.y4_yolo_loss_mask_output_f32(ptr(mo), ptr(obj), *dims, ptr(ws), nbytes, stream()), 'mask_output')
        check(L.y4_yolo_loss_bwd_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), *dims, ptr(ws), nbytes, stream()), 'bwd')
    torch.cuda.synchronize()
    r = dict(obj_mask=obj, parts=parts, target=target, tgt_mask=tgt_mask, tgt_scale=tgt_scale, grad=g, mutated=mo,
             grad_masked=g2, ws=ws)
    return {k: t.cpu().numpy() for k, t in r.items()}


class Worst:
    """the largest figures of a test, printed at its end"""

    def __init__(self):
        self.parts = self.grad = 0.0

    def report(self, tag):
        print('%s: largest part error / |ref| %.3g (bar 1e-4), largest gradient ratio %.3f (bar 1)' % (tag, self.parts, self.grad))


def _check(got, ref, base, opt, l, tag, worst, saturated=False):
    """parts 1e-4 relative; gradient HC.close(1e-5, 1e-4) unscaled with no element excluded (saturated: finite and the
    project's scaled form); masks exact; what the options must leave alone bit-equal to `base`, the run without them."""
    o = LO.options(opt, l)
    bits = LO.TERM_BITS[o['focal_terms']] if o['focal_gamma'] > 0 else 0
    obj_alone = not bits & 1 and o['obj_iou_ratio'] == 0 and o['obj_gain'] == 1
    cls_alone = not bits & 2 and o['cls_gain'] == 1
    assert np.array_equal(got['obj_mask'], ref['obj_mask']), tag
    assert np.array_equal(got['tgt_mask'], ref['tgt_mask']), tag
    for k in ('obj_mask', 'tgt_mask', 'tgt_scale', 'mutated'):
        assert _same(got[k], base[k]), (tag, k)
    assert _same(got['target'][..., :4], base['target'][..., :4]) and _same(got['target'][..., 5:], base['target'][..., 5:]), tag
    assert _same(got['parts'][:2], base['parts'][:2]), (tag, 'box parts')
    if obj_alone:
        assert _same(got['parts'][2:3], base['parts'][2:3]), (tag, 'obj part')
    if cls_alone:
        assert _same(got['parts'][3:], base['parts'][3:]), (tag, 'cls part')
    names = ('xy', 'wh', 'obj', 'cls')
    for q, name in enumerate(names):
        e = abs(got['parts'][q] - ref[name])
        rel = e / abs(ref[name]) if ref[name] else e
        worst.parts = max(worst.parts, rel)
        print('%s %s: %.12g ref %.12g relative error %.3g' % (tag, name, got['parts'][q], ref[name], rel))
    loss = float(got['parts'].sum())
    print('%s sum: %.12g ref %.12g' % (tag, loss, ref['loss']))
    for key in ('grad', 'grad_masked'):
        ratio = LO.grad_ratio(got[key], ref['grad_output'])
        print('%s %s: ratio to close(1e-5, 1e-4) %.3f' % (tag, key, ratio))
        if not saturated:
            worst.grad = max(worst.grad, ratio)
    assert np.isfinite(got['parts']).all(), tag
    for q, name in enumerate(names):
        assert abs(got['parts'][q] - ref[name]) <= 1e-4 * abs(ref[name]), (tag, name, got['parts'][q], ref[name])
    assert abs(loss - ref['loss']) <= 1e-4 * abs(ref['loss']), (tag, loss, ref['loss'])
    for key in ('grad', 'grad_masked'):
        assert np.isfinite(got[key]).all(), (tag, key)
        HC.close(got[key], ref['grad_output'], 1e-5, 1e-4, scale=saturated)
        # the channels the option leaves alone
        assert _same(got[key][..., :4], base[key][..., :4]), (tag, key, 'box channels')
        if obj_alone:
            assert _same(got[key][..., 4], base[key][..., 4]), (tag, key, 'objectness channel')
        if cls_alone:
            assert _same(got[key][..., 5:], base[key][..., 5:]), (tag, key, 'class channels')


# ------------------------------------------------------------------------------------------ the defaults
@pytest.mark.parametrize('K', (64, 65))
@pytest.mark.parametrize('C', (1, 33))
def test_defaults_give_the_existing_bits(dev, C, K):
    """The *_opts entries with the defaults against the first entries and, with iou_thresh / label_smooth set, against the
    _ex entries: every output and every byte of the workspace."""
    labels, cfg, layers = LO.plain_layers(C, K)
    for l, (out, pred) in enumerate(layers):
        for entry, iou, eps in (('old', 1.0, 0.0), ('ex', 1.0, 0.0), ('ex', 0.213, 0.1)):
            a = _run(dev, out, pred, labels, l, C, None, iou, eps, entry)
            b = _run(dev, out, pred, labels, l, C, None, iou, eps, 'opts')
            for k in KEYS + ('ws',):
                assert _same(a[k], b[k]), (k, l, entry)
            assert a['parts'][2] > 0


# ------------------------------------------------------------------------------------------ focal loss and the gains
@pytest.mark.parametrize('CK', LO.SETS, ids=lambda ck: 'C%d-K%d' % ck)
@pytest.mark.parametrize('opt', LO.FOCAL_SETS + LO.GAIN_SETS, ids=LO.opt_id)
def test_focal_and_gains_against_the_reference(dev, opt, CK):
    C, K = CK
    labels, cfg, layers = LO.plain_layers(C, K)
    worst = Worst()
    for l, (out, pred) in enumerate(layers):
        base = _run(dev, out, pred, labels, l, C)
        got = _run(dev, out, pred, labels, l, C, opt)
        _check(got, LO.reference(C, K, 'plain', l, opt), base, opt, l, 'C%d K%d layer %d' % (C, K, l), worst)
    worst.report('%s C%d K%d' % (LO.opt_id(opt), C, K))


@pytest.mark.parametrize('opt', LO.GAIN_SETS, ids=LO.opt_id)
def test_gains_scale_the_gain_one_results_exactly(dev, opt):
    """parts[2:4] are the gain-1 parts times the gains to 1 ulp of fp64 (one fp64 product); the gradient channels are the
    fp32 product g * gain of the gain-1 run bit for bit -- with focal loss on as well."""
    C, K = 33, 64
    labels, cfg, layers = LO.plain_layers(C, K)
    for focal in ({}, dict(focal_gamma=1.5)):
        for l, (out, pred) in enumerate(layers):
            o = LO.options(opt, l)
            base = _run(dev, out, pred, labels, l, C, focal)
            got = _run(dev, out, pred, labels, l, C, dict(focal, **opt))
            for q, gain in ((2, o['obj_gain']), (3, o['cls_gain'])):
                want = base['parts'][q] * gain
                ulps = abs(got['parts'][q] - want) / np.spacing(abs(want))
                print('layer %d part %d: %.17g against %.17g, %.1f ulp' % (l, q, got['parts'][q], want, ulps))
                assert ulps <= 1.0
            assert _same(got['parts'][:2], base['parts'][:2])
            for key in ('grad', 'grad_masked'):
                assert _same(got[key][..., 4], base[key][..., 4] * F32(o['obj_gain'])), (l, key)
                assert _same(got[key][..., 5:], base[key][..., 5:] * F32(o['cls_gain'])), (l, key)
                assert _same(got[key][..., :4], base[key][..., :4]), (l, key)


def test_saturated_logits_with_focal_loss(dev):
    """+-30 logits, cells with o == 1.0f in the objectness channel: finite, the gradient under the project's scaled
    close(1e-5, 1e-4)."""
    C, K = 33, 64
    labels, cfg, layers = LO.plain_layers(C, K, True)
    worst = Worst()
    for opt in (dict(focal_gamma=2.0), dict(focal_gamma=0.5, focal_alpha=0.0), LO.ALL_ON):
        box = opt is LO.ALL_ON
        for l, (out, pred) in enumerate(layers):
            assert (out[..., 4] == F32(1)).any()
            iou, eps = (0.213, 0.1) if box else (1.0, 0.0)
            base = _run(dev, out, pred, labels, l, C, None, iou, eps)
            got = _run(dev, out, pred, labels, l, C, opt, iou, eps)
            ref = LO.reference(C, K, 'sat', l, opt, iou, eps)
            _check(got, ref, base, opt, l, 'saturated %s layer %d' % (LO.opt_id(opt)[:20], l), worst, saturated=True)
    worst.report('saturated')


# ------------------------------------------------------------------------------------------ IoU-aware objectness
def _t_obj(got, cells):
    return got['target'][tuple(cells.T) + (4,)] if len(cells) else np.zeros(0, F32)


@pytest.mark.parametrize('CK', LO.SETS, ids=lambda ck: 'C%d-K%d' % ck)
@pytest.mark.parametrize('kind', BC.KINDS)
def test_iou_aware_objectness(dev, kind, CK):
    """r in (0.5, 1) on the planted boxes of headopt_cases.box_case (several anchors, scaled centres): t_obj through the
    dense targets within BOX_FACTOR x the fp32 yardstick's largest t_obj error of the float64 reference, and bit-equal
    to (1 - r) + r * max(X, 0) with max(X, 0) read from the run with r = 1; loss parts and gradient at the bars of
    _check, the box channels and class channels bit-equal to the run without the option."""
    C, K = CK
    labels, cfg, layers = LO.box_layers(C, K)
    e32 = LO.t_obj_fp32_error(kind)
    bound = BC.BOX_FACTOR * e32
    worst, ratio = Worst(), 0.0
    for l, (out, pred) in enumerate(layers):
        base = _run(dev, out, pred, labels, l, C, None, 0.213)
        x_dev = None
        for r in (1.0, 0.5):
            opt = dict(obj_iou_ratio=r, obj_iou_kind=kind)
            ref = LO.reference(C, K, 'box', l, opt, 0.213)
            got = _run(dev, out, pred, labels, l, C, opt, 0.213)
            t = _t_obj(got, ref['cells'])
            if not len(t):
                continue
            err = float(np.abs(t.astype(np.float64) - ref['t_obj']).max())
            ratio = max(ratio, err / e32)
            print('%s C%d K%d layer %d r %g: largest |t_obj - ref64| %.3g, fp32 yardstick %.3g, bound %.3g, %d records, '
                  '%d with X <= 0' % (kind, C, K, l, r, err, e32, bound, len(t), int((ref['X'] <= 0).sum())))
            assert err <= bound
            if r == 1.0:
                x_dev = t
                assert (t >= 0).all()
            else:
                assert _same(t, (F32(1) - F32(r)) + F32(r) * x_dev)
            _check(got, ref, base, opt, l, '%s r %g C%d K%d layer %d' % (kind, r, C, K, l), worst)
    print('%s C%d K%d: kernel t_obj error / fp32-restatement error %.3f (allowed %.1f)' % (kind, C, K, ratio, BC.BOX_FACTOR))
    worst.report('%s C%d K%d' % (kind, C, K))


def test_nan_in_a_positive_cells_pred(dev):
    """A NaN in one record's pred with r > 0: parts[2] is NaN, that cell's channel-4 gradient is NaN, every other gradient
    element has the bits of the clean run (so does parts[3])."""
    C, K = 33, 64
    labels, cfg, layers = LO.box_layers(C, K)
    out, pred0 = layers[1]
    opt = dict(obj_iou_ratio=0.5, obj_iou_kind='ciou', focal_gamma=2.0)
    ref = LO.reference(C, K, 'box', 1, opt, 0.213)
    clean = _run(dev, out, pred0, labels, 1, C, opt, 0.213)
    b, a, j, i = ref['cells'][5]
    for comp in (0, 3):
        pred = pred0.copy()
        pred[b, a, j, i, comp] = np.nan
        got = _run(dev, out, pred, labels, 1, C, opt, 0.213)
        assert np.isnan(got['parts'][2]) and _same(got['parts'][3:], clean['parts'][3:]) and np.isfinite(got['parts'][:2]).all()
        assert np.isnan(got['target'][b, a, j, i, 4])
        for key in ('grad', 'grad_masked'):
            assert np.isnan(got[key][b, a, j, i, 4])
            other = np.ones(got[key].shape, bool)
            other[b, a, j, i, 4] = False
            assert _same(got[key][other], clean[key][other]), (comp, key)


# ------------------------------------------------------------------------------------------ record order, determinism
def test_k64_and_k65_agree_exactly_with_all_options_on_and_two_runs_agree(dev):
    C, K = 33, 64
    labels, cfg, layers = LO.box_layers(C, K)
    more = np.concatenate([labels, np.zeros((3, 1, 5))], 1)
    iou, eps = LO.ALL_ON_HEAD['iou_thresh'], LO.ALL_ON_HEAD['label_smooth']
    for l, (out, pred) in enumerate(layers):
        a = _run(dev, out, pred, labels, l, C, LO.ALL_ON, iou, eps)
        b = _run(dev, out, pred, more, l, C, LO.ALL_ON, iou, eps)
        c = _run(dev, out, pred, labels, l, C, LO.ALL_ON, iou, eps)
        assert a['parts'][2] > 0 and a['parts'][3] > 0
        for k in KEYS:
            assert _same(a[k], b[k]), (k, l, 'K = 65')
            assert _same(a[k], c[k]), (k, l, 'second run')
        assert _same(a['ws'], c['ws'])


@pytest.mark.parametrize('CK', LO.SETS, ids=lambda ck: 'C%d-K%d' % ck)
def test_all_options_together(dev, CK):
    """focal (2, 0.25) on both terms, r = 0.5 of CIoU, obj_gain (4, 1, 0.4), cls_gain 2.5, iou_thresh 0.213,
    label_smooth 0.1 on the inputs decoded with scale_x_y (1.2, 1.1, 1.05)."""
    C, K = CK
    labels, cfg, layers = LO.box_layers(C, K)
    iou, eps = LO.ALL_ON_HEAD['iou_thresh'], LO.ALL_ON_HEAD['label_smooth']
    worst = Worst()
    for l, (out, pred) in enumerate(layers):
        base = _run(dev, out, pred, labels, l, C, None, iou, eps)
        got = _run(dev, out, pred, labels, l, C, LO.ALL_ON, iou, eps)
        _check(got, LO.reference(C, K, 'box', l, LO.ALL_ON, iou, eps), base, LO.ALL_ON, l, 'all C%d K%d layer %d' % (C, K, l), worst)
    worst.report('all options C%d K%d' % (C, K))


# ------------------------------------------------------------------------------------------ YOLOLayer + YOLOLoss
E2E_C, E2E_K = 33, 64
E2E_SCALE = [1.2, 1.1, 1.05]


@pytest.mark.parametrize('mutate', (True, False), ids=('mutate', 'keep'))
def test_options_through_yololayer_and_yololoss(dev, mutate):
    """YOLOLayer (SCALE_X_Y) -> YOLOLoss(box_loss='ciou', every option on) -> backward to the logits, against the composed
    float64 restatement evaluated on the output / pred the layers produced: objectness and class parts 1e-4 relative,
    g_output (read through the logits' gradient outside the box channels of the record cells, which
    tests/test_gpu_headopt.py covers) HC.close(1e-5, 1e-4); build_target's target[..., 4] holds t_obj."""
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    gain = 0.05
    d = HO.loss_inputs(E2E_C, E2E_K)
    cfg = dict(d['cfg'], SCALE_X_Y=E2E_SCALE)
    kw = dict(LO.ALL_ON)
    kind = kw.pop('obj_iou_kind')
    crit = YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=mutate, box_loss=kind, box_gain=gain, iou_thresh=0.213,
                    label_smooth=0.1, **kw)
    lgs = [torch.from_numpy(np.array(lay[0])).to(dev).requires_grad_(True) for lay in d['layers']]
    ods = [YOLOLayer(cfg, l, device=dev).train()(lg) for l, lg in enumerate(lgs)]
    outs = [od['output'].detach().clone().cpu().numpy() for od in ods]
    preds = [od['pred'].detach().clone().cpu().numpy() for od in ods]
    labels = torch.from_numpy(np.array(d['labels']))
    loss = crit(ods, {'padded_labels': labels})
    loss.backward()
    torch.cuda.synchronize()
    n_ch = 5 + E2E_C
    total = 0.0
    for l in range(3):
        lg = d['layers'][l][0]
        B, _, F, _ = lg.shape
        ref = LO.loss_ref(outs[l], preds[l], l, d['labels'], cfg, 0.7, 0.213, 0.1, LO.ALL_ON)
        parts = crit.last[l]['parts'].cpu().numpy()
        total += parts.sum()
        for q, name in ((2, 'obj'), (3, 'cls')):
            rel = abs(parts[q] - ref[name]) / abs(ref[name])
            print('layer %d %s: %.12g ref %.12g relative error %.3g' % (l, name, parts[q], ref[name], rel))
            assert rel <= 1e-4
        assert parts[1] == 0.0 and parts[0] > 0
        final = ods[l]['output'].detach().cpu().numpy()
        if mutate:
            HC.close(final, ref['mutated_output'], 1e-6, 1e-6, scale=False)
        else:
            assert _same(final, outs[l])
        nhwc = np.ascontiguousarray(lg.transpose(0, 2, 3, 1)).reshape(-1, 3 * n_ch)
        pos = np.zeros(ref['grad_output'].shape[:4], bool)
        pos[tuple(ref['cells'].T)] = True
        gref, _ = HC.decode_bwd_ref64(nhwc, 3 * n_ch, B, F, 3, E2E_C, H.masked_anchors(cfg, l), ref['grad_output'], None)
        gref = gref.reshape(B, F, F, 3, n_ch).transpose(0, 3, 1, 2, 4)
        g = lgs[l].grad.cpu().numpy().reshape(B, 3, n_ch, F, F).transpose(0, 1, 3, 4, 2)
        assert np.isfinite(g).all()
        box = np.zeros(g.shape, bool)
        box[..., :4] = pos[..., None]
        HC.close(np.where(box, 0.0, g), np.where(box, 0.0, gref), 1e-5, 1e-4)
        tgt, om, tm, ts = crit.build_target(torch.from_numpy(outs[l]).to(dev), torch.from_numpy(preds[l]).to(dev), l, labels)
        assert np.array_equal(om.cpu().numpy(), ref['obj_mask']) and np.array_equal(tm.cpu().numpy(), ref['tgt_mask'])
        t = tgt.cpu().numpy()
        HC.close(t[..., :4], ref['target'][..., :4], 1e-6, 1e-6, scale=False)
        HC.close(t[..., 5:], ref['target'][..., 5:], 1e-6, 1e-6, scale=False)
        e = float(np.abs(t[..., 4] - ref['target'][..., 4]).max())
        print('layer %d: largest |target[..., 4] - ref64| %.3g (bound %.3g)' % (l, e, BC.BOX_FACTOR * LO.t_obj_fp32_error(kind)))
        assert e <= BC.BOX_FACTOR * LO.t_obj_fp32_error(kind)
        assert ((t[..., 4][pos] >= 0.5) & (t[..., 4][pos] <= 1.0)).all() and (t[..., 4][~pos] == 0).all()
    assert abs(float(loss.detach()) - total) <= 2.0 ** -22 * abs(total)


def test_default_constructor_is_bit_equal_to_the_explicit_defaults(dev):
    """YOLOLoss(cfg) and YOLOLoss(cfg, every new keyword at its default) against the first C entries: loss parts and the
    gradient of `output` bit for bit."""
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    C, K = 33, 64
    labels, cfg, layers = LO.plain_layers(C, K)
    lab = torch.from_numpy(np.array(labels))
    for crit in (YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=False),
                 YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=False, focal_gamma=0.0, focal_alpha=0.25, focal_terms='obj+cls',
                          obj_iou_ratio=0.0, obj_gain=1.0, cls_gain=1.0)):
        ods = []
        for l, (out, pred) in enumerate(layers):
            ods.append(dict(layer_no=l, output=_up(out, dev).requires_grad_(True), pred=_up(pred, dev)))
        crit(ods, {'padded_labels': lab}).backward()
        torch.cuda.synchronize()
        for l, (out, pred) in enumerate(layers):
            old = _run(dev, out, pred, labels, l, C, entry='old')
            assert _same(crit.last[l]['parts'].cpu().numpy(), old['parts'])
            assert _same(ods[l]['output'].grad.cpu().numpy(), old['grad'])
            assert crit.last[l]['nbytes'] == old['ws'].size
