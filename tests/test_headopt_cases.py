# -*- coding: utf-8 -*-
"""Without a GPU: the restatement of tests/headopt_cases.py against oracle.head with the options off, the properties
the GPU tests of the YOLOv4 head options rely on (so that none of them can pass by missing its branch), and the host
side of the new entry points: symbols, workspace sizes, errors before any launch, constructor checks."""
import copy
import ctypes
import inspect

import numpy as np
import pytest
import torch

import head_cases as HC
import headopt_cases as HO
import recipe
from oracle import head as H

F32 = np.float32
FAKE = 0x1000                            # a non-NULL device pointer that no host code dereferences


# ------------------------------------------------------------------------------------------ the restatement, options off
@pytest.mark.parametrize('C,K', [(1, 1), (33, 64), (33, 65), (1, 100)])
def test_loss_restatement_equals_the_oracle_with_the_options_off(C, K):
    d = HO.loss_inputs(C, K)
    for l, (lg, out, pred) in enumerate(d['layers']):
        r = HO.loss_ref(out, pred, l, d['labels'], d['cfg'], dtype=F32)
        o = H.yolo_loss_layer(out, pred, l, d['labels'], d['cfg'])
        for k in ('target', 'obj_mask', 'tgt_mask', 'tgt_scale'):
            assert np.array_equal(r[k], o[k]), (k, l)
        for k in ('xy', 'wh', 'obj', 'cls', 'loss'):
            assert abs(r[k] - o[k]) <= 1e-12 * abs(o[k]), (k, l, r[k], o[k])
        assert np.array_equal(r['grad_output'], o['grad_output'])
        # the float64 evaluation is the same function a few fp32 roundings away
        r64 = HO.loss_ref(out, pred, l, d['labels'], d['cfg'])
        assert np.array_equal(r64['tgt_mask'], o['tgt_mask']) and np.array_equal(r64['obj_mask'], o['obj_mask'])
        HC.close(r64['target'], o['target'], 1e-6, 1e-6, scale=False)
        assert abs(r64['loss'] - o['loss']) <= 1e-5 * abs(o['loss'])


@pytest.mark.parametrize('case', HC.DECODE_CASES[:4] + HC.DECODE_CASES[6:8], ids=lambda c: 'C%d-A%d-F%d-B%d-ld%d' % c)
def test_decode_restatement_with_scale_one(case):
    C, A, F, B, ldl = case
    lg, _ = HC.make_logits(B, F, A, C, ldl, 5)
    anc = HC.decode_anchors(A, 1)
    out, pred, S = HO.decode_ref64(lg, ldl, B, F, A, C, anc, 8.0, True, 1.0)
    o0, p0 = HC.decode_ref64(lg, ldl, B, F, A, C, anc, 8.0, True)
    assert np.array_equal(out, o0)
    assert np.array_equal(pred, p0)                                        # (o * 1 - 0) + i is o + i, in float64 too
    assert (S[..., 0] >= np.abs(pred[..., 0])).all()
    rows, Se = HO.decode_ref64(lg, ldl, B, F, A, C, anc, 8.0, False, 1.0)
    r0 = HC.decode_ref64(lg, ldl, B, F, A, C, anc, 8.0, False)
    np.testing.assert_allclose(rows, r0, rtol=2.0 ** -50, atol=0)
    go = np.random.RandomState(1).standard_normal((B, A, F, F, 5 + C))
    gp = np.random.RandomState(2).standard_normal((B, A, F, F, 4))
    a = HO.decode_bwd_ref64(lg, ldl, B, F, A, C, anc, go, gp, 1.0)
    b = HC.decode_bwd_ref64(lg, ldl, B, F, A, C, anc, go, gp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_decode_restatement_against_the_oracle_decode():
    """the model-shaped case through oracle.head.yolo_decode (fp32): the float64 restatement at s = 1 is within fp32
    rounding of it, and the scaled centre moves by exactly (s - 1) * (sigma - 0.5)"""
    cfg = HC.cfg_with_classes(3)
    lg = recipe.synth_head_logits(2, 8, 3, n_ch=24).numpy()
    out, pred = H.yolo_decode(lg, 1, cfg, True)
    nhwc = lg.transpose(0, 2, 3, 1).reshape(-1, 24)
    anc = H.masked_anchors(cfg, 1)
    o64, p64, _ = HO.decode_ref64(nhwc, 24, 2, 8, 3, 3, anc, 16.0, True, 1.0)
    np.testing.assert_allclose(out, o64, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(pred, p64, rtol=1e-6, atol=1e-7)
    _, p2, _ = HO.decode_ref64(nhwc, 24, 2, 8, 3, 3, anc, 16.0, True, 2.0)
    np.testing.assert_allclose(p2[..., :2] - p64[..., :2], o64[..., :2] - 0.5, atol=1e-12)
    assert np.array_equal(p2[..., 2:], p64[..., 2:])
    assert HO.s_h(1.2) == (float(F32(1.2)), float((F32(1.2) - F32(1)) * F32(0.5)))


# ------------------------------------------------------------------------------------------ the cases hold what they claim
def test_multi_anchor_case_properties():
    cfg = HC.cfg_with_classes(33)
    lab64 = HC.make_labels(64, 33, 164)[0]
    p = HO.assign_props(lab64, cfg, 0.213)
    assert [q['max_records'] for q in p] == [72, 65, 20]                  # > K on layers 0 and 1: the grown capacity
    assert [q['extra'] for q in p] == [57, 83, 30]
    assert [q['collisions'] for q in p] == [8, 26, 14]
    assert p[0]['all_three'] == 10 and p[1]['all_three'] == 19
    lab100 = HC.make_labels(100, 33, 200)[0]
    p100 = HO.assign_props(lab100, cfg, 0.213)
    assert p100[0]['max_records'] == 133
    # the fp32 positive set is well defined: nothing within 100 ulp of the threshold
    d = min(HO.closest_to_thresh(lab64, cfg, 0.213), HO.closest_to_thresh(lab100, cfg, 0.213))
    assert d >= 100 * 2.0 ** -24 * 0.213 * 2, d
    # with the option off there is one pair per positive label, in label order
    for l, Fs in enumerate(HC.LOSS_F):
        asg = HO.assign(lab64, l, cfg, Fs, 1.0)
        assert not any(q[4] for pp in asg['pairs'] for q in pp)
        assert all(len({q[0] for q in pp}) == len(pp) for pp in asg['pairs'])


def test_record_order_is_first_hit_in_label_then_slot_order():
    cfg = HC.cfg_with_classes(33)
    d = HO.loss_inputs(33, 64)
    for l, (lg, out, pred) in enumerate(d['layers']):
        info = HO.build_target(out, pred, l, d['labels'], cfg, 0.7, 0.213)[4]
        asg = HO.assign(d['labels'], l, cfg, HC.LOSS_F[l], 0.213)
        for b, inf in enumerate(info):
            pairs = asg['pairs'][b]
            assert pairs == sorted(pairs, key=lambda q: (q[0], q[1]))
            assert inf['records'] == HO.records_of(pairs) and len(set(inf['records'])) == len(inf['records'])
            for rec, tr in zip(inf['records'], inf['truth']):               # last writer wins
                t_last = [q[0] for q in pairs if (q[1], q[2], q[3]) == rec][-1]
                assert np.array_equal(tr, (d['labels'][b, t_last, :4].astype(F32) / F32(H.STRIDES[l])))
        assert any(any(inf['first_extra']) for inf in info)


def test_planted_threshold_is_strict():
    cfg = HC.cfg_with_classes(33)
    lab = HC.make_labels(64, 33, 164)[0]
    for l in (0, 1):
        thr, b, t, a = HO.planted_tie(lab, cfg, l)
        assert thr == float(F32(thr)) and 0 < thr < 1
        at = HO.assign(lab, l, cfg, HC.LOSS_F[l], thr)['pairs'][b]
        below = HO.assign(lab, l, cfg, HC.LOSS_F[l], float(np.nextafter(F32(thr), F32(0))))['pairs'][b]
        assert not any(q[0] == t and q[1] == a for q in at)
        assert any(q[0] == t and q[1] == a and q[4] for q in below)


def test_smoothed_targets_and_box_case():
    lo, hi = HO.smooth_targets(0.1)
    assert lo == float(F32(0.5) * F32(0.1)) and hi == float(F32(1) - F32(0.5) * F32(0.1))
    assert HO.smooth_targets(0.0) == (0.0, 1.0)
    d = HO.loss_inputs(33, 64)
    lg, out, pred = d['layers'][1]
    r = HO.loss_ref(out, pred, 1, d['labels'], d['cfg'], 0.7, 0.213, 0.1)
    pos = r['tgt_mask'][..., 0] > 0
    cls = r['target'][..., 5:]
    assert set(np.unique(cls[pos])) == {lo, hi} and not cls[~pos].any()
    assert (r['target'][..., 4][pos] == 1).all()                           # objectness is not smoothed
    r0 = HO.loss_ref(out, pred, 1, d['labels'], d['cfg'], 0.7, 0.213, 0.0)
    assert r['cls'] > r0['cls'] and r['obj'] == r0['obj'] and r['xy'] == r0['xy']
    case = HO.box_case(33, 64)
    n = {}
    for l, lay in enumerate(case['layers']):
        for k in lay['plants']:
            n[k] = n.get(k, 0) + 1
        assert HO.s_h(HO.scale_of(case['scale'], l))[1] > 0
    assert len(n) == 9 and min(n.values()) >= 10
    assert any(any(inf['first_extra']) for lay in case['layers'] for inf in lay['info'])
    # saturated logits exist on positive and background cells
    sat = HO.loss_inputs(33, 64, True)
    assert sat['props']['planted_positive'] > 0 and sat['props']['planted_background'] > 0


# ------------------------------------------------------------------------------------------ the C ABI without a GPU
NEW_SYMBOLS = ('y4_yolo_decode_train_ex_f32', 'y4_yolo_decode_eval_ex_f32', 'y4_yolo_decode_bwd_ex_f32',
               'y4_yolo_loss_workspace_ex', 'y4_yolo_loss_fwd_ex_f32', 'y4_yolo_loss_bwd_ex_f32',
               'y4_yolo_loss_mask_output_ex_f32', 'y4_yolo_loss_dense_targets_ex_f32', 'y4_yolo_box_loss_fwd_ex_f32',
               'y4_yolo_box_loss_bwd_ex_f32')
NAN = float('nan')


def _lib():
    import yolov4_amd
    return yolov4_amd.lib()


def test_new_symbols_are_exported():
    from yolov4_amd import _lib as B
    L = _lib()
    for s in NEW_SYMBOLS:
        assert s in B.PROTOTYPES and hasattr(L, s), s


def test_capacity_aware_workspace_query():
    L = _lib()
    for B, F, K, C in ((4, 76, 60, 80), (3, 16, 1, 1), (3, 4, 100, 33)):
        base = L.y4_yolo_loss_workspace(B, F, 3, K, C)
        assert L.y4_yolo_loss_workspace_ex(B, F, 3, K, C, 1.0) == base
        on = L.y4_yolo_loss_workspace_ex(B, F, 3, K, C, 0.213)
        cw = (C + 31) // 32
        assert on >= base + B * 2 * K * 4 * (1 + 5 + cw + 4) - 4 * 16 and on > base
    for bad in (0.0, -0.5, 1.5, NAN):
        assert L.y4_yolo_loss_workspace_ex(4, 76, 3, 60, 80, bad) == 0
    assert L.y4_yolo_loss_workspace_ex(0, 76, 3, 60, 80, 0.5) == 0


def test_decode_option_errors_before_any_launch():
    from yolov4_amd._lib import float_array
    L = _lib()
    anc = float_array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert L.y4_yolo_decode_train_ex_f32(None, 24, FAKE, FAKE, 1, 4, 3, 3, anc, 1.2, None) == 2
    assert L.y4_yolo_decode_eval_ex_f32(FAKE, 24, None, 48, 0, 1, 4, 3, 3, anc, 8.0, 1.2, None) == 2
    assert L.y4_yolo_decode_bwd_ex_f32(FAKE, 24, None, None, None, 1, 4, 3, 3, anc, 1.2, None) == 2
    for s in (0.999, 2.001, -1.0, NAN, float('inf')):
        assert L.y4_yolo_decode_train_ex_f32(FAKE, 24, FAKE, FAKE, 1, 4, 3, 3, anc, s, None) == 1, s
        assert L.y4_yolo_decode_eval_ex_f32(FAKE, 24, FAKE, 48, 0, 1, 4, 3, 3, anc, 8.0, s, None) == 1, s
        assert L.y4_yolo_decode_bwd_ex_f32(FAKE, 24, FAKE, FAKE, FAKE, 1, 4, 3, 3, anc, s, None) == 1, s
    assert L.y4_yolo_decode_train_ex_f32(FAKE, 23, FAKE, FAKE, 1, 4, 3, 3, anc, 1.2, None) == 1       # pitch < A * (5 + C)


def test_loss_option_errors_before_any_launch():
    from yolov4_amd._lib import float_array, int_array
    L = _lib()
    cfg = HC.cfg_with_classes(3)
    anchors = float_array(H.all_anchors(cfg, 0).ravel())
    mask = int_array(cfg['ANCHOR_MASK'][0])
    B, F, A, K, C = 2, 16, 3, 8, 3
    big = 1 << 30

    def fwd(iou=0.213, eps=0.1, ws=FAKE, nbytes=big, out=FAKE, m=mask, k=K):
        return L.y4_yolo_loss_fwd_ex_f32(out, FAKE, FAKE, k, B, F, A, C, 8.0, 0.7, anchors, 9, m, iou, eps, FAKE, FAKE, ws,
                                         nbytes, None)

    assert fwd(out=None) == 2 and fwd(ws=None) == 2 and fwd(m=None) == 2
    for iou in (0.0, -0.1, 1.0001, NAN):
        assert fwd(iou=iou) == 1, iou
    for eps in (-0.01, 1.0, 2.0, NAN):
        assert fwd(eps=eps) == 1, eps
    assert fwd(k=0) == 1
    assert fwd(m=int_array([1, 0, 2])) == 1                  # several anchors need mask[a] % 3 == a ...
    assert fwd(iou=1.0, m=int_array([1, 0, 2]), nbytes=0) == 4        # ... one anchor does not: it gets as far as the workspace
    need = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, 0.213)
    assert fwd(nbytes=need - 1) == 4
    assert fwd(nbytes=L.y4_yolo_loss_workspace(B, F, A, K, C)) == 4           # the one-anchor size is too small
    short = need - 1
    one = FAKE
    calls = {
        'bwd': lambda iou, eps, n: L.y4_yolo_loss_bwd_ex_f32(FAKE, 0, FAKE, one, FAKE, B, F, A, K, C, iou, eps, FAKE, n, None),
        'mask': lambda iou, eps, n: L.y4_yolo_loss_mask_output_ex_f32(FAKE, FAKE, B, F, A, K, C, iou, FAKE, n, None),
        'dense': lambda iou, eps, n: L.y4_yolo_loss_dense_targets_ex_f32(FAKE, FAKE, FAKE, B, F, A, K, C, iou, eps, FAKE, n,
                                                                          None),
        'box_fwd': lambda iou, eps, n: L.y4_yolo_box_loss_fwd_ex_f32(FAKE, 4, 1.0, B, F, A, K, C, iou, FAKE, FAKE, n, None),
        'box_bwd': lambda iou, eps, n: L.y4_yolo_box_loss_bwd_ex_f32(FAKE, 4, 1.0, one, FAKE, B, F, A, K, C, iou, 1.2, FAKE,
                                                                      n, None),
    }
    for name, call in calls.items():
        assert call(0.213, 0.1, short) == 4, name
        assert call(0.0, 0.1, big) == 1 and call(NAN, 0.1, big) == 1, name
    assert calls['bwd'](0.213, 1.0, big) == 1 and calls['dense'](0.213, NAN, big) == 1
    assert L.y4_yolo_loss_bwd_ex_f32(None, 0, FAKE, one, FAKE, B, F, A, K, C, 0.213, 0.1, FAKE, big, None) == 2
    assert L.y4_yolo_loss_mask_output_ex_f32(None, FAKE, B, F, A, K, C, 0.213, FAKE, big, None) == 2
    assert L.y4_yolo_loss_dense_targets_ex_f32(FAKE, None, FAKE, B, F, A, K, C, 0.213, 0.1, FAKE, big, None) == 2
    assert L.y4_yolo_box_loss_fwd_ex_f32(None, 4, 1.0, B, F, A, K, C, 0.213, FAKE, FAKE, big, None) == 2
    assert L.y4_yolo_box_loss_bwd_ex_f32(FAKE, 4, 1.0, None, FAKE, B, F, A, K, C, 0.213, 1.2, FAKE, big, None) == 2
    assert L.y4_yolo_box_loss_fwd_ex_f32(FAKE, 9, 1.0, B, F, A, K, C, 0.213, FAKE, FAKE, big, None) == 1
    for s in (0.5, 2.5, NAN):
        assert L.y4_yolo_box_loss_bwd_ex_f32(FAKE, 4, 1.0, one, FAKE, B, F, A, K, C, 0.213, s, FAKE, big, None) == 1, s


# ------------------------------------------------------------------------------------------ the Python surface
def test_constructors_reject_bad_options_without_a_gpu():
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    cfg = recipe.MODEL_CFG
    for s in (0.9, 2.1, float('nan'), [1.2, 1.1], [1.2, 1.1, 0.5]):
        bad = dict(cfg, SCALE_X_Y=s)
        with pytest.raises(ValueError):
            YOLOLayer(bad, 2)
        with pytest.raises(ValueError):
            YOLOLoss(bad, 0.7, box_loss='ciou')
    with pytest.raises(ValueError):
        YOLOLoss(dict(cfg, SCALE_X_Y=[1.2, 1.1, 1.05]), 0.7)                      # 'mse' with s != 1
    with pytest.raises(ValueError):
        YOLOLoss(dict(cfg, SCALE_X_Y=1.05), 0.7, box_loss='mse')
    for thr in (0.0, -0.2, 1.2, float('nan')):
        with pytest.raises(ValueError):
            YOLOLoss(cfg, 0.7, iou_thresh=thr)
    for eps in (1.0, 1.5, -0.1, float('nan')):
        with pytest.raises(ValueError):
            YOLOLoss(cfg, 0.7, label_smooth=eps)
    ok = YOLOLoss(dict(cfg, SCALE_X_Y=[1.2, 1.1, 1.05]), 0.7, box_loss='ciou', iou_thresh=0.213, label_smooth=0.1)
    assert ok.scale_xy == [1.2, 1.1, 1.05] and ok.iou_thresh == 0.213 and ok.label_smooth == 0.1
    assert YOLOLoss(dict(cfg, SCALE_X_Y=1.0), 0.7).scale_xy == [1.0, 1.0, 1.0]         # 'mse' with s = 1 is fine
    lc = ok._layer_cfg(1)
    assert lc['scale_xy'] == 1.1 and lc['iou_thresh'] == 0.213 and lc['label_smooth'] == 0.1
    assert [YOLOLayer(dict(cfg, SCALE_X_Y=[1.2, 1.1, 1.05]), l).scale_xy for l in range(3)] == [1.2, 1.1, 1.05]
    assert YOLOLayer(dict(cfg, SCALE_X_Y=2), 0).scale_xy == 2.0 and YOLOLayer(cfg, 0).scale_xy == 1.0
    d = YOLOLoss(cfg, 0.7)
    assert d.iou_thresh == 1.0 and d.label_smooth == 0.0 and d.box_loss == 'mse'


def test_signatures_and_factory():
    from yolov4_amd import ops
    from yolov4_amd.yolo.model.build import build_criterion
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    sig = inspect.signature(YOLOLoss.__init__).parameters
    assert list(sig)[1:4] == ['cfg', 'ignore_thresh', 'device']
    assert sig['iou_thresh'].default == 1.0 and sig['label_smooth'].default == 0.0
    assert list(inspect.signature(YOLOLayer.__init__).parameters)[1:] == ['cfg', 'layer_no', 'device']
    assert inspect.signature(ops.yolo_decode_eval).parameters['scale_xy'].default == 1.0
    assert inspect.signature(ops.YoloDecodeTrainFn.forward).parameters['scale_xy'].default == 1.0
    full = copy.deepcopy(recipe.FULL_CFG)
    full['CRITERION'].update(BOX_LOSS='ciou', IOU_THRESH=0.213, LABEL_SMOOTH=0.1)
    full['MODEL']['SCALE_X_Y'] = [1.2, 1.1, 1.05]
    c = build_criterion(full, device=torch.device('cpu'))
    assert (c.iou_thresh, c.label_smooth, c.box_loss, c.scale_xy) == (0.213, 0.1, 'ciou', [1.2, 1.1, 1.05])
    c0 = build_criterion(recipe.FULL_CFG, device=torch.device('cpu'))
    assert (c0.iou_thresh, c0.label_smooth, c0.scale_xy) == (1.0, 0.0, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        ops.check_scale_xy(3.0)
    with pytest.raises(ValueError):
        ops.check_loss_options(0.0, 0.0)
