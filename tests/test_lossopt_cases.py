# -*- coding: utf-8 -*-
"""Without a GPU: the restatement of focal loss, IoU-aware objectness and the gains (tests/lossopt_cases.py) against torch
float64 autograd and against headopt_cases.loss_ref, what the inputs of tests/test_gpu_lossopt.py hold, the fp32
yardstick's own distance from the float64 reference, option validation in Python and at the C ABI, and the cfg keys."""
import copy
import ctypes
import inspect

import numpy as np
import pytest

import boxloss_cases as BC
import head_cases as HC
import headopt_cases as HO
import lossopt_cases as LO
import recipe

F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------ the closed form
@pytest.mark.parametrize('ga', ((2.0, 0.25), (1.5, 0.0), (0.5, 0.5), (5.0, 0.75)), ids=lambda ga: 'g%g-a%g' % ga)
def test_closed_form_focal_equals_torch_autograd(ga):
    """4096 random (o, t), o in [1e-4, 1 - 1e-4], a third of the targets 0, a third 1, a third soft: loss and gradient of
    the closed form against torch float64 autograd of a * bce * (1 - p_t)^gamma, 1e-10 relative."""
    gamma, alpha = ga
    rng = np.random.RandomState(5)
    o = rng.uniform(1e-4, 1 - 1e-4, 4096)
    o[:64] = np.r_[np.full(32, 1e-4), np.full(32, 1 - 1e-4)]
    t = rng.uniform(0, 1, 4096)
    t[0::3] = 0.0
    t[1::3] = 1.0
    fl, g = LO.focal(o, t, gamma, alpha, np.float64)
    fl_t, g_t = LO.focal_torch64(o, t, gamma, alpha)
    e_l = float((np.abs(fl - fl_t) / np.maximum(np.abs(fl_t), 1e-300)).max())
    e_g = float((np.abs(g - g_t) / np.maximum(np.abs(g_t), 1e-300)).max())
    print('gamma %g alpha %g: largest relative difference loss %.3g, gradient %.3g' % (gamma, alpha, e_l, e_g))
    assert e_l <= 1e-10 and e_g <= 1e-10


def test_focal_is_zero_where_q_is_zero():
    for dt in (np.float64, F32):
        fl, g = LO.focal(np.array([1.0, 0.0], dt), np.array([1.0, 0.0], dt), 2.0, 0.25, dt)
        assert (fl == 0).all() and (g == 0).all()
        fl, g = LO.focal(np.array([0.5], dt), np.array([np.nan], dt), 2.0, 0.25, dt)
        assert np.isnan(fl).all() and np.isnan(g).all()


# ------------------------------------------------------------------------------------------ options off
@pytest.mark.parametrize('dt', (np.float64, F32), ids=('f64', 'f32'))
def test_with_every_option_off_the_restatement_is_headopt_loss_ref(dt):
    for (C, K), iou, eps in (((33, 64), 1.0, 0.0), ((1, 65), 0.213, 0.1)):
        labels, cfg, layers = LO.plain_layers(C, K)
        for l, (out, pred) in enumerate(layers):
            a = HO.loss_ref(out, pred, l, labels, cfg, 0.7, iou, eps, dt)
            b = LO.loss_ref(out, pred, l, labels, cfg, 0.7, iou, eps, None, dt)
            for k in ('xy', 'wh', 'obj', 'cls', 'loss'):
                assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, l)
            for k in ('grad_output', 'target', 'obj_mask', 'tgt_mask', 'tgt_scale', 'mutated_output'):
                assert _same(a[k], b[k]), (k, l)
            t = LO.build_target(out, pred, l, labels, cfg, 0.7, iou, eps, None, dt)
            assert _same(t[0], a['target'])


# ------------------------------------------------------------------------------------------ what the inputs hold
def test_inputs_hold_what_they_are_named_for():
    """Positives on every layer of every set; ignored cells on every layer of the plain sets (where the focal objectness
    term has its negatives) and somewhere in every planted set (there the planted boxes of a crowded layer can turn
    every ignored cell into a positive one: (33, 100), layer 1).  K = 1 is the set in which layers have no record at all."""
    empty = [int(LO.reference(33, 1, 'plain', l)['tgt_mask'][..., 0].sum()) == 0 for l in range(3)]
    assert any(empty) and not all(empty)
    for C, K in HO.BOX_SETS:
        for source, iou in (('plain', 1.0), ('box', 0.213)):
            ignored = []
            for l in range(3):
                ref = LO.reference(C, K, source, l, None, iou, 0.0)
                assert ref['tgt_mask'][..., 0].sum() > 0, (C, K, source, l)
                ignored.append(int((ref['obj_mask'] == 0).sum()))
            print('C%d K%d %s: ignored cells per layer %s' % (C, K, source, ignored))
            assert all(ignored) if source == 'plain' else any(ignored), (C, K, source, ignored)
    labels, cfg, layers = LO.plain_layers(33, 64, True)
    n_one = [int((out[..., 4] == F32(1)).sum()) for out, _ in layers]
    print('saturated set (33, 64): cells with o == 1.0f in the objectness channel per layer', n_one)
    assert all(n > 0 for n in n_one)
    for kind in ('giou', 'diou', 'ciou'):
        x = np.concatenate([LO.reference(33, 64, 'box', l, dict(obj_iou_ratio=1.0, obj_iou_kind=kind), 0.213)['X']
                            for l in range(3)])
        assert (x < 0).any() and (x > 0.9).any(), kind
    x = np.concatenate([LO.reference(33, 64, 'box', l, dict(obj_iou_ratio=1.0, obj_iou_kind='iou'), 0.213)['X']
                        for l in range(3)])
    assert (x > 0.9).any() and (x == 0).any()


def test_iou_aware_targets_follow_the_formula():
    o = dict(obj_iou_ratio=0.5, obj_iou_kind='giou')
    ref = LO.reference(33, 64, 'box', 1, o, 0.213)
    assert np.array_equal(ref['t_obj'], 0.5 + 0.5 * np.maximum(ref['X'], 0))
    assert (ref['t_obj'] >= 0.5).all() and (ref['t_obj'] <= 1.0).all() and (ref['t_obj'] == 0.5).any()
    assert np.array_equal(ref['target'][tuple(ref['cells'].T) + (4,)], ref['t_obj'])
    base = LO.reference(33, 64, 'box', 1, None, 0.213)
    assert _same(ref['grad_output'][..., :4], base['grad_output'][..., :4])            # X is a constant
    assert ref['xy'] == base['xy'] and ref['wh'] == base['wh'] and ref['cls'] == base['cls'] and ref['obj'] != base['obj']


# ------------------------------------------------------------------------------------------ the fp32 yardstick
@pytest.mark.parametrize('opt', LO.FOCAL_SETS + (LO.ALL_ON,), ids=LO.opt_id)
def test_fp32_yardstick_meets_the_gradient_bar_with_a_factor_two_to_spare(opt):
    """On the unsaturated sets the restatement evaluated in float32 is within HC.close(atol=1e-5, rtol=1e-4, scale=False)
    of the float64 reference with both numbers halved: the bar of the GPU test is one plain fp32 arithmetic can meet."""
    worst = 0.0
    source, iou, eps = ('box', 0.213, 0.1) if opt is LO.ALL_ON else ('plain', 1.0, 0.0)
    for C, K in LO.SETS:
        for l in range(3):
            g64 = LO.reference(C, K, source, l, opt, iou, eps)['grad_output']
            g32 = LO.reference(C, K, source, l, opt, iou, eps, True)['grad_output']
            assert g32.dtype == F32
            worst = max(worst, LO.grad_ratio(g32, g64, 0.5e-5, 0.5e-4))
            print('C%d K%d layer %d: largest gradient %.3g, ratio to the halved bar so far %.3f'
                  % (C, K, l, float(np.abs(g64).max()), worst))
            HC.close(g32, g64, atol=0.5e-5, rtol=0.5e-4, scale=False)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------ validation
BAD = (dict(focal_gamma=0.3), dict(focal_gamma=5.5), dict(focal_gamma=-1.0), dict(focal_gamma=float('nan')),
       dict(focal_gamma=2.0, focal_alpha=1.0), dict(focal_gamma=2.0, focal_alpha=-0.1),
       dict(focal_gamma=2.0, focal_alpha=float('nan')), dict(focal_gamma=2.0, focal_terms='box'),
       dict(focal_gamma=2.0, focal_terms=None), dict(obj_iou_ratio=-0.1, box_loss='ciou'),
       dict(obj_iou_ratio=1.5, box_loss='ciou'), dict(obj_iou_ratio=float('nan'), box_loss='ciou'),
       dict(obj_iou_ratio=0.5), dict(obj_iou_ratio=0.5, box_loss='mse'),
       dict(obj_gain=0.0), dict(obj_gain=-1.0), dict(obj_gain=float('inf')), dict(obj_gain=float('nan')),
       dict(obj_gain=(1.0, 2.0)), dict(obj_gain=(1.0, 0.0, 1.0)), dict(cls_gain=0.0), dict(cls_gain=float('inf')),
       dict(cls_gain=float('nan')))


@pytest.mark.parametrize('bad', BAD, ids=LO.opt_id)
def test_invalid_options_raise_without_a_gpu(bad):
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    with pytest.raises(ValueError):
        YOLOLoss(recipe.MODEL_CFG, 0.7, **bad)


def test_valid_options_and_defaults():
    from yolov4_amd import ops
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    names = list(inspect.signature(YOLOLoss.__init__).parameters)
    assert names[names.index('label_smooth') + 1:] == ['focal_gamma', 'focal_alpha', 'focal_terms', 'obj_iou_ratio', 'obj_gain',
                                                      'cls_gain']
    c = YOLOLoss(recipe.MODEL_CFG, 0.7)
    assert (c.focal_gamma, c.focal_alpha, c.focal_terms, c.obj_iou_ratio, c.obj_gain, c.cls_gain) == \
        (0.0, 0.25, 'obj+cls', 0.0, [1.0, 1.0, 1.0], 1.0)
    YOLOLoss(recipe.MODEL_CFG, 0.7, focal_alpha=7.0, focal_terms='nonsense')       # not looked at with gamma = 0
    c = YOLOLoss(recipe.MODEL_CFG, 0.7, box_loss='giou', focal_gamma=0.5, focal_alpha=0.0, focal_terms='cls', obj_iou_ratio=1.0,
                 obj_gain=(4.0, 1.0, 0.4), cls_gain=2.5)
    cfgs = [c._layer_cfg(l) for l in range(3)]
    assert [x['obj_gain'] for x in cfgs] == [4.0, 1.0, 0.4]
    for x in cfgs:
        assert (x['focal_gamma'], x['focal_alpha'], x['focal_terms'], x['obj_iou_ratio'], x['cls_gain']) == \
            (0.5, 0.0, 'cls', 1.0, 2.5)
    o = ops.loss_opts_struct(cfgs[2])
    assert (o.focal_gamma, o.focal_alpha, o.focal_terms, o.obj_iou_ratio, o.obj_iou_kind) == (0.5, 0.0, 2, 1.0, BC.KIND_IDS['giou'])
    assert o.obj_gain == F32(0.4) and o.cls_gain == 2.5
    assert ops.check_loss_options(0.5, 0.1) == (0.5, 0.1)                          # its signature stays


def test_build_criterion_reads_the_cfg_keys():
    from yolov4_amd.yolo.model.build import build_criterion
    cfg = {'MODEL': copy.deepcopy(recipe.MODEL_CFG), 'CRITERION': {'IGNORE_THRESH': 0.7}}
    c = build_criterion(cfg)
    assert (c.focal_gamma, c.focal_alpha, c.focal_terms, c.obj_iou_ratio, c.obj_gain, c.cls_gain) == \
        (0.0, 0.25, 'obj+cls', 0.0, [1.0, 1.0, 1.0], 1.0)
    cfg['CRITERION'].update(BOX_LOSS='ciou', FOCAL_GAMMA=1.5, FOCAL_ALPHA=0.5, FOCAL_TERMS='obj', OBJ_IOU_RATIO=0.5,
                            OBJ_GAIN=[4.0, 1.0, 0.4], CLS_GAIN=0.5)
    c = build_criterion(cfg)
    assert (c.focal_gamma, c.focal_alpha, c.focal_terms, c.obj_iou_ratio, c.obj_gain, c.cls_gain) == \
        (1.5, 0.5, 'obj', 0.5, [4.0, 1.0, 0.4], 0.5)
    cfg['CRITERION']['OBJ_GAIN'] = 2
    assert build_criterion(cfg).obj_gain == [2.0, 2.0, 2.0]


# ------------------------------------------------------------------------------------------ the C ABI on the host
def _opts(**kw):
    from yolov4_amd._lib import LossOpts
    d = dict(iou_thresh=1.0, label_smooth=0.0, focal_gamma=0.0, focal_alpha=0.25, focal_terms=3, obj_iou_ratio=0.0,
             obj_iou_kind=4, obj_gain=1.0, cls_gain=1.0)
    d.update(kw)
    return LossOpts(*[d[k] for k, _ in LossOpts._fields_])


def test_workspace_query_of_the_opts_entries():
    import yolov4_amd
    L = yolov4_amd.lib()
    assert ctypes.sizeof(_opts()) == 36
    for B, F, A, K, C in ((3, 16, 3, 64, 33), (64, 76, 3, 60, 80), (1, 4, 3, 1, 1), (5, 8, 3, 7, 65)):
        for iou in (1.0, 0.213):
            ex = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, iou)
            assert ex > 0
            assert L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(_opts(iou_thresh=iou))) == ex
            assert L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(_opts(iou_thresh=iou, focal_gamma=2.0,
                                                                                    obj_gain=0.4, cls_gain=2.5))) == ex
            R = K * A if iou < 1 else K
            for r in (0.5, 1.0):
                got = L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(_opts(iou_thresh=iou, obj_iou_ratio=r)))
                assert got == ex + (4 * B * R + 15) // 16 * 16, (B, F, K, C, iou, r)
    assert L.y4_yolo_loss_workspace(3, 16, 3, 64, 33) == L.y4_yolo_loss_workspace_opts(3, 16, 3, 64, 33, ctypes.byref(_opts()))
    assert L.y4_yolo_loss_workspace_opts(3, 16, 3, 64, 33, None) == 0


BAD_ABI = (dict(iou_thresh=0.0), dict(label_smooth=1.0), dict(focal_gamma=0.3), dict(focal_gamma=5.5),
           dict(focal_gamma=float('nan')), dict(focal_gamma=2.0, focal_alpha=1.0), dict(focal_gamma=2.0, focal_alpha=-0.5),
           dict(focal_gamma=2.0, focal_alpha=float('nan')), dict(focal_gamma=2.0, focal_terms=0),
           dict(focal_gamma=2.0, focal_terms=4), dict(obj_iou_ratio=-0.5), dict(obj_iou_ratio=1.5),
           dict(obj_iou_ratio=float('nan')), dict(obj_iou_ratio=0.5, obj_iou_kind=0), dict(obj_iou_ratio=0.5, obj_iou_kind=5),
           dict(obj_gain=0.0), dict(obj_gain=float('inf')), dict(obj_gain=float('nan')), dict(cls_gain=-1.0),
           dict(cls_gain=float('inf')), dict(cls_gain=float('nan')))


@pytest.mark.parametrize('bad', BAD_ABI, ids=LO.opt_id)
def test_bad_opts_are_refused_before_any_launch(bad):
    """fake pointers, never dereferenced: the option check comes before anything is launched (as tests/test_abi.py)"""
    import yolov4_amd
    from yolov4_amd._lib import float_array, int_array
    L = yolov4_amd.lib()
    fake = 0x1000
    o = _opts(**bad)
    B, F, A, K, C = 3, 16, 3, 64, 33
    shape = L.y4_yolo_loss_fwd_ex_f32(fake, fake, fake, K, B, F, A, C, 8.0, 0.7, float_array([1.0] * 18), 9, int_array([0, 1, 2]),
                                      0.0, 0.0, fake, fake, fake, 1 << 30, None)     # what a bad iou_thresh returns
    assert shape != 0
    assert L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(o)) == 0
    assert L.y4_yolo_loss_fwd_opts_f32(fake, fake, fake, K, B, F, A, C, 8.0, 0.7, float_array([1.0] * 18), 9,
                                       int_array([0, 1, 2]), ctypes.byref(o), fake, fake, fake, 1 << 30, None) == shape
    assert L.y4_yolo_loss_bwd_opts_f32(fake, 0, fake, fake, fake, B, F, A, K, C, ctypes.byref(o), fake, 1 << 30, None) == shape
    assert L.y4_yolo_loss_dense_targets_opts_f32(fake, fake, fake, B, F, A, K, C, ctypes.byref(o), fake, 1 << 30, None) == shape


def test_null_opts_and_small_workspace_are_refused_before_any_launch():
    import yolov4_amd
    from yolov4_amd._lib import float_array, int_array
    L = yolov4_amd.lib()
    fake = 0x1000
    B, F, A, K, C = 3, 16, 3, 64, 33
    null = L.y4_yolo_loss_bwd_ex_f32(None, 0, fake, fake, fake, B, F, A, K, C, 1.0, 0.0, fake, 1 << 30, None)
    assert null != 0
    assert L.y4_yolo_loss_bwd_opts_f32(fake, 0, fake, fake, fake, B, F, A, K, C, None, fake, 1 << 30, None) == null
    assert L.y4_yolo_loss_dense_targets_opts_f32(fake, fake, fake, B, F, A, K, C, None, fake, 1 << 30, None) == null
    assert L.y4_yolo_loss_fwd_opts_f32(fake, fake, fake, K, B, F, A, C, 8.0, 0.7, float_array([1.0] * 18), 9, int_array([0, 1, 2]),
                                       None, fake, fake, fake, 1 << 30, None) == null
    # with obj_iou_ratio > 0 the workspace of the _ex query is too small by pos_obj
    o = _opts(obj_iou_ratio=0.5)
    ex = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, 1.0)
    small = L.y4_yolo_loss_bwd_ex_f32(fake, 0, fake, fake, fake, B, F, A, K, C, 1.0, 0.0, fake, 16, None)
    assert small not in (0, null)
    assert L.y4_yolo_loss_bwd_opts_f32(fake, 0, fake, fake, fake, B, F, A, K, C, ctypes.byref(o), fake, ex, None) == small
    assert L.y4_yolo_loss_dense_targets_opts_f32(fake, fake, fake, B, F, A, K, C, ctypes.byref(o), fake, ex, None) == small
