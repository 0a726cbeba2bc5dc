# -*- coding: utf-8 -*-
"""CPU checks of tests/boxloss_cases.py -- the float64 restatement of the IoU-family box losses and the inputs that
tests/test_gpu_boxloss.py feeds to the kernels -- and of the host side of the feature (constructor and cfg keys)."""
import copy
import math

import numpy as np
import pytest
import torch

import boxloss_cases as BC
import recipe
from oracle import head as H
from yolov4_amd.yolo.model.build import build_criterion
from yolov4_amd.yolo.model.yololoss import YOLOLoss


def _torch_loss(p, t, kind):
    """the issue's formulas in torch, alpha detached: what autograd differentiates"""
    eps = BC.EPS
    px, py, pw, ph = p.unbind(1)
    tx, ty, tw, th = t.unbind(1)
    pl, pr, pt, pb = px - pw / 2, px + pw / 2, py - ph / 2, py + ph / 2
    tl, tr, tt, tb = tx - tw / 2, tx + tw / 2, ty - th / 2, ty + th / 2
    iw = (torch.minimum(pr, tr) - torch.maximum(pl, tl)).clamp(min=0)
    ih = (torch.minimum(pb, tb) - torch.maximum(pt, tt)).clamp(min=0)
    inter = iw * ih
    union = pw * ph + tw * th - inter + eps
    iou = inter / union
    cw = torch.maximum(pr, tr) - torch.minimum(pl, tl)
    ch = torch.maximum(pb, tb) - torch.minimum(pt, tt)
    if kind == 'iou':
        x = iou
    elif kind == 'giou':
        x = iou - (cw * ch + eps - union) / (cw * ch + eps)
    else:
        x = iou - ((px - tx) ** 2 + (py - ty) ** 2) / (cw ** 2 + ch ** 2 + eps)
        if kind == 'ciou':
            v = 4 / math.pi ** 2 * (torch.atan(tw / (th + eps)) - torch.atan(pw / (ph + eps))) ** 2
            alpha = (v / (1 - iou + v + eps)).detach()
            x = x - alpha * v
    return 1 - x


def _random_pairs(n, seed):
    rng = np.random.RandomState(seed)
    t = np.stack([rng.uniform(0.2, 15.8, n), rng.uniform(0.2, 15.8, n), np.exp(rng.uniform(np.log(0.3), np.log(20), n)),
                  np.exp(rng.uniform(np.log(0.3), np.log(20), n))], 1)
    p = t.copy()
    p[:, :2] += rng.uniform(-1.0, 1.0, (n, 2)) * t[:, 2:] * 0.6
    p[:, 2:] *= np.exp(rng.normal(0, 0.8, (n, 2)))
    p[: n // 16, 2:] *= 0.05                                 # small boxes off centre: many disjoint pairs
    p[n // 16: n // 8, :2] += 30.0                           # far away
    return p, t


@pytest.mark.parametrize('kind', BC.KINDS)
def test_closed_form_gradient_is_autograd(kind):
    """box_eval's gradient against torch float64 autograd of the same expression (alpha detached) over 4096 random
    pairs, overlapping, nested and disjoint: 1e-10 of the record's largest component."""
    p, t = _random_pairs(4096, 5)
    loss, grad = BC.box_eval(p, t, kind)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    tl = _torch_loss(tp, torch.tensor(t, dtype=torch.float64), kind)
    tl.sum().backward()
    g = tp.grad.numpy().copy()
    g[:, 2] *= p[:, 2]
    g[:, 3] *= p[:, 3]
    np.testing.assert_allclose(loss, tl.detach().numpy(), rtol=1e-12, atol=1e-12)
    iou = BC.box_quantities(p, t)[0]
    assert (iou == 0).sum() >= 100 and (iou > 0.5).sum() >= 100
    assert BC.row_rel_err(grad, g).max() <= 1e-10, float(BC.row_rel_err(grad, g).max())
    scale = np.maximum(np.abs(g).max(axis=1), 1e-300)
    assert (np.abs(grad - g).max(axis=1) <= 1e-10 * scale + 1e-300).all()


def test_values_lie_in_range():
    p, t = _random_pairs(4096, 6)
    for case in (BC.make_case(1, 64), BC.make_case(33, 65)):
        for l, lay in enumerate(case['layers']):
            r = BC.layer_box_loss(lay['output'], lay['pred'], case['labels'], case['cfg'], 'iou', 1.0, l)
            p, t = np.concatenate([p, r['p']]), np.concatenate([t, r['t']])
    iou, giou, diou, ciou = BC.box_quantities(p, t)
    assert (iou >= 0).all() and (iou <= 1).all()
    for x in (giou, diou):
        assert (1 - x >= 0).all() and (1 - x <= 2).all()
    assert (1 - ciou >= 1 - diou).all()


@pytest.mark.parametrize('C', BC.BOX_C)
@pytest.mark.parametrize('K', BC.BOX_K)
def test_planted_classes_are_present(C, K):
    """Every geometric class is planted in the K >= 64 cases (K = 1 has one positive), and is what its name says."""
    case = BC.make_case(C, K)
    n = BC.plant_counts(case)
    if K == 1:
        assert sum(n.values()) == 1
        return
    assert all(v > 0 for v in n.values()), n
    seen = {k: 0 for k in BC.PLANTS}
    for l, lay in enumerate(case['layers']):
        r = BC.layer_box_loss(lay['output'], lay['pred'], case['labels'], case['cfg'], 'iou', 1.0, l)
        iou = 1.0 - r['per_record']
        for q, name in enumerate(lay['plants']):
            (px, py, pw, ph), (tx, ty, tw, th) = r['p'][q], r['t'][q]
            if tw == 0 or th == 0:
                continue                                     # the zero label row of image 1: every class degenerates
            ok = {'equal': iou[q] > 1 - 1e-5 and r['ties'][q],
                  'disjoint': iou[q] == 0 and px - pw / 2 > tx + tw / 2,
                  'pred_in_truth': abs(iou[q] - pw * ph / (tw * th)) < 1e-5,
                  'truth_in_pred': abs(iou[q] - tw * th / (pw * ph)) < 1e-5,
                  'aspect_1_40': abs(ph / pw - 40) < 1e-3,
                  'aspect_40_1': abs(pw / ph - 40) < 1e-3,
                  'touching': iou[q] < 1e-6 and abs((px - pw / 2) - (tx + tw / 2)) <= 2.0 ** -22 * (tx + tw),
                  'thin': pw == np.float32(1e-3),
                  'generic': True}[name]
            assert ok, (l, q, name, r['p'][q], r['t'][q], iou[q])
            seen[name] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_two_labels_on_one_cell_take_the_last():
    """Image 1 of head_cases.make_labels puts label pairs (rows 0/1, 2/3, 4/5) on one cell and anchor, one pair per
    layer: the record's truth is the second label of the pair."""
    case = BC.make_case(33, 64)
    lab = np.asarray(case['labels'], np.float32)
    found = 0
    for l, lay in enumerate(case['layers']):
        cells, truth, idx = BC.positives(lay['output'], lay['pred'], case['labels'], case['cfg'], l)
        first, second = 2 * l, 2 * l + 1
        st = np.float32(H.STRIDES[l])
        ci, cj = int(lab[1, first, 0] / st), int(lab[1, first, 1] / st)
        assert (ci, cj) == (int(lab[1, second, 0] / st), int(lab[1, second, 1] / st))
        rows = [q for q, (b, a, j, i) in enumerate(cells) if b == 1 and (j, i) == (cj, ci)]
        assert len(rows) == 1, (l, rows)
        q = rows[0]
        assert idx[q] == second
        assert np.array_equal(truth[q], lab[1, second, :4] / st) and not np.array_equal(truth[q], lab[1, first, :4] / st)
        found += 1
    assert found == 3


def test_fp32_yardstick_is_nonzero_and_small():
    """The plain-fp32 evaluation's own error, from which the kernels' bounds are made: not 0, and of fp32 size."""
    for kind in BC.KINDS:
        for gain in BC.GAINS:
            e_loss, e_grad = BC.fp32_errors(kind, gain)
            print('%s gain %g: fp32 restatement error: loss %.3g (%.1f x 2^-24), gradient row-relative %.3g (%.1f x 2^-24)'
                  % (kind, gain, e_loss, e_loss / 2.0 ** -24, e_grad, e_grad / 2.0 ** -24))
            assert 0 < e_loss < 1e-4 and 0 < e_grad < 1e-2


def test_unknown_box_loss_raises_without_gpu():
    with pytest.raises(ValueError):
        YOLOLoss(recipe.MODEL_CFG, 0.7, box_loss='eiou')
    for name in ('mse',) + BC.KINDS:
        c = YOLOLoss(recipe.MODEL_CFG, 0.7, box_loss=name, box_gain=0.05)
        assert c.box_loss == name and c.box_gain == 0.05
    c = YOLOLoss(recipe.MODEL_CFG, 0.7)
    assert c.box_loss == 'mse' and c.box_gain == 1.0
    assert c._layer_cfg(0)['box_loss'] == 'mse'


def test_build_criterion_passes_the_cfg_keys():
    cfg = copy.deepcopy(recipe.FULL_CFG)
    c = build_criterion(cfg, device=torch.device('cpu'))
    assert c.box_loss == 'mse' and c.box_gain == 1.0
    cfg['CRITERION']['BOX_LOSS'] = 'ciou'
    cfg['CRITERION']['BOX_LOSS_GAIN'] = 0.07
    c = build_criterion(cfg, device=torch.device('cpu'))
    assert c.box_loss == 'ciou' and c.box_gain == 0.07
    lc = c._layer_cfg(2)
    assert lc['box_loss'] == 'ciou' and lc['box_gain'] == 0.07
    cfg['CRITERION']['BOX_LOSS'] = 'focal'
    with pytest.raises(ValueError):
        build_criterion(cfg, device=torch.device('cpu'))


def test_new_entry_points_report_errors_before_any_launch():
    import yolov4_amd
    L = yolov4_amd.lib()
    fake = 0x1000
    need = L.y4_yolo_loss_workspace(2, 4, 3, 8, 5)
    assert need >= 2 * 8 * 4 * 4
    assert L.y4_yolo_box_loss_fwd_f32(None, 4, 1.0, 2, 4, 3, 8, 5, fake, fake, need, None) == 2
    assert L.y4_yolo_box_loss_fwd_f32(fake, 4, 1.0, 2, 4, 3, 8, 5, None, fake, need, None) == 2
    assert L.y4_yolo_box_loss_fwd_f32(fake, 4, 1.0, 2, 4, 3, 8, 5, fake, None, need, None) == 2
    assert L.y4_yolo_box_loss_fwd_f32(fake, 4, 1.0, 2, 4, 3, 8, 5, fake, fake, need - 1, None) == 4
    for kind in (0, 5, -1):
        assert L.y4_yolo_box_loss_fwd_f32(fake, kind, 1.0, 2, 4, 3, 8, 5, fake, fake, need, None) == 1
        assert L.y4_yolo_box_loss_bwd_f32(fake, kind, 1.0, fake, fake, 2, 4, 3, 8, 5, fake, need, None) == 1
    assert L.y4_yolo_box_loss_bwd_f32(None, 4, 1.0, fake, fake, 2, 4, 3, 8, 5, fake, need, None) == 2
    assert L.y4_yolo_box_loss_bwd_f32(fake, 4, 1.0, None, fake, 2, 4, 3, 8, 5, fake, need, None) == 2
    assert L.y4_yolo_box_loss_bwd_f32(fake, 4, 1.0, fake, None, 2, 4, 3, 8, 5, fake, need, None) == 2
    assert L.y4_yolo_box_loss_bwd_f32(fake, 4, 1.0, fake, fake, 2, 4, 3, 8, 5, None, need, None) == 2
    assert L.y4_yolo_box_loss_bwd_f32(fake, 4, 1.0, fake, fake, 2, 4, 3, 8, 5, fake, need - 1, None) == 4
    assert L.y4_yolo_box_loss_fwd_f32(fake, 4, 1.0, 0, 4, 3, 8, 5, fake, fake, need, None) == 1
