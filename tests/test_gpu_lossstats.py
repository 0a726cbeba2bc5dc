# -*- coding: utf-8 -*-
"""The per-layer training statistics of the loss (y4_yolo_loss_stats_f64 through YOLOLoss(stats=True)) against the
restatement of tests/lossstats_cases.py: counts exactly, the sums of `output` values within the derived bound of an fp64
summation order, sum_iou by the project's rule for X (BOX_FACTOR x the fp32 yardstick).  DESIGN.md section 24."""
import math

import numpy as np
import pytest
import torch

import boxloss_cases as BC
import lossopt_cases as LO
import lossstats_cases as LS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _up(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(dev)     # a copy: the shared inputs are read-only


def _outputs(layers, dev, grad=False):
    return [dict(layer_no=l, output=_up(o, dev).requires_grad_(grad), pred=_up(p, dev))
            for l, (o, p) in enumerate(layers)]


def _crit(cfg, dev, **kw):
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    return YOLOLoss(cfg, 0.7, device=dev, **kw)


def _rows(crit):
    torch.cuda.synchronize()
    return crit.stats.cpu().numpy()


def _check_row(got, row, extras, tag):
    """counts and the exact sums of one row; sum_iou is the caller's"""
    for q in LS.COUNTS:
        assert got[q] == row[q], (tag, LS.ROWS[q], got[q], row[q])
    for q in LS.EXACT_SUMS:
        bound = LS.sum_bound(extras, q)
        err = abs(got[q] - row[q])
        print('%s %s: %.17g ref %.17g error %.3g (derived bound %.3g, %d terms)' % (tag, LS.ROWS[q], got[q], row[q], err,
                                                                                    bound, extras['n'][q]))
        assert err <= bound, (tag, LS.ROWS[q])


@pytest.mark.parametrize('mutate', (True, False), ids=('mutate', 'keep'))
@pytest.mark.parametrize('iou_thresh', LS.IOU_THRESH)
@pytest.mark.parametrize('source', LS.SOURCES)
@pytest.mark.parametrize('CK', LO.SETS, ids=lambda ck: 'C%d-K%d' % ck)
def test_rows_against_the_restatement(dev, CK, source, iou_thresh, mutate):
    C, K = CK
    labels, cfg, layers = LS.layers_of(C, K, source)
    crit = _crit(cfg, dev, iou_thresh=iou_thresh, mutate_outputs=mutate, stats=True)
    crit(_outputs(layers, dev), {'padded_labels': torch.from_numpy(np.array(labels))})
    got = _rows(crit)
    e32 = LS.sum_iou_fp32_error()
    worst = 0.0
    for l in range(3):
        row, extras = LS.set_reference(C, K, source, l, iou_thresh)
        tag = 'C%d K%d %s layer %d iou_thresh %g' % (C, K, source, l, iou_thresh)
        _check_row(got[l], row, extras, tag)
        err = abs(got[l][LS.SUM_IOU] - row[LS.SUM_IOU])
        worst = max(worst, err / e32)
        print('%s sum_iou: %.17g ref64 %.17g error %.3g, fp32 yardstick %.3g, %d records' % (
            tag, got[l][LS.SUM_IOU], row[LS.SUM_IOU], err, e32, int(row[1])))
    print('C%d K%d %s iou_thresh %g: kernel sum_iou error / fp32-restatement error %.3f (allowed %.1f)' % (
        C, K, source, iou_thresh, worst, BC.BOX_FACTOR))
    assert worst <= BC.BOX_FACTOR
    for l, m in enumerate(crit.stats_summary()):
        ref = LS.summary_ref(LS.set_reference(C, K, source, l, iou_thresh)[0])
        assert set(m) == set(ref)
        for k in ('count', 'ignored', 'r50', 'r75', 'top1'):    # ratios of equal integers; nan where there is no positive
            assert m[k] == ref[k] or (math.isnan(m[k]) and math.isnan(ref[k])), (l, k, m[k], ref[k])


@pytest.mark.parametrize('name', sorted(LS.EDGES))
def test_edge_shapes(dev, name):
    """B = 1 and F = 1; C = 1; an image / a batch without labels; one block and two cells (A = 3: 257 cannot be had).  The
    bound of sum_iou here is n_pos x BOX_FACTOR x the yardstick's largest per-record X error: each term by the rule for
    X, added up."""
    e = LS.edge_case(name)
    l = e['l']
    crit = _crit(e['cfg'], dev, stats=True)
    crit([dict(layer_no=l, output=_up(e['output'], dev), pred=_up(e['pred'], dev))],
         {'padded_labels': torch.from_numpy(np.array(e['labels']))})
    got = _rows(crit)
    _check_row(got[l], e['row'], e['extras'], name)
    bound = e['row'][1] * BC.BOX_FACTOR * LS.x_fp32_error()
    err = abs(got[l][LS.SUM_IOU] - e['row'][LS.SUM_IOU])
    print('%s sum_iou: %.17g ref64 %.17g error %.3g (bound %.3g)' % (name, got[l][LS.SUM_IOU], e['row'][LS.SUM_IOU], err, bound))
    assert err <= bound
    for other in range(3):
        if other != l:
            assert not got[other].any()
    m = crit.stats_summary()[l]
    if e['row'][1] == 0:
        assert m['count'] == 0 and got[l][3] == 0 and got[l][6] == 0 and got[l][9] == 0
        for k in ('avg_iou', 'r50', 'r75', 'obj', 'cls', 'top1'):
            assert math.isnan(m[k])
        assert not math.isnan(m['no_obj'])


def test_nan_in_a_positive_cells_pred(dev):
    """sum_iou of that layer is NaN; its counts are the clean run's, less the planted record in n_iou50 / n_iou75 where it
    counted; the rows of the other layers have the clean run's bits."""
    C, K, it = 33, 64, 0.213
    labels, cfg, layers = LS.layers_of(C, K, 'box')
    lab = {'padded_labels': torch.from_numpy(np.array(labels))}
    clean = _crit(cfg, dev, iou_thresh=it, stats=True)
    clean(_outputs(layers, dev), lab)
    clean = _rows(clean)
    row, extras = LS.set_reference(C, K, 'box', 1, it)
    q = int(np.argmax(extras['X']))                            # a record that counts in n_iou50
    assert extras['X'][q] > 0.5 + LS.MARGIN
    b, a, j, i = extras['cells'][q]
    for comp in (0, 3):
        pred = np.array(layers[1][1])
        pred[b, a, j, i, comp] = np.nan
        planted = [layers[0], (layers[1][0], pred), layers[2]]
        crit = _crit(cfg, dev, iou_thresh=it, stats=True)
        crit(_outputs(planted, dev), lab)
        got = _rows(crit)
        assert math.isnan(got[1][LS.SUM_IOU])
        for k in (0, 1, 2, 8, 10, 11):
            assert got[1][k] == clean[1][k], LS.ROWS[k]
        assert got[1][4] == clean[1][4] - 1
        assert got[1][5] == clean[1][5] - (1 if extras['X'][q] > 0.75 else 0)
        for k in LS.EXACT_SUMS:
            assert got[1][k] == clean[1][k]
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
        assert math.isnan(crit.stats_summary()[1]['avg_iou'])


def test_calls_accumulate_and_reset_zeroes(dev):
    C, K = 33, 64
    labels, cfg, plain = LS.layers_of(C, K, 'plain')
    _, _, box = LS.layers_of(C, K, 'box')
    lab = {'padded_labels': torch.from_numpy(np.array(labels))}
    single = []
    for layers in (plain, box):
        crit = _crit(cfg, dev, stats=True)
        crit(_outputs(layers, dev), lab)
        single.append(_rows(crit))
    crit = _crit(cfg, dev, stats=True)
    crit(_outputs(plain, dev), lab)
    first = crit.stats
    crit(_outputs(box, dev), lab)
    assert crit.stats is first                                 # the same device tensor, added to
    assert np.array_equal(_rows(crit), single[0] + single[1])
    # build_target never accumulates
    crit.build_target(_up(plain[1][0], dev), _up(plain[1][1], dev), 1, lab['padded_labels'])
    assert np.array_equal(_rows(crit), single[0] + single[1])
    crit.reset_stats()
    assert not _rows(crit).any()
    crit(_outputs(plain, dev), lab)
    assert np.array_equal(_rows(crit), single[0])


@pytest.mark.parametrize('mutate', (True, False), ids=('mutate', 'keep'))
def test_stats_change_nothing_else(dev, mutate):
    """loss, outputs[*]['output'] after the call and the gradient are torch.equal with stats on and off"""
    C, K = 33, 64
    labels, cfg, layers = LS.layers_of(C, K, 'box')
    lab = {'padded_labels': torch.from_numpy(np.array(labels))}
    res = []
    for stats in (False, True):
        crit = _crit(cfg, dev, iou_thresh=0.213, mutate_outputs=mutate, box_loss='ciou', stats=stats)
        outs = _outputs(layers, dev, grad=True)
        loss = crit(outs, lab)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach(), [o['output'].detach() for o in outs], [o['output'].grad for o in outs]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
        assert torch.equal(a, b)


def test_off_means_no_call(dev, monkeypatch):
    import yolov4_amd
    C, K = 33, 64
    labels, cfg, layers = LS.layers_of(C, K, 'plain')

    def boom(*a, **k):
        raise AssertionError('y4_yolo_loss_stats_f64 called with stats off')
    monkeypatch.setattr(yolov4_amd.lib(), 'y4_yolo_loss_stats_f64', boom)
    crit = _crit(cfg, dev)
    loss = crit(_outputs(layers, dev), {'padded_labels': torch.from_numpy(np.array(labels))})
    assert crit.stats is None and math.isfinite(float(loss))
    assert crit.stats_summary() == []
    on = _crit(cfg, dev, stats=True)
    with pytest.raises(AssertionError):
        on(_outputs(layers, dev), {'padded_labels': torch.from_numpy(np.array(labels))})
