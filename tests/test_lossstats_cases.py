# -*- coding: utf-8 -*-
"""The restatement of the loss's training statistics (tests/lossstats_cases.py) and the inputs of the GPU tests, checked
without a GPU: a layer worked out by hand, two labels sharing a cell, and the conditions that keep a comparison of the
kernel against the restatement from hiding a flip (no X near 0.5 / 0.75, no tie at a class maximum)."""
import math

import numpy as np
import pytest

import head_cases as HC
import lossopt_cases as LO
import lossstats_cases as LS

F32 = np.float32


def _hand_layer(labels):
    """F = 2, A = 3, C = 3 on layer 2 (stride 32, a 64-px image).  The label (40, 20, 142, 110) has exactly the shape of
    anchor 6, slot 0 of the layer, and falls into cell i = 1, j = 0: grid box (1.25, 0.625, 4.4375, 3.4375)."""
    cfg = HC.cfg_with_classes(3)
    output = np.zeros((1, 3, 2, 2, 8), F32)
    pred = np.zeros((1, 3, 2, 2, 4), F32)
    pred[...] = (0.1, 0.1, 0.01, 0.01)                         # far from every truth box: background, not ignored
    output[..., 4] = 0.25
    output[..., 5:] = 0.5
    pred[0, 0, 0, 1] = (1.25, 0.625, 0.8 * 4.4375, 3.4375)     # the positive cell: the truth box at 0.8 of its width
    output[0, 0, 0, 1, 4] = 0.9
    output[0, 0, 0, 1, 5:] = (0.2, 0.7, 0.1)
    pred[0, 1, 1, 0] = (1.25, 0.625, 4.4375, 3.4375)           # the truth box itself elsewhere: IoU 1 > 0.7, ignored
    output[0, 1, 1, 0, 4] = 0.6
    lab = np.zeros((1, len(labels), 5))
    lab[0] = labels
    with np.errstate(invalid='ignore'):                         # the box is larger than the 2 x 2 map: tgt_scale is NaN, unused here
        ref = LO.loss_ref(output, pred, 2, lab, cfg, 0.7, 1.0, 0.0)
    return LS.stats_ref(output, pred, ref)


def test_a_layer_worked_out_by_hand():
    row, extras = _hand_layer([(40, 20, 142, 110, 1)])
    s = dict(zip(LS.ROWS, row))
    assert s['n_cells'] == 12 and s['n_pos'] == 1 and s['n_ign'] == 1 and s['n_bg'] == 10
    assert abs(s['sum_iou'] - 0.8) < 1e-6                      # same box at 0.8 of the width; 1e-7 in the union, fp32 0.8 w
    assert s['n_iou50'] == 1 and s['n_iou75'] == 1
    assert s['sum_obj_pos'] == float(F32(0.9)) and s['sum_obj_bg'] == 2.5
    assert s['sum_cls'] == float(F32(0.7)) and s['n_cls'] == 1 and s['n_top1'] == 1
    m = LS.summary_ref(row)
    assert m['count'] == 1 and m['ignored'] == 1 and m['no_obj'] == 0.25 and m['r50'] == 1.0 and m['top1'] == 1.0


def test_two_labels_in_one_cell_are_one_record_with_two_class_bits():
    row, extras = _hand_layer([(40, 20, 142, 110, 1), (41, 21, 142, 110, 2)])
    s = dict(zip(LS.ROWS, row))
    assert s['n_pos'] == 1 and s['n_cls'] == 2 and s['n_top1'] == 1
    assert s['sum_cls'] == float(F32(0.7)) + float(F32(0.1))
    # the box is the last writer's: centre (41, 21) / 32 against a pred centred on the first label's
    assert s['sum_iou'] < 0.8 - 1e-3 and s['n_iou50'] == 1


def test_top1_takes_the_lowest_index_on_a_tie_and_misses_an_unset_bit():
    row, _ = _hand_layer([(40, 20, 142, 110, 0)])              # arg-max is class 1, the bit is class 0
    assert dict(zip(LS.ROWS, row))['n_top1'] == 0


def test_zero_denominators_give_nan():
    m = LS.summary_ref(np.zeros(12))
    assert m['count'] == 0 and m['ignored'] == 0
    for k in ('avg_iou', 'r50', 'r75', 'obj', 'no_obj', 'cls', 'top1'):
        assert math.isnan(m[k])


def test_the_gpu_inputs_cannot_hide_a_flip():
    """No positive's float64 X within MARGIN of 0.5 or 0.75, no positive cell with two class channels equal at its
    maximum; the inputs cover what the GPU test is about."""
    seen_pos = seen_none = seen_two_words = seen_ign = 0
    for tag, row, extras in LS.gpu_inputs():
        s = dict(zip(LS.ROWS, row))
        assert LS.flip_margin(extras['X']) > LS.MARGIN, tag
        assert LS.max_ties(extras['cls']) == 0, tag
        assert s['n_pos'] + s['n_bg'] + s['n_ign'] == s['n_cells'], tag      # a positive cell is never masked out
        seen_pos += s['n_pos'] > 0
        seen_none += s['n_pos'] == 0
        seen_ign += s['n_ign'] > 0
        seen_two_words += extras['bits'].shape[1] > 32 and bool(extras['bits'][:, 32:].any())
    assert seen_pos and seen_none and seen_ign and seen_two_words


def test_the_edge_shapes_are_what_they_are_named():
    e = LS.edge_case('cells-258')
    assert e['output'].shape[:4] == (86, 3, 1, 1) and e['row'][0] == 258 and e['row'][1] > 0
    assert LS.edge_case('no-labels')['row'][1] == 0 and np.all(LS.edge_case('no-labels')['row'][[3, 6, 9]] == 0)
    assert LS.edge_case('one-empty-image')['row'][1] > 0
    assert LS.edge_case('B1-F1')['output'].shape[:4] == (1, 3, 1, 1) and LS.edge_case('B1-F1')['row'][1] > 0
    assert LS.edge_case('C1')['output'].shape[-1] == 6 and LS.edge_case('C1')['row'][1] > 0


def test_the_yardsticks_are_not_degenerate():
    assert 0 < LS.x_fp32_error() < 1e-5 and 0 < LS.sum_iou_fp32_error() < 1e-3
    mixed = [LS.set_reference(33, 64, 'box', l, 0.213)[0] for l in range(3)]
    assert any(0 < r[4] < r[1] for r in mixed)                 # some X above 0.5 and some below: the counts can go wrong


@pytest.mark.parametrize('iou_thresh', LS.IOU_THRESH)
def test_more_positive_anchors_give_more_records(iou_thresh):
    a = LS.set_reference(33, 64, 'plain', 1, 1.0)[0]
    b = LS.set_reference(33, 64, 'plain', 1, iou_thresh)[0]
    assert b[1] >= a[1] and b[0] == a[0]
