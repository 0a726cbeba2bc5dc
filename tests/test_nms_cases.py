# -*- coding: utf-8 -*-
"""The restatement of postprocess_nms (tests/nms_cases.py) against the oracle, and the inputs of tests/test_gpu_nms_ext.py
against the properties they are named for.  No GPU."""
import numpy as np
import pytest

import head_cases as HC
import nms_cases as NC

F32 = np.float32


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize('kind', HC.POST_KINDS)
def test_default_options_equal_the_oracle(kind):
    p, C, conf, thre, props = HC.make_post_case(kind)
    q = p.copy()
    got, _ = NC.postprocess_nms_ref(q, C, conf, thre)
    _same(got, props['ref'])
    assert np.array_equal(q[:, :, :4].view(np.int32), props['xyxy'].view(np.int32))


def test_diou_case_changes_the_survivors_and_has_a_zero_diagonal_pair():
    p, C, conf, thre = NC.make_diou_case()
    q = p.copy()
    iou, _ = NC.postprocess_nms_ref(q, C, conf, thre, metric='iou')
    diou, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, metric='diou')
    m = NC.measure(q[0, 1, :4], q[0, 0, :4], 'diou', parts=True)
    assert m['iou'] >= F32(thre) > m['diou']
    assert len(diou[0]) == len(iou[0]) + 1                  # box 1 survives under DIoU only
    z = NC.measure(q[0, 3, :4], q[0, 2, :4], 'diou', parts=True)
    assert z['c2'] == 0 and np.isnan(z['diou'])             # 0 / 0 in the IoU, penalty 0: the pair is kept
    assert (diou[0][:, 0] == 300).sum() == 2
    # a nested pair: lower DIoU than IoU but still suppressed by neither (IoU 0.64 >= 0.45 drops it under both)
    assert (diou[0][:, 0] == 410).sum() == 0 and (iou[0][:, 0] == 410).sum() == 0


def test_soft_case_has_decayed_rows_late_prunes_and_key_ties():
    p, C, conf, thre = NC.make_soft_case()
    got, info = NC.postprocess_nms_ref(p.copy(), C, conf, thre, soft='linear')
    assert sorted(info['segments']) == [(0, 0), (0, 1)]
    for seg in info['segments'].values():
        assert seg['kept_decayed'] >= 1 and seg['pruned_after_decay'] >= 1 and seg['key_ties'] >= 1
        assert seg['emitted'] == 4 and seg['n'] == 5
    rows = got[0][got[0][:, 6] == 0]
    assert np.array_equal(rows[:, 4] * rows[:, 5], np.array([0.9, 0.5, 0.5, 0.8 * 0.5], F32))
    assert rows[1, 0] < rows[2, 0]                          # the tie: the lower box index first
    hard, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre)
    assert len(hard[0]) == 6                                # hard NMS drops what Soft-NMS keeps at a lower score


def test_agnostic_case_suppresses_across_classes():
    p, C, conf, thre = NC.make_agnostic_case()
    per, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre)
    agn, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, agnostic=True)
    assert len(per[0]) == 4 and len(agn[0]) == 2
    assert np.array_equal(agn[0][:, 6], np.array([0, 1], F32))          # selection order: 0.8 (class 0), 0.7 (class 1)
    assert np.array_equal(agn[0][:, 5], np.array([0.8, 0.7], F32))      # of box 0's two classes only the higher one


def test_maxdet_case_cuts_inside_a_segment_and_on_a_tie():
    p, C, conf, thre = NC.make_maxdet_case()
    full, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre)
    assert len(full[0]) == 8
    for md in (8, 9):
        got, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, max_det=md)
        assert np.array_equal(got[0], full[0])
    got, info = NC.postprocess_nms_ref(p.copy(), C, conf, thre, max_det=5)
    assert info['cap_gap'] == 0                             # the cut falls on a score tie
    assert np.array_equal(got[0][:, 6], np.array([0, 0, 0, 1, 2], F32))
    assert np.array_equal(got[0][:, 5], np.array([0.9, 0.8, 0.5, 0.85, 0.6], F32))
    one, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, max_det=1)
    assert len(one[0]) == 1 and one[0][0, 5] == F32(0.9)


@pytest.mark.parametrize('R', NC.SEG_SIZES)
def test_sized_cases_have_their_segment_sizes(R):
    p, C, conf, _ = NC.make_seg_case(R, 'class')
    assert int(((p[0, :, 5] * p[0, :, 4]) >= F32(conf)).sum()) == R
    p, C, conf, _ = NC.make_seg_case(R, 'image')
    assert int(((p[0, :, 5:] * p[0, :, 4:5]) >= F32(conf)).sum()) == R


@pytest.mark.parametrize('R', NC.SEG_SIZES + (NC.GAUSS_BIG,))
def test_gaussian_sized_cases_keep_the_margin(R):
    p, C, conf, thre, _ = NC.make_gauss_case(R)
    assert int(((p[0, :, 5] * p[0, :, 4]) >= F32(conf)).sum()) == R
    assert NC.gauss_margin_ok(p, C, conf, thre)
    _, info = NC.postprocess_nms_ref(p.copy(), C, conf, thre, soft='gaussian', sigma=NC.GAUSS_SIGMA, f64=True)
    seg = info['segments'][(0, 0)]
    assert seg['n'] == R and seg['key_ties'] == 0
    if R >= 255:
        assert seg['kept_decayed'] >= 1 and seg['pruned_after_decay'] >= R // 2


@pytest.mark.parametrize('kind', ('n63', 'n64', 'n65'))
def test_gaussian_tile_cases_keep_the_margin(kind):
    p, C, conf, thre, _ = NC.make_gauss_tile_case(kind)
    assert p.shape[0] == 3 and C == 4 and p.shape[1] == int(kind[1:])
    assert NC.gauss_margin_ok(p, C, conf, thre)
    assert NC.gauss_margin_ok(*NC.make_gauss_tile_case(kind, max_det=10)[:4], max_det=10)
    assert NC.gauss_margin_ok(*NC.make_gauss_tile_case(kind, agnostic=True)[:4], agnostic=True)


def test_wide_and_overflow_cases_reach_their_paths():
    p, C, conf, _ = NC.make_wide_case('wide')
    assert 5 + C > 255 and int(((p[..., 5:] * p[..., 4:5]) >= F32(conf)).sum()) > 1000
    p, C, conf, _ = NC.make_wide_case('overflow')
    B, N = p.shape[:2]
    assert int(((p[..., 5:] * p[..., 4:5]) >= F32(conf)).sum()) > max(B * N // 2, 1 << 16)


def test_float64_mode_agrees_with_float32_on_linear_decay():
    """the two modes of the restatement describe the same procedure"""
    p, C, conf, thre = NC.make_soft_case()
    a, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, soft='linear')
    b, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, soft='linear', f64=True)
    assert np.array_equal(a[0][:, [0, 1, 2, 3, 4, 6]], b[0][:, [0, 1, 2, 3, 4, 6]].astype(F32))
    assert np.allclose(a[0][:, 5], b[0][:, 5], rtol=1e-6, atol=0)
