# -*- coding: utf-8 -*-
"""The references and inputs of tests/test_gpu_head_edges.py, checked with the oracle alone (no GPU): the fp64 decode
agrees with oracle.head, and every input builder really has the property its case exists for -- so a GPU test cannot
pass by missing the kernel path it names.  These are conditions on seeds and sizes, not measurements."""
import numpy as np
import pytest

import head_cases as HC
import recipe
from oracle import head as H

CFG = recipe.MODEL_CFG


@pytest.mark.parametrize('l', [0, 1, 2])
def test_decode_ref64_agrees_with_oracle(l):
    B, F, A, C = 2, 5, 3, 80
    nt = A * (5 + C)
    rng = np.random.RandomState(40 + l)
    lg = (rng.standard_normal((B, nt, F, F)) * 2.0).astype(np.float32)           # NCHW, as the oracle takes it
    rows = np.ascontiguousarray(lg.transpose(0, 2, 3, 1)).reshape(B * F * F, nt)
    anc = H.masked_anchors(CFG, l)
    out, pred = HC.decode_ref64(rows, nt, B, F, A, C, anc, H.STRIDES[l], True)
    o_ref, p_ref = H.yolo_decode(lg, l, CFG, True)
    HC.close(o_ref, out, 1e-6, 1e-6, scale=False)
    HC.close(p_ref, pred, 1e-5, 1e-5)
    ev = HC.decode_ref64(rows, nt, B, F, A, C, anc, H.STRIDES[l], False)
    HC.close(H.yolo_decode(lg, l, CFG, False), ev, 1e-5, 1e-5)
    # a pitch with pad columns changes nothing
    padded = np.full((B * F * F, 256), np.nan, np.float32)
    padded[:, :nt] = rows
    o2, p2 = HC.decode_ref64(padded, 256, B, F, A, C, anc, H.STRIDES[l], True)
    assert np.array_equal(o2, out) and np.array_equal(p2, pred)
    # backward, with g_output only, g_pred only and both
    go = rng.standard_normal(out.shape).astype(np.float32)
    gp = rng.standard_normal(pred.shape).astype(np.float32)
    for a, b in ((go, None), (None, gp), (go, gp)):
        g, S = HC.decode_bwd_ref64(padded, 256, B, F, A, C, anc, a, b)
        g_ref = H.yolo_decode_backward(lg, a, b, l, CFG)
        assert not g[:, nt:].any() and not S[:, nt:].any()
        HC.close(g_ref.transpose(0, 2, 3, 1).reshape(B * F * F, nt), g[:, :nt], 1e-5, 1e-5)
        assert (np.abs(g) <= S * (1 + 1e-12)).all()
        # the oracle's own fp32 arithmetic sits inside the bound the kernels are held to
        assert HC.decode_bwd_accept(g_ref.transpose(0, 2, 3, 1).reshape(B * F * F, nt), g[:, :nt], S[:, :nt]).all()


def test_decode_acceptance_is_tighter_than_the_project_bar():
    """(|v| + 8) * 2^-23 stays under the 1e-5 relative bar for |v| <= 8, rejects NaN, accepts a flush to zero and a
    common +inf, and the oracle's fp32 decode of the planted logits passes it."""
    v = np.array([0.0, 8.0, -8.0, 3.0])
    ref = np.array([1.0, 2.0, 1e-3, 5.0])
    assert not HC.decode_accept(ref * (1 + 1e-5), ref, v).any()
    assert HC.decode_accept(ref * (1 + 2.0 ** -23), ref, v).all()
    assert (HC.DEC_CONST + 8) * 2.0 ** -23 < 1e-5
    assert not HC.decode_accept(np.array([np.nan]), np.array([1.0]), np.array([0.0]))[0]
    assert HC.decode_accept(np.array([0.0]), np.array([1e-40]), np.array([-92.0]))[0]
    assert HC.decode_accept(np.array([np.inf]), np.array([1e43]), np.array([100.0]))[0]
    assert not HC.decode_accept(np.array([-np.inf]), np.array([-1e43]), np.array([100.0]))[0]
    assert not HC.decode_accept(np.array([1e38]), np.array([1e43]), np.array([100.0]))[0]


@pytest.mark.parametrize('case', HC.DECODE_CASES)
def test_decode_cases_reach_their_paths(case):
    C, A, F, B, ldl = case
    nt = A * (5 + C)
    lg, props = HC.make_logits(B, F, A, C, ldl, 5)
    assert lg.shape == (B * F * F, ldl) and np.isnan(lg[:, nt:]).all() and np.isfinite(lg[:, :nt]).all()
    if props['npix'] >= 16:
        for ch in HC.roles(C):
            have = set(props['planted'][ch])
            assert have >= {s * m for m in HC.PLANT for s in (1.0, -1.0)}, (ch, have)
        every = set().union(*[set(p) for p in props['planted'].values()])
        assert every >= {s * m for m in HC.PLANT_FEW for s in (1.0, -1.0)}
    # the same logits at another pitch
    other, _ = HC.make_logits(B, F, A, C, ldl + 4, 5)
    assert np.array_equal(other[:, :nt], lg[:, :nt])
    # reference values: finite logits give no NaN; +-1e4 gives 0, 1 or inf
    anc = HC.decode_anchors(A, 1)
    out, pred = HC.decode_ref64(lg, ldl, B, F, A, C, anc, 8.0, True)
    assert not np.isnan(out).any() and not np.isnan(pred).any()


def test_decode_case_list_covers_the_dispatch_edges():
    tiled = [c for c in HC.DECODE_CASES if HC.decode_takes_tiled(c[0], c[1], c[4])]
    plain = [c for c in HC.DECODE_CASES if not HC.decode_takes_tiled(c[0], c[1], c[4])]
    assert (80, 3, 19, 2, 256) in tiled and (80, 3, 19, 2, 255) in plain
    assert (1, 3, 4, 3, 20) in tiled and (1, 3, 4, 3, 32) in tiled
    assert (20, 3, 3, 2, 76) in tiled and (20, 3, 3, 2, 75) in plain
    assert (59, 4, 1, 5, 256) in tiled and 4 * (5 + 59) == 256
    assert any(c[1] == 1 for c in tiled) and any(c[1] == 1 for c in plain)
    assert {c[2] for c in tiled} >= {1, 3, 4, 19, 100}
    assert [HC.decode_tile(c[3], c[2]) for c in HC.DECODE_CASES].count(32) == 1
    assert 19 * 19 % 16 == 9 and 100 * 100 % 32 == 16 and 10 * 100 * 100 >= 100000
    # eval decode: the four 16-byte phases of a run's first float, over the box offsets the GPU test uses
    for C, A, F, B, ldl in tiled:
        if (5 + C) % 2 == 1 and B * F * F < 100000:
            ph = set()
            for off in (0, 1, 2, 3):
                ph |= {next(iter(HC.eval_run_phases(1, 1, 1, C, 1 + off, off)))}
            assert ph == {0, 1, 2, 3}
    got = set()
    for C, A, F, B, ldl in tiled:
        for off in (0, 1, 2, 3):
            got |= HC.eval_run_phases(B, F, A, C, A * F * F + off + 2, off)
    assert got == {0, 1, 2, 3}


@pytest.mark.parametrize('C', HC.LOSS_CLASSES)
@pytest.mark.parametrize('K', HC.LOSS_K)
def test_label_sets_have_their_properties(K, C):
    lab, props = HC.make_labels(K, C, 100 + K)
    assert lab.shape == (3, K, 5) and lab.dtype == np.float64
    assert props['n_eq_K'] and props['n'][0] == K
    assert props['class_in_last_word'] and props['positives'] > 0
    assert lab[..., 4].max() == C - 1 and lab[..., 4].min() >= 0
    if K >= 8:
        assert props['zero_row_between']
        assert props['n'][1] == min(K, 20) - 1
        if C >= 2:
            assert props['cells_with_two_classes'] >= 3          # one pair per layer
    # the K = 64 content with one more zero row: the same labels under the other assignment kernel
    if K == 64:
        more = np.concatenate([lab, np.zeros((3, 1, 5))], 1)
        assert HC.label_props(more, C)['n'] == props['n']


def test_saturated_loss_logits_are_planted_on_both_kinds_of_cell():
    C = 33
    lab, _ = HC.make_labels(64, C, 164)
    lgs, props = HC.make_loss_logits(C, 900, lab, saturate=True)
    assert props['planted_positive'] >= 8 and props['planted_background'] >= 8
    cfg = HC.cfg_with_classes(C)
    for l, lg in enumerate(lgs):
        assert np.isfinite(lg).all() and (np.abs(lg) == 30.0).sum() >= 8
        o, p = H.yolo_decode(lg, l, cfg, True)
        r = H.yolo_loss_layer(o, p, l, lab, cfg, 0.7)
        assert (o == 1.0).any()                                  # the fp32 sigmoid saturates: BCE hits its -100 clamp
        assert np.isfinite(r['grad_output']).all() and np.abs(r['grad_output']).max() >= 1e11   # the 1e-12 floor


def test_iou_boxes_hold_every_kind_of_pair():
    tot = dict(identical=0, nested=0, touching=0, zero_area=0, nan_boxes=0)
    for Na, Nb in HC.IOU_SHAPES:
        a, b, props = HC.make_iou_boxes(Na, Nb, 7)
        assert a.shape == (Na, 4) and b.shape == (Nb, 4) and a.dtype == np.float32
        for k in tot:
            tot[k] += props[k]
        for xyxy in (True, False):
            r = H.bboxes_iou(a, b, xyxy)
            if Na * Nb > 1:
                assert np.isnan(r).any() and not np.isnan(r).all()
    assert sorted(Na * Nb for Na, Nb in HC.IOU_SHAPES) == [1, 255, 257, 5 * 4097]
    assert all(v > 0 for v in tot.values()), tot


def test_nms_grid_case_has_its_properties():
    box, score, thr = HC.make_nms_grid()
    p = HC.nms_props(box, score, thr, limit=HC.NMS_LIMIT)
    assert p['survivors'] > 512
    assert 256 < HC.NMS_LIMIT < p['survivors'] and p['kept_with_limit'] == HC.NMS_LIMIT
    assert 256 <= p['limit_pos'] < 512                           # the limit expires inside the second chunk
    assert p['cross256'] >= 1 and p['second_trip'] >= 1
    assert p['iou_eq_thresh'] >= 1 and p['zero_area'] >= 1 and p['max_tie_group'] >= 3
    # without scores the order is the index order: still more than 512 survivors and a chain across chunks
    q = HC.nms_props(box, None, thr)
    assert q['survivors'] > 512 and q['cross256'] >= 1


@pytest.mark.parametrize('R', HC.NMS_SIZES)
def test_nms_cluster_cases(R):
    box, score, thr = HC.make_nms_clusters(R, 20 + R)
    p = HC.nms_props(box, score, thr)
    assert p['R'] == R and 1 <= p['survivors'] <= R
    if R >= 255:
        assert p['survivors'] < R and p['max_tie_group'] >= 3
    if R > 256:
        assert p['cross256'] >= 1


@pytest.fixture(scope='module')
def post_cases():
    return {k: HC.make_post_case(k) for k in HC.POST_KINDS}


def test_postprocess_cases_have_their_properties(post_cases):
    p, C, conf, thre, props = post_cases['big']
    assert C == 2 and props['cand'][0, 0] > 2048 and props['surv'][0, 0] > 512
    assert 0 < props['cand'][1, 0] <= 2048
    p, C, conf, thre, props = post_cases['four']
    assert p.shape[:2] == (5, 20) and props['images_in_first_tile'] == 4 and props['cand_rows_third_image_on'] >= 4
    assert all(props['images_with_candidates'])
    for k, n in (('n63', 63), ('n64', 64), ('n65', 65)):
        p, C, conf, thre, props = post_cases[k]
        assert p.shape[1] == n and all(props['images_with_candidates']) and (props['cand'] > 0).all()
    p, C, conf, thre, props = post_cases['c1']
    assert C == 1 and props['max_cand'] > 0 and props['max_surv'] < props['max_cand']
    p, C, conf, thre, props = post_cases['last']
    assert props['cand'][0, :4].sum() == 0 and props['cand'][0, 4] > 0
    assert props['images_with_candidates'] == [True, False, True]
    assert props['ref'][1] is None and props['ref'][0] is not None
