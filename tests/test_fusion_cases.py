# -*- coding: utf-8 -*-
"""What tests/fusion_cases.py's restatements promise, and what its WBF cases contain, shown without a GPU."""
import numpy as np
import pytest

import fusion_cases as FC
import nms_cases as NC

F32 = np.float32
F64 = np.float64


# ------------------------------------------------------------------------------------------ view
def test_view_identity_and_mirror():
    x = FC.view_input()
    assert FC.view_geometry(40, 72, 1.0, 8)[:4] == (40, 72, 40, 72)
    assert np.array_equal(FC.view_ref(x, 1.0, False, stride=8).view(np.int32), x.view(np.int32))
    assert np.array_equal(FC.view_ref(x, 1.0, True, stride=8).view(np.int32), x[..., ::-1].view(np.int32))


@pytest.mark.parametrize('r', FC.VIEW_SCALES)
@pytest.mark.parametrize('flip', (False, True))
def test_view_geometry_padding_and_range(r, flip):
    x = FC.view_input()
    ch, cw, Hv, Wv, ry, rx = FC.view_geometry(40, 72, r)
    assert (ch, cw) == (max(1, int(40 * r)), max(1, int(72 * r))) and Hv % 32 == 0 and Wv % 32 == 0
    assert 0 <= Hv - ch < 32 and 0 <= Wv - cw < 32 and ry.dtype == F32 and rx.dtype == F32
    v = FC.view_ref(x, r, flip)
    assert v.shape == (2, 3, Hv, Wv) and v.dtype == F32
    cols = slice(Wv - cw, Wv) if flip else slice(0, cw)
    pad = np.ones((Hv, Wv), bool)
    pad[:ch, cols] = False
    assert (v[:, :, pad] == FC.FILL).all() and FC.FILL == F32(114) / F32(255)
    inner = v[:, :, :ch, cols]
    assert inner.min() >= x.min() and inner.max() <= x.max()           # a convex combination of four taps
    # against float64 bilinear sampling: three lerps, a few ulp of values below 1
    sy = np.clip((np.arange(ch) + 0.5) * F64(ry) - 0.5, 0, 39)
    sx = np.clip((np.arange(cw) + 0.5) * F64(rx) - 0.5, 0, 71)
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    y1, x1 = np.minimum(y0 + 1, 39), np.minimum(x0 + 1, 71)
    fy, fx = (sy - y0)[:, None], sx - x0
    X = x.astype(F64)
    top = X[:, :, y0][..., x0] * (1 - fx) + X[:, :, y0][..., x1] * fx
    bot = X[:, :, y1][..., x0] * (1 - fx) + X[:, :, y1][..., x1] * fx
    want = top * (1 - fy) + bot * fy
    got = inner[..., ::-1] if flip else inner
    assert np.abs(got - want).max() < 1e-5


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize('r,flip', [(1.0, False), (1.0, True), (0.83, True), (0.67, False), (1.25, True)])
def test_merge_round_trip(r, flip):
    """a box at a known base position, pushed through the forward map in float64, comes back within 2 ulp of its largest
    addend: the view coordinate's rounding, the subtraction's (mirrored views) and the product's."""
    H, W = 64, 96
    m = FC.merge_meta(H, W, r, flip)
    rng = np.random.RandomState(2)
    base = np.stack([rng.uniform(0, W, 200), rng.uniform(0, H, 200), rng.uniform(1, 60, 200), rng.uniform(1, 60, 200)], 1)
    isx, isy = F64(m['inv_sx']), F64(m['inv_sy'])
    fwd = np.stack([base[:, 0] / isx, base[:, 1] / isy, base[:, 2] / isx, base[:, 3] / isy], 1)
    if flip:
        fwd[:, 0] = m['Wv'] - fwd[:, 0]
    pred = np.zeros((1, 200, 8), F32)
    pred[0, :, :4] = fwd
    pred[0, :, 4:] = rng.uniform(0, 1, (200, 4))
    out = FC.merge_one_ref(pred, m)
    assert np.array_equal(out[..., 4:], pred[..., 4:])
    big = np.abs(fwd).astype(F32)
    if flip:
        big[:, 0] = np.maximum(big[:, 0], F32(m['Wv']))
    tol = 2 * np.spacing(big).astype(F64) * np.array([isx, isy, isx, isy])
    assert (np.abs(out[0, :, :4].astype(F64) - base) <= tol).all()
    if r == 1.0 and not flip:
        assert np.array_equal(out.view(np.int32), pred.view(np.int32))   # the identity view keeps its bits


def test_merge_ref_stacks_views_in_order():
    p = FC.merge_pred(63, 8)
    metas = [FC.merge_meta(64, 96, 1.0, False), FC.merge_meta(64, 96, 0.83, True)]
    out = FC.merge_ref([p, p], metas)
    assert out.shape == (2, 126, 8) and np.array_equal(out[:, :63].view(np.int32), p.view(np.int32))
    assert np.array_equal(out[:, 63:, 4:], p[:, :, 4:]) and not np.array_equal(out[:, 63:, :4], p[:, :, :4])


# ------------------------------------------------------------------------------------------ WBF: properties
def _candidates(p, C, conf):
    """(image, box, class) of every candidate in output order for thresholds >= 1: class ascending, key order inside"""
    out = []
    for b in range(len(p)):
        sc = p[b][:, 5:5 + C] * p[b][:, 4:5]
        rows = []
        for c in range(C):
            idx = np.nonzero(sc[:, c] >= F32(conf))[0]
            idx = idx[np.argsort(-sc[idx, c], kind='stable')]
            rows += [(i, c) for i in idx]
        out.append(rows)
    return out


@pytest.mark.parametrize('thre', (1.0, 2.0))
def test_threshold_one_keeps_every_candidate(thre):
    p, C, conf, _ = FC.make_wbf_seg_case(257, 'class')
    q = p.copy()
    out, info = FC.postprocess_wbf_ref(q, C, conf, thre, views=1)
    for b, rows in enumerate(_candidates(q, C, conf)):
        assert len(out[b]) == len(rows)
        for r, (i, c) in zip(out[b], rows):
            assert np.array_equal(r[:4].view(np.int32), q[b, i, :4].view(np.int32))
            assert r[4] == 1 and r[6] == c
            assert r[5].view(np.int32) == (q[b, i, 4] * q[b, i, 5 + c]).view(np.int32)
    assert info['multi'] == 0


@pytest.mark.parametrize('K', (2, 3, 4))
def test_copies_fuse_into_the_single_copy_clusters(K):
    """K copies of the same rows with views = K: as many clusters as one copy gives with views = 1.  For K a power of two the
    K-fold sums are exact, which leaves one product and one division per coordinate: boxes within 2 ulp of the inputs, scores
    (S / K with f = 1) within 2 ulp of the single-copy ones.  K = 3 rounds its sums twice more: the count and the classes."""
    p, C, conf, thre = FC.make_wbf_separate_case()
    one, _ = FC.postprocess_wbf_ref(p.copy(), C, conf, thre, views=1)
    many, info = FC.postprocess_wbf_ref(np.concatenate([p] * K, axis=1), C, conf, thre, views=K)
    assert len(one[0]) == len(many[0]) == 8 and info['single'] == 0
    assert all((seg['members'] == K).all() for seg in info['segments'].values())
    assert np.array_equal(one[0][:, 6], many[0][:, 6])
    if K in (2, 4):
        assert (np.abs(many[0][:, :4] - one[0][:, :4]) <= 2 * np.spacing(np.abs(one[0][:, :4]))).all()
        assert (np.abs(many[0][:, 5] - one[0][:, 5]) <= 2 * np.spacing(one[0][:, 5])).all()


def test_separate_boxes_are_hard_nms_but_for_the_score_columns():
    p, C, conf, thre = FC.make_wbf_separate_case()
    wbf, info = FC.postprocess_wbf_ref(p.copy(), C, conf, thre)
    nms, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre)
    cols = [0, 1, 2, 3, 6]
    assert np.array_equal(wbf[0][:, cols].view(np.int32), nms[0][:, cols].view(np.int32)) and info['multi'] == 0
    assert np.array_equal(wbf[0][:, 4] * wbf[0][:, 5], nms[0][:, 4] * nms[0][:, 5])
    capped, _ = FC.postprocess_wbf_ref(p.copy(), C, conf, thre, max_det=5)
    ncap, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, max_det=5)
    assert np.array_equal(capped[0][:, cols], ncap[0][:, cols])


def test_short_clusters_are_scaled_by_members_over_views():
    p, C, conf, thre = FC.make_wbf_separate_case()
    one, _ = FC.postprocess_wbf_ref(p.copy(), C, conf, thre, views=1)
    three, _ = FC.postprocess_wbf_ref(p.copy(), C, conf, thre, views=3)
    assert np.array_equal(three[0][:, 5], one[0][:, 5] * (F32(1) / F32(3)))
    assert np.array_equal(three[0][:, :5], one[0][:, :5])


def test_property_block_is_what_it_says():
    p = FC.property_rows(2)[None]
    out, info = FC.postprocess_wbf_ref(p.copy(), 2, FC.WBF_CONF, FC.WBF_THRE)
    seg = info['segments'][(0, 0)]
    assert seg['n'] == 8 and sorted(seg['members']) == [1, 1, 1, 1, 1, 3] and seg['eq'] == 1 and seg['nan'] == 1
    q = p.copy()
    NC.postprocess_nms_ref(q, 2, 0.0, 0.5)                  # (corners in place)
    assert NC.measure(q[0, 1, :4], q[0, 0, :4], 'iou') == F32(FC.WBF_THRE)
    assert np.isnan(NC.measure(q[0, 3, :4], q[0, 2, :4], 'iou'))
    fused = out[0][4]                                       # creation order: 0.9, 0.85 (the cluster of three), 0.8, ...
    assert out[0][1, 5] == (F32(0.85) + F32(0.75) + F32(0.65)) / F32(3) and fused[5] == F32(0.6)
    assert 498 < out[0][1, 0] < 505 and 3000 < out[0][1, 1] < 3005


# ------------------------------------------------------------------------------------------ WBF: what every case contains
@pytest.mark.parametrize('case', FC.WBF_CASES, ids=lambda c: '%s-%s' % (c[0], c[1] if isinstance(c[1], str) else '%d-%s' % c[1]))
def test_every_wbf_case_has_the_four_situations(case):
    agn = case[0] == 'seg' and case[1][1] == 'image'
    out, info, xyxy = FC.wbf_reference(case, (('agnostic', True),) if agn else ())
    assert info['multi'] >= 1 and info['single'] >= 1 and info['eq'] >= 1 and info['nan'] >= 1, info
    assert all(np.isfinite(o).all() for o in out if o is not None)
    p, C, conf, thre = FC.wbf_case(case)
    if case[0] == 'seg':
        R = case[1][0]
        assert info['segments'][(0, -1 if agn else 0)]['n'] == R
    elif case[1] == 'wide':
        assert 5 + C > 255                                  # beyond the LDS-tiled count / fill kernels
    else:
        B, N = p.shape[:2]
        assert info['candidates'] > max(B * N // 2, 1 << 16)                # the first capacity guess
        assert max(s['n'] for s in info['segments'].values()) <= 1024


def test_sizes_straddle_the_kernel_bounds():
    assert set((1, 255, 256, 257, 513)) <= set(FC.WBF_SIZES)
    assert any(1024 < R <= 2048 for R in FC.WBF_SIZES) and any(R > 2048 for R in FC.WBF_SIZES)
