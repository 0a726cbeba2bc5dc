# -*- coding: utf-8 -*-
"""NumPy float32 restatements of the test-time-augmentation kernels (csrc/tta.hip: view, merge) and of weighted box fusion
(csrc/postprocess.hip: post_wbf_kernel), DESIGN.md section 22, and the inputs of their tests.

Every step is one float32 operation in the documented order (NumPy's float32 + - * / are correctly rounded, like the
kernels', which are built without fma contraction), so the kernels are compared bit for bit: rows, order and every float.

tests/test_fusion_cases.py shows without a GPU that the restatements have the properties the semantics promise and that
every WBF case holds what the GPU comparison relies on: a multi-member cluster, a singleton, a candidate whose measure equals
the threshold exactly (it must not match) and a NaN measure from a degenerate box pair."""
import functools

import numpy as np

import nms_cases as NC

F32 = np.float32
F64 = np.float64
FILL = F32(114) / F32(255)                                  # letterbox_batch's canvas grey: float(114) / 255.0f


# ------------------------------------------------------------------------------------------ view
def view_geometry(H, W, r, stride=32):
    ch, cw = max(1, int(H * r)), max(1, int(W * r))
    Hv, Wv = -(-ch // stride) * stride, -(-cw // stride) * stride
    return ch, cw, Hv, Wv, F32(H) / F32(ch), F32(W) / F32(cw)


def _taps(n_out, ratio, size):
    """(i0, i1, frac) of output coordinates 0 .. n_out - 1: sy = (float(y) + 0.5f) * ry - 0.5f, clamped, floor, fraction"""
    s = (np.arange(n_out).astype(F32) + F32(0.5)) * F32(ratio) - F32(0.5)
    s = np.minimum(np.maximum(s, F32(0)), F32(size - 1)).astype(F32)
    f0 = np.floor(s).astype(F32)
    i0 = f0.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), (s - f0).astype(F32)


def view_ref(x, r, flip, stride=32, fill=FILL):
    """x [B, C, H, W] float32 -> the view [B, C, Hv, Wv] of y4_tta_view_f32 with the host's geometry for scale r"""
    x = np.asarray(x)
    assert x.dtype == F32
    B, C, H, W = x.shape
    ch, cw, Hv, Wv, ry, rx = view_geometry(H, W, r, stride)
    out = np.full((B, C, Hv, Wv), F32(fill), F32)
    xs = (Wv - 1 - np.arange(Wv)) if flip else np.arange(Wv)
    inside = xs < cw
    y0, y1, fy = _taps(ch, ry, H)
    x0, x1, fx = _taps(Wv, rx, W)                            # indexed by xs below
    x0, x1, fx = x0[xs[inside]], x1[xs[inside]], fx[xs[inside]]
    a, b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    c, d = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    top = a + (b - a) * fx
    bot = c + (d - c) * fx
    val = top + (bot - top) * fy[:, None]
    assert val.dtype == F32
    out[:, :, :ch, inside] = val
    return out


@functools.lru_cache(maxsize=None)
def view_input(W=72, seed=3):
    """[2, 3, 40, W] float32, no zeros (a + 0 would lose the sign of a -0)"""
    rng = np.random.RandomState(seed + W)
    return rng.uniform(0.01, 1.0, (2, 3, 40, W)).astype(F32)


VIEW_SCALES = (1.0, 0.67, 0.83, 1.25)


# ------------------------------------------------------------------------------------------ merge
def merge_meta(H, W, r, flip, stride=32):
    ch, cw, Hv, Wv, _, _ = view_geometry(H, W, r, stride)
    return dict(flip=bool(flip), Wv=Wv, Hv=Hv, ch=ch, cw=cw, inv_sx=F32(W) / F32(cw), inv_sy=F32(H) / F32(ch))


def merge_one_ref(pred, meta):
    """one view's rows [B, N, n_ch] mapped to the base canvas (y4_tta_merge_f32's arithmetic)"""
    p = np.asarray(pred)
    assert p.dtype == F32
    q = p.copy()
    if not meta['flip'] and meta['inv_sx'] == F32(1) and meta['inv_sy'] == F32(1):
        return q                                            # copied, not multiplied
    cx = (F32(meta['Wv']) - p[..., 0]) if meta['flip'] else p[..., 0]
    q[..., 0] = cx * F32(meta['inv_sx'])
    q[..., 1] = p[..., 1] * F32(meta['inv_sy'])
    q[..., 2] = p[..., 2] * F32(meta['inv_sx'])
    q[..., 3] = p[..., 3] * F32(meta['inv_sy'])
    return q


def merge_ref(preds, metas):
    return np.concatenate([merge_one_ref(p, m) for p, m in zip(preds, metas)], axis=1)


@functools.lru_cache(maxsize=None)
def merge_pred(N, n_ch, seed=9):
    """[2, N, n_ch] float32: boxes of a 96 x 64 view, the other columns random"""
    rng = np.random.RandomState(seed + N + n_ch)
    p = rng.uniform(0.0, 1.0, (2, N, n_ch)).astype(F32)
    p[..., 0] = rng.uniform(0, 96, (2, N))
    p[..., 1] = rng.uniform(0, 64, (2, N))
    p[..., 2:4] = rng.uniform(1, 60, (2, N, 2))
    return p


MERGE_N = (63, 64, 65, 257)
MERGE_NCH = (8, 85)                                         # a row of 85 floats is not 16-byte aligned


# ------------------------------------------------------------------------------------------ weighted box fusion
def wbf_segment(box, s, cls, thr, views):
    """candidates in key order -> (rows [T, 7] float32 in creation order, info)"""
    n = len(box)
    thr = F32(thr)
    F = np.zeros((n, 4), F32)
    Sum = np.zeros((n, 4), F32)
    S = np.zeros(n, F32)
    cnt = np.zeros(n, np.int64)
    ccl = np.zeros(n, np.int64)
    T = 0
    info = dict(n=n, eq=0, nan=0)
    for j in range(n):
        t = -1
        if T:
            m = NC.measure(box[j][None, :], F[:T], 'iou')
            info['eq'] += int((m == thr).sum())
            info['nan'] += int(np.isnan(m).sum())
            with np.errstate(invalid='ignore'):
                hit = m > thr                               # strict; a NaN never matches
            if hit.any():
                best = m[hit].max()
                t = int(np.nonzero(hit & (m == best))[0][0])                # ties: the lowest t
        prod = (s[j] * box[j]).astype(F32)
        if t >= 0:
            Sum[t] = Sum[t] + prod
            S[t] = S[t] + s[j]
            cnt[t] += 1
            F[t] = Sum[t] / S[t]
        else:
            Sum[T] = prod
            S[T] = s[j]
            cnt[T] = 1
            ccl[T] = cls[j]
            F[T] = box[j]                                   # the candidate's box itself, no arithmetic
            T += 1
    rows = np.zeros((T, 7), F32)
    rows[:, :4] = F[:T]
    rows[:, 4] = F32(1)
    mean = S[:T] / cnt[:T].astype(F32)
    f = np.minimum(cnt[:T], views).astype(F32) / F32(views)
    rows[:, 5] = mean * f
    rows[:, 6] = ccl[:T]
    info.update(clusters=T, multi=int((cnt[:T] > 1).sum()), single=int((cnt[:T] == 1).sum()), members=cnt[:T].copy())
    return rows, info


def postprocess_wbf_ref(prediction, num_classes, conf_thre, iou_thre=0.55, views=1, agnostic=False, max_det=0):
    """-> (list of [n, 7] float32 arrays or None, info); `prediction` (float32) is converted to corners in place.
    info['segments'][(b, c)] (c = -1: agnostic) as wbf_segment reports it; the totals 'multi', 'single', 'eq', 'nan'."""
    p = prediction
    assert p.dtype == F32
    C = num_classes
    corner = np.empty_like(p[:, :, :4])
    corner[:, :, 0] = p[:, :, 0] - p[:, :, 2] / F32(2)
    corner[:, :, 1] = p[:, :, 1] - p[:, :, 3] / F32(2)
    corner[:, :, 2] = p[:, :, 0] + p[:, :, 2] / F32(2)
    corner[:, :, 3] = p[:, :, 1] + p[:, :, 3] / F32(2)
    p[:, :, :4] = corner
    out = [None] * len(p)
    info = dict(segments={}, multi=0, single=0, eq=0, nan=0, candidates=0)
    conf = F32(conf_thre)
    for b in range(len(p)):
        ip = p[b]
        sc = ip[:, 5:5 + C] * ip[:, 4:5]
        box_idx, cls_idx = np.nonzero(sc >= conf)           # row-major: box ascending, then class
        if len(box_idx) == 0:
            continue
        s_all = sc[box_idx, cls_idx]
        rows = []
        for c in ([-1] if agnostic else list(np.unique(cls_idx))):
            m = np.ones(len(box_idx), bool) if agnostic else cls_idx == c
            bi, ci, s0 = box_idx[m], cls_idx[m], s_all[m]
            order = np.argsort(-s0, kind='stable')          # score descending, then key index (box, or box * C + class)
            bi, ci, s0 = bi[order], ci[order], s0[order]
            r, seg = wbf_segment(ip[bi, :4], s0, ci, iou_thre, views)
            info['segments'][(b, int(c))] = seg
            for k in ('multi', 'single', 'eq', 'nan'):
                info[k] += seg[k]
            info['candidates'] += seg['n']
            rows.append(r)
        rows = np.concatenate(rows, 0)
        if max_det and len(rows) > max_det:
            score = rows[:, 4] * rows[:, 5]
            order = np.lexsort((np.arange(len(rows)), -score))
            rows = rows[np.sort(order[:max_det])]
        out[b] = rows
    return out, info


WBF_THRE = 0.5
WBF_CONF = 0.04
PROP_AT = (0.0, 3000.0)                                     # the property block lies far below everything else


def property_rows(C, cls=0):
    """Eight rows [8, 5 + C] of class `cls`, objectness 1 (the score is the class confidence, exactly), integer corners:
      0, 1   100 x 100 (0.9) and its upper half (0.8): IoU = 5000 / ((10000 + 5000) - 5000) = 0.5 = WBF_THRE exactly:
             no match, two singletons;
      2, 3   the same point twice (0.7, 0.6): 0 / ((0 + 0) - 0) is NaN: no match, two singletons;
      4 .. 6 three strongly overlapping boxes (0.85, 0.75, 0.65): one cluster of three;
      7      a box on its own (0.5)."""
    ox, oy = PROP_AT
    box = np.array([[0, 0, 100, 100], [0, 0, 100, 50], [300, 300, 300, 300], [300, 300, 300, 300],
                    [500, 0, 600, 100], [505, 5, 605, 105], [498, 0, 600, 98], [800, 0, 860, 60]], F64)
    box[:, [0, 2]] += ox
    box[:, [1, 3]] += oy
    p = NC._to_pred(box, C)
    p[:, 4] = 1.0
    p[:, 5 + cls] = [0.9, 0.8, 0.7, 0.6, 0.85, 0.75, 0.65, 0.5]
    return p.astype(F32)


def _pad_rows(p, N):
    out = np.zeros((N, p.shape[1]), F32)
    out[:len(p)] = p
    out[len(p):, 0:2] = 50.0
    out[len(p):, 2:4] = 10.0                                # objectness 0: never a candidate
    return out


WBF_SIZES = NC.SEG_SIZES + (1100, 2100)                     # 1100: above the 1024-cluster LDS bound; 2100: and above the sort's


@functools.lru_cache(maxsize=None)
def make_wbf_seg_case(R, mode):
    """(pred [2, N, 7], C = 2, conf, thre).  Image 0: nms_cases.make_seg_case's clustered boxes, the (0, 0) segment ('class')
    or the image's agnostic segment ('image') holding exactly R candidates.  Image 1: the property block."""
    p0 = NC.make_seg_case(R, mode)[0][0]
    N = max(R, 8)
    return np.stack([_pad_rows(p0, N), _pad_rows(property_rows(2), N)]).astype(F32), 2, WBF_CONF, WBF_THRE


@functools.lru_cache(maxsize=None)
def make_wbf_wide_case(kind):
    """'wide': nms_cases' C = 252 case (rows of 257 floats: the row-per-thread count / fill kernels).
    'overflow': C = 48, N = 800 at conf 1e-6: about 76 000 candidates, more than the first buffer guess of 65 536, so the call
    repeats with room after its host read (segments of almost 800; no candidate has score 0, whose cluster would be 0 / 0).
    Both with the property block at the head of image 1."""
    if kind == 'wide':
        p, C, conf, _ = NC.make_wide_case('wide')
        p = p.copy()
    else:
        C, N, conf = 48, 800, 1e-6
        rng = np.random.RandomState(7)
        p = np.zeros((2, N, 5 + C), F32)
        p[..., 0:2] = rng.uniform(50, 550, (2, N, 2))
        p[..., 2:4] = rng.uniform(10, 200, (2, N, 2))
        p[..., 4] = rng.uniform(0.05, 1.0, (2, N))
        p[..., 5:] = rng.uniform(0, 1, (2, N, C)) ** 2
    p[1, :8] = property_rows(C)
    return p.astype(F32), C, conf, WBF_THRE


def make_wbf_separate_case():
    """Three classes of disjoint boxes (nms_cases.make_maxdet_case) and no degenerate box: every candidate is its own
    cluster, and hard NMS keeps every candidate."""
    return NC.make_maxdet_case()


def wbf_case(case):
    kind, arg = case
    if kind == 'seg':
        return make_wbf_seg_case(*arg)
    if kind == 'wide':
        return make_wbf_wide_case(arg)
    raise KeyError(kind)


WBF_CASES = ([('seg', (R, 'class')) for R in WBF_SIZES] + [('seg', (R, 'image')) for R in WBF_SIZES] +
             [('wide', 'wide'), ('wide', 'overflow')])


@functools.lru_cache(maxsize=None)
def wbf_reference(case, kw):
    """the restatement's result for a case (computed once): (rows per image, info, xyxy); kw: sorted (key, value) pairs"""
    p, C, conf, thre = wbf_case(case)
    q = p.copy()
    out, info = postprocess_wbf_ref(q, C, conf, thre, **dict(kw))
    return out, info, q[:, :, :4].copy()
