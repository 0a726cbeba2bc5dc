# -*- coding: utf-8 -*-
"""NumPy restatement of postprocess_nms (include/yolov4_amd.h) and the inputs of its tests.

`postprocess_nms_ref` has two modes.  float32 follows the documented operation order step by step (NumPy's float32
+ - * / are correctly rounded, like the kernel's, which is built without fma contraction): hard NMS with either measure
and linear Soft-NMS are compared bit for bit.  float64 is the reference of Gaussian Soft-NMS (expf is not correctly
rounded): there the rows and their order must agree, which the cases guarantee by keeping every selection and every
prune decision at least 4 * tol away from its alternative, tol = (rows emitted in the segment + 1) * 16 * 2^-24 being the
bound on the relative error of a decayed fp32 score.

tests/test_nms_cases.py shows without a GPU that every case has the property it is named for."""
import functools

import numpy as np

import head_cases as HC

F32 = np.float32
F64 = np.float64
TOL_UNIT = 16.0 * 2.0 ** -24


def gauss_tol(rows_emitted):
    """Bound on the relative error of the kernel's decayed score after `rows_emitted` decay factors: each factor carries a
    few ulp from expf and its argument (measure, square, division), far fewer than 16 (derived, not measured)."""
    return (rows_emitted + 1) * TOL_UNIT


def measure(a, o, metric, T=F32, parts=False):
    """Overlap of candidates a [..., 4] against selected boxes o [..., 4] (xyxy, broadcast), in the documented order."""
    a = np.asarray(a).astype(T)
    o = np.asarray(o).astype(T)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_o = (o[..., 2] - o[..., 0]) * (o[..., 3] - o[..., 1])
        tlx, tly = np.fmax(a[..., 0], o[..., 0]), np.fmax(a[..., 1], o[..., 1])
        brx, bry = np.fmin(a[..., 2], o[..., 2]), np.fmin(a[..., 3], o[..., 3])
        en = ((tlx < brx) & (tly < bry)).astype(T)
        inter = ((brx - tlx) * (bry - tly)) * en
        iou = inter / ((area_a + area_o) - inter)
        if metric == 'iou' and not parts:
            return iou
        dx = ((a[..., 0] + a[..., 2]) - (o[..., 0] + o[..., 2])) * T(0.5)
        dy = ((a[..., 1] + a[..., 3]) - (o[..., 1] + o[..., 3])) * T(0.5)
        rho2 = dx * dx + dy * dy
        ew = np.fmax(a[..., 2], o[..., 2]) - np.fmin(a[..., 0], o[..., 0])
        eh = np.fmax(a[..., 3], o[..., 3]) - np.fmin(a[..., 1], o[..., 1])
        c2 = ew * ew + eh * eh
        pen = np.where(c2 == 0, T(0), rho2 / np.where(c2 == 0, T(1), c2)).astype(T)
        diou = iou - pen
    if parts:
        return dict(iou=iou, diou=diou, rho2=rho2, c2=c2)
    return diou if metric == 'diou' else iou


def _hard(box, thr, metric, limit):
    """greedy in sorted order -> (kept positions, info)"""
    n = len(box)
    alive = np.ones(n, bool)
    kept = []
    for i in range(n):
        if not alive[i]:
            continue
        kept.append(i)
        if limit and len(kept) >= limit:
            break
        rest = np.nonzero(alive[i + 1:])[0] + i + 1
        if len(rest):
            with np.errstate(invalid='ignore'):
                alive[rest[measure(box[rest], box[i], metric) >= thr]] = False
    return np.asarray(kept, np.int64), dict(n=n, emitted=len(kept))


def _soft(box, s0, thr, conf, metric, kind, sigma, limit, f64):
    T = F64 if f64 else F32
    n = len(box)
    s0 = s0.astype(T)
    thr, conf, sigma = T(F32(thr)), T(F32(conf)), T(F32(sigma))
    W = np.ones(n, T)
    alive = np.ones(n, bool)
    emitted, weights = [], []
    info = dict(n=n, kept_decayed=0, pruned_after_decay=0, key_ties=0, sel_gap=np.inf, prune_gap=np.inf)
    while True:
        idx = np.nonzero(alive)[0]
        if len(idx) == 0 or (limit and len(emitted) >= limit):
            break
        cur = s0[idx] * W[idx]
        best = cur.max()
        at = int(np.argmax(cur))                            # first of equal scores: the lower sorted position
        sel = int(idx[at])
        others = np.delete(cur, at)
        if len(others):
            second = others.max()
            info['key_ties'] += int(second == best)
            info['sel_gap'] = min(info['sel_gap'], float((best - second) / best))
        emitted.append(sel)
        weights.append(W[sel])
        info['kept_decayed'] += int(W[sel] < 1)
        alive[sel] = False
        rem = np.nonzero(alive)[0]
        if len(rem) == 0:
            continue
        m = measure(box[rem], box[sel], metric, T)
        with np.errstate(invalid='ignore'):
            ov = np.where(m > 0, m, T(0)).astype(T)
        if kind == 'linear':
            w = np.where(ov >= thr, T(1) - ov, T(1)).astype(T)
        else:
            w = np.exp(-(ov * ov) / sigma).astype(T)
        W[rem] = W[rem] * w
        cur = s0[rem] * W[rem]
        info['prune_gap'] = min(info['prune_gap'], float(np.abs(cur - conf).min() / conf))
        gone = cur < conf
        info['pruned_after_decay'] += int(gone.sum())
        alive[rem[gone]] = False
    info['emitted'] = len(emitted)
    return np.asarray(emitted, np.int64), np.asarray(weights, T), info


def postprocess_nms_ref(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, metric='iou', soft=None, sigma=0.5,
                        agnostic=False, max_det=0, f64=False):
    """-> (list of [n, 7] arrays or None, info).  `prediction` (float32) is converted to corners in place, like the
    reference.  Rows are float32, or float64 when f64 (columns 0-4 and 6 hold float32 values either way).
    info['segments'][(b, c)] (c = -1 for an agnostic segment) describes what happened in a segment, info['cap_gap'] the
    smallest relative score gap across a max_det cut."""
    p = prediction
    assert p.dtype == F32
    C = num_classes
    T = F64 if (f64 and soft) else F32
    corner = np.empty_like(p[:, :, :4])
    corner[:, :, 0] = p[:, :, 0] - p[:, :, 2] / F32(2)
    corner[:, :, 1] = p[:, :, 1] - p[:, :, 3] / F32(2)
    corner[:, :, 2] = p[:, :, 0] + p[:, :, 2] / F32(2)
    corner[:, :, 3] = p[:, :, 1] + p[:, :, 3] / F32(2)
    p[:, :, :4] = corner
    out = [None] * len(p)
    info = dict(segments={}, cap_gap=np.inf)
    conf, thr = F32(conf_thre), F32(nms_thre)
    for b in range(len(p)):
        ip = p[b]
        sc = ip[:, 5:5 + C] * ip[:, 4:5]
        box_idx, cls_idx = np.nonzero(sc >= conf)           # row-major: box ascending, then class
        if len(box_idx) == 0:
            continue
        s_all = sc[box_idx, cls_idx]
        seg_ids = [-1] if agnostic else list(np.unique(cls_idx))
        rows = []
        for c in seg_ids:
            m = np.ones(len(box_idx), bool) if agnostic else cls_idx == c
            bi, ci, s0 = box_idx[m], cls_idx[m], s_all[m]
            order = np.argsort(-s0, kind='stable')          # score descending, then key index (box, or box * C + class)
            bi, ci, s0 = bi[order], ci[order], s0[order]
            box = ip[bi, :4]
            if soft is None:
                kept, seg = _hard(box, thr, metric, max_det)
                wts = np.ones(len(kept), F32)
            else:
                kept, wts, seg = _soft(box, s0, nms_thre, conf_thre, metric, soft, sigma, max_det, f64)
            info['segments'][(b, int(c))] = seg
            r = np.zeros((len(kept), 7), T)
            r[:, :5] = ip[bi[kept], :5]
            r[:, 5] = ip[bi[kept], 5 + ci[kept]].astype(T) * wts.astype(T)
            r[:, 6] = ci[kept]
            rows.append(r)
        rows = np.concatenate(rows, 0)
        if max_det and len(rows) > max_det:
            score = rows[:, 4] * rows[:, 5]                 # fp32 product in fp32 mode
            order = np.lexsort((np.arange(len(rows)), -score))
            lo, hi = score[order[max_det]], score[order[max_det - 1]]
            info['cap_gap'] = min(info['cap_gap'], float((hi - lo) / hi))
            rows = rows[np.sort(order[:max_det])]
        out[b] = rows
    return out, info


# ------------------------------------------------------------------------------------------ cases
def _to_pred(box_xyxy, C):
    """[N, 5 + C] rows in centre / size form around the given corners, objectness and classes zero"""
    b = np.asarray(box_xyxy, F64)
    p = np.zeros((len(b), 5 + C), F32)
    p[:, 0] = (b[:, 0] + b[:, 2]) / 2
    p[:, 1] = (b[:, 1] + b[:, 3]) / 2
    p[:, 2] = b[:, 2] - b[:, 0]
    p[:, 3] = b[:, 3] - b[:, 1]
    return p


SEG_SIZES = HC.NMS_SIZES                                    # 1, 255, 256, 257, 513: around the 256-candidate chunk
SEG_CONF, SEG_THRE = 0.04, 0.45


@functools.lru_cache(maxsize=None)
def make_seg_case(R, mode, seed=5):
    """(pred [2, R, 7], C = 2, conf, thre).  Image 0 holds make_nms_clusters' R clustered boxes (scores on a 0.01 lattice:
    many ties).  mode 'class': all R are candidates of class 0 (and some of class 1 too): the (0, 0) segment has exactly R.
    mode 'image': every box is a candidate in exactly one class: the agnostic segment of image 0 has exactly R.
    Image 1 is R random boxes, most of them candidates in both classes."""
    rng = np.random.RandomState(seed + R)
    box, score, thre = HC.make_nms_clusters(R, seed + R)
    p0 = _to_pred(box, 2)
    p0[:, 4] = 0.9
    if mode == 'class':
        p0[:, 5] = score
        p0[:, 6] = np.round(rng.uniform(0.05, 1.0, R), 2) * (rng.uniform(size=R) < 0.5)
    else:
        k = rng.randint(0, 2, R)
        p0[np.arange(R), 5 + k] = score
    p1 = HC._grid_pred(rng, 1, R, 2, img=300.0)[0]
    return np.stack([p0, p1]).astype(F32), 2, SEG_CONF, thre


GAUSS_CONF, GAUSS_THRE, GAUSS_SIGMA = 0.25, 0.45, 0.5
GAUSS_BIG = 2100                                            # above the 2048-candidate LDS bound


def _gauss_build(R, seed):
    rng = np.random.RandomState(seed)
    ncl = max(1, min(8, R // 16))
    boxes, scores = [], []
    cx = 100.0 + 250.0 * np.arange(ncl)
    for k in range(ncl):                                    # leaders: disjoint 60 x 60 boxes, scores 3 % apart
        boxes.append([cx[k] - 30, 70, cx[k] + 30, 130]); scores.append(0.95 - 0.03 * k)
    nmid = min(2 * ncl, max(0, R - ncl))
    for m in range(nmid):                                   # mids: IoU ~ 0.26 with their leader -> kept with W ~ 0.87
        k, d = m % ncl, m // ncl
        j = rng.uniform(-1, 1, 2)
        dx, dy = (35 + j[0], j[1]) if d == 0 else (j[0], 35 + j[1])
        boxes.append([cx[k] - 30 + dx, 70 + dy, cx[k] + 30 + dx, 130 + dy]); scores.append(0.62 - 0.03 * k - 0.012 * d)
    for q in range(R - ncl - nmid):                         # crowd: on top of a leader, gone once it is selected
        k = q % ncl
        j = rng.uniform(-3, 3, 4)
        boxes.append([cx[k] - 30 + j[0], 70 + j[1], cx[k] + 30 + j[2], 130 + j[3]])
        scores.append(GAUSS_CONF * rng.uniform(1.02, 1.5))
    perm = rng.permutation(R)
    p = _to_pred(np.asarray(boxes)[perm], 2)
    p[:, 4] = 0.8
    p[:, 5] = (np.asarray(scores)[perm] / 0.8).astype(F32)
    p[:, 6] = rng.uniform(0.0, 1.0, R) * (rng.uniform(size=R) < 0.02)        # a few candidates of class 1
    return p[None].astype(F32)


def gauss_margin_ok(pred, C, conf, thre, sigma=GAUSS_SIGMA, **kw):
    """every selection, prune and cap decision of the float64 restatement is >= 4 * tol from its alternative"""
    _, info = postprocess_nms_ref(pred.copy(), C, conf, thre, soft='gaussian', sigma=sigma, f64=True, **kw)
    worst = 0
    for seg in info['segments'].values():
        tol = gauss_tol(seg['emitted'])
        if min(seg['sel_gap'], seg['prune_gap']) < 4 * tol:
            return False
        worst = max(worst, seg['emitted'])
    return info['cap_gap'] >= 4 * gauss_tol(worst)


@functools.lru_cache(maxsize=None)
def make_gauss_case(R, **kw):
    """(pred [1, R, 7], C = 2, conf, thre, seed): leaders, partly overlapping mids and a crowd on top of the leaders, the
    (0, 0) segment holding exactly R candidates; the first seed whose decisions all keep the 4 * tol margin."""
    for seed in range(200):
        p = _gauss_build(R, 1000 + seed)
        if gauss_margin_ok(p, 2, GAUSS_CONF, GAUSS_THRE, **kw):
            return p, 2, GAUSS_CONF, GAUSS_THRE, seed
    raise AssertionError('no seed keeps the margin at R = %d' % R)


@functools.lru_cache(maxsize=None)
def make_gauss_tile_case(kind, **kw):
    """head_cases' 'n63' / 'n64' / 'n65' shape (B = 3, C = 4), the first seed that keeps the margin"""
    for seed in range(200):
        p, C, conf, thre, _ = HC.make_post_case(kind, seed=100 + seed)
        if gauss_margin_ok(p, C, conf, thre, **kw):
            return p, C, conf, thre, seed
    raise AssertionError('no seed keeps the margin for ' + kind)


DIOU_THRE = 0.45


def make_diou_case():
    """One class.  Boxes 0 / 1: 100 x 100, offset (20, 20): IoU 0.4706 >= 0.45 > DIoU 0.4428, so box 1 falls under IoU and
    stays under DIoU.  Boxes 2 / 3: the same point (zero width and height): c2 == 0.  Boxes 4..: nested and distant."""
    box = np.array([[0, 0, 100, 100], [20, 20, 120, 120], [300, 300, 300, 300], [300, 300, 300, 300],
                    [400, 0, 500, 100], [410, 10, 490, 90], [0, 400, 80, 480]], F64)
    p = _to_pred(box, 1)
    p[:, 4] = 1.0
    p[:, 5] = [0.9, 0.8, 0.7, 0.6, 0.85, 0.5, 0.4]
    return p[None].astype(F32), 1, 0.25, DIOU_THRE


def make_soft_case():
    """Two classes with the same layout (class 1 shifted by 1000 px), linear decay, conf 0.25, thre 0.45.  Per class:
    L (0.9); M, IoU 0.5 with L, 0.8 -> kept with W = 0.5; P, IoU 0.6 with L, 0.3 -> pruned after its decay;
    T1 / T2: disjoint, both 0.5, never decayed: a tie in current score that the key decides."""
    rows, cls, sc = [], [], []
    for c in range(2):
        x = 1000.0 * c
        for bx, s in (([0, 0, 100, 100], 0.9), ([0, 0, 100, 50], 0.8), ([0, 0, 100, 60], 0.3),
                      ([300, 0, 360, 60], 0.5), ([500, 0, 560, 60], 0.5)):
            rows.append([bx[0] + x, bx[1], bx[2] + x, bx[3]]); cls.append(c); sc.append(s)
    p = _to_pred(np.asarray(rows), 2)
    p[:, 4] = 1.0
    p[np.arange(len(rows)), 5 + np.asarray(cls)] = sc
    return p[None].astype(F32), 2, 0.25, 0.45


def make_agnostic_case():
    """Three classes.  Box 0 is a candidate of class 0 (0.8) and class 1 (0.6): agnostic keeps only the class-0 row.  Box 1
    (class 2, 0.5) has IoU 0.7 with box 0: kept per class, suppressed across classes.  Box 2 is far away."""
    box = np.array([[0, 0, 100, 100], [0, 0, 100, 70], [300, 300, 380, 380]], F64)
    p = _to_pred(box, 3)
    p[:, 4] = 1.0
    p[0, 5], p[0, 6] = 0.8, 0.6
    p[1, 7] = 0.5
    p[2, 6] = 0.7
    return p[None].astype(F32), 3, 0.25, 0.45


def make_maxdet_case():
    """Three classes of disjoint boxes (8 survivors): class 0: 0.9 0.8 0.5 0.4; class 1: 0.85 0.5 0.3; class 2: 0.6.
    max_det = 5 cuts inside class 0 and class 1 and falls on the 0.5 tie (the lower class stays)."""
    sc = [(0, 0.9), (0, 0.8), (0, 0.5), (0, 0.4), (1, 0.85), (1, 0.5), (1, 0.3), (2, 0.6)]
    box = np.array([[150.0 * i, 0, 150.0 * i + 100, 100] for i in range(len(sc))], F64)
    p = _to_pred(box, 3)
    p[:, 4] = 1.0
    for i, (c, s) in enumerate(sc):
        p[i, 5 + c] = s
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])               # box order is not score order
    return p[perm][None].astype(F32), 3, 0.25, 0.45


@functools.lru_cache(maxsize=None)
def make_wide_case(kind):
    """'wide': C = 252, rows of 257 floats: beyond the LDS-tiled count / fill kernels, the row-per-thread ones run.
    'overflow': C = 80, N = 1500 at conf 0.002: more candidates than the first buffer guess max(B * N / 2, 65536), so the
    call repeats with room after its host read.  -> (pred [2, N, 5 + C], C, conf, thre)"""
    C, N, conf = dict(wide=(252, 300, 0.3), overflow=(80, 1500, 0.002))[kind]
    rng = np.random.RandomState(5)
    p = np.zeros((2, N, 5 + C), F32)
    p[..., 0:2] = rng.uniform(50, 550, (2, N, 2))
    p[..., 2:4] = rng.uniform(10, 200, (2, N, 2))
    p[..., 4] = rng.uniform(0.05, 1.0, (2, N))
    p[..., 5:] = rng.uniform(0, 1, (2, N, C)) ** (2 if kind == 'overflow' else 6)
    return p, C, conf, 0.45
