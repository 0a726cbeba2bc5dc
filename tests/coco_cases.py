# -*- coding: utf-8 -*-
"""COCO bbox evaluation: the fp64 restatement the kernels of csrc/coco_eval.hip are compared with, and the cases.

The restatement is written in the ORIGINAL formulation of the protocol -- per (cell, area range, threshold) a single pass
over the gts stably sorted ignored-last with the early `break`, `searchsorted` for the recall thresholds, and one
separate matching per maxDets value on the detections cut to that many -- so the kernels (two side-by-side passes, one
run over 100 detections filtered by rank, a backward running-maximum scan) reach the same numbers by another route.
Plain loops; every intermediate is a Python float or a numpy fp64, i.e. IEEE double without fused multiply-add.

Acceptance: match codes, npig, precision and recall are compared with `array_equal` -- every output is an integer or one
correctly rounded fp64 quotient of integers -- and the hand values below hold within 1e-12.
"""
import functools

import numpy as np

IOU = np.linspace(.5, .95, 10)
REC = np.linspace(0, 1, 101)
AREA = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
MAXDETS = [1, 10, 100]
T, R, A, M = 10, 101, 4, 3
EPS = float(np.spacing(1))


def iou1(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    da = d[2] * d[3]
    ga = g[2] * g[3]
    u = da if crowd else da + ga - i
    return i / u


def _match_cell(d, g, ar, ious):
    """original evaluateImg: d = detections in rank order, g = gts in annotation order.  -> dtm, dig [T, nd] (matched,
    ignored), the gt ignore flags in annotation order and the number of matches to a crowd gt."""
    ig0 = [1 if (x.get('iscrowd', 0) or x['area'] < ar[0] or x['area'] > ar[1]) else 0 for x in g]
    order = [int(i) for i in np.argsort(np.array(ig0, dtype=np.int64), kind='mergesort')] if g else []
    ig = [ig0[i] for i in order]
    crowd = [int(g[i].get('iscrowd', 0)) for i in order]
    nd, ng = len(d), len(g)
    dtm = np.zeros((T, nd), np.int64)
    dig = np.zeros((T, nd), np.int64)
    ncrowd = 0
    for t in range(T):
        thr = float(IOU[t])
        gtm = [0] * ng
        for di in range(nd):
            row = ious[di]
            best = min(thr, 1 - 1e-10)
            m = -1
            for gi in range(ng):
                if gtm[gi] > 0 and not crowd[gi]:
                    continue
                if m > -1 and ig[m] == 0 and ig[gi] == 1:
                    break
                v = row[order[gi]]
                if v < best:
                    continue
                best = v
                m = gi
            if m == -1:
                continue
            dig[t, di] = ig[m]
            dtm[t, di] = 1
            gtm[m] = di + 1
            ncrowd += crowd[m]
    da = np.array([x['bbox'][2] * x['bbox'][3] for x in d], dtype=np.float64)
    out = ((da < ar[0]) | (da > ar[1])) if nd else np.zeros(0, bool)
    dig = dig | ((dtm == 0) & out[None, :])
    return dtm, dig, ig0, ncrowd


def evaluate(ann, records, image_ids):
    """-> dict: precision [T,R,K,A,M], recall [T,K,A,M], stats [12]; cells [(k, image index)], kept (record index of every
    kept detection, in cell order then rank), det_off, codes uint32 [A, n_kept] (2 bits per threshold), npig [n_cells, A];
    counters crowd_matches, ignored (codes 2 or 3), truncated (cells cut to 100) and minus_one (precision entries)."""
    img_ids = sorted(set(int(i) for i in image_ids))
    cat_ids = sorted(int(c['id']) for c in ann['categories'])
    known = set(int(i['id']) for i in ann['images'])
    for r in records:
        if int(r['image_id']) not in known:
            raise ValueError('unknown image id %r' % (r['image_id'],))
    K = len(cat_ids)
    gts_by, dts_by = {}, {}
    for x in ann['annotations']:
        gts_by.setdefault((x['category_id'], x['image_id']), []).append(x)
    for j, x in enumerate(records):
        dts_by.setdefault((x['category_id'], x['image_id']), []).append((j, x))
    prec = -np.ones((T, R, K, A, M))
    rec = -np.ones((T, K, A, M))
    cells, kept, det_off, codes, npig = [], [], [0], [[] for _ in range(A)], []
    crowd_matches = ignored = truncated = 0
    for k, c in enumerate(cat_ids):
        per = {(a, m): [] for a in range(A) for m in range(M)}
        for ii, im in enumerate(img_ids):
            g = gts_by.get((c, im), [])
            dj = dts_by.get((c, im), [])
            if not g and not dj:
                continue
            srt = np.argsort(np.array([-x['score'] for _, x in dj], dtype=np.float64), kind='mergesort')
            truncated += len(dj) > 100
            dj = [dj[int(i)] for i in srt][:100]
            d = [x for _, x in dj]
            ious = [[iou1(x['bbox'], y['bbox'], int(y.get('iscrowd', 0))) for y in g] for x in d]
            cells.append((k, ii))
            kept.extend(j for j, _ in dj)
            det_off.append(det_off[-1] + len(d))
            row = []
            for a, ar in enumerate(AREA):
                for m, md in enumerate(MAXDETS):                      # one separate matching per maxDets
                    dtm, dig, ig0, nc = _match_cell(d[:md], g, ar, ious[:md])
                    per[a, m].append((np.array([x['score'] for x in d[:md]], dtype=np.float64), dtm, dig, ig0))
                    if md == 100:
                        crowd_matches += nc
                        ignored += int(dig.sum())
                        cd = np.where(dtm != 0, np.where(dig != 0, 3, 1), np.where(dig != 0, 2, 0)).astype(np.uint32)
                        codes[a].extend(int(sum(int(cd[t, i]) << (2 * t) for t in range(T))) for i in range(len(d)))
                        row.append(ig0.count(0))
            npig.append(row)
        for a in range(A):
            for m in range(M):
                E = per[a, m]
                if not E:
                    continue
                sc = np.concatenate([e[0] for e in E])
                inds = np.argsort(-sc, kind='mergesort')
                dm = np.concatenate([e[1] for e in E], 1)[:, inds]
                di = np.concatenate([e[2] for e in E], 1)[:, inds]
                gi = np.array([v for e in E for v in e[3]], dtype=np.int64)
                n = int(np.count_nonzero(gi == 0))
                if n == 0:
                    continue
                tps = np.cumsum((dm != 0) & (di == 0), 1).astype(np.float64)
                fps = np.cumsum((dm == 0) & (di == 0), 1).astype(np.float64)
                for t in range(T):
                    tp, fp = tps[t], fps[t]
                    nd = len(tp)
                    rc = tp / n
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    q = np.zeros(R)
                    rec[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, REC, side='left')):
                        if pi < nd:
                            q[ri] = pr[pi]
                    prec[t, :, k, a, m] = q
    return {'precision': prec, 'recall': rec, 'stats': summarize(prec, rec), 'cells': cells,
            'kept': np.array(kept, dtype=np.int64), 'det_off': np.array(det_off, dtype=np.int32),
            'codes': np.array(codes, dtype=np.uint32).reshape(A, len(kept)),
            'npig': np.array(npig, dtype=np.int32).reshape(len(cells), A),
            'crowd_matches': crowd_matches, 'ignored': ignored, 'truncated': int(truncated),
            'minus_one': int((prec == -1).sum())}


def _mean(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(s.mean())


def summarize(prec, rec):
    ap = lambda t=None, a=0, m=2: _mean(prec[:, :, :, a, m] if t is None else prec[t:t + 1, :, :, a, m])   # noqa: E731
    ar = lambda a=0, m=2: _mean(rec[:, :, a, m])                                                         # noqa: E731
    return np.array([ap(), ap(0), ap(5), ap(None, 1), ap(None, 2), ap(None, 3),
                     ar(0, 0), ar(0, 1), ar(0, 2), ar(1), ar(2), ar(3)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ cases

def G(im, c, b, area=None, crowd=0):
    b = [float(v) for v in b]
    return dict(image_id=im, category_id=c, bbox=b, area=float(b[2] * b[3] if area is None else area), iscrowd=crowd)


def D(im, c, b, s):
    return dict(image_id=im, category_id=c, bbox=[float(v) for v in b], score=float(s), segmentation=[])


def case(name, gts, dts, image_ids, cats, images=None, **kw):
    images = sorted(set(image_ids) | set(g['image_id'] for g in gts)) if images is None else images
    ann = {'images': [{'id': i} for i in images], 'annotations': [dict(g, id=n + 1) for n, g in enumerate(gts)],
           'categories': [{'id': c} for c in cats]}
    return dict(kw, name=name, ann=ann, records=dts, image_ids=list(image_ids))


def _perfect():
    gts, dts = [], []
    for im in (1, 2, 3):
        for c, b in ((1, [5, 5, 20, 20]), (2, [50, 40, 60, 50]), (3, [10, 200, 150, 120])):     # small, medium, large
            b = [b[0] + im, b[1], b[2], b[3]]
            gts.append(G(im, c, b))
            dts.append(D(im, c, b, 0.5 + 0.1 * im))
    return case('perfect', gts, dts, [1, 2, 3], [1, 2, 3])


def _fp_above_tp():
    return case('fp_above_tp', [G(1, 1, [10, 10, 50, 50])],
                [D(1, 1, [200, 200, 50, 50], .9), D(1, 1, [10, 10, 50, 50], .8)], [1], [1])


def _half_found():
    return case('half_found', [G(1, 1, [0, 0, 100, 100]), G(1, 1, [300, 300, 100, 100])], [D(1, 1, [0, 0, 100, 62], .9)], [1], [1])


def _empty_sides():
    return case('empty_sides', [G(1, 1, [0, 0, 100, 100]), G(1, 3, [0, 0, 100, 100])],
                [D(1, 1, [0, 0, 100, 100], .9), D(1, 2, [0, 0, 10, 10], .9)], [1], [1, 2, 3])


def _crowd():
    return case('crowd', [G(1, 1, [0, 0, 100, 100], crowd=1), G(1, 1, [200, 0, 50, 50])],
                [D(1, 1, [10, 10, 20, 20], .9), D(1, 1, [40, 40, 20, 20], .8), D(1, 1, [200, 0, 50, 50], .7)], [1], [1])


def _area():
    # area fields that put a gt into another range than w*h would: 40x40 box with area 900 (small), 30x30 box with area
    # 1100 (medium), 100x100 box with area 9000 (medium), 90x90 box with area 9300 (large); exactly 32^2 and 96^2 are in both
    gts = [G(1, 1, [0, 0, 40, 40], area=900), G(1, 1, [100, 0, 30, 30], area=1100), G(1, 1, [0, 100, 100, 100], area=9000),
           G(1, 1, [200, 100, 90, 90], area=9300), G(2, 1, [0, 0, 32, 32], area=1024), G(2, 1, [100, 100, 96, 96], area=9216)]
    dts = [D(1, 1, [0, 0, 40, 40], .9), D(1, 1, [100, 0, 30, 30], .8), D(1, 1, [0, 100, 100, 100], .7),
           D(1, 1, [200, 100, 90, 90], .6), D(1, 1, [300, 300, 10, 10], .95), D(1, 1, [300, 0, 50, 50], .85),
           D(1, 1, [0, 300, 200, 200], .75), D(2, 1, [0, 0, 32, 32], .9), D(2, 1, [100, 100, 96, 96], .8),
           D(2, 1, [300, 300, 32, 32], .7), D(2, 1, [300, 0, 96, 96], .6)]
    return case('area', gts, dts, [1, 2], [1])


def _maxdets():
    rng = np.random.default_rng(5)
    gts = [G(1, 1, [10 * i, 0, 8, 8 + i]) for i in range(12)] + [G(2, 1, [0, 0, 30, 30])]
    dts = []
    for i in range(130):                                           # image 1: 130 detections in one cell
        j = i % 12
        dts.append(D(1, 1, [10 * j + float(rng.integers(-1, 2)), 0, 8, 8 + j], float(rng.integers(1, 64)) / 64))
    dts += [D(2, 1, [0, 0, 30, 30], .3), D(2, 1, [50, 50, 30, 30], .9)]
    return case('maxdets', gts, dts, [1, 2], [1])


def _ties():
    gts, dts = [], []
    # two gts at the same IoU from the detection: the later one is taken, so the second detection still finds the first
    gts += [G(1, 1, [0, 0, 100, 100]), G(1, 1, [20, 0, 100, 100])]
    dts += [D(1, 1, [10, 0, 100, 100], 12 / 16), D(1, 1, [0, 0, 100, 100], 8 / 16)]
    # IoU exactly iouThrs[j] (for every j where h = 100 * thr gives that quotient exactly; j = 0 always does)
    exact = []
    for j in range(T):
        h = float(IOU[j]) * 100
        if iou1([0, 0, 100, h], [0, 0, 100, 100], 0) == IOU[j]:
            exact.append(j)
            gts.append(G(2 + j, 1, [0, 0, 100, 100]))
            dts.append(D(2 + j, 1, [0, 0, 100, h], 8 / 16))
    # scores quantised to 1/16 over images 20..27, hits and misses mixed: ties are broken by image order
    rng = np.random.default_rng(11)
    for im in range(20, 28):
        for n in range(3):
            b = [40 * n, 0, 30, 30]
            gts.append(G(im, 1, b))
            dts.append(D(im, 1, [b[0] + float(rng.integers(0, 3)) * 6, 0, 30, 30], float(rng.integers(6, 10)) / 16))
            dts.append(D(im, 1, [40 * n, 100, 30, 30], float(rng.integers(6, 10)) / 16))
    ids = sorted(set(g['image_id'] for g in gts))
    return case('ties', gts, dts, ids, [1], exact=exact)


def _filters():
    gts = [G(1, 1, [0, 0, 50, 50]), G(2, 1, [0, 0, 50, 50]), G(4, 1, [0, 0, 50, 50]), G(1, 2, [60, 60, 40, 40])]
    dts = [D(1, 1, [0, 0, 50, 50], .9), D(2, 1, [0, 0, 50, 48], .8),
           D(4, 1, [0, 0, 50, 50], .99),                            # image 4 is in the file but not in image_ids
           D(1, 7, [0, 0, 50, 50], .99),                            # category 7 is not in categories
           D(1, 2, [60, 60, 40, 40], .7)]
    return case('filters', gts, dts, [1, 2, 3, 2], [1, 2], images=[1, 2, 3, 4],
                bad_records=dts + [D(99, 1, [0, 0, 5, 5], .5)])     # image 3: nothing; image 99: not in the file


def _grid_cell(name, n_gt, n_det, seed):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for i in range(n_gt):                                          # one cell, gts on a grid 20 wide
        x, y = 30 * (i % 20), 30 * (i // 20)
        gts.append(G(1, 1, [x, y, 24, 24], area=float(rng.choice([500, 576, 1500])), crowd=int(i % 37 == 5)))
    for i in rng.permutation(n_gt)[:n_det]:
        x, y = 30 * (int(i) % 20), 30 * (int(i) // 20)
        dts.append(D(1, 1, [x + float(rng.integers(0, 4)), y + float(rng.integers(0, 4)), 24, 24], float(rng.integers(1, 33)) / 32))
    return case(name, gts, dts, [1], [1])


def _many_gts():
    return _grid_cell('many_gts', 300, 100, 3)     # beyond the matched bits a block keeps on chip: the workspace


def _mid_gts():
    return _grid_cell('mid_gts', 150, 60, 4)       # several staged chunks of gts, matched bits still on chip


def _long_cat():
    rng = np.random.default_rng(9)
    gts, dts = [], []
    for im in range(1, 41):                                         # 40 images x 80 detections of one category
        for n in range(4):
            gts.append(G(im, 1, [60 * n, 0, 40, 40]))
        for n in range(80):
            if n < 4 and rng.random() < .8:
                b = [60 * n + float(rng.integers(0, 5)), float(rng.integers(0, 5)), 40, 40]
            else:
                b = [float(rng.integers(0, 300)), float(rng.integers(100, 300)), 40, 40]
            dts.append(D(im, 1, b, float(rng.integers(1, 1025)) / 1024))
    return case('long_cat', gts, dts, list(range(1, 41)), [1])


def _random(seed):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for im in range(1, 13):
        for c in range(1, 6):
            if rng.random() < .3:
                continue
            for _ in range(int(rng.integers(0, 31)) if rng.random() < .25 else int(rng.integers(0, 5))):
                x, y = rng.integers(0, 400, 2)
                w, h = rng.choice([8, 20, 40, 80, 120], 2)
                b = [float(x), float(y), float(w), float(h)]
                gts.append(G(im, c, b, area=float(w * h) * float(rng.choice([.5, 1.0])), crowd=int(rng.random() < .2)))
                for _ in range(int(rng.integers(0, 3))):
                    j = rng.integers(-3, 4, 4) * int(rng.choice([0, 1, 4]))
                    dts.append(D(im, c, [b[0] + j[0], b[1] + j[1], max(1., b[2] + j[2]), max(1., b[3] + j[3])],
                                 float(rng.integers(1, 17)) / 16))
            for _ in range(int(rng.integers(0, 4))):
                dts.append(D(im, c, [float(rng.integers(0, 400)), float(rng.integers(0, 400)), 30., 30.],
                             float(rng.integers(1, 17)) / 16))
    order = rng.permutation(len(dts))
    return case('random_%d' % seed, gts, [dts[int(i)] for i in order], list(range(1, 13)), [1, 2, 3, 4, 5])


CASES = [_perfect(), _fp_above_tp(), _half_found(), _empty_sides(), _crowd(), _area(), _maxdets(), _ties(), _filters(),
         _many_gts(), _mid_gts(), _long_cat(), _random(1), _random(2), _random(3)]
BY_NAME = {c['name']: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement on one case, computed once and shared (callers must not modify it)"""
    c = BY_NAME[name]
    return evaluate(c['ann'], c['records'], c['image_ids'])


def brute_cells(c):
    """(category index, image index) -> (gt annotation indices, record indices) by brute force, for the packing test"""
    img_ids = sorted(set(c['image_ids']))
    cat_ids = sorted(x['id'] for x in c['ann']['categories'])
    out = {}
    for k, cat in enumerate(cat_ids):
        for ii, im in enumerate(img_ids):
            g = [n for n, x in enumerate(c['ann']['annotations']) if x['image_id'] == im and x['category_id'] == cat]
            d = [n for n, x in enumerate(c['records']) if x['image_id'] == im and x['category_id'] == cat]
            if g or d:
                out[(k, ii)] = (g, d)
    return out
