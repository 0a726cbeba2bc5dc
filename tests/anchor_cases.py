# -*- coding: utf-8 -*-
"""NumPy restatement of the anchor-fitting kernels (csrc/anchors.hip) and of the loops of yolov4_amd/yolo/util/anchors.py,
and the cases tests/test_gpu_anchors.py runs through the C ABI (tests/test_anchor_cases.py shows without a GPU that every
case reaches the branch it is named for).

The IoU is float32 NumPy, one operation per line of the header's expression (NumPy fuses nothing), `argmax` for the first
maximum; the sums are int64 sums of np.rint(x.astype(float64) * 2**16) and * 2**30.  Nothing here imports the package."""
import functools

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64

# the launch shapes of csrc/anchors.hip (tests/test_anchor_cases.py compares them with the source)
ASSIGN_BLOCK, ASSIGN_GRID = 256, 512           # shapes per block and round; grid cap (blocks stride beyond it)
FIT_TILE, FIT_CHUNK, FIT_BLOCKS = 2048, 8, 8192   # shapes per tile; candidates per block; aimed-at blocks per launch


# -------------------------------------------------------------------------------------------------------- restatement
def iou_matrix(wh, anchors):
    """float32 [N, A]"""
    wh, anchors = np.asarray(wh, F32), np.asarray(anchors, F32)
    tw, th = wh[:, 0:1], wh[:, 1:2]
    aw, ah = anchors[None, :, 0], anchors[None, :, 1]
    brx = np.minimum(tw, aw)
    bry = np.minimum(th, ah)
    ai = brx * bry
    iou = ai / ((tw * th + aw * ah) - ai)
    assert iou.dtype == F32
    return iou


def q16(x):
    return np.rint(np.asarray(x, F32).astype(F64) * 2 ** 16).astype(I64)


def q30(x):
    return np.rint(np.asarray(x, F32).astype(F64) * 2 ** 30).astype(I64)


def assign(wh, anchors, iou_thresh):
    """-> (assign uint8 [N], best_iou float32 [N], acc int64 [A, 5])"""
    iou = iou_matrix(wh, anchors)
    n, a = iou.shape
    best = np.argmax(iou, axis=1)
    bi = iou[np.arange(n), best]
    hit = iou > F32(iou_thresh)
    hit[np.arange(n), best] = True
    acc = np.zeros((a, 5), I64)
    np.add.at(acc[:, 0], best, 1)
    np.add.at(acc[:, 1], best, q16(wh[:, 0]))
    np.add.at(acc[:, 2], best, q16(wh[:, 1]))
    np.add.at(acc[:, 3], best, q30(bi))
    acc[:, 4] = hit.sum(axis=0)
    return best.astype(np.uint8), bi, acc


def fitness(wh, cand, thr):
    """-> int64 [G, 2]"""
    cand = np.asarray(cand, F32)
    out = np.zeros((len(cand), 2), I64)
    if cand.shape[1] == 1:                               # one anchor per set: all sets at once, in slabs
        for g0 in range(0, len(cand), 1024):
            iou = iou_matrix(wh, cand[g0:g0 + 1024, 0])  # [N, g]
            out[g0:g0 + 1024, 0] = q30(iou).sum(axis=0)
            out[g0:g0 + 1024, 1] = (iou > F32(thr)).sum(axis=0)
        return out
    for g, anchors in enumerate(cand):
        bi = iou_matrix(wh, anchors).max(axis=1)
        out[g] = (q30(bi).sum(), (bi > F32(thr)).sum())
    return out


def sorted_order(anchors):
    a = np.asarray(anchors, F32).astype(F64)
    return np.lexsort((a[:, 0], a[:, 0] * a[:, 1]))


def mean_update(c, acc):
    new = c.copy()
    for a in range(len(c)):
        if acc[a, 0] > 0:
            d = F64(acc[a, 0]) * 2.0 ** 16
            new[a] = (F32(F64(acc[a, 1]) / d), F32(F64(acc[a, 2]) / d))
    return new


def lloyd(wh, c0, max_iter=300):
    """-> (centroids, final assignment, acc of the centroids, assignment passes)"""
    c, prev = np.asarray(c0, F32).copy(), None
    for it in range(1, max_iter + 1):
        asg, _, acc = assign(wh, c, 1.0)
        if prev is not None and np.array_equal(asg, prev):
            return c, asg, acc, it
        prev = asg
        c = mean_update(c, acc)
    asg, _, acc = assign(wh, c, 1.0)
    return c, asg, acc, max_iter


def kmeans(wh, k, init=None, n_init=8, max_iter=300, seed=0):
    """-> (anchors sorted, info) as yolov4_amd.yolo.util.anchors.kmeans_anchors documents it"""
    wh = np.asarray(wh, F32)
    if init is not None:
        starts = [np.asarray(init, F32)]
    else:
        uniq = np.unique(wh, axis=0)
        rng = np.random.Generator(np.random.PCG64(seed))
        starts = [uniq[rng.choice(len(uniq), size=k, replace=False)] for _ in range(n_init)]
    best = None
    for s, c0 in enumerate(starts):
        c, asg, acc, it = lloyd(wh, c0, max_iter)
        fit = int(acc[:, 3].sum())
        if best is None or fit > best[0]:
            best = (fit, c, asg, acc, it, s)
    fit, c, asg, acc, it, s = best
    o = sorted_order(c)
    return c[o], {'iterations': it, 'fitness': fit, 'counts': acc[o, 0].tolist(), 'start': s,
                  'mean_best_iou': fit / (len(wh) * 2.0 ** 30), 'assign': np.argsort(o)[asg]}


def evolve(wh, anchors, generations, population, sigma=0.1, mutate_prob=0.9, thr=0.213, seed=0, min_size=2.0):
    """-> (anchors sorted, the parent's fitness before the first generation and after each one)"""
    parent = np.asarray(anchors, F32).copy()
    k = len(parent)
    rng = np.random.Generator(np.random.PCG64(seed))
    fit = int(fitness(wh, parent[None], thr)[0, 0])
    track = [fit]
    top = np.nextafter(F32(65536), F32(0))
    for _ in range(generations):
        while True:
            normal = rng.standard_normal((population, k, 2))
            uniform = rng.random((population, k, 2))
            f = np.clip(1.0 + sigma * normal * (uniform < mutate_prob), 0.3, 3.0)
            if (f != 1.0).any():
                break
        cand = np.minimum(np.maximum(parent.astype(F64)[None] * f, min_size).astype(F32), top)
        out = fitness(wh, cand, thr)
        g = int(np.argmax(out[:, 0]))
        if int(out[g, 0]) > fit:
            parent, fit = cand[g], int(out[g, 0])
        track.append(fit)
    return parent[sorted_order(parent)], track


def report(wh, cfg, iou_thresh):
    anchors, masks = np.asarray(cfg['ANCHORS'], F32), cfg['ANCHOR_MASK']
    _, bi, acc = assign(wh, anchors, iou_thresh)
    n = len(wh)
    masked = sorted(set(a for m in masks for a in m))
    return {'n_labels': n, 'mean_best_iou': int(acc[:, 3].sum()) / (n * 2.0 ** 30), 'above_half': int((bi > F32(0.5)).sum()) / n,
            'above_thresh': int((bi > F32(iou_thresh)).sum()) / n, 'counts': acc[:, 0].tolist(),
            'positives': [int(acc[list(m), 4].sum()) for m in masks], 'unassigned': (n - int(acc[masked, 0].sum())) / n}


# -------------------------------------------------------------------------------------------------------------- data
def lognormal_shapes(n, seed, median=60.0, spread=0.8, lo=1.0, hi=600.0):
    rng = np.random.RandomState(seed)
    return np.clip(np.exp(rng.normal(np.log(median), spread, (n, 2))), lo, hi).astype(F32)


CLUSTER_CENTRES = [(8, 8), (16, 32), (48, 24), (64, 128), (256, 160), (400, 480)]


def cluster_shapes(seed=5):
    """six clusters of 40 + 7 i members, each its centre times a uniform factor in [0.9, 1.1] per axis, shuffled
    -> (wh, labels, init: the first drawn member of each cluster)"""
    rng = np.random.RandomState(seed)
    wh, lab, init = [], [], []
    for i, c in enumerate(CLUSTER_CENTRES):
        m = (np.array(c, F64)[None] * rng.uniform(0.9, 1.1, (40 + 7 * i, 2))).astype(F32)
        wh.append(m)
        lab += [i] * len(m)
        init.append(m[0])
    wh, lab = np.concatenate(wh), np.array(lab)
    p = rng.permutation(len(wh))
    return wh[p], lab[p], np.array(init, F32)


# -------------------------------------------------------------------------------------------------------------- cases
CASES = []


def case(name, wh, anchors, iou_thresh, cand, thr, reach):
    """wh [N,2]; the assignment pass runs with (anchors [A,2], iou_thresh), the fitness launch with (cand [G,A',2], thr);
    `reach` names what tests/test_anchor_cases.py shows the case to reach"""
    c = {'name': name, 'wh': np.ascontiguousarray(wh, F32), 'anchors': np.ascontiguousarray(anchors, F32),
         'iou_thresh': float(iou_thresh), 'cand': np.ascontiguousarray(cand, F32), 'thr': float(thr), 'reach': reach}
    assert c['wh'].ndim == 2 and c['anchors'].ndim == 2 and c['cand'].ndim == 3
    CASES.append(c)


def _mutants(anchors, g, seed):
    rng = np.random.RandomState(seed)
    f = np.clip(1.0 + 0.2 * rng.normal(size=(g,) + np.shape(anchors)), 0.3, 3.0)
    f[0] = 1.0                                          # candidate 0 is the set itself
    return (np.asarray(anchors, F64)[None] * f).astype(F32)


def _build():
    sizes = [(1, 'n1'), (63, 'n63'), (64, 'n64'), (65, 'n65'), (ASSIGN_BLOCK - 1, 'n255'), (ASSIGN_BLOCK, 'n256'),
             (ASSIGN_BLOCK + 1, 'n257'), (3 * ASSIGN_BLOCK + 7, 'n775'), (FIT_TILE - 1, 'n2047'), (FIT_TILE, 'n2048'),
             (FIT_TILE + 1, 'n2049'), (3 * FIT_TILE + 7, 'n6151')]
    a_of = [1, 6, 9, 32]
    g_of = [1, 2, FIT_CHUNK + 1]
    for j, (n, nm) in enumerate(sizes):
        a, g = a_of[j % 4], g_of[j % 3]
        wh = lognormal_shapes(n, 100 + j)
        anchors = lognormal_shapes(a, 200 + j, spread=1.0)
        case('%s_a%d_g%d' % (nm, a, g), wh, anchors, 0.213 if j % 2 else 1.0, _mutants(anchors, g, 300 + j), 0.213,
             {'n': n, 'a': a, 'g': g})
    # A = 32 and A = 1 at more than one block; G one more than the chunk with A = 32 (the LDS table full)
    wh = lognormal_shapes(777, 1)
    a32 = lognormal_shapes(32, 2, spread=1.0)
    case('a32_full_chunk', wh, a32, 0.213, _mutants(a32, FIT_CHUNK + 1, 3), 0.3, {'a': 32, 'g': FIT_CHUNK + 1, 'multi': True})
    case('a1', wh, [[50, 70]], 1.0, _mutants([[50, 70]], 2 * FIT_CHUNK + 3, 4), 0.5, {'a': 1, 'g': 2 * FIT_CHUNK + 3})
    # two identical anchors: the lower index takes every shape both are best for
    twins = [[30, 40], [90, 60], [30, 40], [200, 300]]
    case('identical_anchors', lognormal_shapes(500, 5), twins, 0.213, _mutants(twins, 3, 6), 0.213, {'twins': (0, 2)})
    # (4, 4) against (2, 4), (4, 2) and (8, 4): three different anchors, IoU 0.5 each, exactly; thr = 0.5 is that shape's best
    tie_a = [[2, 4], [4, 2], [8, 4], [100, 100]]
    tie_wh = np.concatenate([[[4, 4]], lognormal_shapes(70, 7), [[4, 4], [8, 8], [2, 2]]])
    case('equal_iou_two_anchors', tie_wh, tie_a, 0.5, _mutants(tie_a, 2, 8), 0.5, {'tie_row': 0, 'strict': True})
    # 0.5 px and 65535 px side by side
    ext_wh = [[0.5, 0.5], [65535, 65535], [0.5, 65535], [65535, 0.5], [1, 1], [300, 200], [65535, 65535]]
    ext_a = [[0.5, 0.5], [65535, 65535], [700, 0.75], [16, 16]]
    case('extremes', ext_wh, ext_a, 1.0, np.array([ext_a, ext_a[::-1], [[1, 1], [2, 2], [65535, 1], [40000, 65535]]], F32), 0.213,
         {'extremes': True})
    # an anchor no shape chooses
    case('empty_cluster', lognormal_shapes(300, 9, lo=20, hi=200), [[30, 30], [5000, 3], [120, 90]], 1.0,
         _mutants([[30, 30], [5000, 3], [120, 90]], 2, 10), 0.213, {'empty': 1})
    # iou_thresh low enough that anchors beside the best one hit
    a9 = [[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]
    case('multi_hits', lognormal_shapes(1000, 11), a9, 0.213, _mutants(a9, 4, 12), 0.213, {'multi': True})
    # more shapes than one round of the capped grid of the assignment pass
    n = ASSIGN_GRID * ASSIGN_BLOCK + 300
    case('two_rounds', lognormal_shapes(n, 13), a9, 1.0, _mutants(a9, 2, 14), 0.213, {'rounds': 2})
    # the largest G: one anchor per set, more tiles than blocks along x (blocks stride over the tiles)
    g = 65535
    one = np.exp(np.random.RandomState(15).uniform(np.log(4), np.log(400), (g, 1, 2))).astype(F32)
    case('g_max_strided_tiles', lognormal_shapes(FIT_TILE + 7, 16), [[60, 60]], 1.0, one, 0.3, {'g': g, 'stride': True})


_build()
BY_NAME = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per process; callers do not modify it"""
    c = BY_NAME[name]
    asg, bi, acc = assign(c['wh'], c['anchors'], c['iou_thresh'])
    return {'assign': asg, 'best_iou': bi, 'acc': acc, 'out': fitness(c['wh'], c['cand'], c['thr'])}
