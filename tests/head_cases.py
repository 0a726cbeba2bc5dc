# -*- coding: utf-8 -*-
"""Shared references and seeded inputs for the direct tests of the head, loss, IoU and NMS kernels
(tests/test_head_cases.py checks them with the oracle alone, tests/test_gpu_head_edges.py feeds them to the kernels).

Plain module, no fixtures.  Every builder returns its inputs plus a dict of the properties the case exists for
(candidates per segment, survivors, sorted positions of a suppression chain, ...), computed with `oracle.head`:
test_head_cases.py asserts them, so that a GPU test cannot pass by missing the branch it was written for.
"""
import copy

import numpy as np

import recipe
from oracle import head as H

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -126                       # smallest normal fp32: a result flushed to zero is off by less than this
STRIDES = (8, 16, 32)

# ------------------------------------------------------------------------------------------ decode: cases
# (C, A, F, B, ldl).  nt = A * (5 + C) logit columns per pixel, ldl = pitch of a pixel row in floats.  The launcher
# takes the tiled kernel when ldl is a multiple of 4 and >= nt rounded up to 4 (and nt <= 256, A <= 4); the
# per-channel kernel otherwise.  Tiles are 16 pixels (32 from 100000 pixels on).
DECODE_CASES = [
    (80, 3, 19, 2, 256),        # the model's shape: nt = 255 + one pad column; FF = 361 = 22 tiles + a ragged one of 9
    (80, 3, 19, 2, 255),        # same logits, dense pitch: per-channel kernel
    (1, 3, 4, 3, 20),           # nt = 18, two pad columns; FF = 16, exactly one tile
    (1, 3, 4, 3, 32),           # nt = 18 under a pitch of 32
    (20, 3, 3, 2, 76),          # nt = 75, one pad column; FF = 9 < one tile
    (20, 3, 3, 2, 75),          # dense: per-channel kernel
    (59, 4, 1, 5, 256),         # nt = 256 = the whole LDS row, no pad column, A = 4; FF = 1
    (6, 1, 4, 2, 12),           # A = 1, nt = 11
    (6, 1, 19, 1, 11),          # A = 1, dense: per-channel kernel
    (1, 3, 100, 10, 20),        # 100000 pixels: the 32-pixel tile; FF = 10000 = 312 tiles + a ragged one of 16
]
PLANT = (12.0, 17.0, 30.0, 60.0, 80.0)          # +- each on every channel role
PLANT_FEW = (100.0, 1e4)                        # +- each on a few cells


def decode_takes_tiled(C, A, ldl):
    """The host-side dispatch condition of the decode launchers, for 16-byte aligned buffers."""
    nt = A * (5 + C)
    return nt <= 256 and A <= 4 and ldl % 4 == 0 and ldl >= (nt + 3) // 4 * 4


def decode_tile(B, F):
    return 32 if B * F * F >= 100000 else 16


def decode_anchors(A, seed):
    """A anchors (w, h) in grid units as exact fp32 values, the form the C ABI takes."""
    rng = np.random.RandomState(seed)
    return rng.uniform(0.4, 14.0, (A, 2)).astype(F32)


def roles(C):
    """channel index of every role: x, y, w, h, objectness, first and last class"""
    return sorted({0, 1, 2, 3, 4, 5, 4 + C})


def make_logits(B, F, A, C, ldl, seed):
    """[B*F*F, ldl] fp32 pixel rows: N(0, sd = 2) logits, +-PLANT on every channel role of every anchor, +-PLANT_FEW
    on a few cells, NaN in the pad columns (no kernel may let a pad column reach a result).  The content of the
    nt = A * (5 + C) real columns depends on the seed only, not on ldl."""
    n_ch = 5 + C
    nt = A * n_ch
    npix = B * F * F
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((npix, nt)) * 2.0).astype(F32)
    for a in range(A):
        for ch in roles(C):
            for k, mag in enumerate(PLANT):
                for s, sign in enumerate((1.0, -1.0)):
                    x[(7 * (2 * k + s) + 3 * a + ch) % npix, a * n_ch + ch] = sign * mag
    m = 0
    for mag in PLANT_FEW:
        for sign in (1.0, -1.0):
            for ch in (0, 2, 4, 4 + C):                     # a sigmoid + offset, an exp, and two plain sigmoid channels
                p, col = (11 + 5 * m) % npix, (m % A) * n_ch + ch
                for _ in range(npix):                       # the next cell of the column that holds no planted value
                    if abs(x[p, col]) < 12.0:
                        break
                    p = (p + 1) % npix
                x[p, col] = sign * mag
                m += 1
    full = np.full((npix, ldl), np.nan, dtype=F32)
    full[:, :nt] = x
    planted = {}
    v = x.reshape(npix, A, n_ch)
    for ch in roles(C):
        col = v[:, :, ch]
        planted[ch] = sorted(set(float(t) for t in col[np.abs(col) >= 12.0].ravel()))
    return full, dict(planted=planted, npix=npix, nt=nt, tiled=decode_takes_tiled(C, A, ldl), tile=decode_tile(B, F),
                      ragged=(F * F) % decode_tile(B, F))


def logit_view(logits_nhwc, ldl, B, F, A, C):
    """The logit of every result element: [B, A, F, F, 5 + C] (fp32) view of the pixel rows."""
    n_ch = 5 + C
    lg = np.asarray(logits_nhwc, dtype=F32).reshape(B, F, F, ldl)[..., :A * n_ch]
    return lg.reshape(B, F, F, A, n_ch).transpose(0, 3, 1, 2, 4)


def _sig64(v):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-v))


def decode_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, stride, train):
    """yolo/model/yololayer.py:88-166 in float64 on the fp32 logits [B*F*F, ldl] (pixel rows, channel a*(5+C)+ch).
    train -> (output [B,A,F,F,5+C] with raw w / h logits, pred [B,A,F,F,4] in grid units);
    eval  -> [B, A*F*F, 5+C] in input pixels, box index a*F*F + j*F + i.  exp() past the fp64 range gives inf."""
    n_ch = 5 + C
    v = logit_view(logits_nhwc, ldl, B, F, A, C).astype(np.float64)
    anc = np.asarray(anchors_wh, dtype=np.float64).reshape(A, 2)
    out = v.copy()
    sig = np.r_[0:2, 4:n_ch]
    out[..., sig] = _sig64(v[..., sig])
    pred = out.copy()
    pred[..., 0] += np.arange(F, dtype=np.float64).reshape(1, 1, 1, F)
    pred[..., 1] += np.arange(F, dtype=np.float64).reshape(1, 1, F, 1)
    with np.errstate(over='ignore'):
        pred[..., 2] = np.exp(v[..., 2]) * anc[:, 0].reshape(1, A, 1, 1)
        pred[..., 3] = np.exp(v[..., 3]) * anc[:, 1].reshape(1, A, 1, 1)
    if train:
        return out, pred[..., :4].copy()
    pred[..., :4] *= float(stride)
    return pred.reshape(B, A * F * F, n_ch)


def decode_bwd_ref64(logits_nhwc, ldl, B, F, A, C, anchors_wh, g_output, g_pred):
    """Train-mode backward in float64: (g_logits [B*F*F, ldl], S [B*F*F, ldl]); either gradient may be None.

    g = g_output + d(pred)/d(output) * g_pred, times (1 - o) * o on the sigmoid channels; pad columns are 0.
    S is the sum of the absolute values of the addends of the fully expanded expression: with G = sum |addends of g|,
    S = G on the w / h channels and S = G * (1 + o) * o on the sigmoid channels -- (1 - o) is itself a difference of the
    addends 1 and o, which is what makes an fp32 sigmoid derivative ill-conditioned near o = 1: an error of a few ulp
    in o is an error of a few 2^-24 in (1 - o), however small (1 - o) is.  c * 2^-23 * S therefore bounds what c ulp
    of error in o, exp() and the products can do to the result."""
    n_ch = 5 + C
    nt = A * n_ch
    v = logit_view(logits_nhwc, ldl, B, F, A, C).astype(np.float64)
    anc = np.asarray(anchors_wh, dtype=np.float64).reshape(A, 2)
    g = np.zeros_like(v)
    G = np.zeros_like(v)
    if g_output is not None:
        go = np.asarray(g_output, dtype=np.float64).reshape(v.shape)
        g += go
        G += np.abs(go)
    if g_pred is not None:
        gp = np.asarray(g_pred, dtype=np.float64).reshape(v.shape[:-1] + (4,))
        with np.errstate(over='ignore'):
            fac = np.ones_like(gp)
            fac[..., 2] = np.exp(v[..., 2]) * anc[:, 0].reshape(1, A, 1, 1)
            fac[..., 3] = np.exp(v[..., 3]) * anc[:, 1].reshape(1, A, 1, 1)
        g[..., :4] += gp * fac
        G[..., :4] += np.abs(gp * fac)
    sig = np.r_[0:2, 4:n_ch]
    o = _sig64(v[..., sig])
    g[..., sig] *= (1.0 - o) * o
    G[..., sig] *= (1.0 + o) * o
    gl = np.zeros((B * F * F, ldl), dtype=np.float64)
    S = np.zeros((B * F * F, ldl), dtype=np.float64)
    gl[:, :nt] = g.transpose(0, 2, 3, 1, 4).reshape(B * F * F, nt)
    S[:, :nt] = G.transpose(0, 2, 3, 1, 4).reshape(B * F * F, nt)
    return gl, S


def to_f32_range(ref64):
    """What an exact result becomes in fp32 range terms: beyond FLT_MAX it is an infinity."""
    r = np.array(ref64, dtype=np.float64)
    r[r > FLT_MAX] = np.inf
    r[r < -FLT_MAX] = -np.inf
    return r


DEC_CONST = 8.0                          # measured on an MI355X over DECODE_CASES: 1.10 is the largest constant needed


def decode_accept(got, ref64, v, const=DEC_CONST):
    """Per-element acceptance of a decode result: boolean array, True where ANY of
         |got - ref| <= (|v| + const) * 2^-23 * |ref|      (v: the element's logit)
         |got - ref| <= 2^-126                              (a result flushed to zero)
         both are +inf
    holds.  fp32 rounding of v * log2(e) costs |v| * 2^-24 relative after the exponential; the exponential, the
    reciprocal, the anchor and stride products and the final add cost a few ulp; const = 8 is about twice that.  NaN
    never passes."""
    got = np.asarray(got, dtype=np.float64)
    ref = to_f32_range(ref64)
    av = np.abs(np.asarray(v, dtype=np.float64))
    with np.errstate(invalid='ignore', over='ignore'):
        err = np.abs(got - ref)
        ok = np.isfinite(ref) & (err <= (av + const) * 2.0 ** -23 * np.abs(ref))
        ok |= err <= TINY
    ok |= np.isposinf(got) & np.isposinf(ref)
    ok &= ~np.isnan(got)
    return ok


BWD_CONST = 16.0                         # measured on an MI355X over DECODE_CASES: 1.74 is the largest constant needed


def decode_bwd_accept(got, ref64, S, const=BWD_CONST):
    """|got - ref| <= const * 2^-23 * S, or <= 2^-126, or the same infinity on both sides."""
    got = np.asarray(got, dtype=np.float64)
    ref = to_f32_range(ref64)
    with np.errstate(invalid='ignore', over='ignore'):
        err = np.abs(got - ref)
        ok = np.isfinite(ref) & (err <= const * 2.0 ** -23 * np.minimum(S, FLT_MAX))
        ok |= err <= TINY
    ok |= np.isinf(got) & (got == ref)
    ok &= ~np.isnan(got)
    return ok


def eval_run_phases(B, F, A, C, n_total, box_off):
    """Set of (float offset mod 4) at which the tiled eval decode starts a run, for a 16-byte aligned buffer."""
    n_ch = 5 + C
    tp = decode_tile(B, F)
    ph = set()
    for b in range(B):
        for a in range(A):
            for p0 in range(0, F * F, tp):
                ph.add(((b * n_total + box_off + a * F * F + p0) * n_ch) % 4)
    return ph


def close(a, b, atol=1e-4, rtol=1e-4, scale=True):
    """The project's parity check (tests/test_gpu_parity.py): atol is scaled by the reference's range."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = max(1.0, float(np.abs(b).max())) if scale else 1.0
    np.testing.assert_allclose(a, b, atol=atol * s, rtol=rtol)


# ------------------------------------------------------------------------------------------ loss: cases
LOSS_B, LOSS_IMG, LOSS_F = 3, 128, (16, 8, 4)
LOSS_CLASSES = (1, 32, 33, 64, 65)              # bitmask word boundaries: cw = 1, 1, 2, 2, 3
LOSS_K = (1, 64, 65, 100)                       # 64: last wave-kernel size; 65, 100: the one-thread-per-image kernel


def cfg_with_classes(C):
    cfg = copy.deepcopy(recipe.MODEL_CFG)
    cfg['N_CLASSES'] = C
    return cfg


def make_labels(K, C, seed):
    """[3, K, 5] float64 label rows (xc, yc, w, h, cls) for a 128-px image, valid rows first as the data pipeline emits
    them -- except where a case wants otherwise:
      image 0: every one of the K rows valid (n == K); its last label has the last class;
      image 1: a zero row BETWEEN valid rows (the count n then cuts the last valid row off and keeps the zero row),
               and pairs of labels on one cell and anchor with different classes (the first and the last class);
      image 2: two labels, or none when K < 2.
    One pair per layer: sizes near anchors 0, 4 and 6."""
    rng = np.random.RandomState(seed)
    lab = np.zeros((LOSS_B, K, 5), dtype=np.float64)

    def rand_rows(n):
        r = np.zeros((n, 5))
        r[:, 0:2] = rng.uniform(2.0, 126.0, (n, 2))
        r[:, 2:4] = np.exp(rng.uniform(np.log(6.0), np.log(200.0), (n, 2)))
        r[:, 4] = rng.randint(0, C, n)
        return r

    lab[0] = rand_rows(K)
    lab[0, K - 1, 4] = C - 1
    if K >= 8:
        rows = [r for (x, w, h) in ((40.5, 12.0, 16.0), (72.5, 76.0, 55.0), (104.5, 142.0, 110.0))
                for r in ([x, x, w, h, C - 1], [x + 1.0, x + 1.0, w, h, 0.0])]
        n1 = min(K, 20)
        lab[1, :n1] = rand_rows(n1)
        lab[1, :6] = np.array(rows)
        lab[1, 6] = 0.0                                     # the zero row, valid rows on both sides
        lab[2, :2] = rand_rows(2)
    elif K >= 2:
        lab[2, :2] = rand_rows(2)
    return lab, label_props(lab, C)


def label_props(lab, C):
    B, K, _ = lab.shape
    cfg = cfg_with_classes(C)
    l32 = lab.astype(F32)
    n = (l32.sum(axis=2, dtype=F32) > 0).sum(axis=1)
    valid = l32.sum(axis=2, dtype=F32) > 0
    zero_between = False
    for b in range(B):
        idx = np.nonzero(valid[b])[0]
        if len(idx) >= 2 and not valid[b, idx[0]:idx[-1]].all():
            zero_between = True
    two_classes = 0
    last_word = False
    positives = 0
    for l, Fs in enumerate(LOSS_F):
        out = np.full((B, 3, Fs, Fs, 5 + C), 0.5, F32)
        pred = np.ones((B, 3, Fs, Fs, 4), F32)
        tgt, _, tm, _ = H.build_target(out, pred, l, lab, cfg, 0.7)
        ncls = tgt[..., 5:].sum(axis=-1)
        two_classes += int((ncls >= 2).sum())
        last_word |= bool(tgt[..., 5 + 32 * ((C - 1) // 32):].any())
        positives += int(tm[..., 0].sum())
    return dict(n=[int(t) for t in n], n_eq_K=bool((n == K).any()), zero_row_between=zero_between,
                cells_with_two_classes=two_classes, class_in_last_word=last_word, positives=positives)


def make_loss_logits(C, seed, labels=None, saturate=False):
    """Head logits [3, 3 * (5 + C), F, F] for the three layers (the recipe's law).  saturate: +-30 planted on the
    objectness, class and xy channels of positive cells (found with the oracle) and of background cells."""
    n_ch = 5 + C
    cfg = cfg_with_classes(C)
    out = []
    props = dict(planted_positive=0, planted_background=0)
    for l, Fs in enumerate(LOSS_F):
        lg = recipe.synth_head_logits(LOSS_B, Fs, seed + 2 * l, n_ch=3 * n_ch).numpy().copy()
        if saturate:
            o, p = H.yolo_decode(lg, l, cfg, True)
            _, _, tm, _ = H.build_target(o, p, l, labels, cfg, 0.7)
            v = lg.reshape(LOSS_B, 3, n_ch, Fs, Fs)
            pos = np.argwhere(tm[..., 0] > 0)
            neg = np.argwhere(tm[..., 0] == 0)
            for which, cells in (('planted_positive', pos), ('planted_background', neg[::max(1, len(neg) // 12)])):
                for q, (b, a, j, i) in enumerate(cells):
                    sign = 30.0 if q % 2 == 0 else -30.0
                    chans = ((0, 4, 5), (1, 4 + C), (4, 0), (5, 1))[q % 4]
                    for t, ch in enumerate(chans):
                        v[b, a, ch, j, i] = sign if t % 2 == 0 else -sign
                    props[which] += 1
        out.append(lg)
    return out, props


# ------------------------------------------------------------------------------------------ IoU: cases
IOU_SHAPES = ((1, 1), (15, 17), (257, 1), (5, 4097))        # Na * Nb = 1, 255, 257, 5 * 4097


def make_iou_boxes(Na, Nb, seed):
    """Two box sets on a coarse integer lattice (so that touching, nested and identical pairs are common), with
    zero-area boxes and boxes holding NaN.  The same arrays serve as xyxy corners and as centre / size."""
    rng = np.random.RandomState(seed)

    def boxes(n):
        x1 = rng.randint(0, 6, n).astype(F32) * 4
        y1 = rng.randint(0, 6, n).astype(F32) * 4
        w = rng.randint(0, 4, n).astype(F32) * 4            # 0: zero area
        h = rng.randint(1, 4, n).astype(F32) * 4
        return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(F32)

    a, b = boxes(Na), boxes(Nb)
    if Na * Nb == 1:
        b[0] = a[0] = np.array([4, 4, 12, 16], F32)         # the one pair: identical boxes
    else:
        b[0] = a[0]                                         # identical
        b[-1] = np.array([a[0, 2], a[0, 1], a[0, 2] + 4, a[0, 3]], F32)        # touches a[0] on its right edge
        a[-1, rng.randint(0, 4)] = np.nan
        if Nb > 2:
            b[1, 2] = np.nan
        if Na > 2:
            a[1] = np.array([0, 0, 24, 24], F32)            # everything of b nests in it
            a[2] = np.array([8, 8, 8, 8], F32)              # a point
    fa, fb = np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0)
    A_, B_ = fa[:, None, :], fb[None, :, :]
    nested = ((A_[..., 0] <= B_[..., 0]) & (A_[..., 1] <= B_[..., 1]) & (A_[..., 2] >= B_[..., 2]) & (A_[..., 3] >= B_[..., 3]))
    touching = (A_[..., 2] == B_[..., 0]) | (A_[..., 0] == B_[..., 2]) | (A_[..., 3] == B_[..., 1]) | (A_[..., 1] == B_[..., 3])
    props = dict(identical=int((A_ == B_).all(-1).sum()), nested=int(nested.sum()), touching=int(touching.sum()),
                 zero_area=int((fa[:, 0] == fa[:, 2]).sum() + (fb[:, 0] == fb[:, 2]).sum()),
                 nan_boxes=int(np.isnan(a).any(1).sum() + np.isnan(b).any(1).sum()))
    return a, b, props


# ------------------------------------------------------------------------------------------ NMS: cases
def nms_props(box, score, thresh, limit=None):
    """What the oracle's greedy NMS does on this input, in terms of SORTED positions (256 per chunk in the kernel)."""
    box = np.asarray(box, F32)
    R = len(box)
    order = np.argsort(-np.asarray(score, F32), kind='stable') if score is not None else np.arange(R)
    keep_all = H.nms(box, thresh, score=score)
    keep = H.nms(box, thresh, score=score, limit=limit)
    pos_of = np.empty(R, np.int64)
    pos_of[order] = np.arange(R)
    kept_pos = np.sort(pos_of[keep_all])                    # sorted positions of the survivors, ascending = kept rank
    sb = box[order]
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = H.bboxes_iou(sb, sb[kept_pos], True)          # [candidate position, kept rank]
    is_kept = np.zeros(R, bool)
    is_kept[kept_pos] = True
    cross256 = second_trip = 0
    for p in np.nonzero(~is_kept)[0]:
        sup = np.nonzero((iou[p] >= F32(thresh)) & (kept_pos < p))[0]      # kept ranks that suppress p
        if len(sup) == 0:
            continue
        if p >= 256 and kept_pos[sup].max() <= 255:
            cross256 += 1                                   # only boxes of the first chunk suppress it
        if sup.min() >= 256 and kept_pos[sup].max() // 256 < p // 256:
            second_trip += 1                                # only kept boxes of rank >= 256, from earlier chunks
    sc = np.asarray(score, F32) if score is not None else np.zeros(0, F32)
    _, cnt = np.unique(sc, return_counts=True) if len(sc) else (None, np.zeros(1, int))
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    return dict(R=R, survivors=int(len(keep_all)), kept_with_limit=int(len(keep)), cross256=cross256,
                second_trip=second_trip, iou_eq_thresh=int((iou == F32(thresh)).sum()),
                zero_area=int((area == 0).sum()), max_tie_group=int(cnt.max()),
                limit_pos=int(kept_pos[limit - 1]) if limit and limit <= len(kept_pos) else None)


def make_nms_grid(seed=3, n_base=600):
    """The many-survivor case, thresh 0.5: n_base disjoint 10 x 10 boxes on a 20-px lattice with distinct descending
    scores (all survive: more than 512 survivors, three staging trips of kept boxes), and below them in score
      * shifted copies (IoU 81 / 119) of base boxes of kept rank 5, 300 and 550: suppressed by a kept box of the first
        chunk / of the second staging trip / of the third;
      * boxes nested in a base box with IoU exactly 0.5 = the threshold (suppressed: >=);
      * zero-area boxes, two of them identical (their IoU is 0 / 0: kept);
      * three groups of equal scores;
      * 120 random boxes with scores spread over the whole range."""
    rng = np.random.RandomState(seed)
    side = 25
    base = np.array([[20.0 * (k % side), 20.0 * (k // side), 20.0 * (k % side) + 10, 20.0 * (k // side) + 10]
                     for k in range(n_base)], F32)
    bs = np.linspace(0.99, 0.40, n_base).astype(F32)
    extra, es = [], []
    for r in (5, 300, 550, 7, 301, 551):
        extra.append(base[r] + F32(1.0)); es.append(0.2 + 0.0001 * r)
    for r in (9, 310):
        b = base[r].copy(); b[3] = b[1] + 5.0               # 10 x 5 inside 10 x 10: 50 / (100 + 50 - 50) = 0.5
        extra.append(b); es.append(0.19)
    for b in ([3.0, 3.0, 3.0, 9.0], [3.0, 3.0, 3.0, 9.0], [30.0, 30.0, 40.0, 30.0]):
        extra.append(np.array(b, F32)); es.append(0.18)
    rb = np.zeros((120, 4), F32)
    rb[:, 0:2] = rng.uniform(0, 480, (120, 2))
    rb[:, 2:4] = rb[:, 0:2] + rng.uniform(6, 16, (120, 2))
    rs = rng.uniform(0.1, 1.0, 120).astype(F32)
    rs[:3] = 0.5; rs[3:7] = 0.75
    box = np.concatenate([base, np.array(extra, F32), rb], 0).astype(F32)
    score = np.concatenate([bs, np.array(es, F32), rs]).astype(F32)
    perm = rng.permutation(len(box))                        # index order must not be score order
    return box[perm], score[perm], 0.5


def make_nms_clusters(R, seed):
    """R clustered boxes with scores on a 0.01 lattice (many ties), thresh 0.45."""
    rng = np.random.RandomState(seed)
    nc = max(1, R // 6)
    cx, cy = rng.uniform(40, 560, nc), rng.uniform(40, 560, nc)
    cw, ch = rng.uniform(20, 120, nc), rng.uniform(20, 120, nc)
    k = rng.randint(0, nc, R)
    x = cx[k] + rng.normal(0, 5, R); y = cy[k] + rng.normal(0, 5, R)
    w = cw[k] * np.exp(rng.normal(0, 0.12, R)); h = ch[k] * np.exp(rng.normal(0, 0.12, R))
    box = np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2], 1).astype(F32)
    score = (np.round(rng.uniform(0.05, 1.0, R), 2)).astype(F32)
    return box, score, 0.45


NMS_SIZES = (1, 255, 256, 257, 513)
NMS_LIMIT = 300


# ------------------------------------------------------------------------------------------ postprocess: cases
def post_props(pred, C, conf, nms_thre):
    """Candidates and survivors per (image, class) segment, with the oracle's formulas."""
    p = np.asarray(pred, F32)
    B, N, _ = p.shape
    sc = p[:, :, 5:5 + C] * p[:, :, 4:5]
    cand = (sc >= F32(conf)).sum(axis=1)                    # [B, C]
    pc = p.copy()
    out = H.postprocess(pc, C, conf, nms_thre)              # pc[:, :, :4] is xyxy afterwards
    surv = np.zeros((B, C), np.int64)
    for b in range(B):
        if out[b] is not None:
            for c in range(C):
                surv[b, c] = int((out[b][:, 6] == c).sum())
    rows = (sc >= F32(conf)).any(axis=2).reshape(-1)        # candidate rows, flat over [B * N]
    img_of_row = np.arange(B * N) // N
    first_tile = rows[:64]
    return dict(cand=cand, surv=surv, max_cand=int(cand.max()), max_surv=int(surv.max()),
                images_in_first_tile=int(img_of_row[:64].max()) + 1,
                cand_rows_third_image_on=int(first_tile[img_of_row[:64] >= 2].sum()),
                images_with_candidates=[bool(cand[b].sum()) for b in range(B)], ref=out, xyxy=pc[:, :, :4].copy())


def _grid_pred(rng, B, N, C, img=1400.0):
    p = np.zeros((B, N, 5 + C), F32)
    p[..., 0:2] = rng.uniform(20, img, (B, N, 2))
    p[..., 2:4] = rng.uniform(8, 60, (B, N, 2))
    p[..., 4] = rng.uniform(0.3, 1.0, (B, N))
    p[..., 5:] = rng.uniform(0.0, 1.0, (B, N, C))
    return p


def make_post_case(kind, seed=11):
    """(pred [B, N, 5 + C] fp32 in centre / size form, C, conf_thre, nms_thre, props)
      'big'        C = 2, N = 3000: image 0 / class 0 holds > 2048 candidates (the sort runs in global memory) of which
                   > 512 survive (small boxes spread over a large image);
      'four'       B = 5, N = 20: the first 64-row tile holds images 0..3;
      'n63' 'n64' 'n65'   B = 3, C = 4, N around the tile height;
      'c1'         one class;
      'last'       B = 3, C = 5: image 0 has candidates in its last class only, image 1 none, image 2 some."""
    rng = np.random.RandomState(seed)
    conf, thre = 0.25, 0.45
    if kind == 'big':
        B, N, C = 2, 3000, 2
        p = _grid_pred(rng, B, N, C)
        p[0, :, 5] = rng.uniform(0.85, 1.0, N)              # image 0, class 0: score >= 0.3 * 0.85 everywhere
        p[..., 6] *= 0.3
        p[1, :, 5] *= 0.5
        p[0, 100:104, 4] = 0.5; p[0, 100:104, 5] = 0.9       # four equal scores
    elif kind == 'four':
        B, N, C = 5, 20, 3
        p = _grid_pred(rng, B, N, C, img=300.0)
    elif kind in ('n63', 'n64', 'n65'):
        B, N, C = 3, int(kind[1:]), 4
        p = _grid_pred(rng, B, N, C, img=400.0)
    elif kind == 'c1':
        B, N, C = 2, 100, 1
        p = _grid_pred(rng, B, N, C, img=300.0)
    elif kind == 'last':
        B, N, C = 3, 70, 5
        p = _grid_pred(rng, B, N, C, img=300.0)
        p[0, :, 5:9] *= 0.2                                 # below conf whatever the objectness
        p[1, :, 4] = 0.1
    else:
        raise KeyError(kind)
    return p, C, conf, thre, post_props(p, C, conf, thre)


POST_KINDS = ('big', 'four', 'n63', 'n64', 'n65', 'c1', 'last')
