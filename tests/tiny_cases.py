# -*- coding: utf-8 -*-
"""References, case lists and acceptance rules for YOLOv4-tiny (csrc/tiny.hip, yolo/model/yolov4_tiny.py): numpy and
torch-CPU only.  tests/test_tiny_cases.py checks this module without a GPU, tests/test_gpu_tiny.py feeds it to the kernels.

  * the 2x2 stride-2 max pool from its definition (row-major scan, v > best || isnan(v)): values, int8 codes 2 dy + dx, and the
    backward that writes every input element; all bit-exact;
  * the stride-2 stem conv and its filter gradient in fp64, each with the companion S = sum |x| |w| (sum |x| |dy|) of its terms;
  * a mirror of the wgrad kernel's reduction plan (tiny.hip: wgrad_blocks, stem_s2_wgrad_kernel), which supplies L, the
    longest chain of fp32 additions behind one result; it is never the reference of a value;
  * tiny_oracle: the network restated with torch.nn.functional from a state_dict, the head from oracle.head;
  * seeded inputs and the case lists; the model cases' images are chosen by a conditioning rule on the oracles alone
    (MODEL_INPUT_SEEDS, conditioning()): no pool tie and no LeakyReLU kink within 4 x the local fp32 error.

Acceptance, u = 2^-24, TINY = 2^-126:
  stem forward   one fp32 fma chain of at most 27 terms, then scale / shift (one fma or a multiply and an add) and the
                 activation (leaky: one multiply):  |y - y64| <= |act'| (|scale| (27 + 1) u S + 3 u (|acc64 scale| + |shift|)) + TINY
                 and equal in every bit to y4_conv2d_generic_fwd_f32.
  stem wgrad     |dw - dw64| <= (L + 1) u S + TINY; two runs give the same bits.
  model          error against fp64 <= max(floor, 1.5 x the fp32 oracle's own distance from fp64); floors: loss relative 1e-4,
                 gradients 1e-3 of the tensor's maximum, outputs absolute 1e-4 times max(1, max|reference|)."""
import numpy as np
import torch
import torch.nn.functional as F

import recipe
from bn_cases import ERR_NULL, ERR_SHAPE, F32, F64, SENT, TINY, U, is_sentinel, sentinel  # noqa: F401

ERR_WORKSPACE = 4
THREADS = 256
GRID_CAP = 2048                          # tiny.hip TN_GRID_CAP
WG_MAX_BLOCKS = 1024
WG_MIN_PIX_PER_LANE = 4


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def laps(total, cap=GRID_CAP):
    """trips of the busiest thread through a grid-stride loop of tiny.hip"""
    grid = int(max(min(-(-total // THREADS), cap), 1))
    return -(-total // (grid * THREADS))


# ------------------------------------------------------------------------------------------ max pool 2x2 / stride 2
def pool_ref(x):
    """x [B, H, W, C] fp32 -> (y [B, H//2, W//2, C], code int8): aten's scan"""
    x = np.asarray(x, F32)
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    best = x[:, 0:2 * Ho:2, 0:2 * Wo:2, :].copy()
    code = np.zeros(best.shape, np.int8)
    for k in (1, 2, 3):
        v = x[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2, :]
        with np.errstate(invalid='ignore'):
            take = (v > best) | np.isnan(v)
        best = np.where(take, v, best)
        code = np.where(take, np.int8(k), code)
    return best, code


def pool_bwd_ref(dy, code, H, W):
    """every element of dx [B, H, W, C]: dy where the code points, +0 elsewhere and in a dropped odd row / column"""
    dy = np.asarray(dy, F32)
    B, Ho, Wo, C = dy.shape
    dx = np.zeros((B, H, W, C), F32)
    for k in range(4):
        dx[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2, :] = np.where(code == k, dy, F32(0))
    return dx


NAN_A, NAN_B = 0x7fc01234, 0xffc00077          # two quiet NaNs with payloads


def _f32_from_bits(b):
    return np.array([b], np.uint32).view(F32)[0]


# (name, B, H, W, C, ldx, offx, ldy, offy): x is the channel slice [offx, offx + C) of rows of pitch ldx, y alike
POOL_CASES = [
    ('c4', 2, 6, 6, 4, 4, 0, 4, 0),
    ('c12_pitch_x', 1, 4, 6, 12, 20, 0, 12, 0),
    ('c20_pitch_y', 2, 4, 4, 20, 20, 0, 28, 0),
    ('c64_slice', 1, 8, 4, 64, 128, 64, 64, 0),          # the upper half of a concat buffer (offset 256 B)
    ('c8_slice_both', 2, 4, 4, 8, 24, 4, 16, 8),         # 16-B aligned offsets on both sides
    ('one_output', 1, 2, 2, 12, 12, 0, 12, 0),
    ('odd_7x9', 2, 7, 9, 12, 16, 0, 12, 0),
    ('no_output_1x1', 1, 1, 1, 8, 8, 0, 8, 0),
    ('no_output_1x5', 1, 1, 5, 8, 8, 0, 8, 0),
    ('specials', 1, 4, 8, 4, 4, 0, 4, 0),
]
POOL_GRID_STRIDE = ('grid_stride', 1, 130, 130, 512, 512, 0, 512, 0)      # 65 * 65 * 128 threads of work > 2048 * 256


def pool_input(case):
    name, B, H, W, C = case[:5]
    rng = np.random.RandomState(sum(map(ord, name)))
    x = rng.standard_normal((B, H, W, C)).astype(F32)
    Ho, Wo = H // 2, W // 2
    if name == 'specials':
        w = x[0]                                             # windows of channel 0 at (row 0, cols 0..3) and (row 1, cols 0..3)
        nan_a, nan_b = _f32_from_bits(NAN_A), _f32_from_bits(NAN_B)
        w[0:2, 0:2, 0] = 1.5                                 # four equal values: the first wins
        w[0:2, 2:4, 0] = [[nan_a, 0.0], [1.0, 2.0]]          # NaN first
        w[0:2, 4:6, 0] = [[3.0, 0.0], [1.0, nan_a]]          # NaN last
        w[0:2, 6:8, 0] = [[nan_a, 9.0], [nan_b, 1.0]]        # two NaNs: the last one's payload and code
        w[2:4, 0:2, 0] = [[-np.inf, -np.inf], [-np.inf, -np.inf]]
        w[2:4, 2:4, 0] = [[1.0, np.inf], [np.inf, 2.0]]      # two +inf: the first
        w[2:4, 4:6, 0] = [[-0.0, 0.0], [0.0, -0.0]]          # signed zeros compare equal: the first (-0) stays
        w[2:4, 6:8, 0] = [[-np.inf, -3.0], [-2.0, -2.0]]
    dy = rng.standard_normal((B, Ho, Wo, C)).astype(F32)
    if dy.size:
        dy.reshape(-1)[0] = _f32_from_bits(NAN_B)            # a NaN gradient comes through with its payload
    return x, dy


# (what, argument overrides, return code): every refused argument set of the two pool entry points
def pool_rejects():
    return [('x NULL', dict(x=0), ERR_NULL), ('y NULL', dict(y=0), ERR_NULL), ('C % 4', dict(C=6), ERR_SHAPE),
            ('ldx % 4', dict(ldx=14), ERR_SHAPE), ('ldx < C', dict(ldx=8), ERR_SHAPE), ('ldy < C', dict(ldy=8), ERR_SHAPE),
            ('x misaligned', dict(x_off=4), ERR_SHAPE), ('y misaligned', dict(y_off=8), ERR_SHAPE), ('B = 0', dict(B=0), ERR_SHAPE),
            ('H = 0', dict(H=0), ERR_SHAPE), ('W < 0', dict(W=-2), ERR_SHAPE), ('C = 0', dict(C=0), ERR_SHAPE)]


# ------------------------------------------------------------------------------------------ stem 3 -> Cout, 3x3, stride 2
def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def leaky64(v):
    return np.where(v > 0, v, 0.1 * v)


def stem_fwd64(x, w, scale=None, shift=None, act=0):
    """x [B, 3, H, W], w [Cout, 3, 3, 3] (OIHW) -> (y64, bound) as [B, Ho, Wo, Cout] fp64 arrays"""
    x64, w64 = torch.from_numpy(np.asarray(x, F64)), torch.from_numpy(np.asarray(w, F64))
    acc = F.conv2d(x64, w64, stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    S = F.conv2d(x64.abs(), w64.abs(), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    sc = np.ones(w.shape[0]) if scale is None else np.asarray(scale, F64)
    sh = np.zeros(w.shape[0]) if shift is None else np.asarray(shift, F64)
    v = acc * sc + sh
    bound = np.abs(sc) * 28 * U * S + 3 * U * (np.abs(acc * sc) + np.abs(sh))
    if act == 1:
        return leaky64(v), bound * (1 + 2 * U) + U * np.abs(leaky64(v)) + TINY
    return v, bound + TINY


def stem_wgrad64(x, dy):
    """x [B, 3, H, W], dy [B, Ho, Wo, Cout] -> (dw64 [Cout, 3, 3, 3] OIHW, S = the same sum over |x| |dy|)"""
    out = []
    for fx in (lambda a: a, np.abs):
        x64 = torch.from_numpy(fx(np.asarray(x, F64)))
        g64 = torch.from_numpy(fx(np.asarray(dy, F64))).permute(0, 3, 1, 2)
        w = torch.zeros((dy.shape[3], 3, 3, 3), dtype=torch.float64, requires_grad=True)
        (F.conv2d(x64, w, stride=2, padding=1) * g64).sum().backward()
        out.append(w.grad.numpy())
    return out[0], out[1]


def wgrad_plan(B, H, W, Cout):
    """mirror of the kernel's reduction plan: blocks (slabs), pixels per block T, pixel lanes P per channel group, and L:
    at most ceil(T / P) fma roundings in a lane's chain, then P - 1 fp32 additions across the lanes (the slabs are folded in
    fp64) -- and never more than the M terms there are: adding an exact zero rounds nothing"""
    Ho, Wo = out_hw(H, W)
    M = B * Ho * Wo
    P = THREADS // (Cout // 4)
    nb = max(1, min(WG_MAX_BLOCKS, -(-M // (P * WG_MIN_PIX_PER_LANE))))
    T = -(-M // nb)
    L = min(-(-T // P) + P - 1, M)
    return dict(M=M, P=P, blocks=nb, T=T, L=L, workspace=nb * 27 * Cout * 4)


# (B, H, W, Cout): 8x8, odd 13x9, 2x2 and 1x1 maps; B = 1 and 3; Cout = 32, 64 and 4
STEM_CASES = [(1, 8, 8, 32), (3, 13, 9, 32), (1, 2, 2, 64), (3, 1, 1, 4), (3, 8, 8, 64), (1, 13, 9, 4)]
STEM_WGRAD_MULTI_SLAB = (2, 64, 48, 32)      # M = 1536 pixels, P = 32 lanes: 12 slabs per filter element
STEM_EPILOGUES = ('plain', 'scale_shift_leaky', 'shift_only')


def stem_input(case, seed=0):
    B, H, W, Cout = case
    rng = np.random.RandomState(1000 + 7 * B + 31 * H + W + Cout + seed)
    Ho, Wo = out_hw(H, W)
    return dict(x=rng.standard_normal((B, 3, H, W)).astype(F32), w=(rng.standard_normal((Cout, 3, 3, 3)) * 0.3).astype(F32),
                dy=rng.standard_normal((B, Ho, Wo, Cout)).astype(F32), scale=rng.uniform(0.5, 1.5, Cout).astype(F32),
                shift=rng.standard_normal(Cout).astype(F32))


def krsc(w):
    """OIHW -> the library's [Cout][r][q][c]"""
    return np.ascontiguousarray(np.asarray(w).transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------ the network
ANCHORS = [[10, 14], [23, 27], [37, 58], [81, 82], [135, 169], [344, 319]]
ANCHOR_MASK = [[1, 2, 3], [3, 4, 5]]
STRIDES = (16, 32)
DARKNET_ORDER = [0, 1, 2, 4, 5, 7, 10, 12, 13, 15, 18, 20, 21, 23, 26, 27, 28, 29, 32, 35, 36]
N_PARAMS_80 = 6056606
MODEL_CASES = [(2, 64), (2, 96)]             # (B, S): maps 4 and 2, 6 and 3
MODEL_SEED = 4242
TREE = (['backbone.conv1', 'backbone.conv2'] + ['backbone.block%d.conv%d' % (b, c) for b in (1, 2, 3) for c in (1, 2, 3, 4)]
        + ['backbone.conv3', 'neck.conv1', 'neck.conv2', 'head.yolo2.0', 'head.yolo2.1', 'head.yolo1.0', 'head.yolo1.1'])
NO_BN = ('head.yolo2.1', 'head.yolo1.1')


def expected_keys():
    keys = []
    for pre in TREE:
        keys.append(pre + '.conv.weight')
        if pre in NO_BN:
            keys.append(pre + '.conv.bias')
        else:
            keys += [pre + '.norm.' + s for s in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]
    return keys


def model_cfg(n_classes=80):
    return {'TYPE': 'YOLOv4Tiny', 'BACKBONE_PRETRAINED': None, 'ANCHORS': [list(a) for a in ANCHORS],
            'ANCHOR_MASK': [list(m) for m in ANCHOR_MASK], 'STRIDES': list(STRIDES), 'N_CLASSES': n_classes}


def full_cfg(S=64):
    return {'MODEL': model_cfg(), 'CRITERION': {'TYPE': 'YOLOLoss', 'IGNORE_THRESH': 0.7},
            'TEST': {'IMGSIZE': S, 'CONFTHRE': 0.001, 'NMSTHRE': 0.4}, 'DATA': {'MAX_NUM_LABELS': 60, 'BATCH_SIZE': 2}}


# Which image a model case feeds.  The network's gradient is DISCONTINUOUS in its forward values at two kinds of places: a
# 2 x 2 pool window whose two largest candidates tie (the gradient goes to the selected one) and a LeakyReLU pre-activation at 0
# (slope 1 or 0.1).  The model tests compare gradients with fp64 under a bound that allows the code 1.5 x the fp32 oracle's
# own distance from fp64; a pool selection of the reference survives two candidates moving against each other by that much
# only if their gap exceeds 3 x that distance, a LeakyReLU slope only if |pre-activation| exceeds 1.5 x.  Where the fp64
# reference has a closer pair, which element ANY fp32 evaluation selects is chance, and its gradient -- correct for its own
# forward values -- is a whole element's gradient away from the reference's (seen on an MI355X: seed 596 at S = 96, one
# window of block 3's pool with a gap of 5.98e-6, a third of the local fp32 error, moved backbone.block3.conv1's filter
# gradient by 5.9e-2 of its maximum in conv mode 'f32').  Such an input tests the luck of the rounding, not the code.  So an
# input qualifies when, in the fp64 oracle, every pool window's gap and every LeakyReLU |pre-activation| is at least COND_K = 4
# times the fp32 oracle's own error AT THOSE ELEMENTS (conditioning(), single-threaded oracles: the setting every host
# reproduces) -- the 3 x / 1.5 x above with a third in hand, a statement about the reference alone.  The seed of a case is the
# FIRST one from 500 + S upwards that qualifies; tests/test_tiny_cases.py checks both the qualifying and the "first".
COND_K = 4.0
MODEL_INPUT_SEEDS = {64: 565, 96: 600}       # 564 and 596 .. 599 do not qualify


def model_input(case, seed=None):
    B, S = case
    x = recipe.randn((B, 3, S, S), MODEL_INPUT_SEEDS[S] if seed is None else seed)
    labels = recipe.synth_labels(B, S, 600 + S, counts=[5, 3][:B])
    return x, labels


def conditioning(sd, x):
    """(pool, act): over all 2 x 2 pool windows the smallest (gap of the two largest candidates in the fp64 oracle) / (larger
    of the fp32 oracle's errors at those two elements), and over all LeakyReLU inputs the smallest |fp64 pre-activation| /
    (the fp32 oracle's error there); training-mode statistics, as the train step uses them."""
    seen = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for dt in (torch.float64, torch.float32):
            p = {k: (v.detach().to(dt) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
            with torch.no_grad():
                _logits(p, x.to(dt), True, seen=seen.setdefault(dt, {}))
    finally:
        torch.set_num_threads(threads)

    def windows(t):
        return t.unfold(2, 2, 2).unfold(3, 2, 2).reshape(t.shape[0], t.shape[1], t.shape[2] // 2, t.shape[3] // 2, 4)
    pool = act = float('inf')
    for t, u in zip(seen[torch.float64]['pool'], seen[torch.float32]['pool']):
        top = windows(t).topk(2, dim=-1)
        err = windows((u - t).abs()).gather(-1, top.indices).amax(-1).clamp_min(1e-300)
        pool = min(pool, float(((top.values[..., 0] - top.values[..., 1]) / err).min()))
    for t, u in zip(seen[torch.float64]['act'], seen[torch.float32]['act']):
        act = min(act, float((t.abs() / (u - t).abs().clamp_min(1e-300)).min()))
    return pool, act


class _Strides:
    """oracle.head with STRIDES = (16, 32) for the duration of a with-block"""

    def __enter__(self):
        from oracle import head as H
        self.H, self.old = H, H.STRIDES
        H.STRIDES = STRIDES
        return H

    def __exit__(self, *exc):
        self.H.STRIDES = self.old


def _logits(p, x, training, momentum=0.1, seen=None):
    """seen (optional dict): receives every pool input ('pool') and every LeakyReLU pre-activation ('act'), for conditioning()"""
    def note(kind, t):
        if seen is not None:
            seen.setdefault(kind, []).append(t.detach().double())
        return t

    def cba(x, pre, k, s, act=True, bn=True):
        x = F.conv2d(x, p[pre + '.conv.weight'], p.get(pre + '.conv.bias'), stride=s, padding=(k - 1) // 2)
        if bn:
            if training:
                p[pre + '.norm.num_batches_tracked'] += 1
            x = F.batch_norm(x, p[pre + '.norm.running_mean'], p[pre + '.norm.running_var'], p[pre + '.norm.weight'],
                             p[pre + '.norm.bias'], training=training, momentum=momentum, eps=1e-5)
        return F.leaky_relu(note('act', x), 0.1) if act else x

    x = cba(cba(x, 'backbone.conv1', 3, 2), 'backbone.conv2', 3, 2)
    tap = None
    for b in (1, 2, 3):
        pre = 'backbone.block%d' % b
        x1 = cba(x, pre + '.conv1', 3, 1)
        x2 = cba(x1[:, x1.shape[1] // 2:], pre + '.conv2', 3, 1)          # route groups=2 group_id=1
        x3 = cba(x2, pre + '.conv3', 3, 1)
        tap = cba(torch.cat([x3, x2], 1), pre + '.conv4', 1, 1)
        x = F.max_pool2d(note('pool', torch.cat([x1, tap], 1)), 2, 2)
    x = cba(x, 'backbone.conv3', 3, 1)
    n1 = cba(x, 'neck.conv1', 1, 1)
    lg32 = cba(cba(n1, 'head.yolo2.0', 3, 1), 'head.yolo2.1', 1, 1, act=False, bn=False)
    up = F.interpolate(cba(n1, 'neck.conv2', 1, 1), size=tap.shape[2:], mode='nearest')
    lg16 = cba(cba(torch.cat([up, tap], 1), 'head.yolo1.0', 3, 1), 'head.yolo1.1', 1, 1, act=False, bn=False)
    return [lg16, lg32]


def tiny_oracle(sd, x, dtype, train, labels=None, cfg=None, ignore_thresh=0.7):
    """The network from a state_dict.  train: BatchNorm batch statistics; returns dict(logits=[stride 16, stride 32] numpy,
    loss, grads {key: numpy}) with the loss and its logit gradients from oracle.head (fp32, as the reference computes them) on
    the logits of a `dtype` network, when labels are given.  Eval: the decoded [B, N, 5 + C] array, stride-16 rows first."""
    cfg = cfg or model_cfg()
    p = {}
    for k, v in sd.items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v.to(dtype)
            if 'running_' not in k:
                v.requires_grad_(bool(train))
        p[k] = v
    x = x.to(dtype)
    with _Strides() as H:
        if not train:
            with torch.no_grad():
                lg = _logits(p, x, False)
            return np.concatenate([H.yolo_decode(t.float().numpy(), l, cfg, False) for l, t in enumerate(lg)], 1)
        lg = _logits(p, x, True)
        out = dict(logits=[t.detach().numpy().astype(F64) for t in lg])
        if labels is not None:
            loss, glog = H.yolo_loss([t.detach().float().numpy() for t in lg], np.asarray(labels), cfg, ignore_thresh)
            torch.autograd.backward(lg, [torch.from_numpy(g).to(dtype) for g in glog])
            out['loss'] = float(loss)
            out['grads'] = {k: v.grad.numpy().astype(F64) for k, v in p.items() if v.requires_grad and v.grad is not None}
    return out


def within(err, ref_err, floor):
    """the classifier test's rule: the error may be the floor, or 1.5 x the fp32 oracle's own distance from fp64"""
    return err <= max(floor, 1.5 * ref_err)
