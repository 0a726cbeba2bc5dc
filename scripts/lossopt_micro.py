# -*- coding: utf-8 -*-
"""Times what focal loss, IoU-aware objectness and the objectness / class gains cost on the MI355X, at the training
shape: the detection loss forward + backward (with the CIoU box loss) over the three layers of a 608-px step (F = 76, 38,
19) at --batch images with --labels label rows each, through the *_opts entries, with the options off and with

    focal     focal_gamma 2, focal_alpha 0.25 on objectness and classes
    iou_obj   obj_iou_ratio 0.5 of CIoU
    gains     obj_gain 0.4, cls_gain 2.5
    all       the three together

device events around --steps calls after --warmup calls each, the variants alternated --rounds times:

    loss_fwd      y4_yolo_loss_fwd_opts_f32 + y4_yolo_box_loss_fwd_ex_f32    memset + assign + dense loss + reduction + box sum
    loss_bwd      y4_yolo_loss_bwd_opts_f32 + y4_yolo_box_loss_bwd_ex_f32    dense gradient + box gradient

    python scripts/lossopt_micro.py [--batch 64] [--labels 60] [--steps 200] [--warmup 20] [--rounds 3]

Prints one JSON line (microseconds per call of all three layers: the best round and every round of each variant; the
loss workspace bytes per layer of each variant)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import recipe  # noqa: E402
from yolov4_amd import ops  # noqa: E402
from yolov4_amd._lib import FOCAL_TERMS, LossOpts, check, float_array, int_array, lib  # noqa: E402

CIOU = ops.BOX_LOSS_KINDS['ciou']


def opts(gamma=0.0, r=0.0, obj_gain=1.0, cls_gain=1.0):
    return LossOpts(1.0, 0.0, gamma, 0.25, FOCAL_TERMS['obj+cls'], r, CIOU, obj_gain, cls_gain)


VARIANTS = {'off': opts(), 'focal': opts(gamma=2.0), 'iou_obj': opts(r=0.5), 'gains': opts(obj_gain=0.4, cls_gain=2.5),
            'all': opts(2.0, 0.5, 0.4, 2.5)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--labels', type=int, default=60)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lossopt_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    L, ptr, stream = lib(), ops._ptr, ops._stream
    cfg = recipe.MODEL_CFG
    C, A, B, K, S = cfg['N_CLASSES'], 3, args.batch, args.labels, 608
    n_ch = 5 + C
    labels = recipe.synth_labels(B, S, 5, max_labels=K, counts=[K] * B).to(device=dev, dtype=torch.float32).contiguous()
    rng = np.random.RandomState(0)
    one = torch.ones(1, device=dev)
    layers = []
    for l, stride in enumerate((8, 16, 32)):
        F = S // stride
        anchors = [(float(np.float32(w / stride)), float(np.float32(h / stride))) for w, h in cfg['ANCHORS']]
        mask = list(cfg['ANCHOR_MASK'][l])
        logits = ops.empty_nhwc(B, A * n_ch, F, F, dev, pad_to=32)
        logits.copy_(torch.from_numpy(rng.standard_normal((B, A * n_ch, F, F)).astype(np.float32)))
        lg, ldl = ops.as_nhwc(logits, need_vec4=False)
        output = torch.empty((B, A, F, F, n_ch), device=dev)
        pred = torch.empty((B, A, F, F, 4), device=dev)
        check(L.y4_yolo_decode_train_f32(ptr(lg), ldl, ptr(output), ptr(pred), B, F, A, C,
                                         float_array([v for m in mask for v in anchors[m]]), stream()), 'decode_train')
        d = dict(F=F, stride=float(stride), output=output, pred=pred, anchors=float_array([v for wh in anchors for v in wh]),
                 mask=int_array(mask), obj=torch.empty((B, A, F, F), device=dev),
                 parts=torch.empty(4, dtype=torch.float64, device=dev), g=torch.empty_like(output))
        for name, o in VARIANTS.items():
            nbytes = L.y4_yolo_loss_workspace_opts(B, F, A, K, C, ctypes.byref(o))
            d['nbytes_' + name] = nbytes
            d['ws_' + name] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        layers.append(d)

    def variants(name, o):
        op = ctypes.byref(o)

        def loss_fwd():
            for d in layers:
                ws, nb = d['ws_' + name], d['nbytes_' + name]
                check(L.y4_yolo_loss_fwd_opts_f32(ptr(d['output']), ptr(d['pred']), ptr(labels), K, B, d['F'], A, C, d['stride'],
                                                  0.7, d['anchors'], 9, d['mask'], op, ptr(d['obj']), ptr(d['parts']), ptr(ws),
                                                  nb, stream()), 'loss_fwd')
                check(L.y4_yolo_box_loss_fwd_ex_f32(ptr(d['pred']), CIOU, 0.05, B, d['F'], A, K, C, 1.0, ptr(d['parts']), ptr(ws),
                                                    nb, stream()), 'box_loss_fwd')

        def loss_bwd():
            for d in layers:
                ws, nb = d['ws_' + name], d['nbytes_' + name]
                check(L.y4_yolo_loss_bwd_opts_f32(ptr(d['output']), 0, ptr(d['obj']), ptr(one), ptr(d['g']), B, d['F'], A, K, C,
                                                  op, ptr(ws), nb, stream()), 'loss_bwd')
                check(L.y4_yolo_box_loss_bwd_ex_f32(ptr(d['pred']), CIOU, 0.05, ptr(one), ptr(d['g']), B, d['F'], A, K, C, 1.0,
                                                    1.0, ptr(ws), nb, stream()), 'box_loss_bwd')

        return {'loss_fwd': loss_fwd, 'loss_bwd': loss_bwd}

    table = {name: variants(name, o) for name, o in VARIANTS.items()}
    rounds = {name: {k: [] for k in table[name]} for name in table}
    for _ in range(args.rounds):
        for k in ('loss_fwd', 'loss_bwd'):
            for name in table:
                table[name]['loss_fwd']()                       # the backward reads the workspace of its own forward
                rounds[name][k].append(timed(table[name][k], args.steps, args.warmup))
    torch.cuda.synchronize()
    out = {'batch': B, 'labels': K, 'layers': [d['F'] for d in layers], 'steps': args.steps, 'warmup': args.warmup,
           'workspace_bytes': {name: [d['nbytes_' + name] for d in layers] for name in VARIANTS}}
    for name in table:
        for k, v in rounds[name].items():
            out['%s_%s_us' % (k, name)] = round(min(v), 2)
            out['%s_%s_us_rounds' % (k, name)] = [round(t, 2) for t in v]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
