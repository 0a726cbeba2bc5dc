# -*- coding: utf-8 -*-
"""Times what the YOLOv4 head options cost on the MI355X, at the training shape: the detection loss forward + backward
(with the CIoU box loss) and the three decodes over the three layers of a 608-px step (F = 76, 38, 19) at --batch images
with --labels label rows each, once with the options off (scale_x_y = 1, iou_thresh = 1, label_smooth = 0) and once with
scale_x_y = (1.2, 1.1, 1.05), iou_thresh = 0.213, label_smooth = 0.1; device events around --steps calls after --warmup
calls each, the variants alternated --rounds times:

    loss_fwd      y4_yolo_loss_fwd_ex_f32 + y4_yolo_box_loss_fwd_ex_f32      memset + assign + dense loss + reduction + box sum
    loss_bwd      y4_yolo_loss_bwd_ex_f32 + y4_yolo_box_loss_bwd_ex_f32      dense gradient + box gradient
    dec_train     y4_yolo_decode_train_ex_f32
    dec_eval      y4_yolo_decode_eval_ex_f32 into one [B, N, 5 + C] buffer
    dec_bwd       y4_yolo_decode_bwd_ex_f32

    python scripts/headopt_micro.py [--batch 64] [--labels 60] [--steps 50] [--warmup 10] [--rounds 3]

Prints one JSON line (microseconds per call of all three layers: the best round and every round of each variant, `off`
and `on`; the loss workspace bytes per layer either way)."""
import argparse
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
from yolov4_amd._lib import check, float_array, int_array, lib  # noqa: E402

ON = dict(scale=(1.2, 1.1, 1.05), iou=0.213, eps=0.1)
OFF = dict(scale=(1.0, 1.0, 1.0), iou=1.0, eps=0.0)


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
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('headopt_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    L, ptr, stream = lib(), ops._ptr, ops._stream
    cfg = recipe.MODEL_CFG
    C, A, B, K, S = cfg['N_CLASSES'], 3, args.batch, args.labels, 608
    n_ch = 5 + C
    kind = ops.box_loss_kind('ciou')
    labels = recipe.synth_labels(B, S, 5, max_labels=K, counts=[K] * B).to(device=dev, dtype=torch.float32).contiguous()
    rng = np.random.RandomState(0)
    n_total = sum(A * (S // st) ** 2 for st in (8, 16, 32))
    evalbuf = torch.empty((B, n_total, n_ch), device=dev)
    one = torch.ones(1, device=dev)
    layers = []
    off = 0
    for l, stride in enumerate((8, 16, 32)):
        F = S // stride
        anchors = [(float(np.float32(w / stride)), float(np.float32(h / stride))) for w, h in cfg['ANCHORS']]
        mask = list(cfg['ANCHOR_MASK'][l])
        logits = ops.empty_nhwc(B, A * n_ch, F, F, dev, pad_to=32)
        logits.copy_(torch.from_numpy(rng.standard_normal((B, A * n_ch, F, F)).astype(np.float32)))
        lg, ldl = ops.as_nhwc(logits, need_vec4=False)
        output = torch.empty((B, A, F, F, n_ch), device=dev)
        pred = torch.empty((B, A, F, F, 4), device=dev)
        masked = float_array([v for m in mask for v in anchors[m]])
        d = dict(F=F, stride=float(stride), lg=lg, ldl=ldl, output=output, pred=pred, masked=masked,
                 anchors=float_array([v for wh in anchors for v in wh]), mask=int_array(mask), box_off=off,
                 obj=torch.empty((B, A, F, F), device=dev), parts=torch.empty(4, dtype=torch.float64, device=dev),
                 g=torch.empty_like(output), gp=torch.zeros_like(pred),
                 gl=ops.empty_nhwc(B, A * n_ch, F, F, dev, pad_to=32))
        assert ops.nhwc_pitch(d['gl']) == ldl
        for name, o in (('off', OFF), ('on', ON)):
            nbytes = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, o['iou'])
            d['nbytes_' + name] = nbytes
            d['ws_' + name] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        layers.append(d)
        off += A * F * F

    def variants(name, o):
        def dec_train():
            for l, d in enumerate(layers):
                check(L.y4_yolo_decode_train_ex_f32(ptr(d['lg']), d['ldl'], ptr(d['output']), ptr(d['pred']), B, d['F'], A, C,
                                                    d['masked'], o['scale'][l], stream()), 'decode_train')

        def dec_eval():
            for l, d in enumerate(layers):
                check(L.y4_yolo_decode_eval_ex_f32(ptr(d['lg']), d['ldl'], ptr(evalbuf), n_total, d['box_off'], B, d['F'], A, C,
                                                   d['masked'], d['stride'], o['scale'][l], stream()), 'decode_eval')

        def dec_bwd():
            for l, d in enumerate(layers):
                check(L.y4_yolo_decode_bwd_ex_f32(ptr(d['lg']), d['ldl'], ptr(d['g']), ptr(d['gp']), ptr(d['gl']), B, d['F'], A,
                                                  C, d['masked'], o['scale'][l], stream()), 'decode_bwd')

        def loss_fwd():
            for d in layers:
                ws, nb = d['ws_' + name], d['nbytes_' + name]
                check(L.y4_yolo_loss_fwd_ex_f32(ptr(d['output']), ptr(d['pred']), ptr(labels), K, B, d['F'], A, C, d['stride'],
                                                0.7, d['anchors'], 9, d['mask'], o['iou'], o['eps'], ptr(d['obj']),
                                                ptr(d['parts']), ptr(ws), nb, stream()), 'loss_fwd')
                check(L.y4_yolo_box_loss_fwd_ex_f32(ptr(d['pred']), kind, 0.05, B, d['F'], A, K, C, o['iou'], ptr(d['parts']),
                                                    ptr(ws), nb, stream()), 'box_loss_fwd')

        def loss_bwd():
            for l, d in enumerate(layers):
                ws, nb = d['ws_' + name], d['nbytes_' + name]
                check(L.y4_yolo_loss_bwd_ex_f32(ptr(d['output']), 0, ptr(d['obj']), ptr(one), ptr(d['g']), B, d['F'], A, K, C,
                                                o['iou'], o['eps'], ptr(ws), nb, stream()), 'loss_bwd')
                check(L.y4_yolo_box_loss_bwd_ex_f32(ptr(d['pred']), kind, 0.05, ptr(one), ptr(d['g']), B, d['F'], A, K, C,
                                                    o['iou'], o['scale'][l], ptr(ws), nb, stream()), 'box_loss_bwd')

        return {'dec_train': dec_train, 'dec_eval': dec_eval, 'dec_bwd': dec_bwd, 'loss_fwd': loss_fwd, 'loss_bwd': loss_bwd}

    table = {name: variants(name, o) for name, o in (('off', OFF), ('on', ON))}
    rounds = {name: {k: [] for k in table[name]} for name in table}
    for _ in range(args.rounds):
        for k in table['off']:
            for name in ('off', 'on'):
                if k.startswith('loss'):
                    table[name]['dec_train']()              # the loss reads the decode of its own scale
                    table[name]['loss_fwd']()
                rounds[name][k].append(timed(table[name][k], args.steps, args.warmup))
    torch.cuda.synchronize()
    out = {'batch': B, 'labels': K, 'layers': [d['F'] for d in layers], 'steps': args.steps, 'warmup': args.warmup,
           'on': {'scale_x_y': ON['scale'], 'iou_thresh': ON['iou'], 'label_smooth': ON['eps']},
           'workspace_bytes': {name: [d['nbytes_' + name] for d in layers] for name in ('off', 'on')}}
    for name in ('off', 'on'):
        for k, v in rounds[name].items():
            out['%s_%s_us' % (k, name)] = round(min(v), 2)
            out['%s_%s_us_rounds' % (k, name)] = [round(t, 2) for t in v]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
