# -*- coding: utf-8 -*-
"""Times what an IoU-family box loss adds to the detection loss on the MI355X: the two extra launches
(y4_yolo_box_loss_fwd_f32, y4_yolo_box_loss_bwd_f32) beside the existing loss launches of the same run, over the three
layers of a 608-px step (F = 76, 38, 19) at --batch images with --labels label rows each; device events around --steps
calls after --warmup calls each, the variants alternated --rounds times:

    loss_fwd      y4_yolo_loss_fwd_f32          memset + assign + dense loss + final reduction, x 3 layers
    loss_bwd      y4_yolo_loss_bwd_f32          dense gradient, x 3 layers
    box_fwd       y4_yolo_box_loss_fwd_f32      one block over the B * K record slots, x 3 layers
    box_bwd       y4_yolo_box_loss_bwd_f32      one thread per record slot, x 3 layers

    python scripts/boxloss_micro.py [--batch 64] [--labels 60] [--kind ciou] [--steps 50] [--warmup 10] [--rounds 3]

Prints one JSON line (microseconds per call of all three layers, the best round of each variant, and every round)."""
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
    ap.add_argument('--kind', default='ciou', choices=['iou', 'giou', 'diou', 'ciou'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('boxloss_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    L, ptr, stream = lib(), ops._ptr, ops._stream
    cfg = recipe.MODEL_CFG
    C, A, B, K, S = cfg['N_CLASSES'], 3, args.batch, args.labels, 608
    kind = ops.box_loss_kind(args.kind)
    labels = recipe.synth_labels(B, S, 5, max_labels=K, counts=[K] * B).to(device=dev, dtype=torch.float32).contiguous()
    rng = np.random.RandomState(0)
    layers = []
    for l, stride in enumerate((8, 16, 32)):
        F = S // stride
        anchors = [(float(np.float32(w / stride)), float(np.float32(h / stride))) for w, h in cfg['ANCHORS']]
        mask = list(cfg['ANCHOR_MASK'][l])
        output = torch.from_numpy(rng.uniform(0.05, 0.95, (B, A, F, F, 5 + C)).astype(np.float32)).to(dev)
        pred = torch.empty((B, A, F, F, 4), device=dev)
        pred[..., 0] = output[..., 0] + torch.arange(F, device=dev).view(1, 1, 1, F)
        pred[..., 1] = output[..., 1] + torch.arange(F, device=dev).view(1, 1, F, 1)
        for a, m in enumerate(mask):
            pred[:, a, :, :, 2] = torch.exp(output[:, a, :, :, 2] - 0.5) * anchors[m][0]
            pred[:, a, :, :, 3] = torch.exp(output[:, a, :, :, 3] - 0.5) * anchors[m][1]
        nbytes = L.y4_yolo_loss_workspace(B, F, A, K, C)
        layers.append(dict(F=F, stride=float(stride), output=output, pred=pred.contiguous(), nbytes=nbytes,
                           ws=torch.empty(nbytes, dtype=torch.uint8, device=dev),
                           obj=torch.empty((B, A, F, F), device=dev), parts=torch.empty(4, dtype=torch.float64, device=dev),
                           g=torch.empty_like(output), anchors=float_array([v for wh in anchors for v in wh]),
                           mask=int_array(mask)))
    one = torch.ones(1, device=dev)

    def loss_fwd():
        for d in layers:
            check(L.y4_yolo_loss_fwd_f32(ptr(d['output']), ptr(d['pred']), ptr(labels), K, B, d['F'], A, C, d['stride'], 0.7,
                                         d['anchors'], 9, d['mask'], ptr(d['obj']), ptr(d['parts']), ptr(d['ws']),
                                         d['nbytes'], stream()), 'loss_fwd')

    def loss_bwd():
        for d in layers:
            check(L.y4_yolo_loss_bwd_f32(ptr(d['output']), 0, ptr(d['obj']), ptr(one), ptr(d['g']), B, d['F'], A, K, C,
                                         ptr(d['ws']), d['nbytes'], stream()), 'loss_bwd')

    def box_fwd():
        for d in layers:
            check(L.y4_yolo_box_loss_fwd_f32(ptr(d['pred']), kind, 1.0, B, d['F'], A, K, C, ptr(d['parts']), ptr(d['ws']),
                                             d['nbytes'], stream()), 'box_loss_fwd')

    def box_bwd():
        for d in layers:
            check(L.y4_yolo_box_loss_bwd_f32(ptr(d['pred']), kind, 1.0, ptr(one), ptr(d['g']), B, d['F'], A, K, C,
                                             ptr(d['ws']), d['nbytes'], stream()), 'box_loss_bwd')

    loss_fwd()                                              # fills the workspaces the other three read
    torch.cuda.synchronize()
    variants = {'loss_fwd': loss_fwd, 'loss_bwd': loss_bwd, 'box_fwd': box_fwd, 'box_bwd': box_bwd}
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(timed(fn, args.steps, args.warmup))
    torch.cuda.synchronize()
    out = {'kind': args.kind, 'batch': B, 'labels': K, 'layers': [d['F'] for d in layers], 'steps': args.steps,
           'warmup': args.warmup, 'box_loss_parts0': [float(d['parts'][0]) for d in layers]}
    for k, v in rounds.items():
        out[k + '_us'] = round(min(v), 2)
        out[k + '_us_rounds'] = [round(t, 2) for t in v]
    out['box_added_us'] = round(out['box_fwd_us'] + out['box_bwd_us'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
