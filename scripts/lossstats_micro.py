# -*- coding: utf-8 -*-
"""Cost of the loss statistics: the loss forward of the three layers at bs 64, 608 x 608, K = 60,
C = 80 with YOLOLoss(stats=False) and (stats=True), alternated within one process, timed with device events.

    python scripts/lossstats_micro.py [--rounds 7] [--iters 50]

Prints per round the microseconds of one three-layer forward for either setting, then the medians and their spread, the
difference (the six launches the statistics add) and the bytes the statistics kernels have to move over that time."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import recipe  # noqa: E402
from yolov4_amd import ops  # noqa: E402
from yolov4_amd.yolo.model.yololoss import YOLOLoss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = recipe.MODEL_CFG
    B, C = args.batch, cfg['N_CLASSES']
    labels = recipe.synth_labels(B, 608, 5).to(dev)
    torch.manual_seed(0)
    outs = []
    for l, f in enumerate((76, 38, 19)):
        lg = (torch.randn(B, 3 * (5 + C), f, f, device=dev) * 0.5).contiguous(memory_format=torch.channels_last)
        st = 8 * 2 ** l
        anchors = [(float(w) / st, float(h) / st) for w, h in [cfg['ANCHORS'][i] for i in cfg['ANCHOR_MASK'][l]]]
        out, pred = ops.YoloDecodeTrainFn.apply(lg, anchors, C)
        outs.append({'layer_no': l, 'output': out, 'pred': pred})
    # mutate_outputs=False: every call sees the same `output` (the in-place masking is not part of what is compared)
    crits = {name: YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=False, stats=on) for name, on in (('off', False), ('on', True))}
    target = {'padded_labels': labels}

    def run(name, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            a.record()
            for _ in range(n):
                crits[name](outs, target)
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    for name in crits:
        run(name, 10)
    times = {'off': [], 'on': []}
    for r in range(args.rounds):
        for name in (('off', 'on') if r % 2 == 0 else ('on', 'off')):
            times[name].append(run(name, args.iters))
        print('round %d: off %.1f us, on %.1f us' % (r, times['off'][-1], times['on'][-1]))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print('%s: median %.1f us (min %.1f, max %.1f) per three-layer loss forward' % (k, med[k], min(v), max(v)))
    rows = crits['on'].stats.cpu()
    calls = rows[0, 0].item() / (B * 3 * 76 * 76)
    n_pos = (rows[:, 1] / calls).tolist()
    # what the statistics have to read: pos_index, obj_mask and the objectness word of every cell (one 4-byte word each; the
    # objectness words sit 4 * (5 + C) bytes apart, so the fabric moves more), a positive cell's pred, box, class bits and
    # class row, and the block partials once written and once read
    cells = sum(B * 3 * f * f for f in (76, 38, 19))
    need = cells * 12 + sum(n_pos) * (16 + 16 + 4 * ((C + 31) // 32) + 4 * C) + 2 * 8 * 11 * sum(-(-B * 3 * f * f // 256) for f in (76, 38, 19))
    lines = cells * 8 + cells * min(128, 4 * (5 + C))         # with whole 128-byte lines for the strided objectness words
    diff = med['on'] - med['off']
    print('positives per call and layer: %s' % ['%.0f' % v for v in n_pos])
    print('statistics (on - off): %.1f us for 6 launches; %.1f MB needed -> %.2f TB/s; %.1f MB as whole lines -> %.2f TB/s'
          % (diff, need / 1e6, need / diff / 1e6, lines / 1e6, lines / diff / 1e6))


if __name__ == '__main__':
    main()
