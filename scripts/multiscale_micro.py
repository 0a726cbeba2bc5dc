# -*- coding: utf-8 -*-
"""Multi-scale training in one process: full YOLOv4, bs 64, forward + YOLOLoss + backward at 608,
then one pass over the ten sizes 320 ... 608 of the default schedule and back to 320; 2 warm-up + 3 timed steps each.

    python scripts/multiscale_micro.py [--batch 64] [--timed 3] [--warmup 2]

Prints images/s and, after every size, torch.cuda.max_memory_allocated of that visit (the peak statistics are reset when a
visit begins), what is still allocated and what the caching allocator holds -- do the per-shape workspaces and caches pile
up over ten shapes? -- and images/s at 608 before and after the sweep."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import recipe  # noqa: E402
from yolov4_amd.yolo.data.multiscale import MultiScale  # noqa: E402
from yolov4_amd.yolo.model.yololoss import YOLOLoss  # noqa: E402
from yolov4_amd.yolo.model.yolov4 import YOLOv4  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timed', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = recipe.MODEL_CFG
    model = YOLOv4(cfg, device=dev)
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 1234)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    crit = YOLOLoss(cfg, ignore_thresh=0.7, device=dev)
    B = args.batch

    def visit(S, tag):
        g = torch.Generator(device='cpu')
        g.manual_seed(1000 + S)
        x = torch.randn((B, 3, S, S), generator=g).to(dev)
        labels = recipe.synth_labels(B, S, 2000 + S).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            loss = crit(model(x), {'padded_labels': labels})
            loss.backward()
            return loss
        torch.cuda.reset_peak_memory_stats()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.timed):
            loss = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rate = B * args.timed / dt
        print('%-14s S %3d: %7.1f images/s (%.1f ms/step), loss %.4f, peak allocated %.2f GiB, allocated now %.2f GiB, '
              'reserved %.2f GiB' % (tag, S, rate, dt / args.timed * 1e3, float(loss.detach()), torch.cuda.max_memory_allocated() / 2 ** 30,
                                     torch.cuda.memory_allocated() / 2 ** 30, torch.cuda.memory_reserved() / 2 ** 30))
        return rate

    before = visit(608, 'before')
    rates = {}
    for S in MultiScale().sizes:
        rates[S] = visit(S, 'sweep')
    again = visit(320, 'back')
    print('608 before the sweep %.1f images/s, at its end %.1f (%.3fx); 320 first %.1f, revisited %.1f (%.3fx)'
          % (before, rates[608], rates[608] / before, rates[320], again, again / rates[320]))


if __name__ == '__main__':
    main()
