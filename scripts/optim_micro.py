# -*- coding: utf-8 -*-
"""Times the optimizer step of the full YOLOv4 (327 tensors, 64.9 M elements) on the MI355X, three ways, and one
ModelEMA.update; device events around --steps calls after --warmup calls each, the variants alternated --rounds times:

    unguarded     FusedAdam.step()                                              1 launch
    guarded       FusedAdam(max_grad_norm, skip_nonfinite).step()               sumsq + guard + guarded step
    stock         torch.nn.utils.clip_grad_norm_ + FusedAdam.step()             the alternative from Python
    ema           ModelEMA.update(model, guard)                                 1 launch

    python scripts/optim_micro.py [--steps 20] [--warmup 5] [--rounds 3] [--sgd]

step() walks the model's parameters in Python before it launches, so on this model the four figures above are bound by
the host; the kernel_* figures repeat the launches alone (no Python between them) and give the time on the device.

Prints one JSON line (milliseconds per call, the best round of each variant, and every round)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import recipe  # noqa: E402
from yolov4_amd import ops  # noqa: E402
from yolov4_amd._lib import check, lib  # noqa: E402
from yolov4_amd.yolo.model.yolov4 import YOLOv4  # noqa: E402
from yolov4_amd.yolo.optim.optimizers.build import FusedAdam, FusedSGD  # noqa: E402
from yolov4_amd.yolo.util.ema import ModelEMA  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sgd', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = YOLOv4(recipe.MODEL_CFG, device=dev).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p, memory_format=torch.preserve_format) * 1e-3
    n = sum(p.numel() for p in params)
    make = (lambda **kw: FusedSGD(params, lr=1e-4, **kw)) if args.sgd else (lambda **kw: FusedAdam(params, lr=1e-5, **kw))
    plain, guarded = make(), make(max_grad_norm=10.0, skip_nonfinite=True)
    ema = ModelEMA(model)

    def stock():
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        plain.step()

    variants = {'unguarded': plain.step, 'guarded': guarded.step, 'stock_clip_grad_norm': stock,
                'ema_update': lambda: ema.update(model, guarded.guard)}
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(timed(fn, args.steps, args.warmup))
    torch.cuda.synchronize()
    # step() is host-bound on this model (it walks 327 parameters in Python before its launch), which hides the guard's
    # device time above: the same launches again over the tables the optimizers built, with no Python between them
    table, nchunks = guarded._table, guarded._table.shape[0]
    hyper = ops.float_array([v for g in guarded.param_groups for v in guarded._hyper_row(g, 10)])
    nh = len(guarded.param_groups)
    gptr = ops._ptr(guarded.guard)
    ema_table = ema._table
    kernels = {'kernel_sumsq_guard': lambda: guarded._guard_launches(table, nchunks, dev),
               'kernel_step_unguarded': lambda: plain._launch(table, nchunks, hyper, nh),
               'kernel_step_guarded': lambda: guarded._launch(table, nchunks, hyper, nh, gptr),
               'kernel_ema': lambda: check(lib().y4_ema_multi_f32(ops._ptr(ema_table), ema_table.shape[0], 1e-4, gptr,
                                                                  ops._stream()), 'ema_multi')}
    for _ in range(args.rounds):
        for k, fn in kernels.items():
            rounds.setdefault(k, []).append(timed(fn, args.steps, args.warmup))
    torch.cuda.synchronize()
    out = {'optimizer': 'sgd' if args.sgd else 'adam', 'tensors': len(params), 'elements': n, 'steps': args.steps,
           'warmup': args.warmup, 'guard': guarded.guard_state()}
    for k, v in rounds.items():
        out[k + '_ms'] = round(min(v), 4)
        out[k + '_ms_rounds'] = [round(t, 4) for t in v]
    # what the guard adds on the device: the two extra launches + the difference between the two step kernels
    added = out['kernel_sumsq_guard_ms'] + out['kernel_step_guarded_ms'] - out['kernel_step_unguarded_ms']
    out['guard_added_device_ms'] = round(added, 4)
    out['grad_read_TBps_in_sumsq_guard'] = round(4.0 * n / 1e12 / (out['kernel_sumsq_guard_ms'] / 1e3), 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
