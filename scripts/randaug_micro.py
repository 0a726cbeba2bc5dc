# -*- coding: utf-8 -*-
"""Micro-benchmark of RandAugment on the device (yolov4_amd/darknet/data.py on csrc/randaug.hip).

    python scripts/randaug_micro.py [--batch 256] [--size 256] [--iters 50] [--warmup 5] [--step]

The geometry of scripts/imagenet_micro.py: B device-resident 500 x 375 BGR sources -> [B, 3, S, S], RandomResizedCrop + flip,
device events after warm-up around whole library calls on one uploaded table:
  plain_ms            y4_rcrop_u8_f32 (two launches)
  ops0_ms             y4_rcrop_randaug_u8_f32 with n_ops = 0: the same two launches
  copy_ms             a device-to-device copy of one uint8 batch (B S S 3 bytes each way), the yardstick of a round
  one_<class>_ms      n_ops = 1, every sample the same operation: tables + uint8 gather (+ statistics) + final apply
  two_<class>_ms      n_ops = 2, the operation twice
  round_<class>_ms    two_ - one_: what one more round costs (a statistics launch where the class has one, and a uint8 -> uint8
                      apply launch); round_<class>_x_copy is that over copy_ms
  stats_ms            round_contrast - round_brightness: the same blend with and without the statistics launch
  default_ms          RandAugment() drawn per sample (two operations, mixed over the batch); default_extra_ms is that minus
                      plain_ms
  classes: point (Solarize), brightness, contrast (statistics + blend), lut (Equalize: statistics + table), filter
  (Sharpness, 3 x 3), gather (Rotate).
--step also times one CSPDarknet53 train step at bs 64 (scripts/classifier_micro.py's) and reports default_extra_ms as a share
of the step time of B images.  Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from yolov4_amd.darknet import data as D  # noqa: E402

CLASSES = {'point': ('Solarize', 178.5), 'brightness': ('Brightness', 0.27), 'contrast': ('Contrast', 0.27),
           'lut': ('Equalize', 0.0), 'filter': ('Sharpness', 0.27), 'gather': ('Rotate', 9.0)}


def events(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def timed(imgs, params, S, out, a):
    plan = D.upload_jobs(imgs, params, S)
    for _ in range(a.warmup):
        D.launch_jobs(plan, out)
    torch.cuda.synchronize()
    ms = events(lambda: D.launch_jobs(plan, out), a.iters)
    assert bool(torch.isfinite(out).all())
    return ms


def train_step_ms(dev, reps=10):
    import classifier_cases as CC
    from yolov4_amd.darknet.darknet import CSPDarknet53
    from yolov4_amd.darknet.loss import CrossEntropyLoss
    from yolov4_amd.darknet.train import train_step
    from yolov4_amd.yolo.optim.optimizers.build import FusedAdam
    bs, S, N = 64, 256, 1000
    model = CSPDarknet53(N)
    sd = model.state_dict()
    CC.fill_classifier_(sd, 1)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    crit, opt = CrossEntropyLoss(label_smoothing=0.1), FusedAdam(model.parameters(), lr=1e-4)
    g = torch.Generator(device='cpu').manual_seed(0)
    xin, tin = torch.randn((bs, 3, S, S), generator=g).to(dev), torch.randint(0, N, (bs,), generator=g).to(dev)
    for _ in range(3):
        train_step(model, crit, opt, xin, tin)
    torch.cuda.synchronize()
    return events(lambda: train_step(model, crit, opt, xin, tin), reps), bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--src-h', type=int, default=375)
    ap.add_argument('--src-w', type=int, default=500)
    ap.add_argument('--step', action='store_true', help='also time one classifier train step')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'randaug_micro needs an MI355X'
    dev = torch.device('cuda:0')
    B, S, h, w = a.batch, a.size, a.src_h, a.src_w
    g = torch.Generator(device='cpu').manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(B)]
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    train = [D.train_params(h, w, S, rng) for _ in range(B)]
    res = {'bench': 'randaug_micro', 'batch': B, 'size': S, 'src': [h, w], 'iters': a.iters, 'batch_u8_bytes': 3 * B * S * S}

    res['plain_ms'] = round(timed(imgs, train, S, out, a), 4)
    # n_ops = 0 through the new entry point: an operation table of one Identity per sample, passed with n_ops = 0
    plan = D.upload_jobs(imgs, [p._replace(aug=(('Identity', 0.0),)) for p in train], S)
    from yolov4_amd._lib import check, lib

    def ops0():
        st = torch.cuda.current_stream().cuda_stream
        m, s = D._f32_array(D.MEAN), D._f32_array(D.STD)
        check(lib().y4_rcrop_randaug_u8_f32(plan['table'].data_ptr(), plan['host'].data_ptr(), B, S, m, s, out.data_ptr(),
                                            out.stride(0), out.stride(1), out.stride(2), out.stride(3), plan['ws'].data_ptr(),
                                            plan['ws'].numel(), plan['table'].data_ptr() + plan['ops_at'],
                                            plan['host'].data_ptr() + plan['ops_at'], 0, plan['ws2'].data_ptr(),
                                            plan['ws2'].numel(), st), 'y4_rcrop_randaug_u8_f32')
    for _ in range(a.warmup):
        ops0()
    res['ops0_ms'] = round(events(ops0, a.iters), 4)

    src8, dst8 = torch.empty(3 * B * S * S, dtype=torch.uint8, device=dev), torch.empty(3 * B * S * S, dtype=torch.uint8, device=dev)
    for _ in range(a.warmup):
        dst8.copy_(src8)
    res['copy_ms'] = round(events(lambda: dst8.copy_(src8), a.iters), 4)

    for cls, op in CLASSES.items():
        one = timed(imgs, [p._replace(aug=(op,)) for p in train], S, out, a)
        two = timed(imgs, [p._replace(aug=(op, op)) for p in train], S, out, a)
        res['one_%s_ms' % cls], res['two_%s_ms' % cls] = round(one, 4), round(two, 4)
        res['round_%s_ms' % cls] = round(two - one, 4)
        res['round_%s_x_copy' % cls] = round((two - one) / res['copy_ms'], 2)
    res['stats_ms'] = round(res['round_contrast_ms'] - res['round_brightness_ms'], 4)

    ra = D.RandAugment()
    res['default_ms'] = round(timed(imgs, [p._replace(aug=ra.sample(S, rng)) for p in train], S, out, a), 4)
    res['default_extra_ms'] = round(res['default_ms'] - res['plain_ms'], 4)
    if a.step:
        ms, bs = train_step_ms(dev)
        res['train_step_ms'], res['train_step_batch'] = round(ms, 2), bs
        res['default_extra_share_of_step'] = round(res['default_extra_ms'] / (ms * B / bs), 5)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
