# -*- coding: utf-8 -*-
"""Micro-benchmark of the training augmentation (yolov4_amd/yolo/data/transform.py: train_batch on csrc/augment.hip).

    python scripts/augment_micro.py [--batch 64] [--size 608] [--iters 50] [--warmup 5]

B mosaic samples of four synthetic 640x480 BGR sources each, already on the device, S = 608, reference-default jitter.
Three figures per batch, all after warm-up and all ending in a device synchronise:
  kernels_ms  device events around the sums launch + the gather launch alone, on one uploaded descriptor table
              (sums_ms, gather_ms: each launch on its own)
  device_ms   device events around `train_batch` with parameters drawn beforehand: host box arithmetic, descriptor upload
              and both launches (bounded by the host when the host is slower than the device)
  wall_ms     host clock around `sample_train_params` + `train_batch`: what a loader thread pays per batch
Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov4_amd.yolo.data import transform as T  # noqa: E402

CFG = {'AUGMENTATION': {'JITTER': 0.3, 'RANDOM_HORIZONTAL_FLIP': True, 'COLOR_DITHERING': True, 'HUE': 0.1,
                        'SATURATION': 1.5, 'EXPOSURE': 1.5, 'IS_MOSAIC': True, 'MIN_OFFSET': 0.2},
       'DATA': {'MAX_NUM_LABELS': 60}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--src-h', type=int, default=480)
    ap.add_argument('--src-w', type=int, default=640)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'augment_micro needs an MI355X'
    dev = torch.device('cuda:0')
    B, S, h, w = a.batch, a.size, a.src_h, a.src_w
    g = torch.Generator(device='cpu').manual_seed(0)
    pool = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4 * B)]
    rs = np.random.RandomState(0)
    boxes = [np.concatenate([rs.uniform(0, w / 2, (8, 1)), rs.uniform(0, h / 2, (8, 1)), rs.uniform(8, w / 2, (8, 1)),
                             rs.uniform(8, h / 2, (8, 1)), rs.randint(0, 80, (8, 1))], 1) for _ in range(4 * B)]
    items = [(pool[4 * b:4 * b + 4], boxes[4 * b:4 * b + 4]) for b in range(B)]
    rng = random.Random(0)

    def draw():
        return [T.sample_train_params(CFG, [(h, w)] * 4, S, rng, [8] * 4) for _ in range(B)]

    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    for _ in range(a.warmup):
        T.train_batch(items, S, CFG, params=draw(), out=out)
    torch.cuda.synchronize()

    drawn = [draw() for _ in range(a.iters)]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for p in drawn:
        T.train_batch(items, S, CFG, params=p, out=out)
    stop.record()
    torch.cuda.synchronize()
    device_ms = start.elapsed_time(stop) / a.iters

    plan = T.upload_batch(items, drawn[0], S, 60, dev)             # the two launches alone, on one uploaded table
    T.launch_batch(plan, out)
    torch.cuda.synchronize()
    start.record()
    for _ in range(a.iters):
        T.launch_batch(plan, out)
    stop.record()
    torch.cuda.synchronize()
    kernels_ms = start.elapsed_time(stop) / a.iters

    from yolov4_amd._lib import check, lib                        # each launch on its own
    hp, dp, nb, st = plan['host'].data_ptr(), plan['table'].data_ptr(), plan['src_bytes'], torch.cuda.current_stream().cuda_stream
    start.record()
    for _ in range(a.iters):
        check(lib().y4_augment_means_u8(dp, hp, plan['n_table'], plan['sums'].data_ptr(), st))
    stop.record()
    torch.cuda.synchronize()
    sums_ms = start.elapsed_time(stop) / a.iters
    start.record()
    for _ in range(a.iters):
        check(lib().y4_augment_mosaic_u8_f32(dp, hp, plan['n_table'], dp + nb, hp + nb, B, plan['sums'].data_ptr(), out.data_ptr(),
                                             out.stride(0), out.stride(1), out.stride(2), out.stride(3), S, st))
    stop.record()
    torch.cuda.synchronize()
    gather_ms = start.elapsed_time(stop) / a.iters

    t0 = time.perf_counter()
    for _ in range(a.iters):
        T.train_batch(items, S, CFG, params=draw(), out=out)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / a.iters

    assert torch.isfinite(out).all() and float(out.min()) >= 0 and float(out.max()) <= 1
    written = 3 * 4 * S * S * B
    print(json.dumps({'bench': 'augment_micro', 'batch': B, 'size': S, 'src': [h, w], 'mosaic': True, 'iters': a.iters,
                      'kernels_ms_per_batch': round(kernels_ms, 4), 'sums_ms_per_batch': round(sums_ms, 4),
                      'gather_ms_per_batch': round(gather_ms, 4), 'bytes_summed_per_batch': 4 * B * h * w * 3,
                      'device_ms_per_batch': round(device_ms, 4),
                      'wall_ms_per_batch': round(wall_ms, 4), 'images_per_s_kernels': round(B / kernels_ms * 1e3, 1),
                      'images_per_s_wall': round(B / wall_ms * 1e3, 1),
                      'source_images_per_s_wall': round(4 * B / wall_ms * 1e3, 1),
                      'bytes_written_per_batch': written, 'write_GBps_kernels': round(written / kernels_ms / 1e6, 1)}))


if __name__ == '__main__':
    main()
