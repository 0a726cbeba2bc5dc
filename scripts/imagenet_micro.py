# -*- coding: utf-8 -*-
"""Micro-benchmark of the classifier's input pipeline (yolov4_amd/darknet/data.py on csrc/resample.hip).

    python scripts/imagenet_micro.py [--batch 256] [--size 256] [--val-size 288] [--iters 50] [--warmup 5] [--files 512]

B device-resident 500 x 375 BGR sources -> [B, 3, S, S], the train geometry (RandomResizedCrop + flip, and the same with a
CutMix paste) and the val geometry (Resize + CenterCrop) timed separately, all after warm-up:
  kernels_ms   device events around the two launches alone, on one uploaded job table
  coeffs_ms    the table launch on its own
  model_ms     the byte model: every byte of the crops read once and the fp32 batch written once, at the measured HBM copy
               rate of 6.29 TB/s; bytes_* are what the model counts
  host_ms      host clock around drawing the parameters (`sample_crop`) and writing + uploading the job table
  loader       the whole ImageNetBatchLoader over JPEG files written to a temporary directory with the native encoder:
               file reads, Huffman decoding on the host threads, device decode, this pipeline; images per second
Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov4_amd._lib import check, lib  # noqa: E402
from yolov4_amd.darknet import data as D  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def events(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def geometry(name, imgs, params, S, out, a):
    plan = D.upload_jobs(imgs, params, S)
    for _ in range(a.warmup):
        D.launch_jobs(plan, out)
    torch.cuda.synchronize()
    kernels_ms = events(lambda: D.launch_jobs(plan, out), a.iters)
    st = torch.cuda.current_stream().cuda_stream
    coeffs_ms = events(lambda: check(lib().y4_rcrop_coeffs_i32(plan['table'].data_ptr(), plan['host'].data_ptr(), plan['B'], S,
                                                               plan['ws'].data_ptr(), plan['ws'].numel(), st)), a.iters)
    assert bool(torch.isfinite(out).all())
    read = sum(3 * p.crop_w * p.crop_h for p in params)
    written = 4 * out.numel()
    model_ms = (read + written) / HBM_BYTES_PER_S * 1e3
    return {name + '_kernels_ms': round(kernels_ms, 4), name + '_coeffs_ms': round(coeffs_ms, 4),
            name + '_bytes_read': read, name + '_bytes_written': written, name + '_model_ms': round(model_ms, 4),
            name + '_GBps': round((read + written) / kernels_ms / 1e6, 1),
            name + '_images_per_s_kernels': round(len(imgs) / kernels_ms * 1e3, 1)}


def write_files(root, n, h, w, dev):
    """n smooth synthetic JPEGs (a noise image's entropy-coded size would not be a photograph's) in 4 class directories"""
    from yolov4_amd.yolo.data.jpeg_enc import encode_jpeg_batch
    g = torch.Generator(device='cpu').manual_seed(1)
    for at in range(0, n, 64):
        low = torch.rand((min(64, n - at), 3, h // 16 + 1, w // 16 + 1), generator=g).to(dev)
        img = torch.nn.functional.interpolate(low, size=(h, w), mode='bilinear', align_corners=False)
        img = (img + 0.03 * torch.randn_like(img)).clamp_(0, 1).mul_(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        for k, data in enumerate(encode_jpeg_batch(list(img), quality=90)):
            d = os.path.join(root, 'class%d' % ((at + k) % 4))
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, '%06d.jpg' % (at + k)), 'wb') as f:
                f.write(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--val-size', type=int, default=288)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--src-h', type=int, default=375)
    ap.add_argument('--src-w', type=int, default=500)
    ap.add_argument('--files', type=int, default=512, help='JPEG files of the loader figure (0: skip it)')
    ap.add_argument('--workers', type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'imagenet_micro needs an MI355X'
    dev = torch.device('cuda:0')
    B, S, h, w = a.batch, a.size, a.src_h, a.src_w
    g = torch.Generator(device='cpu').manual_seed(0)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(B)]
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    res = {'bench': 'imagenet_micro', 'batch': B, 'size': S, 'val_size': a.val_size, 'src': [h, w], 'iters': a.iters}

    train = [D.train_params(h, w, S, rng) for _ in range(B)]
    res.update(geometry('train', imgs, train, S, out, a))
    mix = D.sample_cutmix(B, S, rng, 1.0)
    res.update(geometry('train_cutmix', imgs, D.with_cutmix(train, mix), S, out, a))
    res['cutmix_box'] = list(mix[1])
    res.update(geometry('val', imgs, [D.val_params(h, w, a.val_size, S)] * B, S, out, a))

    t0 = time.perf_counter()
    for _ in range(a.iters):
        params = [D.train_params(h, w, S, rng) for _ in range(B)]
    t1 = time.perf_counter()
    for _ in range(a.iters):
        D.upload_jobs(imgs, params, S)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res['host_sample_crop_ms'] = round((t1 - t0) * 1e3 / a.iters, 4)
    res['host_table_fill_ms'] = round((t2 - t1) * 1e3 / a.iters, 4)

    if a.files > 0:
        with tempfile.TemporaryDirectory() as root:
            write_files(root, a.files, h, w, dev)
            ds = D.ImageFolder(root)
            res['loader_file_bytes_mean'] = int(np.mean([os.path.getsize(p) for p, _ in ds.samples]))
            for train_mode in (True, False):
                loader = D.ImageNetBatchLoader(ds, B, train=train_mode, crop_size=S, val_size=a.val_size, shuffle=train_mode,
                                               workers=a.workers, cutmix_prob=1.0 if train_mode else 0.0)
                for _ in loader:                                    # warm-up epoch
                    pass
                torch.cuda.synchronize()
                t0, seen = time.perf_counter(), 0
                for epoch in range(3):
                    loader.set_epoch(epoch + 1)
                    for x, _ in loader:
                        seen += x.shape[0]
                torch.cuda.synchronize()
                res['loader_%s_images_per_s' % ('train' if train_mode else 'val')] = round(seen / (time.perf_counter() - t0), 1)
            res['loader_files'], res['loader_workers'] = len(ds), a.workers
    print(json.dumps(res))


if __name__ == '__main__':
    main()
