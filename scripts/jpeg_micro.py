# -*- coding: utf-8 -*-
"""Micro-benchmark of JPEG decoding (yolov4_amd/yolo/data/jpeg.py on csrc/jpeg_host.h + csrc/jpeg.hip).

    python scripts/jpeg_micro.py [--dir DIR] [--batch 256] [--iters 20] [--warmup 3] [--threads 16]

The files: every *.jpg / *.jpeg under --dir (unsupported ones are skipped and counted), or, without --dir and with Pillow
importable, 32 synthetic 640x480 4:2:0 files at quality 90 (a textured picture, about 100 KB each); the batch cycles through them.
Figures, all after warm-up:
  host_ms_per_image_per_thread    y4_jpeg_parse_host + y4_jpeg_entropy_host on ONE thread, per image.  16 host threads feeding
                                  4 GPUs at 464 images/s of 4-image mosaic leave at most 8.6 ms per image per thread.
  pil_ms_per_image                Pillow's FULL decode (Huffman + IDCT + colour) of the same files on one thread, for
                                  comparison only (absent without Pillow)
  host_ms_per_batch_threads       `entropy_batch` of the whole batch on --threads threads into pinned memory
  device_ms_per_batch             device events around `decode_entropy_batch`: the pinned copy and the two launches
  kernels_ms_per_batch            the two launches alone, on coefficients already on the device
  share_of_step                   device_ms_per_batch / 139.8 ms, the bs = 64 training step one batch of 256 images feeds
Prints one JSON line.  The device figures need an MI355X: there is no fallback (--host-only skips them)."""
import argparse
import glob
import io
import json
import os
import sys
import time

import ctypes
import numpy as np
import torch            # before the library is loaded, as everywhere in this tree: one HIP runtime, the one torch brings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov4_amd._lib import JpegInfo, lib  # noqa: E402

STEP_MS = 139.8


def synth(n):
    from PIL import Image
    rs = np.random.RandomState(0)
    out = []
    for i in range(n):
        y, x = np.mgrid[0:480, 0:640].astype(np.float64)
        img = np.stack([128 + 100 * np.sin(x / (7.0 + i) + y / 13.0), 128 + 100 * np.cos(x / 11.0 - y / (5.0 + i)),
                        (x + y + 37 * i) % 256], axis=2)
        blocks = rs.randint(0, 256, (30, 40, 3)).astype(np.float64)                    # 16-pixel colour patches: edges in every MCU
        img = 0.6 * img + 0.4 * np.kron(blocks, np.ones((16, 16, 1))) + rs.randn(480, 640, 3) * 8
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format='JPEG', quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def host_one_thread(files, iters):
    L = lib()
    infos, bufs, qt = [], [], np.zeros((3, 64), np.uint16)
    for d in files:
        info = JpegInfo()
        assert L.y4_jpeg_parse_host(d, len(d), ctypes.byref(info)) == 0
        infos.append(info)
        bufs.append(np.empty(info.coef_count, np.int16))
    t0 = time.perf_counter()
    for _ in range(iters):
        for d, info, b in zip(files, infos, bufs):
            L.y4_jpeg_parse_host(d, len(d), ctypes.byref(info))
            rc = L.y4_jpeg_entropy_host(d, len(d), ctypes.byref(info), b.ctypes.data, info.coef_count, qt.ctypes.data)
            assert rc == 0
    return (time.perf_counter() - t0) * 1e3 / (iters * len(files))


def pil_one_thread(files, iters):
    try:
        from PIL import Image
    except ImportError:
        return None
    t0 = time.perf_counter()
    for _ in range(iters):
        for d in files:
            im = Image.open(io.BytesIO(d))
            im.load()
    return (time.perf_counter() - t0) * 1e3 / (iters * len(files))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dir')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-only', action='store_true')
    a = ap.parse_args()
    skipped = 0
    if a.dir:
        paths = sorted(glob.glob(os.path.join(a.dir, '**', '*.jp*g'), recursive=True))
        files = []
        for p in paths:
            with open(p, 'rb') as f:
                d = f.read()
            info = JpegInfo()
            if lib().y4_jpeg_parse_host(d, len(d), ctypes.byref(info)) == 0:
                files.append(d)
            else:
                skipped += 1
        source = a.dir
    else:
        files = synth(32)
        source = 'synthetic 640x480 4:2:0 q90'
    assert files, 'no decodable JPEG files'
    res = {'bench': 'jpeg_micro', 'source': source, 'files': len(files), 'skipped': skipped,
           'mean_file_bytes': int(np.mean([len(d) for d in files])), 'batch': a.batch, 'threads': min(a.threads, 16)}
    host_one_thread(files, 1)
    res['host_ms_per_image_per_thread'] = round(host_one_thread(files, max(1, a.iters // 4)), 4)
    res['host_bound_ms_per_image_per_thread'] = 8.6
    pil = pil_one_thread(files, max(1, a.iters // 4))
    if pil is not None:
        res['pil_ms_per_image'] = round(pil, 4)

    batch = [files[i % len(files)] for i in range(a.batch)]
    if not a.host_only:
        from concurrent.futures import ThreadPoolExecutor
        from yolov4_amd.yolo.data.jpeg import decode_entropy_batch, entropy_batch
        assert torch.cuda.is_available(), 'the device figures need an MI355X'
        with ThreadPoolExecutor(max_workers=min(a.threads, 16)) as pool:
            for _ in range(a.warmup):
                hb = entropy_batch(batch, pool=pool)
            t0 = time.perf_counter()
            for _ in range(a.iters):
                hb = entropy_batch(batch, pool=pool)
            res['host_ms_per_batch_threads'] = round((time.perf_counter() - t0) * 1e3 / a.iters, 3)
        for _ in range(a.warmup):
            out = decode_entropy_batch(hb)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            out = decode_entropy_batch(hb)
        stop.record()
        torch.cuda.synchronize()
        res['device_ms_per_batch'] = round(start.elapsed_time(stop) / a.iters, 4)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            out = decode_entropy_batch(hb)
        torch.cuda.synchronize()
        res['wall_ms_per_batch_device_stage'] = round((time.perf_counter() - t0) * 1e3 / a.iters, 4)

        # the two launches alone: the table and the coefficients stay where the last call put them
        dev = torch.empty(hb.host.numel(), dtype=torch.uint8, device='cuda')
        ws = torch.empty(sum((int(hb.infos[i].coef_count) + 15) & ~15 for i in hb.jobs_of), dtype=torch.uint8, device='cuda')
        for j in range(len(hb.jobs_of)):
            hb.jobs[j].coef = dev.data_ptr() + hb.coef_offsets[j]
        dev.copy_(hb.host)
        st = torch.cuda.current_stream().cuda_stream
        args = (dev.data_ptr(), hb.host.data_ptr(), len(hb.jobs_of), ws.data_ptr(), ws.numel(), st)
        assert lib().y4_jpeg_decode_u8(*args) == 0
        torch.cuda.synchronize()
        start.record()
        for _ in range(a.iters):
            lib().y4_jpeg_decode_u8(*args)
        stop.record()
        torch.cuda.synchronize()
        res['kernels_ms_per_batch'] = round(start.elapsed_time(stop) / a.iters, 4)
        res['share_of_step'] = round(res['device_ms_per_batch'] / STEP_MS, 5)
        res['coef_bytes_per_batch'] = int(sum(2 * hb.infos[i].coef_count for i in hb.jobs_of))
        res['pixel_bytes_per_batch'] = int(sum(t.shape[0] * t.shape[1] * 3 for t in out))
        res['images_per_s_device'] = round(a.batch / res['device_ms_per_batch'] * 1e3, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
