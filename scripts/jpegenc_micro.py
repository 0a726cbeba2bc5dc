# -*- coding: utf-8 -*-
"""Micro-benchmark of JPEG encoding and box drawing (yolov4_amd/yolo/data/jpeg_enc.py on csrc/jpeg_enc.hip +
csrc/jpeg_enc_host.h; yolov4_amd/yolo/util/vis.py on csrc/draw.hip).

    python scripts/jpegenc_micro.py [--batch 64] [--iters 20] [--warmup 3] [--threads 16] [--boxes 100]

The images: --batch device-resident 640x480 BGR pictures (smooth gradients, 16-pixel colour patches and mild noise; they cycle
through 8 different ones), encoded at 4:2:0, quality 95 -- cv2.imwrite's defaults.  Figures, all after warm-up:
  encode_kernel_ms_per_batch      device events around y4_jpeg_encode_u8 alone (one launch), table already on the device
  copy_back_ms_per_batch          device events around the ONE device -> host copy of the coefficients into pinned memory
  device_stage_wall_ms_per_batch  wall time of `coefficients_batch`: table upload, launch, copy back, the wait
  host_ms_per_image_one_thread    y4_jpeg_encode_host (markers + Huffman) on ONE thread, per image
  host_ms_per_batch_threads       `huffman_batch` of the whole batch on --threads threads; .._per_image is that / batch
  pil_ms_per_image                Pillow's FULL `save` (colour, FDCT, Huffman) of the same pixels on one thread: the yardstick
  draw_ms_per_batch               device events around the table upload and the one launch of `draw_detections` with --boxes
                                  labelled boxes per image; draw_wall_ms_per_batch: the whole call, host preparation included
  share_of_step                   (encode kernel + copy back) / 139.8 ms, the bs = 64 training step
Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch            # before the library is loaded, as everywhere in this tree: one HIP runtime, the one torch brings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov4_amd._lib import JpegEncJob, lib  # noqa: E402

STEP_MS = 139.8
W, H = 640, 480


def synth(n):
    rs = np.random.RandomState(0)
    out = []
    for i in range(n):
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        img = np.stack([128 + 100 * np.sin(x / (7.0 + i) + y / 13.0), 128 + 100 * np.cos(x / 11.0 - y / (5.0 + i)),
                        (x + y + 37 * i) % 256], axis=2)
        blocks = rs.randint(0, 256, (H // 16, W // 16, 3)).astype(np.float64)
        img = 0.6 * img + 0.4 * np.kron(blocks, np.ones((16, 16, 1))) + rs.randn(H, W, 3) * 8
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def events(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--boxes', type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    from yolov4_amd.yolo.data.jpeg_enc import coefficients_batch, huffman_batch
    from yolov4_amd.yolo.util.vis import class_colors, draw_detections, plan_draw, run_draw
    L = lib()
    pictures = synth(8)
    images = [torch.from_numpy(np.ascontiguousarray(pictures[i % 8][..., ::-1])).cuda() for i in range(a.batch)]
    res = {'bench': 'jpegenc_micro', 'batch': a.batch, 'size': [W, H], 'quality': 95, 'subsampling': '420',
           'threads': min(a.threads, 16), 'boxes_per_image': a.boxes}

    for _ in range(a.warmup):
        eb = coefficients_batch(images)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        eb = coefficients_batch(images)
    res['device_stage_wall_ms_per_batch'] = round((time.perf_counter() - t0) * 1e3 / a.iters, 4)

    # the launch alone, and the copy alone, on a table that stays on the device
    n = a.batch
    table = torch.zeros(n * ctypes.sizeof(JpegEncJob), dtype=torch.uint8, pin_memory=True)
    jobs = (JpegEncJob * n).from_buffer(table.numpy())
    dev_coef = torch.empty(eb.host.numel(), dtype=torch.uint8, device='cuda')
    for i, t in enumerate(images):
        jobs[i].pixels, jobs[i].coef, jobs[i].pitch = t.data_ptr(), dev_coef.data_ptr() + eb.offsets[i], t.stride(0)
        jobs[i].info, jobs[i].qt = eb.infos[i], eb.qts[i]
    dev_table = table.cuda()
    st = torch.cuda.current_stream().cuda_stream
    launch = lambda: L.y4_jpeg_encode_u8(dev_table.data_ptr(), table.data_ptr(), n, st)
    assert launch() == 0
    torch.cuda.synchronize()
    assert torch.equal(dev_coef.cpu(), eb.host), 'the bare launch and coefficients_batch disagree'
    events(launch, a.warmup)
    res['encode_kernel_ms_per_batch'] = round(events(launch, a.iters), 4)
    pinned = torch.empty(eb.host.numel(), dtype=torch.uint8, pin_memory=True)
    copy = lambda: pinned.copy_(dev_coef, non_blocking=True)
    events(copy, a.warmup)
    res['copy_back_ms_per_batch'] = round(events(copy, a.iters), 4)
    res['coef_bytes_per_batch'] = int(eb.host.numel())
    res['pixel_bytes_per_batch'] = int(n * W * H * 3)

    huffman_batch(eb, workers=1)
    t0 = time.perf_counter()
    reps = max(1, a.iters // 4)
    for _ in range(reps):
        files = huffman_batch(eb, workers=1)
    res['host_ms_per_image_one_thread'] = round((time.perf_counter() - t0) * 1e3 / (reps * n), 4)
    res['mean_file_bytes'] = int(np.mean([len(f) for f in files]))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(a.threads, 16)) as pool:
        for _ in range(a.warmup):
            huffman_batch(eb, pool=pool)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            huffman_batch(eb, pool=pool)
        res['host_ms_per_batch_threads'] = round((time.perf_counter() - t0) * 1e3 / a.iters, 3)
    res['host_ms_per_image_threads'] = round(res['host_ms_per_batch_threads'] / n, 4)

    try:
        from PIL import Image
        pil = [Image.fromarray(p) for p in pictures]
        same = io.BytesIO()
        pil[0].save(same, format='JPEG', quality=95, subsampling=2)
        res['bytes_equal_pillow'] = bool(same.getvalue() == files[0])
        t0 = time.perf_counter()
        for _ in range(reps):
            for i in range(n):
                pil[i % 8].save(io.BytesIO(), format='JPEG', quality=95, subsampling=2)
        res['pil_ms_per_image'] = round((time.perf_counter() - t0) * 1e3 / (reps * n), 4)
    except ImportError:
        pass

    rs = np.random.RandomState(1)
    boxes, labels, colors = [], [], []
    palette = class_colors(80)
    for _ in range(n):
        x1, y1 = rs.randint(0, W - 40, a.boxes), rs.randint(0, H - 40, a.boxes)
        bw, bh = rs.randint(20, 300, a.boxes), rs.randint(20, 300, a.boxes)
        cls = rs.randint(0, 80, a.boxes)
        boxes.append(np.stack([x1, y1, x1 + bw, y1 + bh], axis=1))
        labels.append(['class%d 0.%02d' % (c, c) for c in cls])
        colors.append(palette[cls])
    plan = plan_draw(images, boxes, labels, colors)
    events(lambda: run_draw(plan), a.warmup)
    res['draw_ms_per_batch'] = round(events(lambda: run_draw(plan), a.iters), 4)
    draw = lambda: draw_detections(images, boxes, labels, colors)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        draw()
    torch.cuda.synchronize()
    res['draw_wall_ms_per_batch'] = round((time.perf_counter() - t0) * 1e3 / a.iters, 4)
    res['share_of_step'] = round((res['encode_kernel_ms_per_batch'] + res['copy_back_ms_per_batch']) / STEP_MS, 5)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
