# -*- coding: utf-8 -*-
"""Times letterboxed / rectangular-batch inference on the MI355X (GPU only), device events around --steps calls after
--warmup calls, for --batch (default 32) device-resident 640 x 480 sources at S = 608:

    preprocess   whole CALLS of val_batch (one y4_preprocess_u8_f32 launch per image, stretch to 608 x 608) against
                 letterbox_batch (one y4_letterbox_batch_u8_f32 launch per batch) in 'square' (608 x 608) and 'rect'
                 (480 x 608) mode: host work (geometry, the pinned table, its copy, the allocation) and enqueue included
    launches     the C entries alone, on a table and a destination prepared once: 32 y4_preprocess_u8_f32 launches against one
                 y4_letterbox_batch_u8_f32 launch ('square' and 'rect'), --kernel-steps calls per window (default 2000), with
                 the bytes written (12 per output pixel) and the bytes/s that makes
    infer        images/s of model + decode + postprocess_nms(max_det=100) on 608 x 608 against 480 x 608 inputs: the same
                 weights, BatchNorm statistics calibrated as recipe.calibrate_bn_ does, alternated --rounds times within
                 this process; `rect_over_square` is the ratio of the best rounds (the pixel ratio is 608 / 480 = 1.27)
    layers       with --layers: every ConvBNAct of the model timed alone at both shapes (forward hooks around device
                 events), the layers whose 480 x 608 time is not below their 608 x 608 time listed

    python scripts/letterbox_micro.py [--batch 32] [--steps 10] [--warmup 3] [--rounds 3] [--kernel-steps 2000] [--layers]

Prints one JSON line."""
import argparse
import ctypes
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
from yolov4_amd._lib import LetterboxSrc, lib  # noqa: E402
from yolov4_amd.yolo.data.transform import (letterbox_batch, letterbox_canvas, letterbox_geometry, letterbox_offsets,  # noqa: E402
                                            val_batch)
from yolov4_amd.yolo.model.yolov4 import YOLOv4  # noqa: E402
from yolov4_amd.yolo.util.utils import postprocess_nms  # noqa: E402

S, SRC_H, SRC_W = 608, 480, 640


def timed(fn, steps, warmup):
    """microseconds per call"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def layer_times(model, x, steps):
    """name -> microseconds of every leaf conv module's forward at this input, device events in forward hooks"""
    from yolov4_amd.darknet.darknet import ConvBNAct
    events, hooks = {}, []
    for name, mod in model.named_modules():
        if isinstance(mod, ConvBNAct):
            def pre(m, inp, name=name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events.setdefault(name, []).append([e, None])

            def post(m, inp, out, name=name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events[name][-1][1] = e
            hooks += [mod.register_forward_pre_hook(pre), mod.register_forward_hook(post)]
    with torch.no_grad():
        for _ in range(steps + 1):
            model(x)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    return {n: min(a.elapsed_time(b) for a, b in ev[1:]) * 1e3 for n, ev in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--layers', action='store_true')
    ap.add_argument('--kernel-steps', type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('letterbox_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    B = args.batch
    res = {'size': S, 'source': [SRC_H, SRC_W], 'batch': B, 'conv_mode': int(lib().y4_get_conv_mode())}

    # ---- preprocess: B device-resident sources
    rng = np.random.RandomState(0)
    srcs = [torch.from_numpy(rng.randint(0, 256, (SRC_H, SRC_W, 3)).astype(np.uint8)).to(dev) for _ in range(B)]
    pre = {}
    rounds = []
    for _ in range(args.rounds):
        rounds.append((timed(lambda: val_batch(srcs, S), args.steps * 100, args.warmup),
                       timed(lambda: letterbox_batch(srcs, S, 'square', 32), args.steps * 100, args.warmup),
                       timed(lambda: letterbox_batch(srcs, S, 'rect', 32), args.steps * 100, args.warmup)))
    x_rect, infos = letterbox_batch(srcs, S, 'rect', 32)
    Hc, Wc = int(x_rect.shape[2]), int(x_rect.shape[3])
    for k, (name, pix) in enumerate((('val_batch', S * S), ('letterbox_square', S * S), ('letterbox_rect', Hc * Wc))):
        us = min(r[k] for r in rounds)
        out_bytes = B * pix * 12
        pre[name] = {'us': us, 'launches': B if k == 0 else 1, 'bytes_written': out_bytes, 'GBps_written': out_bytes / us / 1e3}
    pre['rounds_us'] = rounds
    pre['rect_canvas'] = [Hc, Wc]
    pre['square_over_val_batch'] = pre['letterbox_square']['us'] / pre['val_batch']['us']
    pre['rect_over_val_batch'] = pre['letterbox_rect']['us'] / pre['val_batch']['us']
    res['preprocess'] = pre

    # ---- the launches alone: table and destination prepared once, the C entries called directly
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    kern = {}
    dst_sq = torch.empty((B, 3, S, S), device=dev)

    def per_image():
        for b, t in enumerate(srcs):
            d = dst_sq[b]
            L.y4_preprocess_u8_f32(t.data_ptr(), SRC_H, SRC_W, t.stride(0), 1, d.data_ptr(), d.stride(0), d.stride(1), d.stride(2), S, stream)
    calls = {'preprocess_32_launches': (per_image, S * S)}
    keep = []
    for mode in ('square', 'rect'):
        geo = [letterbox_geometry(SRC_H, SRC_W, S)] * B
        hc, wc = letterbox_canvas(geo, S, mode, 32)
        host = (LetterboxSrc * B)()
        for r, t, (nh, nw) in zip(host, srcs, geo):
            top, left = letterbox_offsets(nh, nw, hc, wc)
            r.src, r.h, r.w, r.pitch, r.swap_rb, r.nh, r.nw, r.top, r.left = t.data_ptr(), SRC_H, SRC_W, t.stride(0), 1, nh, nw, top, left
        tdev = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(dev)
        dst = torch.empty((B, 3, hc, wc), device=dev)
        keep.append((host, tdev, dst))

        def one(host=host, tdev=tdev, dst=dst, hc=hc, wc=wc):
            L.y4_letterbox_batch_u8_f32(tdev.data_ptr(), ctypes.addressof(host), B, dst.data_ptr(), *dst.stride(), hc, wc, 114, stream)
        calls['letterbox_' + mode] = (one, hc * wc)
    rounds = [[timed(fn, args.kernel_steps, 20) for fn, _ in calls.values()] for _ in range(args.rounds)]
    for k, (name, (_, pix)) in enumerate(calls.items()):
        us = min(r[k] for r in rounds)
        kern[name] = {'us': us, 'bytes_written': B * pix * 12, 'GBps_written': B * pix * 12 / us / 1e3}
    kern['rounds_us'] = rounds
    res['launches'] = kern

    # ---- model + decode + NMS at both shapes, same weights and statistics
    model = YOLOv4(recipe.MODEL_CFG, device=dev)
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 7)
    model.load_state_dict(sd)
    model = model.to(dev)
    recipe.calibrate_bn_(model, recipe.randn((8, 3, 128, 128), 3).to(dev))
    model.eval()
    x_sq, _ = letterbox_batch(srcs, S, 'square', 32)
    inputs = {'square': x_sq, 'rect': x_rect}

    def infer(x):
        with torch.no_grad():
            postprocess_nms(model(x), 80, 0.5, 0.45, max_det=100)
    rounds = []
    for _ in range(args.rounds):
        rounds.append((timed(lambda: infer(x_sq), args.steps, args.warmup), timed(lambda: infer(x_rect), args.steps, args.warmup)))
    t_sq, t_rect = min(r[0] for r in rounds), min(r[1] for r in rounds)
    res['infer'] = {'square': {'shape': list(x_sq.shape[2:]), 'us': t_sq, 'img_s': B / t_sq * 1e6},
                    'rect': {'shape': [Hc, Wc], 'us': t_rect, 'img_s': B / t_rect * 1e6},
                    'rounds_us': rounds, 'rect_over_square': t_sq / t_rect, 'pixel_ratio': S * S / (Hc * Wc)}
    if args.layers:
        lt = {k: layer_times(model, v, 3) for k, v in inputs.items()}
        losers = {n: [lt['square'][n], lt['rect'][n]] for n in lt['square'] if lt['rect'][n] >= lt['square'][n]}
        res['layers'] = {'conv_sum_us': {k: sum(v.values()) for k, v in lt.items()}, 'rect_not_faster': losers,
                         'n_layers': len(lt['square'])}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
