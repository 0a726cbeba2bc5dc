# -*- coding: utf-8 -*-
"""Times the test-time-augmentation pieces on the MI355X.

    python scripts/tta_micro.py [--what view,merge,wbf,e2e] [--batch 32] [--steps 5] [--warmup 2] [--rounds 3]

  view   y4_tta_view_f32 at batch x 3 x 608 x 608, r = 0.83 mirrored: microseconds per launch and achieved bytes / s against
         the bytes it must move (the view written + the input read once); for information the same view composed from torch
         ops (F.interpolate + flip + pad: the same geometry, not the same bits).
  merge  y4_tta_merge_f32 at batch x 22 743 x 85 per view (mirrored, scaled): microseconds per launch and bytes / s (read +
         written); for information torch.cat of three views plus the four column operations on one of them.
  wbf    postprocess_wbf against postprocess_nms's defaults on a three-view prediction made from scripts/nms_micro.py's
         synthetic one (views 2 and 3: its boxes jittered by a few per cent, merged by the merge kernel), at conf 0.001 and
         0.25, per class and agnostic, without and with max_det = 100: rows per image and milliseconds per call.
  e2e    model + decode + post-process in images / s at 608 x 608: no TTA, 3-view TTA + NMS, 3-view TTA + WBF (random
         calibrated weights; the confidence threshold leaves about 500 candidates per image and view, as bench.py --infer).

Every variant is warmed up, the variants of a group alternate --rounds times, the best round counts; a call is timed with
the host clock around the launches and the device synchronisation.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.append(p)

from yolov4_amd import ops  # noqa: E402
from yolov4_amd._lib import check, lib  # noqa: E402
from yolov4_amd.yolo.util import tta as T  # noqa: E402
from yolov4_amd.yolo.util import utils as U  # noqa: E402


def best_of(variants, steps, warmup, rounds):
    """{name: fn} -> {name: (best seconds per call, every round)}; fn() launches, the clock includes the synchronisation"""
    for fn in variants.values():
        for _ in range(max(1, warmup)):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / steps)
    return {k: (min(v), v) for k, v in res.items()}


def bench_view(args, dev):
    B, S, r = args.batch, args.size, 0.83
    x = torch.rand((B, 3, S, S), device=dev)
    ch, cw, Hv, Wv, ry, rx = T.view_geometry(S, S, r, 32)
    out = torch.empty((B, 3, Hv, Wv), device=dev)
    L = lib()

    def hip():
        check(L.y4_tta_view_f32(ops._ptr(x), B, 3, S, S, *x.stride(), ops._ptr(out), Hv, Wv, *out.stride(), ch, cw, ry, rx, 1,
                                T.TTA_FILL, ops._stream()), 'view')

    def torch_ops():
        v = F.interpolate(x, size=(ch, cw), mode='bilinear', align_corners=False, antialias=False)
        v = F.pad(v, (0, Wv - cw, 0, Hv - ch), value=T.TTA_FILL)
        return torch.flip(v, dims=[3])
    t = best_of({'hip': hip, 'torch': torch_ops}, args.steps * 4, args.warmup, args.rounds)
    nbytes = 4.0 * B * 3 * (Hv * Wv + S * S)
    return {'shape': [B, 3, S, S], 'view': [Hv, Wv], 'content': [ch, cw], 'bytes': nbytes,
            'hip_us': t['hip'][0] * 1e6, 'hip_GBps': nbytes / t['hip'][0] / 1e9, 'hip_us_rounds': [v * 1e6 for v in t['hip'][1]],
            'torch_us': t['torch'][0] * 1e6, 'torch_us_rounds': [v * 1e6 for v in t['torch'][1]]}


def bench_merge(args, dev):
    B, N, n_ch = args.batch, args.boxes, 85
    preds = [torch.rand((B, N, n_ch), device=dev) * 600 for _ in range(3)]
    out = torch.empty((B, 3 * N, n_ch), device=dev)
    inv = float(np.float32(608) / np.float32(504))
    L = lib()

    def hip():
        check(L.y4_tta_merge_f32(ops._ptr(preds[1]), B, N, n_ch, ops._ptr(out), 3 * N, N, 512.0, 1, inv, inv, ops._stream()), 'merge')

    def hip_identity():
        check(L.y4_tta_merge_f32(ops._ptr(preds[0]), B, N, n_ch, ops._ptr(out), 3 * N, 0, 608.0, 0, 1.0, 1.0, ops._stream()), 'merge')

    def torch_ops():
        m = torch.cat(preds, dim=1)
        v = m[:, N:2 * N]
        v[..., 0] = (512.0 - v[..., 0]) * inv
        v[..., 1] *= inv
        v[..., 2] *= inv
        v[..., 3] *= inv
        return m
    t = best_of({'hip': hip, 'hip_identity': hip_identity, 'torch_cat3_cols1': torch_ops}, args.steps * 4, args.warmup, args.rounds)
    nbytes = 2.0 * 4 * B * N * n_ch
    return {'shape': [B, N, n_ch], 'bytes_per_view': nbytes,
            'hip_us': t['hip'][0] * 1e6, 'hip_GBps': nbytes / t['hip'][0] / 1e9, 'hip_us_rounds': [v * 1e6 for v in t['hip'][1]],
            'hip_identity_us': t['hip_identity'][0] * 1e6, 'hip_identity_GBps': nbytes / t['hip_identity'][0] / 1e9,
            'torch_cat3_cols1_us': t['torch_cat3_cols1'][0] * 1e6,
            'torch_us_rounds': [v * 1e6 for v in t['torch_cat3_cols1'][1]]}


def three_view_prediction(B, N, C, dev):
    from nms_micro import synth_prediction
    base = synth_prediction(B, N, C, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    preds = [base]
    for _ in range(2):
        v = base.clone()
        j = 1 + 0.04 * (torch.rand((B, N, 4), generator=g, device=dev) - 0.5)
        v[..., :4] *= j
        v[..., 4] *= 0.9 + 0.2 * torch.rand((B, N), generator=g, device=dev)
        preds.append(v.contiguous())
    ident = dict(Wv=608, flip=False, inv_sx=1.0, inv_sy=1.0)
    return base, T.merge_views(preds, [ident] * 3)


def bench_wbf(args, dev):
    B, N, C = args.batch, args.boxes, 80
    base, merged = three_view_prediction(B, N, C, dev)
    out = {}
    for conf in (0.001, 0.25):
        cand = int(((merged[..., 5:] * merged[..., 4:5]) >= conf).sum())
        variants, rows = {}, {}
        variants['postprocess(1 view)'] = lambda conf=conf: U.postprocess(base.clone(), C, conf, 0.45)
        for agn in (False, True):
            for md in (0, 100):
                tag = ('agnostic' if agn else 'per-class') + ('+max_det' if md else '')
                variants['nms ' + tag] = lambda conf=conf, agn=agn, md=md: U.postprocess_nms(merged.clone(), C, conf, 0.45, agnostic=agn, max_det=md)
                variants['wbf ' + tag] = lambda conf=conf, agn=agn, md=md: U.postprocess_wbf(merged.clone(), C, conf, 0.55, views=3, agnostic=agn, max_det=md)
        for k, fn in variants.items():
            res = fn()
            rows[k] = sum(0 if d is None else int(d.shape[0]) for d in res) / B
        t = best_of(variants, args.steps, 1, args.rounds)
        out['conf=%g' % conf] = {'candidates_per_image': cand / B,
                                 **{k: {'ms': round(t[k][0] * 1e3, 3), 'ms_rounds': [round(v * 1e3, 3) for v in t[k][1]],
                                        'rows_per_image': round(rows[k], 1)} for k in variants}}
    out['note'] = 'ms include the clone of the prediction (the post-process rewrites its boxes in place)'
    return out


def bench_e2e(args, dev):
    import recipe
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    B, S = args.batch, args.size
    m = YOLOv4(recipe.MODEL_CFG, device=dev)
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, 1234)
    m.load_state_dict(sd)
    m = m.to(dev)
    recipe.calibrate_bn_(m, recipe.randn((8, 3, S, S), 77).to(dev))
    m.eval()
    x = recipe.randn((B, 3, S, S), 78).to(dev)
    with torch.no_grad():
        o = m(x)
        sc = (o[..., 4:5] * o[..., 5:]).flatten()
        pick = torch.randint(0, sc.numel(), (1000000,), device=dev, generator=torch.Generator(device=dev).manual_seed(79))
        thr = float(torch.quantile(sc[pick], 1 - 500.0 / (o.shape[1] * 80)))
        del o, sc
        nms, wbf = T.TTAOptions(merge='nms'), T.TTAOptions(merge='wbf')
        rows = {}

        def plain():
            rows['no_tta'] = U.postprocess(m(x), 80, thr, 0.4)

        def tta_nms():
            rows['tta3_nms'] = T.tta_postprocess(T.tta_predict(m, x, nms), 80, thr, 0.4, nms)

        def tta_wbf():
            rows['tta3_wbf'] = T.tta_postprocess(T.tta_predict(m, x, wbf), 80, thr, 0.4, wbf)
        t = best_of({'no_tta': plain, 'tta3_nms': tta_nms, 'tta3_wbf': tta_wbf}, args.steps, args.warmup, args.rounds)
    return {'batch': B, 'size': S, 'conf_thre': thr, 'views': list(zip(nms.scales, nms.flips)),
            **{k: {'images_per_s': B / t[k][0], 'ms': t[k][0] * 1e3, 'ms_rounds': [v * 1e3 for v in t[k][1]],
                   'rows_per_image': sum(0 if d is None else len(d) for d in rows[k]) / B} for k in t}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='view,merge,wbf,e2e')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--boxes', type=int, default=22743)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tta_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'rounds': args.rounds}
    for what in args.what.split(','):
        out[what] = {'view': bench_view, 'merge': bench_merge, 'wbf': bench_wbf, 'e2e': bench_e2e}[what](args, dev)
        print(json.dumps({what: out[what]}), flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
