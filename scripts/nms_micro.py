# -*- coding: utf-8 -*-
"""Times postprocess() and the variants of postprocess_nms() on the MI355X, on a synthetic prediction of the validation
shape (608 px: B = 32, N = 22 743, C = 80): per image a dozen objects, 5 % of the boxes scattered around them with a high
objectness and one dominant class, the rest background with objectness 1e-6 .. 3e-3.  Each variant runs at
conf = 0.001 (validation) and conf = 0.25 (detection), without and with max_det = 100.

    python scripts/nms_micro.py [--batch 32] [--steps 5] [--warmup 1] [--rounds 3] [--only-postprocess] [--slow-ms 3000]

A call is timed with the host clock from after the clone of the prediction (postprocess rewrites its boxes in place)
to the return, which follows the call's one device -> host read.  The variants alternate --rounds times; a variant whose
warm-up call takes longer than --slow-ms is timed by that call alone.  Prints one JSON line: milliseconds per call (the
best round, and every round), candidates and detections per image."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)                                   # (behind PYTHONPATH: another build of the package can be timed)

from yolov4_amd.yolo.util import utils as U  # noqa: E402


def synth_prediction(B, N, C, dev, seed=0, size=608.0, objects=12):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)

    def u(*shape):
        return torch.rand(shape, generator=g, device=dev)
    p = torch.empty((B, N, 5 + C), device=dev)
    p[..., 0:2] = u(B, N, 2) * size
    p[..., 2:4] = 8 + u(B, N, 2) * 120
    p[..., 4] = 10 ** (-6 + 3.5 * u(B, N))
    p[..., 5:] = 10 ** (-6 + 4 * u(B, N, C))
    near = N // 20
    oc = 40 + u(B, objects, 2) * (size - 80)
    ow = 30 + u(B, objects, 2) * 200
    ocls = torch.randint(0, C, (B, objects), generator=g, device=dev)
    which = torch.randint(0, objects, (B, near), generator=g, device=dev)
    rows = torch.randperm(N, generator=g, device=dev)[:near]
    bi = torch.arange(B, device=dev)[:, None]
    w = ow[bi, which] * (0.8 + 0.4 * u(B, near, 2))
    p[:, rows, 0:2] = oc[bi, which] + (u(B, near, 2) - 0.5) * 0.4 * w
    p[:, rows, 2:4] = w
    p[:, rows, 4] = 10 ** (-3 + 3 * u(B, near))
    p[bi, rows[None, :], 5 + ocls[bi, which]] = 0.3 + 0.7 * u(B, near)
    return p.contiguous()


def timed_call(fn, pred):
    c = pred.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(c)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--boxes', type=int, default=22743)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--slow-ms', type=float, default=3000.0)
    ap.add_argument('--only-postprocess', action='store_true', help='time postprocess() alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nms_micro.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    B, N, C = args.batch, args.boxes, args.classes
    pred = synth_prediction(B, N, C, dev)
    thre = 0.45
    from yolov4_amd import LIB_PATH
    out = {'lib': os.path.relpath(LIB_PATH, ROOT), 'batch': B, 'boxes': N, 'classes': C, 'nms_thre': thre, 'steps': args.steps, 'rounds': args.rounds, 'results': {}}
    for conf in (0.001, 0.25):
        cand = int(((pred[..., 5:] * pred[..., 4:5]) >= conf).sum())
        variants = {'postprocess': lambda c, conf=conf: U.postprocess(c, C, conf, thre)}
        if not args.only_postprocess:
            for name, kw in (('defaults', {}), ('diou', dict(metric='diou')), ('linear', dict(soft='linear')),
                             ('gaussian', dict(soft='gaussian')), ('agnostic', dict(agnostic=True)),
                             ('agnostic-linear', dict(agnostic=True, soft='linear'))):
                for md in (0, 100):
                    variants[name + ('+max_det' if md else '')] = \
                        lambda c, conf=conf, kw=kw, md=md: U.postprocess_nms(c, C, conf, thre, max_det=md, **kw)
        rounds = {k: [] for k in variants}
        dets, slow = {}, {}
        for k, fn in variants.items():                      # warm-up, and the detection counts
            for _ in range(max(1, args.warmup)):
                ms, res = timed_call(fn, pred)
            dets[k] = sum(0 if d is None else int(d.shape[0]) for d in res) / B
            if ms > args.slow_ms:
                slow[k] = ms
        for _ in range(args.rounds):
            for k, fn in variants.items():
                if k in slow:
                    continue
                rounds[k].append(sum(timed_call(fn, pred)[0] for _ in range(args.steps)) / args.steps)
        key = 'conf=%g' % conf
        out['results'][key] = {'candidates_per_image': cand / B}
        for k in variants:
            r = rounds[k] or [slow[k]]
            out['results'][key][k] = {'ms': round(min(r), 3), 'ms_rounds': [round(t, 3) for t in r],
                                      'detections_per_image': round(dets[k], 1), 'single_call': k in slow}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
