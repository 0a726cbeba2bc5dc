# -*- coding: utf-8 -*-
"""Times of the classifier kernels (csrc/classifier.hip) at the ImageNet shapes -- B = 256 images, an 8 x 8 stage-5 map
(HW = 64), C = 1024 features, N = 1000 classes -- and of one full CSPDarknet53 train step at 256 x 256, bs 64, with device
events after warm-up.  Beside each time: the bytes / flops the operation needs (computed from the shapes) over that time,
and which of the two bounds it (the larger of bytes / HBM rate and flops / fp32 vector rate names the bound).

    python scripts/classifier_micro.py [reps] [--no-step]

Prints one JSON line per measurement.  Needs an MI355X: there is no CPU path and nothing is reported without a run.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_BPS = 8.0e12             # MI355X peak HBM3E rate
VALU_FLOPS = 157.3e12        # MI355X peak fp32 vector rate (the linear kernels are fp32 fma chains, not MFMA)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def report(name, sec, nbytes, flops, launches):
    t_mem, t_alu = nbytes / HBM_BPS, flops / VALU_FLOPS
    print(json.dumps({'kernel': name, 'us': round(sec * 1e6, 2), 'launches': launches, 'bytes': nbytes, 'flops': flops,
                      'GB_per_s': round(nbytes / sec / 1e9, 1), 'GFLOP_per_s': round(flops / sec / 1e9, 1),
                      'bound': 'memory' if t_mem >= t_alu else 'compute',
                      'share_of_bound': round(max(t_mem, t_alu) / sec, 4)}), flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    reps = int(args[0]) if args else 50
    from yolov4_amd import ops
    from yolov4_amd._lib import check, int_array, lib
    assert torch.cuda.is_available(), 'classifier_micro needs an MI355X'
    dev = torch.device('cuda:0')
    L, ptr, stream = lib(), ops._ptr, ops._stream
    B, HW, C, N = 256, 64, 1024, 1000
    g = torch.Generator(device='cpu').manual_seed(0)

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(dev)

    x, f, df = rnd(B, HW, C), torch.empty(B, C, device=dev), rnd(B, C)
    dx = torch.empty(B, HW, C, device=dev)
    report('avgpool_fwd', timed(lambda: check(L.y4_avgpool_global_fwd_f32(ptr(x), C, ptr(f), C, B, HW, C, stream())), reps),
           4 * (B * HW * C + B * C), B * HW * C, 1)
    report('avgpool_bwd', timed(lambda: check(L.y4_avgpool_global_bwd_f32(ptr(df), C, ptr(dx), C, B, HW, C, stream())), reps),
           4 * (B * HW * C + B * C), B * HW * C, 1)

    w, bias, y, dy = rnd(N, C) / 32, rnd(N), torch.empty(B, N, device=dev), rnd(B, N)
    dfe, dw, db = torch.empty(B, C, device=dev), torch.empty(N, C, device=dev), torch.empty(N, device=dev)
    report('linear_fwd', timed(lambda: check(L.y4_linear_fwd_f32(ptr(df), C, ptr(w), ptr(bias), ptr(y), N, B, C, N, stream())), reps),
           4 * (B * C + N * C + N + B * N), 2 * B * C * N, 1)
    report('linear_bwd', timed(lambda: check(L.y4_linear_bwd_f32(ptr(df), C, ptr(w), ptr(dy), N, ptr(dfe), C, ptr(dw), ptr(db),
                                                                 B, C, N, stream())), reps),
           4 * (B * C + N * C + 2 * B * N + B * C + N * C + B * N + N), 4 * B * C * N + B * N, 3)

    t = torch.randint(0, N, (B,), generator=g).to(dev)
    z = rnd(B, N) * 4
    row, out = torch.empty(B, device=dev), torch.empty(2, device=dev, dtype=torch.float64)
    gs, dz = torch.ones(1, device=dev), torch.empty(B, N, device=dev)
    report('ce_smooth_fwd', timed(lambda: check(L.y4_ce_smooth_fwd_f32(ptr(z), N, ptr(t), B, N, 0.1, ptr(row), ptr(out), stream())), reps),
           4 * B * N + 12 * B + 4 * B + 16, 6 * B * N, 2)
    report('ce_smooth_bwd', timed(lambda: check(L.y4_ce_smooth_bwd_f32(ptr(z), N, ptr(t), ptr(out), ptr(gs), ptr(dz), N, B, N, 0.1,
                                                                       stream())), reps),
           8 * B * N + 8 * B, 12 * B * N, 1)
    ks = int_array([1, 5])
    correct = torch.empty(2, device=dev, dtype=torch.int32)
    report('topk_correct', timed(lambda: check(L.y4_topk_correct_f32(ptr(z), N, ptr(t), B, N, ks, 2, ptr(correct), None, stream())), reps),
           4 * B * N + 8 * B, 3 * B * N, 2)

    if '--no-step' in sys.argv:
        return
    import classifier_cases as CC
    from yolov4_amd.darknet.darknet import CSPDarknet53
    from yolov4_amd.darknet.loss import CrossEntropyLoss
    from yolov4_amd.darknet.train import train_step
    from yolov4_amd.yolo.optim.optimizers.build import FusedAdam
    bs, S = 64, 256
    model = CSPDarknet53(N)
    sd = model.state_dict()
    CC.fill_classifier_(sd, 1)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    crit, opt = CrossEntropyLoss(label_smoothing=0.1), FusedAdam(model.parameters(), lr=1e-4)
    xin, tin = rnd(bs, 3, S, S), torch.randint(0, N, (bs,), generator=g).to(dev)
    sec = timed(lambda: train_step(model, crit, opt, xin, tin), max(3, reps // 5), warm=3)
    print(json.dumps({'train_step': f'CSPDarknet53({N}) {S}x{S} bs {bs}: forward + CE + backward + FusedAdam',
                      'ms': round(sec * 1e3, 2), 'images_per_s': round(bs / sec, 1)}), flush=True)


if __name__ == '__main__':
    main()
