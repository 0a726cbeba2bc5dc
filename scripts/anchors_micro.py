# -*- coding: utf-8 -*-
"""Micro-benchmark of anchor fitting (yolov4_amd/yolo/util/anchors.py on csrc/anchors.hip).

    python scripts/anchors_micro.py [--n 860001] [--a 9] [--g 64] [--rounds 5] [--reps 400] [--warmup 10]

Synthetic log-normal shapes of the size of COCO train2017's label set.  Per round, alternating, after a warm-up of every
shape timed:
  assign_us        device events around `reps` assignment launches (one Lloyd iteration's device work), per launch
  fitness_us       device events around `reps` fitness launches of g candidate sets, per launch
  lloyd_iter_ms    host clock around whole Lloyd iterations as kmeans_anchors runs them (upload of the centroids, launch,
                   read-back of the table, mean update), per iteration
  generation_ms    host clock around whole generations as evolve_anchors runs them (draws, children, upload, launch,
                   read-back, selection), per generation
  numpy_assign_ms  host clock around ONE assignment pass of the NumPy restatement (tests/anchor_cases.py) at the same n
Each is reported as [min, median, max] over the rounds.  shape IoUs per fitness launch = n * g * a; their rate follows from
fitness_us.  Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import anchor_cases as C  # noqa: E402
from yolov4_amd import ops  # noqa: E402
from yolov4_amd.yolo.util import anchors as A  # noqa: E402


def spread(v, nd=3):
    return [round(float(x), nd) for x in (np.min(v), np.median(v), np.max(v))]


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=860001)
    ap.add_argument('--a', type=int, default=9)
    ap.add_argument('--g', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'anchors_micro needs an MI355X'
    dev = torch.device('cuda:0')
    wh = C.lognormal_shapes(a.n, 0, median=50.0, spread=1.0, lo=1.5, hi=608.0)
    start = np.unique(wh, axis=0)[np.random.Generator(np.random.PCG64(0)).choice(a.n // 2, a.a, replace=False)]
    wh_d, anc_d = torch.from_numpy(wh).to(dev), torch.from_numpy(start).to(dev)
    rng = np.random.Generator(np.random.PCG64(1))
    cand = A.children_of(start, A.mutation_factors(rng, a.g, a.a, 0.1, 0.9), 2.0)
    cand_d = torch.from_numpy(cand).to(dev)

    def assign():
        ops.anchor_assign_raw(wh_d, anc_d, 1.0, want_assign=False, want_iou=False)

    def fit():
        ops.anchor_fitness_raw(wh_d, cand_d, 0.213)
    for _ in range(a.warmup):
        assign()
        fit()

    def lloyd(iters):
        c = start
        for _ in range(iters):
            c = A._mean_update(c, A._assign(wh_d, c))
    lloyd(2)
    torch.cuda.synchronize()
    rows = {'assign_us': [], 'fitness_us': [], 'lloyd_iter_ms': [], 'generation_ms': []}
    iters, gens = 10, 10
    for _ in range(a.rounds):
        rows['assign_us'].append(events(assign, a.reps))
        rows['fitness_us'].append(events(fit, a.reps))
        t0 = time.perf_counter()
        lloyd(iters)
        t1 = time.perf_counter()
        A.evolve_anchors(wh, start, generations=gens, population=a.g, seed=3)
        t2 = time.perf_counter()
        rows['lloyd_iter_ms'].append((t1 - t0) * 1e3 / iters)
        rows['generation_ms'].append((t2 - t1) * 1e3 / (gens + 1))          # (includes one upload of the shapes)
    t0 = time.perf_counter()
    _, _, acc_ref = C.assign(wh, start, 1.0)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    _, _, acc = ops.anchor_assign_raw(wh_d, anc_d, 1.0)
    assert np.array_equal(acc.cpu().numpy(), acc_ref), 'device table differs from the restatement'
    out = {k: spread(v) for k, v in rows.items()}
    ious = a.n * a.g * a.a
    out.update(numpy_assign_ms=round(numpy_ms, 1), n=a.n, a=a.a, g=a.g, rounds=a.rounds, reps=a.reps,
               fitness_gious_per_s=spread([ious / (us * 1e-6) / 1e9 for us in rows['fitness_us']], 1),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
