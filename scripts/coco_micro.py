# -*- coding: utf-8 -*-
"""Micro-benchmark of the COCO bbox evaluation (yolov4_amd/yolo/util/cocoeval.py on csrc/coco_eval.hip).

    python scripts/coco_micro.py [--images 5000] [--cats 80] [--gts 7] [--dets 100] [--iters 5] [--warmup 1]

A synthetic input of the size of COCO val2017: `images` images, `cats` categories, about `gts` gts (5 % crowd) and `dets`
detections per image; a third of the detections are jittered gts, the rest noise, scores quantised to 1/1024.
Per evaluation, after warm-up, median over `iters`:
  pack_ms          host clock around COCOEvaluator.pack: records (Python dicts) + gts -> CSR cells in numpy
  upload_ms, sort_by_cell_ms, match_ms, sort_by_category_ms, accumulate_ms
                   device events between the stages of COCOEvaluator.run (the two sorts are torch on the device and
                   include their gathers and offsets; match and accumulate are one HIP launch each plus their output
                   allocation); device_ms is their sum
  call_ms          host clock around the whole evaluator call, download and the 12 statistics included
Prints one JSON line.  Needs an MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov4_amd.yolo.util.cocoeval import COCOEvaluator  # noqa: E402


def synth(n_img, n_cat, n_gt, n_det, seed=0):
    rng = np.random.default_rng(seed)
    anns, recs = [], []
    for im in range(1, n_img + 1):
        ng = int(rng.poisson(n_gt))
        xy = rng.uniform(0, 500, (ng, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (ng, 2)))
        cat = rng.integers(1, n_cat + 1, ng)
        crowd = rng.random(ng) < .05
        for j in range(ng):
            b = [float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])]
            anns.append({'id': len(anns) + 1, 'image_id': im, 'category_id': int(cat[j]), 'bbox': b,
                         'area': b[2] * b[3] * float(rng.uniform(.5, 1)), 'iscrowd': int(crowd[j])})
        score = rng.integers(1, 1025, n_det) / 1024
        for j in range(n_det):
            if ng and j % 3 == 0:
                g = int(rng.integers(0, ng))
                jit = rng.normal(0, .08, 4)
                b = [float(xy[g, 0] + jit[0] * wh[g, 0]), float(xy[g, 1] + jit[1] * wh[g, 1]),
                     float(wh[g, 0] * (1 + jit[2])), float(wh[g, 1] * (1 + jit[3]))]
                c = int(cat[g])
            else:
                b = [float(v) for v in np.concatenate([rng.uniform(0, 500, 2), np.exp(rng.uniform(np.log(8), np.log(300), 2))])]
                c = int(rng.integers(1, n_cat + 1))
            recs.append({'image_id': im, 'category_id': c, 'bbox': b, 'score': float(score[j]), 'segmentation': []})
    ann = {'images': [{'id': i} for i in range(1, n_img + 1)], 'annotations': anns,
           'categories': [{'id': c} for c in range(1, n_cat + 1)]}
    return ann, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--cats', type=int, default=80)
    ap.add_argument('--gts', type=float, default=7)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'coco_micro needs an MI355X'
    dev = torch.device('cuda:0')
    ann, recs = synth(a.images, a.cats, a.gts, a.dets)
    ids = list(range(1, a.images + 1))
    ev = COCOEvaluator(ann, device=dev)
    rows = []
    for it in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = ev.pack(recs, ids)
        t1 = time.perf_counter()
        marks = []
        ev.run(p, dev, marks)
        torch.cuda.synchronize()
        stages = {n + '_ms': marks[i][1].elapsed_time(e) for i, (n, e) in enumerate(marks[1:])}    # from the stage before
        t2 = time.perf_counter()
        ev(recs, ids)
        t3 = time.perf_counter()
        if it >= a.warmup:
            rows.append(dict(stages, pack_ms=(t1 - t0) * 1e3, call_ms=(t3 - t2) * 1e3))
    med = {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}
    med['device_ms'] = round(sum(v for k, v in med.items() if k not in ('pack_ms', 'call_ms')), 3)
    med.update(images=a.images, categories=a.cats, gts=len(ann['annotations']), detections=len(recs), cells=p['n_cells'],
               kept=int(p['det_off'][-1]), ap50_95=round(float(ev.stats[0]), 4), ap50=round(float(ev.stats[1]), 4),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(med))


if __name__ == '__main__':
    main()
