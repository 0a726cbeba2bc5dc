# -*- coding: utf-8 -*-
"""COCO bbox evaluation on the device: the `evaluator` of `validate()` (yolo/engine/build.py), in place of the
reference's pycocotools block (its build.py:172-188: COCO.loadRes, COCOeval.evaluate / accumulate / summarize).

    evaluator = COCOEvaluator('instances_val2017.json')          # or the dict json.load gives
    ap50_95, ap50 = validate(val_loader, model, 0.005, 0.45, device, evaluator=evaluator)
    print(evaluator.summary())

The host packs records and gts into (image, category) cells (CSR); the stable sorts and segment sums are torch on the
device; the greedy matching and the precision / recall scans are the two kernels of csrc/coco_eval.hip.  There is no
CPU path: a missing library or a CPU device raises Y4Error.  Semantics: include/yolov4_amd.h, DESIGN.md §11.
"""
import json

import numpy as np
import torch

from ... import ops
from ..._lib import Y4Error, lib

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNG = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)    # all, small, medium, large
MAX_DETS = (1, 10, 100)
KEEP = 100                                      # detections kept per (image, category) cell

_SUMMARY = [  # (is AP, IoU threshold index or None, area index, maxDets index)
    (1, None, 0, 2), (1, 0, 0, 2), (1, 5, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
    (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2)]
_AREA_NAMES = ('all', 'small', 'medium', 'large')


def summarize(precision, recall):
    """The 12 standard statistics: each the mean of the entries > -1 of a slice, or -1 if there are none."""
    stats = np.zeros(12, dtype=np.float64)
    for i, (ap, t, a, m) in enumerate(_SUMMARY):
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if t is not None:
            s = s[t:t + 1]
        s = s[s > -1]
        stats[i] = -1 if s.size == 0 else np.mean(s)
    return stats


class COCOEvaluator:
    """`__call__(records, image_ids) -> (AP50_95, AP50)`; afterwards `.stats` (12 fp64), `.precision` [10,101,K,4,3],
    `.recall` [10,K,4,3] and `.summary()`."""

    def __init__(self, annotations, device=None):
        if not isinstance(annotations, dict):
            with open(annotations) as f:
                annotations = json.load(f)
        self.device = device
        self.cat_ids = np.array(sorted(int(c['id']) for c in annotations['categories']), dtype=np.int64)
        self.known_images = np.unique(np.array([int(im['id']) for im in annotations['images']], dtype=np.int64))
        anns = annotations['annotations']
        img = np.array([int(g['image_id']) for g in anns], dtype=np.int64)
        cat = np.array([int(g['category_id']) for g in anns], dtype=np.int64)
        k, ok = self._lookup(self.cat_ids, cat)
        # gts in annotation order, those of unknown categories dropped
        self.g_img, self.g_k = img[ok], k[ok]
        self.g_box = np.array([g['bbox'] for g in anns], dtype=np.float64).reshape(-1, 4)[ok]
        self.g_area = np.array([g['area'] for g in anns], dtype=np.float64)[ok]
        self.g_crowd = np.array([int(g.get('iscrowd', 0)) for g in anns], dtype=np.int32)[ok]
        self.stats = self.precision = self.recall = None

    @staticmethod
    def _lookup(table, values):
        """index of each value in the sorted unique `table`, and whether it is there"""
        if table.size == 0 or values.size == 0:
            return np.zeros(values.shape, np.int64), np.zeros(values.shape, bool)
        pos = np.minimum(np.searchsorted(table, values), table.size - 1)
        return pos, table[pos] == values

    def pack(self, records, image_ids):
        """Host side: records + gts -> cells in CSR.  Cells are the (category, image) pairs with a gt or a detection, in
        that order; gts are grouped by cell in annotation order; detections stay in record order with their cell index
        (the device sorts them).  Returns a dict of numpy arrays."""
        img_ids = np.unique(np.array([int(i) for i in image_ids], dtype=np.int64))
        n_img, K = int(img_ids.size), int(self.cat_ids.size)
        d_img = np.array([int(r['image_id']) for r in records], dtype=np.int64)
        _, known = self._lookup(self.known_images, d_img)
        if not known.all():
            raise ValueError('detections of image ids that are not in the annotation file: %s'
                             % sorted(set(d_img[~known].tolist()))[:8])
        d_cat = np.array([int(r['category_id']) for r in records], dtype=np.int64)
        d_box = np.array([r['bbox'] for r in records], dtype=np.float64).reshape(-1, 4)
        d_score = np.array([r['score'] for r in records], dtype=np.float64)
        di, ok_i = self._lookup(img_ids, d_img)
        dk, ok_k = self._lookup(self.cat_ids, d_cat)
        keep = ok_i & ok_k
        d_key = dk[keep] * n_img + di[keep]
        gi, ok_g = self._lookup(img_ids, self.g_img)
        g_key = self.g_k[ok_g] * n_img + gi[ok_g]
        cells = np.unique(np.concatenate([g_key, d_key]))
        g_order = np.argsort(g_key, kind='stable')
        g_sel = np.flatnonzero(ok_g)[g_order]
        gt_off = np.append(np.searchsorted(g_key[g_order], cells, side='left'), g_key.size)    # every gt key is a cell
        det_cell = np.searchsorted(cells, d_key)
        count = np.bincount(det_cell, minlength=cells.size) if cells.size else np.zeros(0, np.int64)
        kept = np.minimum(count, KEEP)
        det_off = np.concatenate([[0], np.cumsum(kept)])
        cell_cat = cells // n_img if n_img else cells
        cat_off = np.concatenate([[0], np.cumsum(np.bincount(cell_cat, weights=kept, minlength=K))]) if cells.size \
            else np.zeros(K + 1)
        return {'n_cells': int(cells.size), 'n_cat': K, 'image_ids': img_ids,
                'cell_cat': cell_cat.astype(np.int64), 'cell_img': (cells % n_img if n_img else cells).astype(np.int64),
                'gt_off': gt_off.astype(np.int32), 'g_box': self.g_box[g_sel], 'g_area': self.g_area[g_sel],
                'g_crowd': self.g_crowd[g_sel], 'g_index': g_sel,
                'det_cell': det_cell.astype(np.int64), 'd_box': d_box[keep], 'd_score': d_score[keep],
                'd_index': np.flatnonzero(keep), 'det_off': det_off.astype(np.int32), 'cat_off': cat_off.astype(np.int32)}

    def _device(self):
        lib()                                                     # raises Y4Error when the library has not been built
        dev = torch.device(self.device) if self.device is not None else \
            torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        if dev.type != 'cuda':
            raise Y4Error(f'COCOEvaluator: device is {dev}; the evaluation runs on an MI355X only (no CPU fallback)')
        return dev

    def run(self, p, dev, marks=None):
        """Device side of one evaluation of the pack `p`: -> dict of device tensors (kept rows, codes, npig, precision,
        recall).  One boolean compaction (the cut to 100 per cell) synchronises; nothing else does.  `marks`: optional
        list that receives (stage name, torch.cuda.Event) after every stage (scripts/coco_micro.py)."""
        def mark(name):
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append((name, ev))
        mark('start')
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
        n_cells, K = p['n_cells'], p['n_cat']
        score, cell, box = up(p['d_score'], torch.float64), up(p['det_cell'], torch.int64), up(p['d_box'], torch.float64)
        det_off, gt_off, cat_off = up(p['det_off'], torch.int32), up(p['gt_off'], torch.int32), up(p['cat_off'], torch.int32)
        mark('upload')
        # rows by (cell, -score), stable: equal scores keep record order
        o1 = torch.sort(score, descending=True, stable=True).indices
        o2 = torch.sort(cell[o1], stable=True).indices
        perm = o1[o2]
        cell_s = cell[perm]
        count = torch.bincount(cell_s, minlength=max(n_cells, 1))
        start = torch.cumsum(count, 0) - count
        rank = torch.arange(cell_s.numel(), device=dev) - start[cell_s]
        keep = rank < KEEP
        perm, cell_s, rank = perm[keep], cell_s[keep], rank[keep].to(torch.uint8)
        kbox, kscore = box[perm].contiguous(), score[perm]
        gbox, garea, gcrowd = up(p['g_box'], torch.float64).reshape(-1, 4), up(p['g_area'], torch.float64), up(p['g_crowd'], torch.int32)
        iou_thrs, area_rng, rec_thrs = up(IOU_THRS, torch.float64), up(AREA_RNG, torch.float64), up(REC_THRS, torch.float64)
        mark('sort_by_cell')
        codes, npig = ops.coco_match(kbox, det_off, p['det_off'], gbox, garea, gcrowd, gt_off, p['gt_off'], iou_thrs, area_rng)
        mark('match')
        # rows by (category, -score), stable: ties keep image order, then rank (cells are numbered category-major)
        cell_cat = up(p['cell_cat'], torch.int64)
        s1 = torch.sort(kscore, descending=True, stable=True).indices
        s2 = torch.sort(cell_cat[cell_s[s1]], stable=True).indices if n_cells else s1
        order = s1[s2].to(torch.int32)
        npig_cat = torch.zeros((K, 4), device=dev, dtype=torch.int64)
        if n_cells:
            npig_cat.index_add_(0, cell_cat, npig.to(torch.int64))
        mark('sort_by_category')
        precision, recall = ops.coco_accumulate(codes, rank, order, cat_off, p['cat_off'], npig_cat, rec_thrs, MAX_DETS)
        mark('accumulate')
        return {'perm': perm, 'rank': rank, 'order': order, 'codes': codes, 'npig': npig, 'npig_cat': npig_cat,
                'precision': precision, 'recall': recall}

    def __call__(self, records, image_ids):
        dev = self._device()
        out = self.run(self.pack(records, image_ids), dev)
        self.precision = out['precision'].cpu().numpy()
        self.recall = out['recall'].cpu().numpy()
        self.stats = summarize(self.precision, self.recall)
        return float(self.stats[0]), float(self.stats[1])

    def summary(self):
        if self.stats is None:
            raise Y4Error('COCOEvaluator.summary: nothing has been evaluated yet')
        lines = []
        for v, (ap, t, a, m) in zip(self.stats, _SUMMARY):
            iou = '0.50:0.95' if t is None else '%0.2f' % IOU_THRS[t]
            lines.append(' Average %s     (%s) @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f'
                         % ('Precision' if ap else 'Recall', 'AP' if ap else 'AR', iou, _AREA_NAMES[a], MAX_DETS[m], v))
        return '\n'.join(lines)
