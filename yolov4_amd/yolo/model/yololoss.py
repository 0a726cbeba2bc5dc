# -*- coding: utf-8 -*-
"""Detection loss behind the reference's YOLOLoss API (yolo/model/yololoss.py:94-443):
YOLOv3-style weighted-BCE(xy) + MSE(wh)/2 + BCE(obj) + BCE(cls), summed over batch and
the 3 layers (no CIoU / focal anywhere in the reference).  Opt-in beyond the
reference: box_loss = 'iou' | 'giou' | 'diou' | 'ciou' replaces the xy / wh terms by
box_gain * sum(1 - X) over the positive cells ("IoU-family box losses");
iou_thresh < 1 makes every anchor whose shape IoU with a label exceeds it positive (Darknet's
iou_thresh, 0.213 in yolov4.cfg), label_smooth smooths the class BCE targets, and the model
cfg's SCALE_X_Y reaches the box-loss gradient.  focal_gamma > 0 turns the
objectness and / or class BCE terms into the soft-target focal loss, obj_iou_ratio > 0 trains
objectness towards the box loss's own IoU measure, and obj_gain (one number or one per layer) /
cls_gain weigh the two terms.  stats=True adds per-layer training statistics (positives, their
mean IoU and recall at 0.5 / 0.75, objectness on positives and background, class confidence) to a device tensor as
the loss runs.  Everything is off by default."""
import math
from typing import Dict

import numpy as np
import torch
from torch import nn

from ... import ops
from .yololayer import layer_scale_xy, layer_strides, n_layers


def bboxes_iou(bboxes_a, bboxes_b, xyxy=True):
    """Pairwise IoU [Na,4] x [Nb,4] -> [Na,Nb] (yololoss.py:16-91) as one HIP kernel (y4_bboxes_iou_f32).  The loss
    path does not call it: target assignment and the ignore mask carry the same arithmetic inlined."""
    return ops.bboxes_iou_raw(bboxes_a, bboxes_b, xyxy)


# the columns of YOLOLoss.stats, y4_yolo_loss_stats_f64's row (include/yolov4_amd.h)
STATS_ROWS = ('n_cells', 'n_pos', 'n_ign', 'sum_iou', 'n_iou50', 'n_iou75', 'sum_obj_pos', 'sum_obj_bg', 'n_bg', 'sum_cls',
              'n_cls', 'n_top1')


class YOLOLoss(nn.Module):
    strides = [8, 16, 32]

    def __init__(self, cfg: Dict, ignore_thresh=0.7, device=None, mutate_outputs=True, box_loss='mse', box_gain=1.0,
                 iou_thresh=1.0, stats=False, label_smooth=0.0, focal_gamma=0.0, focal_alpha=0.25, focal_terms='obj+cls',
                 obj_iou_ratio=0.0, obj_gain=1.0, cls_gain=1.0):
        # stats sits before label_smooth because the keywords from label_smooth on are a pinned list
        # (tests/test_lossopt_cases.py); every caller passes these by name
        super().__init__()
        ops.box_loss_kind(box_loss)                 # ValueError for an unknown name, before anything touches a GPU
        self.iou_thresh, self.label_smooth = ops.check_loss_options(iou_thresh, label_smooth)
        per_layer = list(obj_gain) if isinstance(obj_gain, (list, tuple)) else [obj_gain] * n_layers(cfg)
        if len(per_layer) != n_layers(cfg):
            raise ValueError(f'obj_gain must be one number or one per layer ({n_layers(cfg)}), got {obj_gain!r}')
        checked = [ops.check_focal_options(focal_gamma, focal_alpha, focal_terms, obj_iou_ratio, og, cls_gain, box_loss)
                   for og in per_layer]
        self.focal_gamma, self.focal_alpha, self.focal_terms, self.obj_iou_ratio, _, self.cls_gain = checked[0]
        self.obj_gain = [c[4] for c in checked]     # one per layer
        self.scale_xy = [layer_scale_xy(cfg, l) for l in range(n_layers(cfg))]
        if box_loss == 'mse' and any(s != 1.0 for s in self.scale_xy):
            # the xy BCE target is defined against the unscaled sigmoid; Darknet does not combine the two either
            raise ValueError("SCALE_X_Y != 1 needs an IoU-family box_loss ('iou', 'giou', 'diou', 'ciou'), not 'mse'")
        self.box_loss = box_loss
        self.box_gain = float(box_gain)
        self.cfg = cfg
        self.ignore_thresh = ignore_thresh
        self.device = device
        self.anchors = cfg['ANCHORS']
        self.n_classes = cfg['N_CLASSES']
        # yololoss.py:402-407 multiplies the masks into outputs[*]['output'] in place; kept by default
        self.mutate_outputs = mutate_outputs
        self.last = [None] * n_layers(cfg)
        # [n_layers, 12] float64 on the device, created by the first forward (the device is the outputs'); None when off
        self.stats_on = bool(stats)
        self.stats = None

    def _layer_cfg(self, layer_no):
        st = layer_strides(self.cfg, self.strides)[layer_no]
        # anchors / stride in float64, used as fp32 (yololoss.py:155-167)
        grid = [(float(np.float32(w / st)), float(np.float32(h / st))) for w, h in self.anchors]
        return {'stride': st, 'ignore_thresh': float(np.float32(self.ignore_thresh)), 'all_anchors': grid,
                'anch_mask': list(self.cfg['ANCHOR_MASK'][layer_no]), 'mutate_output': self.mutate_outputs,
                'box_loss': self.box_loss, 'box_gain': self.box_gain, 'iou_thresh': self.iou_thresh,
                'label_smooth': self.label_smooth, 'scale_xy': self.scale_xy[layer_no],
                'focal_gamma': self.focal_gamma, 'focal_alpha': self.focal_alpha, 'focal_terms': self.focal_terms,
                'obj_iou_ratio': self.obj_iou_ratio, 'obj_iou_kind': self.box_loss,
                'obj_gain': self.obj_gain[layer_no], 'cls_gain': self.cls_gain}

    def build_target(self, output, pred, layer_no, labels):
        """Dense (target, obj_mask, tgt_mask, tgt_scale) as yololoss.py:118-371 returns them; with the options, every
        positive anchor's cell is filled and target[..., 5:] holds the smoothed class targets there."""
        cfg = self._layer_cfg(layer_no)
        cfg['mutate_output'] = False
        cfg['box_loss'] = 'mse'                     # no box-loss launches; obj_iou_kind keeps the measure of t_obj
        ops.YoloLossLayerFn.apply(output.detach().contiguous(), pred, labels, cfg)
        target, tgt_mask, tgt_scale = ops.yolo_loss_dense_targets(cfg['last'])
        return target, cfg['last']['obj_mask'], tgt_mask, tgt_scale

    def reset_stats(self):
        """Zero the accumulated statistics on the device (no synchronisation)."""
        if self.stats is not None:
            self.stats.zero_()

    def stats_summary(self):
        """One dict per layer of what has accumulated since the last reset_stats(): count, avg_iou, r50, r75, obj,
        no_obj, cls, top1, ignored.  The one place that synchronises; a ratio with a zero denominator is nan."""
        if self.stats is None:
            rows = [[0.0] * len(STATS_ROWS)] * n_layers(self.cfg) if self.stats_on else []
        else:
            rows = self.stats.cpu().tolist()

        def ratio(a, b):
            return a / b if b else math.nan

        out = []
        for r in rows:
            s = dict(zip(STATS_ROWS, r))
            out.append({'count': int(s['n_pos']), 'avg_iou': ratio(s['sum_iou'], s['n_pos']),
                        'r50': ratio(s['n_iou50'], s['n_pos']), 'r75': ratio(s['n_iou75'], s['n_pos']),
                        'obj': ratio(s['sum_obj_pos'], s['n_pos']), 'no_obj': ratio(s['sum_obj_bg'], s['n_bg']),
                        'cls': ratio(s['sum_cls'], s['n_cls']), 'top1': ratio(s['n_top1'], s['n_pos']),
                        'ignored': int(s['n_ign'])})
        return out

    def forward(self, outputs, targets):
        assert isinstance(outputs, list)
        assert isinstance(targets, dict)
        labels = targets['padded_labels']
        total = None
        for od in outputs:
            assert isinstance(od, dict)
            layer_no = od['layer_no']
            cfg = self._layer_cfg(layer_no)
            if self.stats_on:
                if self.stats is None or self.stats.device != od['output'].device:
                    self.stats = torch.zeros((n_layers(self.cfg), len(STATS_ROWS)), dtype=torch.float64,
                                             device=od['output'].device)
                cfg['stats'] = self.stats[layer_no]
            loss = ops.YoloLossLayerFn.apply(od['output'], od['pred'], labels, cfg)
            self.last[layer_no] = cfg['last']
            total = loss if total is None else total + loss
        return total
