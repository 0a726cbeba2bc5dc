# -*- coding: utf-8 -*-
"""YOLO head decode behind the reference's YOLOLayer API
(yolo/model/yololayer.py:16-166), one fused HIP kernel per direction."""
import numpy as np
import torch
from torch import nn

from ... import ops


def n_layers(cfg):
    """Number of detection layers: one per anchor mask (3 for YOLOv4, 2 for YOLOv4-tiny)."""
    return len(cfg['ANCHOR_MASK']) if 'ANCHOR_MASK' in cfg else 3


def layer_strides(cfg, default):
    """cfg['STRIDES'] (one per layer; YOLOv4-tiny: [16, 32]), else the class default [8, 16, 32]."""
    st = [int(v) for v in cfg.get('STRIDES', default)]
    if len(st) < n_layers(cfg):
        raise ValueError(f"STRIDES must name one stride per layer ({n_layers(cfg)}), got {st!r}")
    return st


def layer_scale_xy(cfg, layer_no):
    """The layer's YOLOv4 grid-sensitivity factor from the optional cfg['SCALE_X_Y'] (one number, or one per layer;
    Darknet: 1.2 / 1.1 / 1.05 for strides 8 / 16 / 32); 1.0 when the key is absent.  ValueError outside [1, 2]."""
    v = cfg.get('SCALE_X_Y', 1.0)
    if isinstance(v, (list, tuple)):
        n = n_layers(cfg)
        if len(v) != n:
            raise ValueError(f"SCALE_X_Y must be one number or one per layer ({n}), got {v!r}")
        v = v[layer_no]
    return ops.check_scale_xy(v)


class YOLOLayer(nn.Module):
    strides = [8, 16, 32]

    def __init__(self, cfg, layer_no, device=None):
        super().__init__()
        self.stride = layer_strides(cfg, self.strides)[layer_no]
        self.layer_no = layer_no
        self.anchors = cfg['ANCHORS']
        self.anchor_mask = cfg['ANCHOR_MASK'][layer_no]
        self.n_anchors = len(self.anchor_mask)
        self.all_anchors_grid = [(w / self.stride, h / self.stride) for w, h in self.anchors]
        self.masked_anchors = torch.from_numpy(np.array([self.all_anchors_grid[i] for i in self.anchor_mask]))
        self.n_classes = cfg['N_CLASSES']
        self.scale_xy = layer_scale_xy(cfg, layer_no)
        self.device = device

    def _anchors_f32(self):
        # float64 grid-unit anchors cast to the activation dtype at use (yololayer.py:117-120)
        return [(float(np.float32(w)), float(np.float32(h))) for w, h in self.masked_anchors.tolist()]

    def forward(self, output):
        if self.training:
            out, pred = ops.YoloDecodeTrainFn.apply(output, self._anchors_f32(), self.n_classes, self.scale_xy)
            return {'layer_no': self.layer_no, 'output': out, 'pred': pred}
        return ops.yolo_decode_eval(output, self._anchors_f32(), self.n_classes, self.stride, scale_xy=self.scale_xy)

    def decode_into(self, logits, out, n_total, box_off):
        """eval decode straight into rows [box_off, ...) of the concatenated [B, n_total, 5+C] buffer"""
        return ops.yolo_decode_eval(logits, self._anchors_f32(), self.n_classes, self.stride, out, n_total, box_off,
                                    scale_xy=self.scale_xy)
