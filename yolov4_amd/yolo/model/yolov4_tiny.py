# -*- coding: utf-8 -*-
"""YOLOv4-tiny (Darknet's yolov4-tiny.cfg): 21 convs, 6.06 M parameters, two heads at strides 16 and 32, LeakyReLU(0.1)
throughout.  Same forward contract as YOLOv4 (yolov4.py): per-layer dicts in training, one [B, N, 5 + C] buffer in eval.

None of the seven concats is copied: the two of a block are concat buffers their producers write in place (ops.CatBuffer),
block3.conv4 writes straight into the neck's concat buffer, the upsample into its other slot.  All hand-offs are plain
fp32 (no pre-split operands).  The number in brackets is the layer's index in yolov4-tiny.cfg (util/darknet_weights.py)."""
import os
from collections import OrderedDict
from typing import Dict

import torch
from torch import nn

from ... import ops
from ...darknet.darknet import ConvBNAct
from .yololayer import YOLOLayer
from .yolov4 import Upsample

ANCHORS = [[10, 14], [23, 27], [37, 58], [81, 82], [135, 169], [344, 319]]
ANCHOR_MASK = [[1, 2, 3], [3, 4, 5]]       # Darknet's own: anchor 0 is unused, anchor 3 sits in both layers
STRIDES = [16, 32]
DARKNET_ORDER = [0, 1, 2, 4, 5, 7, 10, 12, 13, 15, 18, 20, 21, 23, 26, 27, 28, 29, 32, 35, 36]


def default_cfg(n_classes=80):
    """The MODEL dict of a YOLOv4-tiny configuration."""
    return {'TYPE': 'YOLOv4Tiny', 'BACKBONE': 'cspdarknet53-tiny', 'BACKBONE_PRETRAINED': None,
            'ANCHORS': [list(a) for a in ANCHORS], 'ANCHOR_MASK': [list(m) for m in ANCHOR_MASK], 'STRIDES': list(STRIDES),
            'N_CLASSES': int(n_classes)}


class TinyBlock(nn.Module):
    """conv1 -> (upper half) conv2 -> conv3 -> conv4(cat[conv3, conv2]) -> maxpool2x2(cat[conv1, conv4]): c -> 2c channels,
    half the map.  Returns (pooled, conv4's result)."""

    def __init__(self, c):
        super().__init__()
        self.conv1 = ConvBNAct(c, c, 3, 1)
        self.conv2 = ConvBNAct(c // 2, c // 2, 3, 1)
        self.conv3 = ConvBNAct(c // 2, c // 2, 3, 1)
        self.conv4 = ConvBNAct(c, c, 1, 1)

    def forward(self, x, tap_slot=None):
        """tap_slot: a slot of somebody else's concat buffer that conv4's result is to be written into (the neck's, for block3).
        The pool then runs once per producer into the two slots of the POOLED concat (pool(cat) == cat(pool), element for
        element); without it conv1 and conv4 write the pool's input buffer and the pool runs once over it."""
        c = self.conv1.conv.out_channels
        mid = ops.cat_buffer(x, [c // 2, c // 2])                # conv4's input: [conv3 | conv2]
        if tap_slot is None:
            wide = ops.cat_buffer(x, [c, c])                     # the pool's input: [conv1 | conv4]
            x1, x1_hi = ops.fork_half(self.conv1(x, out=wide.slot(0)))
        else:
            x1, x1_hi = ops.fork_half(self.conv1(x))
        x2a, x2b = ops.fork(self.conv2(x1_hi, out=mid.slot(1)))
        x3 = self.conv3(x2a, out=mid.slot(0))
        if tap_slot is None:
            x4 = self.conv4(ops.cat([x3, x2b], into=mid), out=wide.slot(1))
            return ops.maxpool2x2(ops.cat([x1, x4], into=wide)), x4
        x4a, x4b = ops.fork(self.conv4(ops.cat([x3, x2b], into=mid), out=tap_slot))
        pooled = ops.cat_buffer(x, [c, c], hw=(x.shape[2] // 2, x.shape[3] // 2))
        p1 = ops.maxpool2x2(x1, out=pooled.slot(0))
        p4 = ops.maxpool2x2(x4a, out=pooled.slot(1))
        return ops.cat([p1, p4], into=pooled), x4b


class TinyBackbone(nn.Module):

    def __init__(self):
        super().__init__()
        self.conv1 = ConvBNAct(3, 32, 3, 2)           # [0]
        self.conv2 = ConvBNAct(32, 64, 3, 2)          # [1]
        self.block1 = TinyBlock(64)                   # [2, 4, 5, 7]
        self.block2 = TinyBlock(128)                  # [10, 12, 13, 15]
        self.block3 = TinyBlock(256)                  # [18, 20, 21, 23]
        self.conv3 = ConvBNAct(512, 512, 3, 1)        # [26]

    def forward(self, x):
        """-> (stride-32 features [B, 512], the neck's concat buffer [up 128 | block3.conv4 256] with its second slot
        written, that slot's tensor)"""
        x = self.conv2(self.conv1(x))
        x, _ = self.block1(x)
        x, _ = self.block2(x)
        neck_cat = ops.cat_buffer(x, [128, 256])
        x, tap = self.block3(x, tap_slot=neck_cat.slot(1))
        return self.conv3(x), neck_cat, tap


class TinyNeck(nn.Module):

    def __init__(self):
        super().__init__()
        self.conv1 = ConvBNAct(512, 256, 1, 1)        # [27]
        self.conv2 = ConvBNAct(256, 128, 1, 1)        # [32]
        self.upsample = Upsample()

    def forward(self, x5, neck_cat, tap):
        """-> (stride-16 features [B, 384] = cat[upsample(conv2(conv1 out)), block3.conv4 out], stride-32 features [B, 256])"""
        p2a, p2b = ops.fork(self.conv1(x5))
        up = self.upsample(self.conv2(p2b), tap.size(), out=neck_cat.slot(0))
        return ops.cat([up, tap], into=neck_cat), p2a


class TinyHead(nn.Module):

    def __init__(self, cfg: Dict, device=None):
        super().__init__()
        oc = (4 + 1 + cfg['N_CLASSES']) * 3
        self.yolo2 = nn.Sequential(ConvBNAct(256, 512, 3, 1),                                       # [28]
                                   ConvBNAct(512, oc, 1, 1, bias=True, bn=False, act='linear'),     # [29]
                                   YOLOLayer(cfg, layer_no=1, device=device))
        self.yolo1 = nn.Sequential(ConvBNAct(384, 256, 3, 1),                                       # [35]
                                   ConvBNAct(256, oc, 1, 1, bias=True, bn=False, act='linear'),     # [36]
                                   YOLOLayer(cfg, layer_no=0, device=device))

    def logits(self, p1, p2):
        return [self.yolo1[1](self.yolo1[0](p1)), self.yolo2[1](self.yolo2[0](p2))]


class YOLOv4Tiny(nn.Module):

    def __init__(self, cfg: Dict, device=None):
        super().__init__()
        if cfg.get('TYPE') != 'YOLOv4Tiny':
            raise ValueError(f"YOLOv4Tiny needs cfg['TYPE'] == 'YOLOv4Tiny', got {cfg.get('TYPE')!r}")
        if len(cfg['ANCHOR_MASK']) != 2 or list(cfg.get('STRIDES', STRIDES)) != STRIDES:
            raise ValueError('YOLOv4Tiny has two heads, at strides 16 and 32')
        self.backbone = TinyBackbone()
        self.neck = TinyNeck()
        self.head = TinyHead(cfg, device=device)
        self._init(ckpt_path=cfg.get('BACKBONE_PRETRAINED'))

    def _init(self, ckpt_path=None):
        # YOLOv4._init's rule: Kaiming-normal(fan_out, relu) conv weights, zero conv bias, BN gamma ~ N(0, 0.01)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)
        if ckpt_path is not None and os.path.isfile(ckpt_path):
            if str(ckpt_path).endswith(('.pth.tar', '.pth', '.pt')):
                # files we did not write are only ever read with weights_only=True
                ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=True)['state_dict']
                ckpt = OrderedDict((k.replace("module.backbone.", ""), v) for k, v in ckpt.items() if 'backbone' in k)
                self.backbone.load_state_dict(ckpt, strict=True)
            else:
                from ..util.darknet_weights import load_darknet_weights
                load_darknet_weights(self, ckpt_path)      # e.g. yolov4-tiny.conv.29: the first 17 convs

    def darknet_convs(self):
        """The 21 ConvBNAct modules in the order Darknet stores them (DARKNET_ORDER names their cfg layer indices)."""
        b, n, h = self.backbone, self.neck, self.head
        out = [b.conv1, b.conv2]
        for blk in (b.block1, b.block2, b.block3):
            out += [blk.conv1, blk.conv2, blk.conv3, blk.conv4]
        return out + [b.conv3, n.conv1, h.yolo2[0], h.yolo2[1], n.conv2, h.yolo1[0], h.yolo1[1]]

    def darknet_layers(self):
        return list(DARKNET_ORDER)

    def forward(self, x):
        if x.dim() != 4 or x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f'YOLOv4Tiny takes [B, 3, H, W] inputs with H and W multiples of 32, got {tuple(x.shape)}')
        if x.dtype != torch.float32:
            x = x.float()
        p1, p2 = self.neck(*self.backbone(x))
        lg1, lg2 = self.head.logits(p1, p2)
        ly1, ly2 = self.head.yolo1[2], self.head.yolo2[2]
        if self.training:
            return [ly1(lg1), ly2(lg2)]
        # eval: both decodes write into one [B, N, 5 + C] buffer, stride-16 rows first
        counts = [ly.n_anchors * lg.shape[2] * lg.shape[3] for ly, lg in ((ly1, lg1), (ly2, lg2))]
        n_total = sum(counts)
        out = torch.empty((x.shape[0], n_total, 5 + ly1.n_classes), device=x.device, dtype=torch.float32)
        ly1.decode_into(lg1, out, n_total, 0)
        ly2.decode_into(lg2, out, n_total, counts[0])
        return out
