# -*- coding: utf-8 -*-
"""The ImageNet classifier that pre-trains the backbone: `Backbone` and `CSPDarknet53` of the reference
(darknet/darknet.py:141-193), importable as yolov4_amd.darknet.darknet.Backbone / CSPDarknet53.

The backbone is the detector's (same six children, hence the same `backbone.*` state_dict keys: a checkpoint saved from
this model is what YOLOv4._init loads through cfg['BACKBONE_PRETRAINED']); behind it the global average pool and the
linear layer run in libyolov4_amd.so (csrc/classifier.hip).  `pool` and `classifier` stay subclasses of the torch
modules the reference uses, so isinstance checks (filter_weight), the state_dict and forward hooks behave as there.
"""
import torch
from torch import nn

from .. import ops
from .._lib import Y4Error
from .darknet import ConvBNAct, CSPDownSample, CSPDownSample0, observed


class Backbone(nn.Module):

    def __init__(self):
        super().__init__()
        self.stem = ConvBNAct(3, 32, 3, 1, act='mish')
        self.stage1 = CSPDownSample0(32, 64, 3, 2, act='mish')
        self.stage2 = CSPDownSample(64, 128, 3, 2, num_blocks=2, act='mish')
        self.stage3 = CSPDownSample(128, 256, 3, 2, num_blocks=8, act='mish')
        self.stage4 = CSPDownSample(256, 512, 3, 2, num_blocks=8, act='mish')
        self.stage5 = CSPDownSample(512, 1024, 3, 2, num_blocks=4, act='mish')

    def forward(self, x):
        """The stage-5 map alone, in fp32 (darknet.py:153-161).  Between the stages a transition conv hands its result to the
        next stage's stride-2 conv pre-split where that conv takes it so and nobody is looking (as the detector's backbone
        does for its single-reader hand-offs); stage 5 has no such reader."""
        quiet = not observed(self)
        stages = (self.stage1, self.stage2, self.stage3, self.stage4, self.stage5)
        x = self.stem(x)
        for st, nxt in zip(stages, stages[1:] + (None,)):
            x = st(x, readers=[nxt.base] if (nxt is not None and quiet and not observed(nxt)) else None)
        return x


class GlobalAvgPool(nn.AdaptiveAvgPool2d):
    """nn.AdaptiveAvgPool2d((1, 1)) on y4_avgpool_global_fwd_f32 / _bwd_f32: [B,C,H,W] -> [B,C,1,1]."""

    def forward(self, x):
        if self.output_size not in (1, (1, 1)):
            raise Y4Error(f'GlobalAvgPool: only output_size (1, 1) has a kernel, got {self.output_size}')
        return ops.AvgPoolGlobalFn.apply(x)


class Linear(nn.Linear):
    """nn.Linear on y4_linear_fwd_f32 / _bwd_f32: [B,in] -> [B,out]."""

    def forward(self, x):
        return ops.LinearFn.apply(x, self.weight, self.bias)


class CSPDarknet53(nn.Module):

    def __init__(self, num_classes=1000):
        super().__init__()
        self.backbone = Backbone()
        self.pool = GlobalAvgPool((1, 1))
        self.classifier = Linear(1024, num_classes)
        self._init()

    def _init(self):
        # darknet.py:174-185
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        if x.dtype != torch.float32:
            x = x.float()
        x = self.backbone(x)
        x = self.pool(x)
        x = x.reshape(x.shape[:2])
        return self.classifier(x)
