# -*- coding: utf-8 -*-
"""Loss and metric of the classifier's training script (darknet/main_amp.py:184, 549-562) on the library's kernels."""
from collections import namedtuple

from torch import nn

from .. import ops
from .._lib import Y4Error


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(label_smoothing=...) as main_amp.py:184 builds it: class-index targets, mean reduction,
    ignore_index -100 (y4_ce_smooth_fwd_f32 / _bwd_f32).  Anything else has no kernel and raises."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction='mean', label_smoothing=0.0):
        super().__init__()
        if weight is not None:
            raise Y4Error('CrossEntropyLoss: class weights are not supported')
        if size_average is not None or reduce is not None or reduction != 'mean':
            raise Y4Error("CrossEntropyLoss: only reduction='mean' is supported")
        if ignore_index != -100:
            raise Y4Error('CrossEntropyLoss: only ignore_index=-100 is supported')
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f'label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}')
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)

    def forward(self, input, target):
        return ops.CESmoothFn.apply(input, target, self.label_smoothing)


# The target of a CutMix batch (darknet/data.py): a the samples' own classes, b their partners', lam the own share.
MixedTarget = namedtuple('MixedTarget', 'a b lam')


def mixed_loss(criterion, output, target):
    """criterion(output, target) for a tensor target; lam * criterion(output, a) + (1 - lam) * criterion(output, b) for a
    MixedTarget (the CutMix paper's loss)."""
    if isinstance(target, MixedTarget):
        return criterion(output, target.a) * target.lam + criterion(output, target.b) * (1.0 - target.lam)
    return criterion(output, target)


def accuracy(output, target, topk=(1,)):
    """Precision@k for each k in topk (main_amp.py:549-562): a list of one-element device tensors correct_k * 100 / B,
    without a host sync.  Ties go to the lower class index (include/yolov4_amd.h, y4_topk_correct_f32)."""
    batch_size = target.size(0)
    correct = ops.topk_correct(output, target, topk)
    res = correct.float().mul_(100.0 / batch_size)
    return [res[i:i + 1] for i in range(len(topk))]
