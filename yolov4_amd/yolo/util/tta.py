# -*- coding: utf-8 -*-
"""Test-time augmentation: the model runs on a few rescaled / mirrored views of the input batch and
the predictions are merged, either by the usual NMS over all of them or by weighted box fusion (postprocess_wbf).

    views (csrc/tta.hip, one launch each; the identity view is the input itself) -> model -> y4_tta_merge_f32 (one launch per
    view: the view's rows of the merged [B, sum N_k, 5 + C] prediction, boxes mapped back to the base canvas) -> post-process

Views are made from the batch the model would have seen (stretched, or the padded letterbox canvas), so boxes come back in
that canvas's pixels and the usual yolobox2* / letterbox2* conversions follow unchanged.  No CPU path.
"""
import dataclasses
from typing import Tuple

import numpy as np
import torch

from ... import ops
from ..._lib import check, lib
from ..data.transform import LETTERBOX_FILL
from .utils import postprocess, postprocess_nms, postprocess_wbf

TTA_MERGES = ('nms', 'wbf')
# the normalised grey of letterbox_batch's canvas: float(fill) / 255.0f, one fp32 division
TTA_FILL = float(np.float32(LETTERBOX_FILL) / np.float32(255.0))


@dataclasses.dataclass
class TTAOptions:
    """scales[k], flips[k]: view k is the input resized by scales[k] (padded up to the model's largest stride) and, with
    flips[k], mirrored left-right.  merge: 'nms' (the usual post-process over all views' rows) or 'wbf' (weighted box fusion at
    IoU threshold wbf_thre)."""
    scales: Tuple[float, ...] = (1.0, 0.83, 0.67)
    flips: Tuple[bool, ...] = (False, True, False)
    merge: str = 'nms'
    wbf_thre: float = 0.55

    def __post_init__(self):
        self.scales = tuple(float(s) for s in self.scales)
        self.flips = tuple(bool(f) for f in self.flips)
        if len(self.scales) != len(self.flips) or not self.scales:
            raise ValueError('TTA: scales and flips must have the same, non-zero length, got %r and %r'
                             % (self.scales, self.flips))
        if not all(0.25 <= s <= 2.0 for s in self.scales):
            raise ValueError('TTA: scales must lie in [0.25, 2], got %r' % (self.scales,))
        if self.merge not in TTA_MERGES:
            raise ValueError("TTA: merge %r is not 'nms' or 'wbf'" % (self.merge,))
        if not float(self.wbf_thre) >= 0:
            raise ValueError('TTA: wbf_thre must be >= 0')

    @classmethod
    def from_cfg(cls, cfg):
        """cfg['TEST']['TTA'] may hold SCALES, FLIPS, MERGE, WBF_THRE; absent (or empty / false) -> None: no TTA"""
        t = ((cfg or {}).get('TEST', {}) or {}).get('TTA')
        if not t:
            return None
        if t is True:
            return cls()
        d = cls()
        return cls(scales=tuple(t.get('SCALES', d.scales)), flips=tuple(t.get('FLIPS', d.flips)),
                   merge=str(t.get('MERGE', d.merge)).lower(), wbf_thre=float(t.get('WBF_THRE', d.wbf_thre)))


def view_geometry(H, W, scale, stride):
    """(ch, cw, Hv, Wv, ry, rx): the resized content's size, the view's size (content rounded up to `stride`) and the fp32
    source steps of y4_tta_view_f32."""
    ch, cw = max(1, int(H * scale)), max(1, int(W * scale))
    Hv, Wv = -(-ch // stride) * stride, -(-cw // stride) * stride
    return ch, cw, Hv, Wv, float(np.float32(H) / np.float32(ch)), float(np.float32(W) / np.float32(cw))


def tta_views(x, opts, stride=32):
    """x [B, C, H, W] float32 on the device -> list of (view, meta), one per (scale, flip) of `opts`.  meta: flip, ch, cw, Hv,
    Wv, and inv_sx / inv_sy, the fp32 factors that take the view's pixels back to x's.  The identity view (scale 1, no flip,
    H and W multiples of `stride`) is x itself, without a launch."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise ops.Y4Error('tta_views expects a float32 [B, C, H, W] tensor on the device (no CPU path)')
    B, C, H, W = (int(v) for v in x.shape)
    stride = int(stride)
    L = lib()
    out = []
    for scale, flip in zip(opts.scales, opts.flips):
        ch, cw, Hv, Wv, ry, rx = view_geometry(H, W, scale, stride)
        meta = dict(scale=scale, flip=bool(flip), ch=ch, cw=cw, Hv=Hv, Wv=Wv,
                    inv_sx=float(np.float32(W) / np.float32(cw)), inv_sy=float(np.float32(H) / np.float32(ch)))
        if scale == 1.0 and not flip and (Hv, Wv) == (H, W):
            out.append((x, meta))
            continue
        v = torch.empty((B, C, Hv, Wv), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(L.y4_tta_view_f32(ops._ptr(x), B, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), ops._ptr(v),
                                    Hv, Wv, v.stride(0), v.stride(1), v.stride(2), v.stride(3), ch, cw, ry, rx, int(flip),
                                    TTA_FILL, ops._stream()), 'y4_tta_view_f32')
        out.append((v, meta))
    return out


def merge_views(preds, metas):
    """The views' eval predictions [B, N_k, 5 + C] -> one [B, sum N_k, 5 + C] tensor, view k's rows behind view k - 1's, boxes
    in the base canvas's pixels; one y4_tta_merge_f32 launch per view."""
    B, _, n_ch = (int(v) for v in preds[0].shape)
    for p in preds:
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.dim() == 3
                and int(p.shape[0]) == B and int(p.shape[2]) == n_ch):
            raise ops.Y4Error('TTA: every view must give a contiguous float32 [B, N, 5 + C] device tensor')
    n_total = sum(int(p.shape[1]) for p in preds)
    out = torch.empty((B, n_total, n_ch), dtype=torch.float32, device=preds[0].device)
    if B == 0:
        return out
    L = lib()
    off = 0
    with torch.cuda.device(out.device):
        for p, m in zip(preds, metas):
            N = int(p.shape[1])
            if N:
                check(L.y4_tta_merge_f32(ops._ptr(p), B, N, n_ch, ops._ptr(out), n_total, off, float(m['Wv']), int(m['flip']),
                                         m['inv_sx'], m['inv_sy'], ops._stream()), 'y4_tta_merge_f32')
            off += N
    return out


def model_stride(model, default=32):
    """the largest stride of the model's detection layers (32 for YOLOv4 and YOLOv4-tiny); `default` for a model without any"""
    from ..model.yololayer import YOLOLayer
    st = [int(m.stride) for m in model.modules() if isinstance(m, YOLOLayer)] if hasattr(model, 'modules') else []
    return max(st) if st else int(default)


def tta_predict(model, x, opts, stride=None):
    """model (eval mode) on every view of x -> the merged [B, sum N_k, 5 + C] prediction.  With the identity view alone the
    result holds model(x)'s bits."""
    views = tta_views(x, opts, model_stride(model) if stride is None else stride)
    preds = [model(v) for v, _ in views]
    return merge_views(preds, [m for _, m in views])


def wbf_kwargs(nms_options):
    """What of an `nms_options` (None, an NMSOptions or a dict) weighted box fusion can take: agnostic and max_det.  Anything
    else that differs from NMSOptions' defaults is a ValueError."""
    from .utils import NMSOptions
    if nms_options is None:
        return {}
    if not isinstance(nms_options, dict):
        nms_options = nms_options.kwargs()
    kw = dict(nms_options)
    base = NMSOptions().kwargs()
    bad = sorted(k for k in kw if k not in ('agnostic', 'max_det') and (k not in base or kw[k] != base[k]))
    if bad:
        raise ValueError("TTA merge 'wbf' takes only agnostic and max_det from nms_options, not %s" % ', '.join(bad))
    NMSOptions(**kw)                                         # the usual checks (max_det >= 0)
    return {k: kw[k] for k in ('agnostic', 'max_det') if k in kw}


def tta_postprocess(merged, num_classes, conf_thre, nms_thre, opts, nms_options=None):
    """The merged prediction -> postprocess's list of [n, 7] tensors.  merge 'nms': postprocess / postprocess_nms exactly as
    without TTA; 'wbf': postprocess_wbf at opts.wbf_thre with views = the number of views."""
    if opts.merge == 'wbf':
        return postprocess_wbf(merged, num_classes, conf_thre, opts.wbf_thre, views=len(opts.scales), **wbf_kwargs(nms_options))
    if nms_options is None:
        return postprocess(merged, num_classes, conf_thre, nms_thre)
    if not isinstance(nms_options, dict):
        nms_options = nms_options.kwargs()
    return postprocess_nms(merged, num_classes, conf_thre, nms_thre, **nms_options)
