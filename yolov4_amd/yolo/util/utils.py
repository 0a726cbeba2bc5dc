# -*- coding: utf-8 -*-
"""Post-processing behind the reference's API (yolo/util/utils.py:32-89, 92-223):
confidence filter + per-class greedy NMS on the GPU.

One host round trip per call (per-image offsets of the compacted result) replaces the
reference's per-class device->host copies and its Python/numpy loops: candidate prefix
sums, key fill, sort + NMS and compaction all run on the device.  Tie order is
DEFINED here (score desc, then lower box index first); the reference's comes from an
unstable numpy argsort and is platform dependent.

postprocess_nms() is the same pipeline with a DIoU measure, Soft-NMS, class-agnostic
segments and a per-image cap; postprocess() stays the reference's rule.
postprocess_wbf() runs weighted box fusion on those stages instead of suppression.
"""
import ctypes
import dataclasses
from typing import Optional

import numpy as np
import torch

from ... import ops
from ..._lib import NMS_METRICS, NMS_SOFT, NmsOpts, check, lib


def _dev():
    if not torch.cuda.is_available():
        raise ops.Y4Error('postprocess / nms run on an MI355X only (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def nms(bbox, thresh, score=None, limit=None):
    """bbox [R,4] xyxy, numpy in / numpy int32 indices out, as utils.py:32-89."""
    bbox = np.asarray(bbox, dtype=np.float32)
    if len(bbox) == 0:
        return np.zeros((0,), dtype=np.int32)
    L = lib()
    dev = _dev()
    R = bbox.shape[0]
    boxes = torch.from_numpy(np.ascontiguousarray(bbox)).to(dev)
    sc = torch.from_numpy(np.ascontiguousarray(np.asarray(score, dtype=np.float32))).to(dev) if score is not None else None
    keep = torch.empty(R, dtype=torch.int32, device=dev)
    nkeep = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.y4_nms_workspace(R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.y4_nms_f32(ops._ptr(boxes), ops._ptr(sc), R, float(thresh), int(limit) if limit is not None else 0,
                       ops._ptr(keep), ops._ptr(nkeep), ops._ptr(ws), nbytes, ops._stream()), 'nms')
    n = int(nkeep.item())
    return keep[:n].cpu().numpy().astype(np.int32)


def postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45):
    """prediction [B,N,5+C] (xc,yc,w,h,obj,cls...) -> list of [n,7] tensors
    (x1,y1,x2,y2,obj,cls_conf,cls_id) or None; rows ordered class asc, score desc.
    Side effect kept from the reference: prediction[:, :, :4] becomes xyxy in place."""
    def stage(L, pred, B, N, seg_off, cap, rows, kept, nseg, st):
        nbytes = L.y4_post_nms_workspace(cap, nseg)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        check(L.y4_post_nms_f32(ops._ptr(pred), B, N, num_classes, float(conf_thre), float(nms_thre),
                                ops._ptr(seg_off), cap, ops._ptr(rows), ops._ptr(kept), ops._ptr(ws), nbytes, st), 'post_nms')
    return _postprocess_segments('postprocess', prediction, num_classes, conf_thre, None, 0, stage)


@dataclasses.dataclass
class NMSOptions:
    """What postprocess_nms() takes beyond the two thresholds.  The defaults are the reference's rule."""
    metric: str = 'iou'
    soft: Optional[str] = None
    sigma: float = 0.5
    agnostic: bool = False
    max_det: int = 0

    def __post_init__(self):
        if self.metric not in NMS_METRICS:
            raise ValueError('metric: %r is not one of %s' % (self.metric, sorted(NMS_METRICS)))
        if self.soft not in NMS_SOFT:
            raise ValueError("soft: %r is not None, 'linear' or 'gaussian'" % (self.soft,))
        if self.soft == 'gaussian' and not float(self.sigma) > 0:
            raise ValueError('sigma must be positive')
        if int(self.max_det) < 0:
            raise ValueError('max_det must be >= 0 (0: no cap)')

    @classmethod
    def from_cfg(cls, cfg):
        """cfg['TEST'] may hold NMS_METRIC, NMS_SOFT, NMS_SIGMA, NMS_AGNOSTIC, MAX_DET; a cfg without them gives the defaults"""
        t = (cfg or {}).get('TEST', {}) or {}
        soft = t.get('NMS_SOFT', None)
        if soft in ('', 'none', 'None', False):
            soft = None
        return cls(metric=str(t.get('NMS_METRIC', 'iou')).lower(), soft=soft.lower() if isinstance(soft, str) else soft,
                   sigma=float(t.get('NMS_SIGMA', 0.5)), agnostic=bool(t.get('NMS_AGNOSTIC', False)),
                   max_det=int(t.get('MAX_DET', 0)))

    def kwargs(self):
        return dataclasses.asdict(self)


def _postprocess_segments(what, prediction, num_classes, conf_thre, agnostic, max_det, stage):
    """The driver of postprocess(), postprocess_nms() and postprocess_wbf(): candidate count, then -- with the capacity retry
    and the one host read -- scan, `stage(L, prediction, B, N, seg_off, cap, rows, kept, nseg, stream)` (key fill, sort and
    suppression or fusion into rows / kept) and compaction or the per-image top-k.  agnostic None is postprocess() itself: the
    reference's rule through the plain count entry, which refuses an empty batch (the other two give [] for one).
    detect.py:115-118 moves the output to the CPU first: a host tensor is taken to the device and gets its xyxy back."""
    L = lib()
    src = prediction
    on_host = not prediction.is_cuda
    if on_host:
        prediction = prediction.to(_dev())
    if prediction.dtype != torch.float32 or not prediction.is_contiguous():
        raise ops.Y4Error(what + ' expects a contiguous float32 [B,N,5+C] tensor')
    B, N, n_ch = prediction.shape
    if n_ch != 5 + num_classes:
        raise ops.Y4Error(what + ': last dim must be 5 + num_classes')
    dev = prediction.device
    out = [None for _ in range(B)]
    if N == 0 or (B == 0 and agnostic is not None):
        return out
    per_img = 1 if agnostic else num_classes
    nseg = B * per_img
    counts = torch.empty(nseg, dtype=torch.int32, device=dev)
    st = ops._stream()
    if agnostic is None:
        check(L.y4_post_count_f32(ops._ptr(prediction), B, N, num_classes, float(conf_thre), 1, ops._ptr(counts), st),
              'post_count')
    else:
        check(L.y4_post_count_ex_f32(ops._ptr(prediction), B, N, num_classes, float(conf_thre), 1, int(bool(agnostic)),
                                     ops._ptr(counts), st), 'post_count_ex')
    if on_host:
        src[:, :, :4] = prediction[:, :, :4].cpu()
    # Everything between the count and the result stays on the device: prefix sums, key fill, sort + NMS, compaction run
    # into buffers sized for `cap` candidates; the ONE host read at the end brings the per-image offsets and the true
    # candidate total (if it exceeded cap -- many classes per box above a low threshold -- the sequence repeats with room).
    cap = int(min(B * N * num_classes, max(B * N // 2, 1 << 16), (1 << 31) - 1))
    seg_off = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    meta = torch.empty(2 + B + 1, dtype=torch.int32, device=dev)          # [total, overflow | img_off[0..B]]
    out_off = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    kept = torch.empty(nseg, dtype=torch.int32, device=dev)
    while True:
        check(L.y4_post_scan_i32(ops._ptr(counts), nseg, cap, ops._ptr(seg_off), ops._ptr(meta), st), 'post_scan')
        rows = torch.empty((cap, 7), dtype=torch.float32, device=dev)
        final = torch.empty((cap, 7), dtype=torch.float32, device=dev)
        stage(L, prediction, B, N, seg_off, cap, rows, kept, nseg, st)
        if max_det > 0:
            tbytes = L.y4_post_topk_workspace(cap, nseg)
            tws = torch.empty(tbytes, dtype=torch.uint8, device=dev)
            check(L.y4_post_topk_compact_f32(ops._ptr(rows), ops._ptr(seg_off), ops._ptr(kept), B, per_img, int(max_det),
                                             cap, ops._ptr(final), ops._ptr(out_off), ops._ptr(meta[2:]), ops._ptr(tws),
                                             tbytes, st), 'post_topk_compact')
        else:
            check(L.y4_post_compact_f32(ops._ptr(rows), ops._ptr(seg_off), ops._ptr(kept), B, per_img, ops._ptr(final),
                                        ops._ptr(out_off), ops._ptr(meta[2:]), st), 'post_compact')
        host = meta.cpu().numpy().astype(np.int64)                        # the host sync
        if not host[1]:
            break
        cap = int(host[0])
    img_off = host[2:]
    n_det = int(img_off[B])
    if n_det == 0:
        return out
    dets = final[:n_det].clone()                                          # (lets the cap-sized buffers go)
    if on_host:
        dets = dets.cpu()
    for b in range(B):
        if img_off[b + 1] > img_off[b]:
            out[b] = dets[img_off[b]:img_off[b + 1]]
    return out


def postprocess_nms(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, *, metric='iou', soft=None, sigma=0.5,
                    agnostic=False, max_det=0):
    """postprocess() with options: metric 'iou' | 'diou', soft None | 'linear' | 'gaussian' (Soft-NMS,
    `sigma` for the Gaussian decay), agnostic (all classes of an image compete), max_det (rows kept per image, 0: all).
    Same return contract and in-place xyxy side effect; with the defaults the same kernels run and the result is
    bit-identical.  Soft-NMS rows carry cls_conf * W, so row[4] * row[5] is the decayed score."""
    o = NMSOptions(metric, soft, sigma, agnostic, max_det)
    opts = NmsOpts(NMS_METRICS[o.metric], NMS_SOFT[o.soft], float(o.sigma), int(bool(o.agnostic)), int(o.max_det))
    popts = ctypes.addressof(opts)

    def stage(L, pred, B, N, seg_off, cap, rows, kept, nseg, st):
        nbytes = L.y4_post_nms_ex_workspace(cap, nseg, popts)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        check(L.y4_post_nms_ex_f32(ops._ptr(pred), B, N, num_classes, float(conf_thre), float(nms_thre), popts,
                                   ops._ptr(seg_off), cap, ops._ptr(rows), ops._ptr(kept), ops._ptr(ws), nbytes, st),
              'post_nms_ex')
    return _postprocess_segments('postprocess_nms', prediction, num_classes, conf_thre, o.agnostic, int(o.max_det), stage)


def postprocess_wbf(prediction, num_classes, conf_thre, iou_thre=0.55, *, views=1, agnostic=False, max_det=0):
    """Weighted box fusion on postprocess_nms()'s stages: overlapping candidates of a segment are
    averaged (score-weighted) instead of suppressed.  `views`: how many predictions per object the input holds (the number of
    TTA views); a cluster with fewer members has its score scaled by members / views.  Rows are
    (x1, y1, x2, y2, 1.0, fused score, cls), so row[4] * row[5] is the score; the return contract, the in-place xyxy side
    effect, the capacity retry and the one host read are postprocess_nms()'s.  No CPU path."""
    if int(views) < 1:
        raise ValueError('views must be >= 1')
    if int(max_det) < 0:
        raise ValueError('max_det must be >= 0 (0: no cap)')
    if not float(iou_thre) >= 0:
        raise ValueError('iou_thre must be >= 0')
    agn = int(bool(agnostic))

    def stage(L, pred, B, N, seg_off, cap, rows, kept, nseg, st):
        nbytes = L.y4_post_wbf_workspace(cap, nseg)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        check(L.y4_post_wbf_f32(ops._ptr(pred), B, N, num_classes, float(conf_thre), float(iou_thre), agn, int(views),
                                ops._ptr(seg_off), cap, ops._ptr(rows), ops._ptr(kept), ops._ptr(ws), nbytes, st), 'post_wbf')
    return _postprocess_segments('postprocess_wbf', prediction, num_classes, conf_thre, agn, int(max_det), stage)


# ------------------------------------------------------------------ detections -> COCO records
# the 80 COCO category ids in class-index order (yolo/data/cocodataset.py:48-51): 1..90 minus the unused ids
COCO_CLASS_IDS = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]


def yolobox2xywh(box, info_img):
    """(y1, x1, y2, x2) in network-input pixels -> [x1, y1, w, h] in source-image pixels
    (yolo/util/utils.py:281-309); `info_img` = (src_h, src_w, dst_h, dst_w)."""
    src_h, src_w, dst_h, dst_w = info_img
    y1, x1, y2, x2 = box
    box_h = (y2 - y1) / dst_h * src_h
    box_w = (x2 - x1) / dst_w * src_w
    return [x1 / dst_w * src_w, y1 / dst_h * src_h, box_w, box_h]


def yolobox2yxyx(box, info_img):
    """(y1, x1, y2, x2) in network-input pixels -> [y1, x1, y2, x2] in source-image pixels
    (yolo/util/utils.py:312-341); `info_img` = (src_h, src_w, dst_h, dst_w).  Python floats or float64 arrays: the
    reference's double arithmetic in its order (multiply, then divide)."""
    src_h, src_w, dst_h, dst_w = info_img
    y1, x1, y2, x2 = box
    return [y1 * src_h / dst_h, x1 * src_w / dst_w, y2 * src_h / dst_h, x2 * src_w / dst_w]


def _clip(v, hi):
    """v limited to [0, hi]; Python floats or float64 arrays (a NaN stays a NaN)"""
    return np.clip(v, 0.0, float(hi)) if isinstance(v, np.ndarray) else min(max(v, 0.0), float(hi))


def letterbox2yxyx(box, info):
    """(y1, x1, y2, x2) in the pixels of a letterboxed network input -> [y1, x1, y2, x2] in source-image pixels, clipped to
    the image.  `info` = (h, w, nh, nw, top, left): the source's size, the size it was resized to and where that lies in
    the canvas (`letterbox_batch`).  Double arithmetic, multiply then divide, as yolobox2yxyx."""
    h, w, nh, nw, top, left = info[:6]
    y1, x1, y2, x2 = box
    return [_clip((y1 - top) * h / nh, h), _clip((x1 - left) * w / nw, w),
            _clip((y2 - top) * h / nh, h), _clip((x2 - left) * w / nw, w)]


def letterbox2xywh(box, info):
    """(y1, x1, y2, x2) in the pixels of a letterboxed network input -> [x1, y1, w, h] in source-image pixels: the corners
    of letterbox2yxyx (clipped to the image), then their differences."""
    y1, x1, y2, x2 = letterbox2yxyx(box, info)
    return [x1, y1, x2 - x1, y2 - y1]


def detections_to_coco(detections, img_info, image_id, class_ids=COCO_CLASS_IDS, pad=None):
    """One image's postprocess() result [n,7] (or None) -> list of COCO result dicts, as validate() builds
    them (yolo/engine/build.py:144-164).  The reference converts every fp32 number to a Python float and
    does the arithmetic in double precision; one device->host copy and the same double arithmetic here.
    pad = (top, left): the input was letterboxed, img_info[:4] = (h, w, nh, nw), and boxes go through letterbox2xywh
    (clipped to the image); None is the reference's stretch arithmetic, without a clip."""
    if detections is None:
        return []
    d = detections.detach().cpu().numpy().astype(np.float64)
    out = []
    if pad is not None:
        info = [float(v) for v in img_info[:4]] + [float(pad[0]), float(pad[1])]
        for r in d:
            out.append({'image_id': image_id,
                        'category_id': class_ids[int(r[6])],
                        'bbox': letterbox2xywh((float(r[1]), float(r[0]), float(r[3]), float(r[2])), info),
                        'score': float(r[4] * r[5]),
                        'segmentation': []})
        return out
    for r in d:
        out.append({'image_id': image_id,
                    'category_id': class_ids[int(r[6])],
                    'bbox': yolobox2xywh((float(r[1]), float(r[0]), float(r[3]), float(r[2])), img_info[:4]),
                    'score': float(r[4] * r[5]),
                    'segmentation': []})
    return out
