# -*- coding: utf-8 -*-
"""Detection on image files: the reference's third entry point (detect.py), batched and without cv2.

    decode (data/jpeg.py) -> val_batch -> model (eval) -> postprocess -> yolobox2yxyx -> draw_detections on the
    ORIGINAL-size image (util/vis.py) -> encode_jpeg_batch (data/jpeg_enc.py)

With `letterbox` ('square' | 'rect') the input keeps the image's aspect on a grey canvas instead (letterbox_batch, one launch per
batch; 'rect': a canvas only as large as the batch needs) and boxes come back through letterbox2yxyx, clipped to the image.

Per batch the device work is a handful of launches, and the host waits twice: postprocess's one read of the detection counts
(the detections themselves come back in the same wait) and the encoder's one copy of the coefficients.

    python -m yolov4_amd.detect --cfg CFG --ckpt CKPT --source IMAGE_OR_DIR --dest runs/detect
"""
import argparse
import dataclasses
import glob
import json
import os

import numpy as np
import torch

from ._lib import Y4Error
from .yolo.data.jpeg import decode_jpeg_batch
from .yolo.data.jpeg_enc import encode_jpeg_batch
from .yolo.data.transform import letterbox_batch, letterbox_mode, val_batch
from .yolo.model.yololayer import layer_strides
from .yolo.util.tta import TTAOptions, tta_postprocess, tta_predict, wbf_kwargs
from .yolo.util.utils import NMSOptions, letterbox2yxyx, postprocess, postprocess_nms, yolobox2yxyx
from .yolo.util.vis import class_colors, draw_detections

LINE_WIDTH = 3          # the reference's show_bbox


def load_names(names):
    """None, a list of class names, or a path to a text file with one name per line -> list or None"""
    if names is None or isinstance(names, (list, tuple)):
        return names
    with open(names, 'r') as f:
        return [line.strip() for line in f if line.strip()]


def _read(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(os.fspath(source), 'rb') as f:
        return f.read()


@torch.no_grad()
def detect_images(model, cfg, sources, conf_thre=None, nms_thre=None, names=None, draw=True, encode=True, batch=8,
                  nms_options=None, letterbox=None, tta=None):
    """sources: JPEG bytes, paths, or [h, w, 3] uint8 BGR device tensors, in any mix -> one dict per source:
      detections  float64 ndarray [n, 7]: (y1, x1, y2, x2, obj, cls_conf, cls) in SOURCE pixels, postprocess's order
      image       [h, w, 3] uint8 BGR device tensor of the source's size, the detections drawn on it when `draw`
                  (a tensor source is copied first, never drawn on)
      jpeg        that image as a JPEG file (cv2.imwrite's defaults: quality 95, 4:2:0) when `encode`, else None
    conf_thre / nms_thre default to cfg['TEST']['CONFTHRE'] / ['NMSTHRE'] (None or negative, the reference's rule).  The
    label is '<name> <cls_conf:.2f>'; without `names` the class index stands for the name.  The model is run in eval mode, in
    batches of `batch` images, and left in eval mode.  `nms_options` (an NMSOptions or a dict of postprocess_nms's keywords):
    DIoU- / Soft- / class-agnostic NMS and the per-image cap; None is the reference's postprocess.
    `letterbox`: None stretches every image to S x S (the reference's rule); 'square' | 'rect' keep its aspect on a grey
    canvas, S x S or -- chosen per chunk of `batch` sources -- only as large as the chunk needs, and clip boxes to the image.
    `tta` (a TTAOptions): the model runs on rescaled / mirrored views of each batch -- of the padded canvas when letterboxed --
    and the predictions are merged by NMS or weighted box fusion (yolo/util/tta.py); None: one forward pass, as ever."""
    if nms_options is not None and not isinstance(nms_options, dict):
        nms_options = nms_options.kwargs()
    if tta is not None and tta.merge == 'wbf':
        wbf_kwargs(nms_options)                             # a ValueError before any work
    letterbox = letterbox_mode(letterbox)
    max_stride = max(layer_strides(cfg['MODEL'], [8, 16, 32])) if letterbox is not None else None
    conf_thre = cfg['TEST']['CONFTHRE'] if conf_thre is None or conf_thre < 0 else conf_thre
    nms_thre = cfg['TEST']['NMSTHRE'] if nms_thre is None or nms_thre < 0 else nms_thre
    img_size = int(cfg['TEST']['IMGSIZE'])
    num_classes = int(cfg['MODEL']['N_CLASSES'])
    names = load_names(names)
    if names is not None and len(names) < num_classes:
        raise ValueError('%d names for %d classes' % (len(names), num_classes))
    palette = class_colors(num_classes)
    sources = list(sources)
    batch = max(1, int(batch))
    model.eval()
    results = []
    for start in range(0, len(sources), batch):
        chunk = sources[start:start + batch]
        images = [None] * len(chunk)
        coded = [k for k, s in enumerate(chunk) if not torch.is_tensor(s)]
        if coded:
            for k, t in zip(coded, decode_jpeg_batch([_read(chunk[k]) for k in coded])):
                images[k] = t
        for k, s in enumerate(chunk):
            if torch.is_tensor(s):
                if not (s.is_cuda and s.dtype == torch.uint8 and s.dim() == 3 and s.shape[2] == 3):
                    raise Y4Error('source %d: a tensor source is a [h, w, 3] uint8 BGR device tensor' % (start + k))
                images[k] = s.clone(memory_format=torch.contiguous_format)
        if letterbox is None:
            x, infos = val_batch(images, img_size)
        else:
            x, infos = letterbox_batch(images, img_size, letterbox, max_stride)
        if tta is not None:
            dets = tta_postprocess(tta_predict(model, x, tta), num_classes, conf_thre, nms_thre, tta, nms_options)
        elif nms_options is None:
            dets = postprocess(model(x), num_classes, conf_thre=conf_thre, nms_thre=nms_thre)
        else:
            dets = postprocess_nms(model(x), num_classes, conf_thre=conf_thre, nms_thre=nms_thre, **nms_options)
        # one device -> host copy for the whole batch (the rows of all images are slices of one tensor already)
        have = [d for d in dets if d is not None]
        rows = torch.cat(have).cpu().numpy().astype(np.float64) if have else np.zeros((0, 7))
        boxes_all, labels_all, colors_all, out_rows, at = [], [], [], [], 0
        for d, info in zip(dets, infos):
            n = 0 if d is None else int(d.shape[0])
            r = rows[at:at + n]
            at += n
            # the reference hands (y1, x1, y2, x2) = postprocess's columns 1, 0, 3, 2 to yolobox2yxyx
            if letterbox is None:
                y1, x1, y2, x2 = yolobox2yxyx([r[:, 1], r[:, 0], r[:, 3], r[:, 2]], info[:4])
            else:
                y1, x1, y2, x2 = letterbox2yxyx([r[:, 1], r[:, 0], r[:, 3], r[:, 2]], info)
            out_rows.append(np.concatenate([np.stack([y1, x1, y2, x2], axis=1), r[:, 4:7]], axis=1).reshape(-1, 7))
            cls = r[:, 6].astype(np.int64)
            # int() truncation like the reference's drawing code; a non-finite box (an untrained net) is pinned far outside
            px = np.nan_to_num(np.clip(np.stack([x1, y1, x2, y2], axis=1), -(1 << 20), 1 << 20)).astype(np.int64)
            boxes_all.append([tuple(int(v) for v in b) for b in px.reshape(-1, 4)])
            labels_all.append(['%s %.2f' % (names[c] if names is not None else str(c), p) for c, p in zip(cls, r[:, 5])])
            colors_all.append(palette[cls].reshape(-1, 3))
        if draw:
            draw_detections(images, boxes_all, labels_all, colors_all, line_width=LINE_WIDTH)
        files = encode_jpeg_batch(images) if encode else [None] * len(images)
        for det, img, data in zip(out_rows, images, files):
            results.append({'detections': det, 'image': img, 'jpeg': data})
    return results


def increment_path(path):
    """runs/exp -> runs/exp, runs/exp2, runs/exp3, ...: the first that does not exist yet (the reference's rule)"""
    if not os.path.exists(path):
        return path
    for n in range(2, 9999):
        if not os.path.exists('%s%d' % (path, n)):
            return '%s%d' % (path, n)
    raise RuntimeError('no free directory name after ' + path)


def load_cfg(path):
    """a cfg file as JSON, or as YAML when the yaml package is there"""
    with open(path, 'r') as f:
        text = f.read()
    try:
        return json.loads(text)
    except ValueError:
        try:
            import yaml
        except ImportError:
            raise Y4Error('%s is not JSON, and the yaml package is not installed' % path)
        return yaml.safe_load(text)


def build_parser():
    ap = argparse.ArgumentParser(description='YOLOv4 detection on JPEG files')
    ap.add_argument('--cfg', required=True)
    ap.add_argument('--ckpt', default=None, help='a checkpoint in the reference format, or (YOLOv4Tiny) a Darknet .weights file')
    ap.add_argument('--source', required=True, help='a .jpg file or a directory of them')
    ap.add_argument('--dest', default='./runs/detect/')
    ap.add_argument('--names', default=None, help='text file with one class name per line')
    ap.add_argument('--conf-thre', type=float, default=-0.1)
    ap.add_argument('--nms-thre', type=float, default=-0.1)
    ap.add_argument('--batch', type=int, default=8)
    add_inference_args(ap)
    return ap


def add_inference_args(ap):
    """The NMS, letterbox and test-time-augmentation flags, shared with yolov4_amd.val"""
    # NMS options: a flag that is given overrides the cfg's TEST.NMS_METRIC / NMS_SOFT / NMS_SIGMA / NMS_AGNOSTIC / MAX_DET
    ap.add_argument('--nms-metric', choices=['iou', 'diou'], default=None)
    ap.add_argument('--soft-nms', choices=['none', 'linear', 'gaussian'], default=None)
    ap.add_argument('--nms-sigma', type=float, default=None)
    ap.add_argument('--agnostic-nms', action='store_true', default=None)
    ap.add_argument('--max-det', type=int, default=None)
    # a flag that is given overrides the cfg's TEST.LETTERBOX (off | square | rect; absent: off, the reference's stretch)
    ap.add_argument('--letterbox', choices=['off', 'square', 'rect'], default=None)
    # test-time augmentation: --tta turns it on (the cfg's TEST.TTA, else the defaults); the other flags override its fields
    ap.add_argument('--tta', action='store_true', default=None)
    ap.add_argument('--tta-scales', default=None, help='comma-separated, e.g. 1,0.83,0.67')
    ap.add_argument('--tta-flips', default=None, help='comma-separated 0/1, one per scale, e.g. 0,1,0')
    ap.add_argument('--tta-merge', choices=['nms', 'wbf'], default=None)


def letterbox_from_args(args, cfg):
    """--letterbox when given, else the cfg's optional TEST.LETTERBOX; None for 'off' / absent."""
    v = args.letterbox if args.letterbox is not None else (cfg.get('TEST') or {}).get('LETTERBOX')
    return letterbox_mode(v)


def tta_from_args(args, cfg):
    """The cfg's optional TEST.TTA with the command line's on top; None when neither asks for it.  Any --tta* flag turns it on."""
    o = TTAOptions.from_cfg(cfg)
    if o is None and not args.tta and args.tta_scales is None and args.tta_flips is None and args.tta_merge is None:
        return None
    o = o or TTAOptions()
    over = {}
    if args.tta_scales is not None:
        over['scales'] = tuple(float(v) for v in args.tta_scales.split(','))
        if args.tta_flips is None and len(over['scales']) != len(o.flips):
            over['flips'] = (False,) * len(over['scales'])
    if args.tta_flips is not None:
        over['flips'] = tuple(v.strip().lower() in ('1', 'true', 'yes') for v in args.tta_flips.split(','))
    if args.tta_merge is not None:
        over['merge'] = args.tta_merge
    return dataclasses.replace(o, **over)


def nms_options_from_args(args, cfg):
    """The cfg's NMS options with the command line's on top; None when nothing asks for more than the reference's rule."""
    o = NMSOptions.from_cfg(cfg)
    over = {}
    if args.nms_metric is not None:
        over['metric'] = args.nms_metric
    if args.soft_nms is not None:
        over['soft'] = None if args.soft_nms == 'none' else args.soft_nms
    if args.nms_sigma is not None:
        over['sigma'] = args.nms_sigma
    if args.agnostic_nms:
        over['agnostic'] = True
    if args.max_det is not None:
        over['max_det'] = args.max_det
    o = dataclasses.replace(o, **over)
    return None if o == NMSOptions() else o


def main(argv=None):
    from .yolo.model.build import build_model
    from .yolo.util.checkpoint import load_checkpoint
    args = build_parser().parse_args(argv)
    cfg = load_cfg(args.cfg)
    paths = [args.source] if os.path.isfile(args.source) else sorted(
        glob.glob(os.path.join(args.source, '*.jpg')) + glob.glob(os.path.join(args.source, '*.jpeg')))
    if not paths:
        raise SystemExit('no .jpg files in ' + args.source)
    device = torch.device('cuda')
    model = build_model(None, cfg, device=device)       # MODEL.TYPE: YOLOv4 or YOLOv4Tiny
    if args.ckpt and hasattr(model, 'darknet_convs') and not args.ckpt.endswith(('.pth.tar', '.pth', '.pt')):
        from .yolo.util.darknet_weights import load_darknet_weights
        load_darknet_weights(model, args.ckpt)          # a Darknet .weights file (yolov4-tiny.weights)
    elif args.ckpt:
        load_checkpoint(model, args.ckpt)
    save_dir = increment_path(os.path.join(args.dest, 'exp'))
    os.makedirs(save_dir)
    out = detect_images(model, cfg, paths, args.conf_thre, args.nms_thre, names=args.names, batch=args.batch,
                        nms_options=nms_options_from_args(args, cfg), letterbox=letterbox_from_args(args, cfg),
                        tta=tta_from_args(args, cfg))
    for path, r in zip(paths, out):
        target = os.path.join(save_dir, os.path.splitext(os.path.basename(path))[0] + '.jpg')
        with open(target, 'wb') as f:
            f.write(r['jpeg'])
        print('%s: %d detections -> %s' % (path, len(r['detections']), target))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
