# -*- coding: utf-8 -*-
"""python -m yolov4_amd.val DATA -c CFG -ckpt PATH: the reference's evaluation script (val.py) on one GPU.

Builds the model of the cfg, loads the checkpoint's 'state_dict' (the averaged weights, when yolov4_amd.train --ema wrote
it), runs validate() over COCODataset('val2017') with the native COCO evaluator and prints its twelve-line summary.
Negative --conf-thre / --nms-thre mean "take the cfg's TEST.CONFTHRE / NMSTHRE", as in the reference.  The NMS,
letterbox and test-time-augmentation options are those of yolov4_amd.detect: a flag that is given overrides the cfg."""
import argparse

import torch

from .detect import add_inference_args, letterbox_from_args, load_cfg, nms_options_from_args, tta_from_args
from .yolo.data.cocodataset import COCOBatchLoader, COCODataset
from .yolo.engine.build import validate
from .yolo.model.build import build_model
from .yolo.util.checkpoint import load_checkpoint
from .yolo.util.cocoeval import COCOEvaluator


def parse(argv=None):
    parser = argparse.ArgumentParser(description='YOLOv4 COCO evaluation on one MI355X')
    parser.add_argument('data', metavar='DIR', help='path to the COCO tree')
    parser.add_argument('-c', '--cfg', required=True, type=str, help='config file, JSON or YAML')
    parser.add_argument('-ckpt', '--checkpoint', type=str, default=None, help='checkpoint in the reference format')
    parser.add_argument('--conf-thre', type=float, default=-0.1, help='confidence threshold; negative: the cfg\'s')
    parser.add_argument('--nms-thre', type=float, default=-0.1, help='NMS threshold; negative: the cfg\'s')
    parser.add_argument('-b', '--batch-size', type=int, default=None, help='default: DATA.BATCH_SIZE')
    parser.add_argument('-j', '--workers', type=int, default=8)
    add_inference_args(parser)
    return parser.parse_args(argv)


def main(argv=None, log=print):
    """Returns (ap50_95, ap50)."""
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit('yolov4_amd.val needs an MI355X: there is no CPU path')
    log('Setting Arguments.. : {}'.format(args))
    cfg = load_cfg(args.cfg)
    device = torch.device('cuda', torch.cuda.current_device())
    model = build_model(args, cfg, device=device)
    if args.checkpoint:
        log("=> loading checkpoint '{}'".format(args.checkpoint))
        load_checkpoint(model, args.checkpoint, strict=True)
    val_set = COCODataset(args.data, name='val2017', img_size=int(cfg['TEST']['IMGSIZE']), model_type=cfg['MODEL']['TYPE'],
                          is_train=False, num_classes=int(cfg['MODEL']['N_CLASSES']))
    batch = args.batch_size if args.batch_size is not None else int(cfg['DATA']['BATCH_SIZE'])
    val_loader = COCOBatchLoader(val_set, batch, cfg, workers=max(1, args.workers), letterbox=letterbox_from_args(args, cfg))
    conf_thre = cfg['TEST']['CONFTHRE'] if args.conf_thre < 0. else args.conf_thre
    nms_thre = cfg['TEST']['NMSTHRE'] if args.nms_thre < 0. else args.nms_thre
    evaluator = COCOEvaluator(val_set.annotation_file)
    log('Begin evaluating ...')
    ap50_95, ap50 = validate(val_loader, model, conf_thre, float(nms_thre), device=device, evaluator=evaluator,
                             num_classes=int(cfg['MODEL']['N_CLASSES']), nms_options=nms_options_from_args(args, cfg),
                             tta=tta_from_args(args, cfg))
    if evaluator.stats is not None:
        log(evaluator.summary())
    else:
        log('no detections above the confidence threshold: AP50:95 0, AP50 0')
    return ap50_95, ap50


if __name__ == '__main__':
    main()
