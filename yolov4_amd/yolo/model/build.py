# -*- coding: utf-8 -*-
"""Factories with the reference's signatures (yolo/model/build.py:19-33)."""
from argparse import Namespace
from typing import Dict

from .yolov4 import YOLOv4
from .yolov4_tiny import YOLOv4Tiny
from .yololoss import YOLOLoss

MODELS = {'YOLOv4': YOLOv4, 'YOLOv4Tiny': YOLOv4Tiny}


def model_class(model_cfg: Dict):
    """The network class cfg['MODEL']['TYPE'] names; ValueError for an unknown one."""
    kind = model_cfg.get('TYPE')
    if kind not in MODELS:
        raise ValueError(f"unknown MODEL.TYPE {kind!r}: one of {sorted(MODELS)}")
    return MODELS[kind]


def build_model(args: Namespace, cfg: Dict, device=None):
    # activations and filters are NHWC / KRSC on this path whatever args.channels_last says
    # (the flag only selected a memory format in the reference, build.py:20-26)
    model = model_class(cfg['MODEL'])(cfg['MODEL'], device=device)
    return model.to(device=device)


def build_criterion(cfg: Dict, device=None):
    crit = cfg['CRITERION']
    return YOLOLoss(cfg['MODEL'], ignore_thresh=float(crit['IGNORE_THRESH']), device=device,
                    box_loss=crit.get('BOX_LOSS', 'mse'), box_gain=float(crit.get('BOX_LOSS_GAIN', 1.0)),
                    iou_thresh=float(crit.get('IOU_THRESH', 1.0)),
                    label_smooth=float(crit.get('LABEL_SMOOTH', 0.0)),
                    focal_gamma=float(crit.get('FOCAL_GAMMA', 0.0)), focal_alpha=float(crit.get('FOCAL_ALPHA', 0.25)),
                    focal_terms=crit.get('FOCAL_TERMS', 'obj+cls'), obj_iou_ratio=float(crit.get('OBJ_IOU_RATIO', 0.0)),
                    obj_gain=crit.get('OBJ_GAIN', 1.0), cls_gain=float(crit.get('CLS_GAIN', 1.0)),
                    stats=bool(crit.get('STATS', False))).to(device)
