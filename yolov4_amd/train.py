# -*- coding: utf-8 -*-
"""python -m yolov4_amd.train DATA -c CFG: the reference's detector training script (main_amp.py:61-231) on one GPU.

DATA is a COCO tree (annotations/instances_{train,val}2017.json, images/{train,val}2017/).  Same flow: load the cfg, build
model, optimizer, LR scheduler and criterion, COCODataset + COCOBatchLoader for both splits (training shuffled, mosaic by
the cfg, multi-scale when AUGMENTATION.RANDOM_RESIZE is set: yolo/data/multiscale.py), then for every epoch from
TRAIN.START_EPOCH -- or the checkpoint's -- to TRAIN.MAX_EPOCHS: train, step the scheduler once warm-up is over, validate
with the native COCO evaluator, write checkpoint.pth.tar with the reference's eight keys into TRAIN.OUTPUT_DIR and copy it
to model_best.pth.tar on a new best AP50 (the first validated epoch always is one).  CRITERION.STATS: true adds Darknet's per-layer statistics to the log.

--resume restores model, optimizer, scheduler, the best APs and (with --ema) the average.  The reference tests
`hasattr(checkpoint, 'optimizer')` on a dict (main_amp.py:159-162), which never holds, so it silently resumes with a
fresh optimizer and scheduler; this script uses `in`.  --ema trains with ModelEMA (yolo/util/ema.py), validates and saves
the AVERAGED weights as 'state_dict', and keeps the average's state -- and the live weights, which a resumed run goes on
training -- under the extra keys 'ema' and 'live_state_dict'.

Not here: apex amp (fp32 only), SyncBN, more than one process (the script exits when WORLD_SIZE > 1)."""
import argparse
import os
import random
import time

import torch

from .detect import letterbox_from_args, load_cfg
from .yolo.data.cocodataset import COCOBatchLoader, COCODataset
from .yolo.data.multiscale import MultiScale
from .yolo.engine.build import train, validate
from .yolo.model.build import build_criterion, build_model
from .yolo.optim.lr_schedulers.build import build_lr_scheduler
from .yolo.optim.optimizers.build import build_optimizer
from .yolo.util.checkpoint import save_checkpoint, strip_module_prefix
from .yolo.util.cocoeval import COCOEvaluator
from .yolo.util.ema import ModelEMA


def parse(argv=None):
    parser = argparse.ArgumentParser(description='YOLOv4 training on one MI355X')
    parser.add_argument('data', metavar='DIR', help='path to the COCO tree')
    parser.add_argument('-c', '--cfg', required=True, type=str, metavar='CFG', help='config file, JSON or YAML')
    parser.add_argument('--print-freq', '-p', default=10, type=int, metavar='N')
    parser.add_argument('--resume', default='', type=str, metavar='PATH', help='path to the latest checkpoint')
    parser.add_argument('-e', '--evaluate', dest='evaluate', action='store_true', help='evaluate on the validation set and exit')
    parser.add_argument('-j', '--workers', default=None, type=int, metavar='N',
                        help='host decoding threads, at most 16 (default: DATA.WORKERS, else 8)')
    parser.add_argument('--seed', default=0, type=int, help='seeds the loader, the schedule of sizes and the initial weights')
    parser.add_argument('--ema', action='store_true', help='train with ModelEMA; validate and save the averaged weights')
    parser.add_argument('--letterbox', choices=['off', 'square', 'rect'], default=None,
                        help="validation input; overrides the cfg's TEST.LETTERBOX")
    return parser.parse_args(argv)


def build_data(args, cfg):
    """(train_loader, val_loader) on COCODataset('train2017') / ('val2017'); build_data of the reference, one process."""
    model_type, n_classes = cfg['MODEL']['TYPE'], int(cfg['MODEL']['N_CLASSES'])
    batch = int(cfg['DATA']['BATCH_SIZE'])
    workers = args.workers if args.workers is not None else int(cfg['DATA'].get('WORKERS', 8))
    multiscale = MultiScale.from_cfg(cfg, seed=args.seed)       # ValueError for a bad range before any GPU work
    train_set = COCODataset(args.data, name='train2017', img_size=int(cfg['TRAIN']['IMGSIZE']), model_type=model_type,
                            is_train=True, num_classes=n_classes)
    val_set = COCODataset(args.data, name='val2017', img_size=int(cfg['TEST']['IMGSIZE']), model_type=model_type,
                          is_train=False, num_classes=n_classes)
    train_loader = COCOBatchLoader(train_set, batch, cfg, shuffle=True, seed=args.seed, workers=max(1, workers),
                                   multiscale=multiscale)
    val_loader = COCOBatchLoader(val_set, batch, cfg, workers=max(1, workers), letterbox=letterbox_from_args(args, cfg))
    return train_loader, val_loader


def resume(path, device, model, optimizer, lr_scheduler, live=True, log=print):
    """Restores model, optimizer and scheduler from the checkpoint at `path` and returns it.  live: take the weights a
    run with --ema went on training ('live_state_dict') where the file has them, else 'state_dict'."""
    log("=> loading checkpoint '{}'".format(path))
    checkpoint = torch.load(path, map_location=device, weights_only=True)
    weights = checkpoint['live_state_dict'] if live and 'live_state_dict' in checkpoint else checkpoint['state_dict']
    model.load_state_dict(strip_module_prefix(weights))
    if 'optimizer' in checkpoint:                               # `in`, not the reference's hasattr() on a dict
        optimizer.load_state_dict(checkpoint['optimizer'])
    if 'lr_scheduler' in checkpoint:
        lr_scheduler.load_state_dict(checkpoint['lr_scheduler'])
    log("=> loaded checkpoint '{}' (epoch {})".format(path, checkpoint['epoch']))
    return checkpoint


def main(argv=None, log=print):
    """Returns (ap50_95, ap50) of the last validation (with --evaluate: of the only one)."""
    args = parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('yolov4_amd.train runs one process on one GPU: WORLD_SIZE is %s' % os.environ['WORLD_SIZE'])
    if not torch.cuda.is_available():
        raise SystemExit('yolov4_amd.train needs an MI355X: there is no CPU path')
    cfg = load_cfg(args.cfg)
    args.distributed, args.world_size = False, 1
    device = torch.device('cuda', torch.cuda.current_device())
    train_loader, val_loader = build_data(args, cfg)
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = build_model(args, cfg, device=device)
    optimizer = build_optimizer(cfg, model)
    lr_scheduler = build_lr_scheduler(cfg, optimizer)
    criterion = build_criterion(cfg, device=device)
    start_epoch, max_epochs = int(cfg['TRAIN']['START_EPOCH']), int(cfg['TRAIN']['MAX_EPOCHS'])
    best_ap50 = best_ap50_95 = None                             # none yet: the first validated epoch is the best so far
    checkpoint = None
    if args.resume:
        if not os.path.isfile(args.resume):
            raise SystemExit("no checkpoint found at '{}'".format(args.resume))
        # --evaluate without --ema judges what the file calls its weights: the averaged ones of a run with --ema
        checkpoint = resume(args.resume, device, model, optimizer, lr_scheduler, live=args.ema or not args.evaluate, log=log)
        start_epoch = int(checkpoint['epoch'])
        best_ap50 = float(checkpoint.get('best_ap50', checkpoint['ap50']))
        best_ap50_95 = float(checkpoint.get('best_ap50_95', checkpoint['ap50_95']))
    ema = ModelEMA(model) if args.ema else None                 # of the restored weights; a file with an average replaces it
    if ema is not None and checkpoint is not None and 'ema' in checkpoint:
        ema.load_state_dict(checkpoint['ema'])

    conf_thresh, nms_thresh = cfg['TEST']['CONFTHRE'], float(cfg['TEST']['NMSTHRE'])
    n_classes = int(cfg['MODEL']['N_CLASSES'])
    evaluator = COCOEvaluator(val_loader.dataset.annotation_file)

    def evaluate():
        # a resumed or finished --ema run holds the averaged weights in the average, the live ones in the model
        if ema is not None:
            with ema.applied_to(model):
                return validate(val_loader, model, conf_thresh, nms_thresh, device=device, evaluator=evaluator,
                                num_classes=n_classes)
        return validate(val_loader, model, conf_thresh, nms_thresh, device=device, evaluator=evaluator, num_classes=n_classes)

    if args.evaluate:
        log('Begin evaluating ...')
        ap50_95, ap50 = evaluate()
        log('AP50:95 {:.4f}  AP50 {:.4f}'.format(ap50_95, ap50))
        return ap50_95, ap50

    log('args: {}'.format(args))
    log('cfg: {}'.format(cfg))
    is_warmup, warmup_epoch = cfg['LR_SCHEDULER']['IS_WARMUP'], int(cfg['LR_SCHEDULER']['WARMUP_EPOCH'])
    ap50_95 = ap50 = 0.0
    for epoch in range(start_epoch, max_epochs):
        train_loader.set_epoch(epoch)
        start = time.time()
        train(args, cfg, train_loader, model, criterion, optimizer, device=device, epoch=epoch, log=log, ema=ema)
        torch.cuda.synchronize()
        log('One epoch train need: {:.3f}'.format(time.time() - start))
        if not (is_warmup and epoch < warmup_epoch):
            lr_scheduler.step()
        log('Begin evaluating ...')
        start = time.time()
        ap50_95, ap50 = evaluate()
        log('One epoch validate need: {:.3f}  AP50:95 {:.4f}  AP50 {:.4f}'.format(time.time() - start, ap50_95, ap50))
        is_best = best_ap50 is None or ap50 > best_ap50
        if is_best:
            best_ap50, best_ap50_95 = ap50, ap50_95
        state = {'epoch': epoch + 1, 'ap50': ap50, 'ap50_95': ap50_95, 'best_ap50': best_ap50, 'best_ap50_95': best_ap50_95,
                 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict(),
                 'lr_scheduler': lr_scheduler.state_dict()}
        if ema is not None:
            avg = ema.state_dict()
            state['ema'] = dict(avg)
            state['live_state_dict'] = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
            avg.pop('updates')
            state['state_dict'] = avg
        save_checkpoint(state, is_best, output_dir=cfg['TRAIN']['OUTPUT_DIR'])
    return ap50_95, ap50


if __name__ == '__main__':
    main()
