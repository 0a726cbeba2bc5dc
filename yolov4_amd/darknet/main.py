# -*- coding: utf-8 -*-
"""python -m yolov4_amd.darknet.main DATA: the reference's classifier training script (darknet/main_amp.py:44-277) on one GPU.

DATA holds train/ and val/, one sub-directory per class (darknet/data.py).  Same flow: CSPDarknet53, Adam at
lr * batch / 256 (the reference parses --momentum and --weight-decay and then builds Adam without them; so does this script),
label-smoothed cross entropy, the step LR schedule with warm-up, validation after every epoch, checkpoint.pth.tar and, on a
new best Prec@1, model_best.pth.tar in the working directory.  The checkpoint's state_dict carries the 'module.' prefix the
reference's DDP wrapper gives it, which is the form YOLOv4's BACKBONE_PRETRAINED path reads.  --randaugment puts
RandAugment(num_ops=2, magnitude=9) behind the flip: passing it is the reference's recipe (main_amp.py:221-227); it is off by
default, and --ra-num-ops / --ra-magnitude change its two parameters.  Not here: apex amp (fp32 only), more than one process.
Beyond the reference: --num-classes, --crop-size, --val-size, --cutmix-prob, --label-smoothing (the YOLOv4 paper's
classifier recipe is CutMix + label smoothing)."""
import argparse
import os
import shutil

import torch

from .classifier import CSPDarknet53
from .data import ImageFolder, ImageNetBatchLoader, RandAugment
from .loss import CrossEntropyLoss
from .train import train, validate
from ..yolo.optim.optimizers.build import FusedAdam


def parse(argv=None):
    parser = argparse.ArgumentParser(description='CSPDarknet53 ImageNet training on one MI355X')
    parser.add_argument('data', metavar='DIR', help='path to dataset (train/ and val/ inside)')
    parser.add_argument('-j', '--workers', default=8, type=int, metavar='N', help='host decoding threads (at most 16)')
    parser.add_argument('--epochs', default=90, type=int, metavar='N')
    parser.add_argument('-b', '--batch-size', default=256, type=int, metavar='N')
    parser.add_argument('--lr', '--learning-rate', default=0.1, type=float, metavar='LR',
                        help='scaled by batch size / 256; warm-up over the first 5 epochs')
    parser.add_argument('--momentum', default=0.9, type=float, metavar='M', help='parsed and unused, as in the reference')
    parser.add_argument('--weight-decay', '--wd', default=1e-4, type=float, metavar='W',
                        help='parsed and unused, as in the reference')
    parser.add_argument('--print-freq', '-p', default=10, type=int, metavar='N')
    parser.add_argument('--resume', default='', type=str, metavar='PATH')
    parser.add_argument('-e', '--evaluate', dest='evaluate', action='store_true')
    parser.add_argument('--num-classes', default=1000, type=int)
    parser.add_argument('--crop-size', default=256, type=int)
    parser.add_argument('--val-size', default=288, type=int)
    parser.add_argument('--cutmix-prob', default=0.0, type=float)
    parser.add_argument('--label-smoothing', default=0.1, type=float)
    parser.add_argument('--randaugment', action='store_true', help="RandAugment behind the flip: the reference's recipe")
    parser.add_argument('--ra-num-ops', default=2, type=int, metavar='N', help='operations per image (at most 8)')
    parser.add_argument('--ra-magnitude', default=9, type=int, metavar='M', help='magnitude bin, 0..30')
    return parser.parse_args(argv)


def save_checkpoint(state, is_best, filename='checkpoint.pth.tar'):
    """main_amp.py:493-496"""
    torch.save(state, filename)
    if is_best:
        shutil.copyfile(filename, 'model_best.pth.tar')


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit('yolov4_amd.darknet.main needs an MI355X: there is no CPU path')
    device = torch.device('cuda', torch.cuda.current_device())
    print('=> creating model CSPDarknet53')
    model = CSPDarknet53(num_classes=args.num_classes).to(device)
    args.lr = args.lr * float(args.batch_size) / 256.
    optimizer = FusedAdam(model.parameters(), lr=args.lr, betas=(0.9, 0.999), eps=1e-08)
    criterion = CrossEntropyLoss(label_smoothing=args.label_smoothing)
    best_prec1, start_epoch = 0, 0
    if args.resume:
        if os.path.isfile(args.resume):
            print("=> loading checkpoint '{}'".format(args.resume))
            checkpoint = torch.load(args.resume, map_location=device, weights_only=True)
            start_epoch, best_prec1 = checkpoint['epoch'], checkpoint['best_prec1']
            model.load_state_dict({k[len('module.'):] if k.startswith('module.') else k: v
                                   for k, v in checkpoint['state_dict'].items()})
            optimizer.load_state_dict(checkpoint['optimizer'])
            print("=> loaded checkpoint '{}' (epoch {})".format(args.resume, checkpoint['epoch']))
        else:
            print("=> no checkpoint found at '{}'".format(args.resume))

    common = dict(crop_size=args.crop_size, val_size=args.val_size, workers=args.workers)
    val_loader = ImageNetBatchLoader(ImageFolder(os.path.join(args.data, 'val')), args.batch_size, train=False, **common)
    print(args)
    if args.evaluate:
        validate(val_loader, model, criterion)
        return
    train_loader = ImageNetBatchLoader(ImageFolder(os.path.join(args.data, 'train')), args.batch_size, train=True,
                                       shuffle=True, cutmix_prob=args.cutmix_prob,
                                       randaugment=RandAugment(args.ra_num_ops, args.ra_magnitude) if args.randaugment else None,
                                       **common)
    for epoch in range(start_epoch, args.epochs):
        train_loader.set_epoch(epoch)
        train(train_loader, model, criterion, optimizer, epoch, args.lr, print_freq=args.print_freq)
        prec1 = validate(val_loader, model, criterion)
        is_best = prec1 > best_prec1
        best_prec1 = max(prec1, best_prec1)
        save_checkpoint({
            'epoch': epoch + 1,
            'arch': 'CSPDarknet53',
            'state_dict': {'module.' + k: v for k, v in model.state_dict().items()},
            'best_prec1': best_prec1,
            'optimizer': optimizer.state_dict(),
        }, is_best)


if __name__ == '__main__':
    main()
