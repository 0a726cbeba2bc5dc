# -*- coding: utf-8 -*-
"""Training helpers of the classifier with the reference's call order (darknet/main_amp.py:335-490, 518-546), without apex
and without the CUDA prefetcher: loaders are plain iterables of (input, target) device batches (darknet/data.py makes them
from image files).  A target is an int64 tensor, or on a CutMix batch a MixedTarget, whose loss is `mixed_loss` and whose
accuracy is scored against the samples' own classes."""
import time

import torch

from .loss import MixedTarget, accuracy, mixed_loss


class AverageMeter(object):
    """main_amp.py:499-515"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def adjust_learning_rate(optimizer, base_lr, epoch, step, len_epoch):
    """main_amp.py:518-546 (base_lr is the script's args.lr): x0.1 at epochs 60, 90 and 110, linear warm-up over the first
    five epochs."""
    if epoch < 60:
        factor = 0
    elif epoch < 90:
        factor = 1
    elif epoch < 110:
        factor = 2
    else:
        factor = 3
    lr = base_lr * (0.1 ** factor)
    if epoch < 5:
        lr = lr * float(1 + step + epoch * len_epoch) / (5. * len_epoch)
    for param_group in optimizer.param_groups:
        param_group['lr'] = lr
    return lr


def train_step(model, criterion, optimizer, input, target):
    """One iteration of main_amp.py:358-376: forward, loss, zero_grad, backward, step.  Returns (output, loss)."""
    output = model(input)
    loss = mixed_loss(criterion, output, target)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return output, loss


def train(train_loader, model, criterion, optimizer, epoch, base_lr, print_freq=10, log=print):
    """One epoch, main_amp.py:335-428; loss and accuracy are read back (a host sync) only every print_freq iterations."""
    batch_time, losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    model.train()
    end = time.time()
    n = len(train_loader)
    for i, (input, target) in enumerate(train_loader, 1):
        lr = adjust_learning_rate(optimizer, base_lr, epoch, i, n)
        output, loss = train_step(model, criterion, optimizer, input, target)
        if i % print_freq == 0:
            own = target.a if isinstance(target, MixedTarget) else target
            prec1, prec5 = accuracy(output.data, own, topk=(1, 5))
            losses.update(float(loss.detach()), input.size(0))
            top1.update(float(prec1), input.size(0))
            top5.update(float(prec5), input.size(0))
            torch.cuda.synchronize()
            batch_time.update((time.time() - end) / print_freq)
            end = time.time()
            if log is not None:
                log(f'Epoch: [{epoch}][{i}/{n}]\tTime {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                    f'Speed {input.size(0) / batch_time.val:.3f} ({input.size(0) / batch_time.avg:.3f})\tLr {lr}\t'
                    f'Loss {losses.val:.10f} ({losses.avg:.4f})\tPrec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
                    f'Prec@5 {top5.val:.3f} ({top5.avg:.3f})')
    return losses.avg


def validate(val_loader, model, criterion, log=print):
    """main_amp.py:431-490: returns the average Prec@1."""
    losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    for input, target in val_loader:
        with torch.no_grad():
            output = model(input)
            loss = criterion(output, target)
        prec1, prec5 = accuracy(output.data, target, topk=(1, 5))
        losses.update(float(loss.detach()), input.size(0))
        top1.update(float(prec1), input.size(0))
        top5.update(float(prec5), input.size(0))
    if log is not None:
        log(f' * Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}')
    return top1.avg
