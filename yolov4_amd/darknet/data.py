# -*- coding: utf-8 -*-
"""The classifier's input pipeline (reference: darknet/main_amp.py:205-332) without torchvision and Pillow.

  ImageFolder            torchvision's class-per-directory dataset: file bytes and class indices (decoding is batched)
  sample_crop            RandomResizedCrop.get_params + RandomHorizontalFlip, drawn on the host
  val_geometry           Resize(val_size) + CenterCrop(crop_size) as a resampled size and a window
  sample_cutmix          the CutMix paper's box and permutation, one of each per batch
  imagenet_batch         device uint8 images + parameters -> [B, 3, S, S] fp32, normalised: one pinned job table, one copy,
                         one call of y4_rcrop_u8_f32 (csrc/resample.hip: Pillow's antialiased bilinear resample, bit for bit)
  ImageNetBatchLoader    files -> (input, target) device batches for darknet/train.py, threaded like COCOBatchLoader

Not here: RandAugment, which the reference applies between the flip and the collate (fourteen PIL operations); Mixup; PNG
input; more than one process.  The random draws use torchvision's distributions; their order is this module's own.
"""
import ctypes
import math
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import RcropJob, check, lib
from ..yolo.data.jpeg import MAX_WORKERS, decode_entropy_batch, entropy_batch
from .loss import MixedTarget

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)      # main_amp.py:284-285: each product in double, rounded to fp32 once
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

# One output sample: crop (x, y, w, h) in the source, the size the crop is resampled to, the S x S window's origin in that
# image, the flip, and the CutMix paste (paste_from -1: none; rectangle x0, y0, x1, y1 in output coordinates).
CropParams = namedtuple('CropParams', 'crop_x crop_y crop_w crop_h res_w res_h win_x win_y flip paste_from paste',
                        defaults=(0, 0, 0, -1, (0, 0, 0, 0)))


class ImageFolder(object):
    """root/<class>/**/<file>: `classes` (sub-directory names, sorted), `class_to_idx`, `samples` [(path, class index)] in
    torchvision's order -- classes in sorted order, inside a class os.walk(followlinks=True) with sorted directories and
    sorted file names; the extension match ignores case; a class without a file raises FileNotFoundError, as does a root
    without a sub-directory.  Item: (the file's bytes, class index)."""

    def __init__(self, root, extensions=('.jpg', '.jpeg')):
        self.root = os.path.expanduser(str(root))
        self.extensions = tuple(e.lower() for e in extensions)
        self.classes = sorted(e.name for e in os.scandir(self.root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError("Couldn't find any class folder in %s." % self.root)
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples, empty = [], []
        for c in self.classes:
            before = len(self.samples)
            for base, _, files in sorted(os.walk(os.path.join(self.root, c), followlinks=True)):
                for name in sorted(files):
                    if name.lower().endswith(self.extensions):
                        self.samples.append((os.path.join(base, name), self.class_to_idx[c]))
            if len(self.samples) == before:
                empty.append(c)
        if empty:
            raise FileNotFoundError('Found no valid file for the classes %s. Supported extensions are: %s'
                                    % (', '.join(empty), ', '.join(self.extensions)))
        self.targets = [t for _, t in self.samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        path, target = self.samples[index]
        with open(path, 'rb') as f:
            return f.read(), target


def sample_crop(h, w, rng, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)):
    """RandomResizedCrop.get_params and the flip coin for an h x w image -> (top, left, crop_h, crop_w, flip).
    rng: a numpy.random.Generator.  Ten attempts: target = h w U(scale), aspect = exp(U(log r0, log r1)),
    cw = int(round(sqrt(target aspect))), ch = int(round(sqrt(target / aspect))), taken when 0 < cw <= w and 0 < ch <= h with
    a uniform integer origin; else the central crop with the aspect clamped to `ratio`.  The flip has probability 0.5."""
    h, w = int(h), int(w)
    area = h * w
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    flip = bool(rng.random() < 0.5)
    for _ in range(10):
        target = area * float(rng.uniform(scale[0], scale[1]))
        aspect = math.exp(float(rng.uniform(lo, hi)))
        cw = int(round(math.sqrt(target * aspect)))
        ch = int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            top = int(rng.integers(0, h - ch + 1))
            left = int(rng.integers(0, w - cw + 1))
            return top, left, ch, cw, flip
    in_ratio = float(w) / float(h)
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw, flip


def val_geometry(h, w, val_size, crop_size):
    """Resize(val_size) + CenterCrop(crop_size) of an h x w image -> (res_h, res_w, win_y, win_x): the short side becomes
    val_size, the long side int(val_size * long / short), the window sits at int(round((res - crop_size) / 2.0))."""
    h, w, val_size, crop_size = int(h), int(w), int(val_size), int(crop_size)
    if val_size < crop_size:
        raise ValueError('val_size %d is below crop_size %d: the centre crop would need padding' % (val_size, crop_size))
    if w <= h:
        res_w, res_h = val_size, int(val_size * h / w)
    else:
        res_h, res_w = val_size, int(val_size * w / h)
    return res_h, res_w, int(round((res_h - crop_size) / 2.0)), int(round((res_w - crop_size) / 2.0))


def train_params(h, w, S, rng, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)):
    top, left, ch, cw, flip = sample_crop(h, w, rng, scale, ratio)
    return CropParams(left, top, cw, ch, int(S), int(S), 0, 0, int(flip))


def val_params(h, w, val_size, crop_size):
    res_h, res_w, win_y, win_x = val_geometry(h, w, val_size, crop_size)
    return CropParams(0, 0, int(w), int(h), res_w, res_h, win_x, win_y, 0)


def sample_cutmix(batch, S, rng, prob, beta=1.0):
    """CutMix (Yun et al. 2019, the authors' train.py) for one batch: None with probability 1 - prob, else
    (perm, (x0, y0, x1, y1), lam): lam ~ Beta(beta, beta), cut = int(S sqrt(1 - lam)), a uniform integer centre, the box
    clipped to [0, S], lam recomputed as the share of the image outside the box.  Sample b receives perm[b]'s pixels."""
    if not float(rng.random()) < float(prob):
        return None
    S = int(S)
    lam = float(rng.beta(beta, beta))
    perm = [int(v) for v in rng.permutation(int(batch))]
    cut = int(S * math.sqrt(1.0 - lam))
    cx, cy = int(rng.integers(0, S)), int(rng.integers(0, S))
    x0, x1 = min(max(cx - cut // 2, 0), S), min(max(cx + cut // 2, 0), S)
    y0, y1 = min(max(cy - cut // 2, 0), S), min(max(cy + cut // 2, 0), S)
    lam = 1.0 - float((x1 - x0) * (y1 - y0)) / float(S * S)
    return perm, (x0, y0, x1, y1), lam


def with_cutmix(params, mix):
    """the batch's CropParams with the paste of `sample_cutmix`'s result written in"""
    if mix is None:
        return list(params)
    perm, box, _ = mix
    return [p._replace(paste_from=perm[b], paste=tuple(box)) for b, p in enumerate(params)]


def _ksize(n_in, n_out):
    return int(math.ceil(max(float(n_in) / float(n_out), 1.0))) * 2 + 1


def job_bytes(p, S):
    """bytes of one sample's coefficient tables (include/yolov4_amd.h: the workspace layout of y4_rcrop_u8_f32)"""
    words = S * (2 + _ksize(p.crop_w, p.res_w)) + S * (2 + _ksize(p.crop_h, p.res_h))
    return (4 * words + 15) & ~15


def _f32_array(values):
    return (ctypes.c_float * 3)(*[float(np.float32(v)) for v in values])


def upload_jobs(images, params, S, swap_rb=True):
    """The host half of `imagenet_batch`: the job table written in pinned memory and copied to the device once
    (asynchronously, on the current stream), the workspace allocated.  Returns what `launch_jobs` needs."""
    S, B = int(S), len(images)
    if B < 1 or len(params) != B:
        raise ValueError('%d images with %d parameter records' % (B, len(params)))
    device = images[0].device
    nbytes = B * ctypes.sizeof(RcropJob)
    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    view = host.numpy()
    jobs = (RcropJob * B).from_buffer(view, 0)
    at = 0
    for b, (im, p) in enumerate(zip(images, params)):
        assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3, 'expect uint8 HWC on the GPU'
        assert im.stride(2) == 1 and im.stride(1) == 3, 'expect packed pixels (any row pitch)'
        j = jobs[b]
        j.src, j.src_pitch, j.src_h, j.src_w = im.data_ptr(), int(im.stride(0)), int(im.shape[0]), int(im.shape[1])
        j.swap_rb = 1 if swap_rb else 0
        j.crop_x, j.crop_y, j.crop_w, j.crop_h = int(p.crop_x), int(p.crop_y), int(p.crop_w), int(p.crop_h)
        j.res_w, j.res_h, j.win_x, j.win_y, j.flip = int(p.res_w), int(p.res_h), int(p.win_x), int(p.win_y), int(bool(p.flip))
        j.paste_from = int(p.paste_from)
        j.paste_x0, j.paste_y0, j.paste_x1, j.paste_y1 = [int(v) for v in p.paste]
        j.ws_offset = at
        if j.crop_w < 1 or j.crop_h < 1 or j.res_w < 1 or j.res_h < 1:
            raise ValueError('sample %d: an empty crop or resampled size' % b)
        at += job_bytes(p, S)
    del jobs, view
    with torch.cuda.device(device):
        table = torch.empty(nbytes, dtype=torch.uint8, device=device)
        table.copy_(host, non_blocking=True)
        ws = torch.empty(max(at, 16), dtype=torch.uint8, device=device)
    return dict(S=S, B=B, host=host, table=table, ws=ws, sources=list(images))


def launch_jobs(plan, out, mean=MEAN, std=STD):
    """The device half: the table launch and the gather launch on the current stream; nothing waits for either."""
    with torch.cuda.device(out.device):
        check(lib().y4_rcrop_u8_f32(plan['table'].data_ptr(), plan['host'].data_ptr(), plan['B'], plan['S'], _f32_array(mean),
                                    _f32_array(std), out.data_ptr(), out.stride(0), out.stride(1), out.stride(2), out.stride(3),
                                    plan['ws'].data_ptr(), plan['ws'].numel(), torch.cuda.current_stream().cuda_stream),
              'y4_rcrop_u8_f32')


def imagenet_batch(images, params, S, mean=MEAN, std=STD, out=None, memory_format=torch.contiguous_format, swap_rb=True):
    """images: B uint8 [h, w, 3] device tensors with stride(2) == 1 and stride(1) == 3 (any row pitch: what
    `decode_jpeg_batch` returns); params: one CropParams each -> [B, 3, S, S] fp32, (u8 - mean[c]) / std[c].
    swap_rb: the sources are BGR (the decoder's default) and channel 0 of the result is red.  out: the batch to write into
    (any strides); else a new one in `memory_format`.  One job table written in pinned memory, one asynchronous copy of it
    and one library call (two launches) on the current stream; nothing synchronises."""
    S, B = int(S), len(images)
    if out is None and B >= 1:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=images[0].device, memory_format=memory_format)
    plan = upload_jobs(images, params, S, swap_rb)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S)
    launch_jobs(plan, out, mean, std)
    return out


class ImageNetBatchLoader(object):
    """Iterable over (input, target) device batches in the form darknet/train.py consumes.

    input   [B, 3, crop_size, crop_size] fp32 on the GPU, normalised with the reference's mean and std
    target  int64 [B] on the GPU; on a training batch where CutMix fired MixedTarget(a, b, lam): a the samples' own
            classes, b their partners', lam the share of the image that is the sample's own

    train: RandomResizedCrop(crop_size) + flip (+ CutMix with probability cutmix_prob per batch), every draw from a
    numpy Generator seeded with (seed, epoch, batch), so the same seed gives the same batches; else Resize(val_size) +
    CenterCrop(crop_size).  shuffle permutes the files per epoch (`set_epoch`); rank / world_size take every world_size-th
    file of that order.  File reads and Huffman decoding run on `workers` threads (at most 16), one batch ahead of the
    device work; one process, none started.  fallback: `decode_jpeg_batch`'s (bytes -> HWC uint8 BGR array) for the files
    the native decoder reports as unsupported (ImageNet holds a few CMYK and progressive ones)."""

    def __init__(self, dataset, batch_size, train, crop_size=256, val_size=288, shuffle=False, seed=0, workers=8, rank=0,
                 world_size=1, cutmix_prob=0.0, fallback=None):
        assert batch_size >= 1 and 0 <= rank < world_size
        if not train and int(val_size) < int(crop_size):
            raise ValueError('val_size %d is below crop_size %d' % (val_size, crop_size))
        self.dataset, self.batch_size, self.train = dataset, int(batch_size), bool(train)
        self.crop_size, self.val_size = int(crop_size), int(val_size)
        self.shuffle, self.seed, self.epoch = bool(shuffle), int(seed), 0
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.rank, self.world_size = int(rank), int(world_size)
        self.cutmix_prob, self.fallback = float(cutmix_prob), fallback

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _order(self):
        order = np.arange(len(self.dataset))
        if self.shuffle:
            order = np.random.default_rng([self.seed, self.epoch]).permutation(len(self.dataset))
        return [int(v) for v in order[self.rank::self.world_size]]

    def __len__(self):
        return -(-len(self._order()) // self.batch_size)

    def _host_batch(self, order, b, pool):
        """file reads + the JPEG host stage of batch b"""
        indices = order[b * self.batch_size:(b + 1) * self.batch_size]
        items = list(pool.map(self.dataset.__getitem__, indices))
        hb = entropy_batch([data for data, _ in items], self.workers, True, self.fallback, pool=pool)
        return [int(t) for _, t in items], hb

    def __iter__(self):
        order = self._order()
        n = -(-len(order) // self.batch_size)
        if n == 0:
            return
        S = self.crop_size
        with ThreadPoolExecutor(max_workers=self.workers) as pool, ThreadPoolExecutor(max_workers=1) as ahead:
            pending = ahead.submit(self._host_batch, order, 0, pool)
            for b in range(n):
                targets, hb = pending.result()
                if b + 1 < n:
                    pending = ahead.submit(self._host_batch, order, b + 1, pool)
                imgs = decode_entropy_batch(hb)
                device = imgs[0].device
                mix = None
                if self.train:
                    rng = np.random.default_rng([self.seed, self.epoch, b])
                    params = [train_params(im.shape[0], im.shape[1], S, rng) for im in imgs]
                    if self.cutmix_prob > 0.0:
                        mix = sample_cutmix(len(imgs), S, rng, self.cutmix_prob)
                        params = with_cutmix(params, mix)
                else:
                    params = [val_params(im.shape[0], im.shape[1], self.val_size, S) for im in imgs]
                x = imagenet_batch(imgs, params, S)
                target = torch.tensor(targets, dtype=torch.int64).to(device, non_blocking=True)
                if mix is not None:
                    target = MixedTarget(target, target[torch.tensor(mix[0], dtype=torch.int64, device=device)], mix[2])
                yield x, target
