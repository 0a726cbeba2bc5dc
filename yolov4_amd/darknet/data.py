# -*- coding: utf-8 -*-
"""The classifier's input pipeline (reference: darknet/main_amp.py:205-332) without torchvision and Pillow.

  ImageFolder            torchvision's class-per-directory dataset: file bytes and class indices (decoding is batched)
  sample_crop            RandomResizedCrop.get_params + RandomHorizontalFlip, drawn on the host
  val_geometry           Resize(val_size) + CenterCrop(crop_size) as a resampled size and a window
  sample_cutmix          the CutMix paper's box and permutation, one of each per batch
  RandAugment            torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins): `sample` draws the operations
  randaug_record         one named operation and its magnitude -> the integers and the float the device sees
  imagenet_batch         device uint8 images + parameters -> [B, 3, S, S] fp32, normalised: one pinned job table, one copy,
                         one call of y4_rcrop_u8_f32 (csrc/resample.hip: Pillow's antialiased bilinear resample, bit for bit)
                         or, when a sample carries operations, of y4_rcrop_randaug_u8_f32 (csrc/randaug.hip: Pillow's
                         fourteen operations between the flip and the normalisation, bit for bit)
  ImageNetBatchLoader    files -> (input, target) device batches for darknet/train.py, threaded like COCOBatchLoader

Not here: Mixup; PNG input; more than one process.  The random draws use torchvision's distributions; their order is this
module's own.
"""
import ctypes
import math
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import RandaugOp, RcropJob, check, lib
from ..yolo.data.jpeg import MAX_WORKERS, decode_entropy_batch, entropy_batch
from .loss import MixedTarget

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)      # main_amp.py:284-285: each product in double, rounded to fp32 once
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

# One output sample: crop (x, y, w, h) in the source, the size the crop is resampled to, the S x S window's origin in that
# image, the flip, the CutMix paste (paste_from -1: none; rectangle x0, y0, x1, y1 in output coordinates) and the RandAugment
# operations [(name, signed magnitude)] applied to the flipped crop before any paste.
CropParams = namedtuple('CropParams', 'crop_x crop_y crop_w crop_h res_w res_h win_x win_y flip paste_from paste aug',
                        defaults=(0, 0, 0, -1, (0, 0, 0, 0), ()))


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


# ---------------------------------------------------------------------------------------------------- RandAugment

RA_OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness',
          'Posterize', 'Solarize', 'AutoContrast', 'Equalize')             # index = the Y4_RA_* code
RA_SIGNED = frozenset(RA_OPS[1:10])
MAX_RA_OPS = 8


def _linspace(lo, hi, n):
    """numpy.linspace(lo, hi, n) in double: lo + i * step, the last value hi itself"""
    if n == 1:
        return [float(lo)]
    step = (float(hi) - float(lo)) / (n - 1)
    return [float(lo) + i * step for i in range(n - 1)] + [float(hi)]


def randaug_bins(name, S, num_bins=31):
    """torchvision's RandAugment._augmentation_space for an S x S image: the magnitudes of one operation (None: it takes
    none), in double"""
    if name in ('ShearX', 'ShearY'):
        return _linspace(0.0, 0.3, num_bins)
    if name in ('TranslateX', 'TranslateY'):
        return _linspace(0.0, 150.0 / 331.0 * S, num_bins)
    if name == 'Rotate':
        return _linspace(0.0, 30.0, num_bins)
    if name in ('Brightness', 'Color', 'Contrast', 'Sharpness'):
        return _linspace(0.0, 0.9, num_bins)
    if name == 'Posterize':
        return [float(8 - int(round(i / ((num_bins - 1) / 4.0)))) for i in range(num_bins)]
    if name == 'Solarize':
        return _linspace(255.0, 0.0, num_bins)
    if name not in RA_OPS:
        raise ValueError('unknown RandAugment operation %r' % (name,))
    return None


class RandAugment(object):
    """torchvision.transforms.RandAugment(num_ops, magnitude, num_magnitude_bins) with interpolation NEAREST and fill None.
    sample(S, rng) -> num_ops (name, signed magnitude): per round a uniform draw from the fourteen operations, the magnitude
    bins[magnitude] of that operation for an S x S image, negated with probability 1/2 where the operation is signed."""

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31):
        self.num_ops, self.magnitude, self.num_magnitude_bins = int(num_ops), int(magnitude), int(num_magnitude_bins)
        if not 0 <= self.num_ops <= MAX_RA_OPS:
            raise ValueError('num_ops %d outside [0, %d]' % (self.num_ops, MAX_RA_OPS))
        if self.num_magnitude_bins < 2 or not 0 <= self.magnitude < self.num_magnitude_bins:
            raise ValueError('magnitude %d outside the %d bins' % (self.magnitude, self.num_magnitude_bins))

    def sample(self, S, rng):
        ops = []
        for _ in range(self.num_ops):
            name = RA_OPS[int(rng.integers(0, len(RA_OPS)))]
            table = randaug_bins(name, S, self.num_magnitude_bins)
            m = 0.0 if table is None else table[self.magnitude]
            if name in RA_SIGNED and int(rng.integers(0, 2)):
                m = -m
            ops.append((name, m))
        return tuple(ops)


def _fix(v):
    """libImaging's FIX: 16.16 fixed point, rounded"""
    t = v * 65536.0 + 0.5
    return int(math.floor(t)) if t < 0.0 else int(t)


def _inverse_affine(center, translate, shear):
    """torchvision's _get_inverse_affine_matrix(center, 0, translate, 1, shear): shear in degrees"""
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(-sy) / math.cos(sy)
    b = -math.cos(-sy) * math.tan(sx) / math.cos(sy)
    c = math.sin(-sy) / math.cos(sy)
    d = -math.sin(-sy) * math.tan(sx) / math.cos(sy) + 1.0
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def randaug_record(name, m, S):
    """One operation of magnitude m on an S x S image -> (code, (a0 .. a5), factor, bits, threshold): the fields of a
    y4_randaug_op (include/yolov4_amd.h).  Pure: the inverse matrix in double and libImaging's 16.16 rounding for the
    geometric operations, 1 + m rounded to fp32 for the enhancers, ceil(m) for Solarize."""
    code = RA_OPS.index(name)
    a, factor, bits, threshold = (0,) * 6, 0.0, 0, 0
    if 1 <= code <= 5:
        if name == 'ShearX':
            mat = _inverse_affine((0.0, 0.0), (0, 0), (math.degrees(math.atan(m)), 0.0))
        elif name == 'ShearY':
            mat = _inverse_affine((0.0, 0.0), (0, 0), (0.0, math.degrees(math.atan(m))))
        elif name == 'TranslateX':
            mat = _inverse_affine((S * 0.5, S * 0.5), (int(m), 0), (0.0, 0.0))
        elif name == 'TranslateY':
            mat = _inverse_affine((S * 0.5, S * 0.5), (0, int(m)), (0.0, 0.0))
        else:                                   # Image.rotate(m, NEAREST) about (S / 2, S / 2)
            t = -math.radians(m % 360.0)
            mat = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
            c = S / 2.0
            mat[2] = mat[0] * -c + mat[1] * -c + mat[2] + c
            mat[5] = mat[3] * -c + mat[4] * -c + mat[5] + c
        a = (_fix(mat[0]), _fix(mat[1]), _fix(mat[2] + mat[0] * 0.5 + mat[1] * 0.5),
             _fix(mat[3]), _fix(mat[4]), _fix(mat[5] + mat[3] * 0.5 + mat[4] * 0.5))
    elif 6 <= code <= 9:
        factor = float(np.float32(1.0 + m))
    elif name == 'Posterize':
        bits = int(m)
    elif name == 'Solarize':
        threshold = int(math.ceil(m))
    return code, a, factor, bits, threshold


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
    nbytes = B * ctypes.sizeof(RcropJob)                # a multiple of 16: the operation table behind it is aligned
    n_ops = max(len(p.aug) for p in params)
    if n_ops > MAX_RA_OPS:
        raise ValueError('%d operations on one sample; the library takes %d' % (n_ops, MAX_RA_OPS))
    host = torch.zeros(nbytes + B * n_ops * ctypes.sizeof(RandaugOp), dtype=torch.uint8).pin_memory()
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
    # the operation table [B][n_ops] behind the jobs, in the same pinned block; shorter lists are padded with Identity
    if n_ops:
        ops = (RandaugOp * (B * n_ops)).from_buffer(host.numpy(), nbytes)
        for b, p in enumerate(params):
            for r, (name, m) in enumerate(p.aug):
                o = ops[b * n_ops + r]
                o.op, a, o.factor, o.bits, o.threshold = randaug_record(name, m, S)
                o.a[:] = a
        del ops
    with torch.cuda.device(device):
        table = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        table.copy_(host, non_blocking=True)
        ws = torch.empty(max(at, 16), dtype=torch.uint8, device=device)
        ws2 = torch.empty(int(lib().y4_randaug_workspace(B, S, n_ops)), dtype=torch.uint8, device=device) if n_ops else None
    return dict(S=S, B=B, host=host, table=table, ws=ws, sources=list(images), n_ops=n_ops, ops_at=nbytes, ws2=ws2)


def launch_jobs(plan, out, mean=MEAN, std=STD):
    """The device half: the table launch and the gather launch on the current stream -- with operations, the launches of
    y4_rcrop_randaug_u8_f32 instead; nothing waits for any of them."""
    with torch.cuda.device(out.device):
        head = (plan['table'].data_ptr(), plan['host'].data_ptr(), plan['B'], plan['S'], _f32_array(mean), _f32_array(std),
                out.data_ptr(), out.stride(0), out.stride(1), out.stride(2), out.stride(3), plan['ws'].data_ptr(),
                plan['ws'].numel())
        stream = torch.cuda.current_stream().cuda_stream
        if not plan.get('n_ops'):
            check(lib().y4_rcrop_u8_f32(*head, stream), 'y4_rcrop_u8_f32')
        else:
            at = plan['ops_at']
            check(lib().y4_rcrop_randaug_u8_f32(*head, plan['table'].data_ptr() + at, plan['host'].data_ptr() + at,
                                                plan['n_ops'], plan['ws2'].data_ptr(), plan['ws2'].numel(), stream),
                  'y4_rcrop_randaug_u8_f32')


def imagenet_batch(images, params, S, mean=MEAN, std=STD, out=None, memory_format=torch.contiguous_format, swap_rb=True):
    """images: B uint8 [h, w, 3] device tensors with stride(2) == 1 and stride(1) == 3 (any row pitch: what
    `decode_jpeg_batch` returns); params: one CropParams each -> [B, 3, S, S] fp32, (u8 - mean[c]) / std[c].
    swap_rb: the sources are BGR (the decoder's default) and channel 0 of the result is red.  out: the batch to write into
    (any strides); else a new one in `memory_format`.  One job table written in pinned memory, one asynchronous copy of it
    and one library call (two launches) on the current stream; nothing synchronises.  When a sample's `aug` holds
    RandAugment operations the call is y4_rcrop_randaug_u8_f32 (at most two more launches per round); samples with fewer
    operations than the longest list are padded with Identity."""
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

    train: RandomResizedCrop(crop_size) + flip (+ the operations of `randaugment`, a RandAugment, drawn per sample after
    all crop parameters) (+ CutMix with probability cutmix_prob per batch), every draw from a numpy Generator seeded with
    (seed, epoch, batch), so the same seed gives the same batches; else Resize(val_size) + CenterCrop(crop_size).  shuffle permutes the files per epoch (`set_epoch`); rank / world_size take every world_size-th
    file of that order.  File reads and Huffman decoding run on `workers` threads (at most 16), one batch ahead of the
    device work; one process, none started.  fallback: `decode_jpeg_batch`'s (bytes -> HWC uint8 BGR array) for the files
    the native decoder reports as unsupported (ImageNet holds a few CMYK and progressive ones)."""

    def __init__(self, dataset, batch_size, train, crop_size=256, val_size=288, shuffle=False, seed=0, workers=8, rank=0,
                 world_size=1, cutmix_prob=0.0, fallback=None, randaugment=None):
        assert batch_size >= 1 and 0 <= rank < world_size
        if not train and int(val_size) < int(crop_size):
            raise ValueError('val_size %d is below crop_size %d' % (val_size, crop_size))
        self.dataset, self.batch_size, self.train = dataset, int(batch_size), bool(train)
        self.crop_size, self.val_size = int(crop_size), int(val_size)
        self.shuffle, self.seed, self.epoch = bool(shuffle), int(seed), 0
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.rank, self.world_size = int(rank), int(world_size)
        self.cutmix_prob, self.fallback = float(cutmix_prob), fallback
        self.randaugment = randaugment

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
                    if self.randaugment is not None:
                        params = [p._replace(aug=self.randaugment.sample(S, rng)) for p in params]
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
