# -*- coding: utf-8 -*-
"""Eval input pipeline on the GPU.

Mirrors what the reference does per validation image on the CPU
(yolo/data/transform.py:429-448 `_get_val_item`, :173-187 `image_resize`, :461): BGR->RGB, cv2.resize to
S x S (INTER_LINEAR, 8-bit), HWC->CHW, /255 -- here one HIP kernel per image writing straight into its slot
of the [B,3,S,S] batch, so batches larger than the reference's bs=1 stop being bound by the host.
`img_info` keeps the reference's meaning: [src_h, src_w, dst_h, dst_w].

Training input pipeline (below `val_batch`): the reference's `Transform._get_train_item` (:385-427) -- crop-and-pad with a
mean fill, flip, float resize, HSV jitter, 4-image mosaic -- split into a host sampler that makes every random draw
(`sample_train_params` -> `MosaicParams`), fp64 box arithmetic on the host (`transform_boxes`, `mosaic_boxes`) and two HIP
launches per batch on csrc/augment.hip (`train_batch`).  `Transform` keeps the reference's constructor and call.
JPEG decoding is in `jpeg.py`, the COCO dataset class and the batch loader in `cocodataset.py`.  Not here: `resize_and_pad`,
which the reference's `Transform` never calls.
"""
import ctypes
import random as _random
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..._lib import AugSample, AugSrc, LetterboxSrc, check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def image_resize_into(img, dst, swap_rb=True):
    """img: uint8 [H,W,3] (numpy array or torch tensor, any device); dst: fp32 [3,S,S] view on the GPU."""
    assert dst.is_cuda and dst.dtype == torch.float32 and dst.dim() == 3 and dst.shape[0] == 3
    assert dst.shape[1] == dst.shape[2], 'the reference resizes to a square'
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, 'expect uint8 HWC, 3 channels'
    if not img.is_cuda:
        img = img.to(dst.device, non_blocking=True)
    if img.stride(2) != 1 or img.stride(1) != 3:
        img = img.contiguous()
    h, w = int(img.shape[0]), int(img.shape[1])
    check(lib().y4_preprocess_u8_f32(img.data_ptr(), h, w, img.stride(0), 1 if swap_rb else 0,
                                     dst.data_ptr(), dst.stride(0), dst.stride(1), dst.stride(2),
                                     int(dst.shape[1]), _stream()))
    return [h, w, int(dst.shape[1]), int(dst.shape[2])]


def val_transform(img, img_size, device=None):
    """One image -> (input [3,S,S] fp32 on the GPU, img_info); transform.py:429-448 + :461."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    out = torch.empty((3, img_size, img_size), dtype=torch.float32, device=device)
    return out, image_resize_into(img, out)


def val_batch(imgs, img_size, device=None):
    """List of BGR images of any sizes -> ([B,3,S,S] fp32 batch, list of img_info)."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    out = torch.empty((len(imgs), 3, img_size, img_size), dtype=torch.float32, device=device)
    infos = [image_resize_into(im, out[i]) for i, im in enumerate(imgs)]
    return out, infos


# ------------------------------------------------------------------------------------------------ letterbox (opt-in)
# Aspect-preserving inference input: the image is resized so that its longer side is S and centred on a grey canvas, either
# S x S ('square') or only as large as the batch needs, rounded up to the model's largest stride ('rect').  The reference has
# no such mode (its evaluation stretches to S x S, `val_batch` above); Darknet's letter_box=1 and the later YOLO code bases do.

LETTERBOX_FILL = 114
LETTERBOX_MODES = ('square', 'rect')


def letterbox_mode(value):
    """None / 'off' -> None; 'square' | 'rect' -> itself; anything else: ValueError."""
    if value is None or value == 'off':
        return None
    if value not in LETTERBOX_MODES:
        raise ValueError("letterbox must be None, 'square' or 'rect', got %r" % (value,))
    return value


def letterbox_geometry(h, w, S):
    """(nh, nw): the size an h x w image is resized to so that its longer side becomes S."""
    h, w, S = int(h), int(w), int(S)
    if h < 1 or w < 1 or S < 1:
        raise ValueError('letterbox_geometry needs positive sizes, got %r' % ((h, w, S),))
    r = S / max(h, w)
    nh = min(S, max(1, int(np.floor(h * r + 0.5))))
    nw = min(S, max(1, int(np.floor(w * r + 0.5))))
    return nh, nw


def letterbox_canvas(sizes, S, mode='rect', G=32):
    """(Hc, Wc) of the canvas that holds a batch of resized (nh, nw) images: (S, S) for 'square'; for 'rect' the largest nh
    and nw, each rounded up to a multiple of G (the model's largest stride).  S must be a multiple of G."""
    S, G = int(S), int(G)
    if mode not in LETTERBOX_MODES:
        raise ValueError("letterbox mode must be 'square' or 'rect', got %r" % (mode,))
    if G < 1 or S % G != 0:
        raise ValueError('the input size %d is not a multiple of the largest stride %d' % (S, G))
    if mode == 'square':
        return S, S
    sizes = list(sizes)
    if not sizes:
        raise ValueError('letterbox_canvas needs at least one image')
    return -(-max(nh for nh, _ in sizes) // G) * G, -(-max(nw for _, nw in sizes) // G) * G


def letterbox_offsets(nh, nw, Hc, Wc):
    """(top, left) of an nh x nw image centred on an Hc x Wc canvas."""
    return (Hc - nh) // 2, (Wc - nw) // 2


def letterbox_batch(imgs, img_size, mode='rect', stride=32, fill=LETTERBOX_FILL, device=None, out=None, swap_rb=True):
    """List of uint8 HWC BGR images of any sizes (numpy arrays or tensors on any device) -> ([B, 3, Hc, Wc] fp32 batch on the
    GPU, infos) with infos[b] = [h, w, nh, nw, top, left].  One descriptor table goes from pinned memory to the device and ONE
    launch (csrc/preprocess.hip) resizes every image with cv2.resize's 8-bit INTER_LINEAR arithmetic and writes the padding
    around it; nothing waits for the device.  out: the batch to write into (any strides; its shape fixes the canvas)."""
    S, B = int(img_size), len(imgs)
    assert B >= 1
    if out is not None:
        device = out.device
    device = device or torch.device('cuda', torch.cuda.current_device())
    srcs = [_as_device_u8(im, device) for im in imgs]
    geo = [letterbox_geometry(t.shape[0], t.shape[1], S) for t in srcs]
    Hc, Wc = letterbox_canvas(geo, S, mode, stride)
    if out is None:
        out = torch.empty((B, 3, Hc, Wc), dtype=torch.float32, device=device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, Hc, Wc)
    host = torch.empty(B * ctypes.sizeof(LetterboxSrc), dtype=torch.uint8).pin_memory()
    view = host.numpy()
    table = (LetterboxSrc * B).from_buffer(view, 0)
    infos = []
    for r, t, (nh, nw) in zip(table, srcs, geo):
        top, left = letterbox_offsets(nh, nw, Hc, Wc)
        r.src, r.h, r.w, r.pitch, r.swap_rb = t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), 1 if swap_rb else 0
        r.nh, r.nw, r.top, r.left, r.reserved = nh, nw, top, left, 0
        infos.append([int(t.shape[0]), int(t.shape[1]), nh, nw, top, left])
    del table, view
    with torch.cuda.device(device):
        dev = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
        check(lib().y4_letterbox_batch_u8_f32(dev.data_ptr(), host.data_ptr(), B, out.data_ptr(), out.stride(0), out.stride(1),
                                              out.stride(2), out.stride(3), Hc, Wc, int(fill), _stream()),
              'y4_letterbox_batch_u8_f32')
    return out, infos


def letterbox_labels(boxes_xywh_cls, info):
    """[K, 5] (x, y, w, h, cls) in source pixels -> (x1, y1, x2, y2, cls) on the letterboxed canvas, float64."""
    h, w, nh, nw, top, left = info[:6]
    b = np.array(boxes_xywh_cls, dtype=np.float64).reshape(-1, 5)
    b[:, 2] += b[:, 0]
    b[:, 3] += b[:, 1]
    b[:, [0, 2]] = b[:, [0, 2]] * nw / w + left
    b[:, [1, 3]] = b[:, [1, 3]] * nh / h + top
    return b


# ------------------------------------------------------------------------------------------------ training: parameters

@dataclass
class AugParams:
    """Every random draw the reference makes for ONE source image (crop_and_pad, left_right_flip, color_dithering).
    Crop offsets may be negative (padding).  `perm`: the order the reference's in-crop shuffle gives the boxes, or None."""
    crop_left: int = 0
    crop_right: int = 0
    crop_top: int = 0
    crop_bottom: int = 0
    flip: bool = False
    color: bool = False
    dhue: float = 0.0
    dsat: float = 1.0
    dexp: float = 1.0
    perm: Optional[Tuple[int, ...]] = None


@dataclass
class MosaicParams:
    """One output sample: the cut point and one AugParams (plain sample) or four (mosaic tiles 0..3)."""
    cut_x: int = 0
    cut_y: int = 0
    tiles: List[AugParams] = field(default_factory=list)


class _DefaultRng(object):
    """The generators the reference draws from: Python's `random` and `numpy.random`."""
    random = staticmethod(_random.random)
    randint = staticmethod(_random.randint)

    @staticmethod
    def normal(mu=0.0, sigma=1.0):
        return mu + sigma * float(np.random.randn())


def _std_normal(rng):
    return rng.gauss(0.0, 1.0) if hasattr(rng, 'gauss') else rng.normal(0.0, 1.0)


def _rand_scale(rng, s):
    lo, hi = (1.0, float(s)) if s >= 1 else (float(s), 1.0)
    u = rng.random() * (hi - lo) + lo
    return u if rng.randint(0, 1) % 2 else 1.0 / u


def sample_train_params(cfg, src_shapes, img_size, rng=None, num_boxes=None):
    """Draw the augmentation parameters of one output sample with the reference's distributions.

    cfg: the configuration with its 'AUGMENTATION' section; src_shapes: (h, w) of the 1 or 4 source images; num_boxes:
    box count per source, for the in-crop shuffle (None: no permutation is stored).  rng: an object with random(),
    randint(a, b) (both ends included) and gauss(mu, sigma) or normal(mu, sigma) -- a `random.Random(seed)` will do; the
    default draws from `random` and `numpy.random`, as the reference does.

      crop    jitter_h, jitter_w = int(h * JITTER), int(w * JITTER); four integers uniform in [-jitter, +jitter]
      flip    RANDOM_HORIZONTAL_FLIP and a standard-normal draw > 0.5: the reference's actual rule (`np.random.randn() > 0.5`),
              which flips about 31 % of the images, not 50 %.  Kept as it is.
      dhue    uniform in [-HUE, HUE]; dsat, dexp: u or 1 / u by a fair coin, u uniform in [1, SATURATION] / [1, EXPOSURE]
      color   COLOR_DITHERING
      cut     two integers uniform in [int(S * MIN_OFFSET), int(S * (1 - MIN_OFFSET))]

    JITTER >= 0.5 is refused (ValueError): the crop could become empty.  The ORDER of the draws is this function's own:
    draw-order parity with the reference is neither claimed nor tested (its module imports cv2 and uses `np.int`, so it
    cannot be imported beside this one)."""
    aug = cfg['AUGMENTATION']
    jitter = float(aug['JITTER'])
    if not 0.0 <= jitter < 0.5:
        raise ValueError('AUGMENTATION.JITTER = %r: outside [0, 0.5) the crop can become empty' % (jitter,))
    if len(src_shapes) not in (1, 4):
        raise ValueError('one source image, or four for a mosaic; got %d' % len(src_shapes))
    rng = rng or _DefaultRng
    S = int(img_size)
    lo, hi = int(S * aug['MIN_OFFSET']), int(S * (1 - aug['MIN_OFFSET']))
    out = MosaicParams(cut_x=rng.randint(lo, hi), cut_y=rng.randint(lo, hi))
    for i, (h, w) in enumerate(src_shapes):
        jh, jw = int(h * jitter), int(w * jitter)
        p = AugParams(crop_left=rng.randint(-jw, jw), crop_right=rng.randint(-jw, jw),
                      crop_top=rng.randint(-jh, jh), crop_bottom=rng.randint(-jh, jh))
        p.flip = bool(aug['RANDOM_HORIZONTAL_FLIP']) and _std_normal(rng) > 0.5
        p.color = bool(aug['COLOR_DITHERING'])
        hue = abs(float(aug['HUE']))
        p.dhue = rng.random() * 2.0 * hue - hue
        p.dsat = _rand_scale(rng, aug['SATURATION'])
        p.dexp = _rand_scale(rng, aug['EXPOSURE'])
        if num_boxes is not None:
            order = list(range(int(num_boxes[i])))
            for j in range(len(order) - 1, 0, -1):              # Fisher-Yates on randint alone
                k = rng.randint(0, j)
                order[j], order[k] = order[k], order[j]
            p.perm = tuple(order)
        out.tiles.append(p)
    return out


# ------------------------------------------------------------------------------------------------ training: boxes (fp64)

def _crop_size(src_shape, p):
    h, w = int(src_shape[0]), int(src_shape[1])
    return h - p.crop_top - p.crop_bottom, w - p.crop_left - p.crop_right


def _clip_and_drop(b, sx, sy):
    """clip xyxy rows to [0, sx] x [0, sy]; drop the rows that collapsed onto an edge (crop_and_pad / filter_truth)"""
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, sx)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, sy)
    gone = (((b[:, 1] == sy) & (b[:, 3] == sy)) | ((b[:, 0] == sx) & (b[:, 2] == sx)) |
            ((b[:, 1] == 0) & (b[:, 3] == 0)) | ((b[:, 0] == 0) & (b[:, 2] == 0)))
    return b[~gone]


def transform_boxes(bboxes_xywh_cls, src_shape, p, img_size):
    """[K, 5] (x, y, w, h, cls) in source pixels -> [K', 5] (x1, y1, x2, y2, cls) in the resized S x S image of this source:
    xywh -> xyxy, (the stored permutation,) minus the crop origin, clip to the crop, drop collapsed boxes, mirror, scale."""
    b = np.array(bboxes_xywh_cls, dtype=np.float64).reshape(-1, 5)
    if p.perm is not None:
        assert sorted(p.perm) == list(range(len(b))), 'perm is not a permutation of the boxes'
        b = b[list(p.perm)]
    crop_h, crop_w = _crop_size(src_shape, p)
    b[:, 2] += b[:, 0]
    b[:, 3] += b[:, 1]
    b[:, [0, 2]] -= p.crop_left
    b[:, [1, 3]] -= p.crop_top
    b = _clip_and_drop(b, crop_w, crop_h)
    if p.flip:
        x1 = crop_w - b[:, 2]
        b[:, 2] = crop_w - b[:, 0]
        b[:, 0] = x1
    b[:, [0, 2]] *= img_size / crop_w
    b[:, [1, 3]] *= img_size / crop_h
    return b


def mosaic_shifts(src_shape, p, cut_x, cut_y, img_size):
    """(left, top, right, bottom) shifts of blend_mosaic: how far the tile's window moves into its resized image so that
    padding is skipped first; left and right crop offsets trade places under a flip."""
    S = int(img_size)
    crop_h, crop_w = _crop_size(src_shape, p)
    cl, cr = (p.crop_right, p.crop_left) if p.flip else (p.crop_left, p.crop_right)
    left = int(min(cut_x, max(0, -int(cl) * S / crop_w)))
    top = int(min(cut_y, max(0, -int(p.crop_top) * S / crop_h)))
    right = int(min(S - cut_x, max(0, -int(cr) * S / crop_w)))
    bottom = int(min(S - cut_y, max(0, -int(p.crop_bottom) * S / crop_h)))
    return min(left, S - cut_x), min(top, S - cut_y), min(right, cut_x), min(bottom, cut_y)


def tile_window(idx, shifts, cut_x, cut_y, img_size):
    """tile idx -> (win_x, win_y, extent_x, extent_y, out_x, out_y): the window's origin in the resized image, its size,
    and where it lands in the output"""
    S = int(img_size)
    left, top, right, bottom = shifts
    wx = cut_x - right if idx & 1 else left
    wy = cut_y - bottom if idx & 2 else top
    ex = S - cut_x if idx & 1 else cut_x
    ey = S - cut_y if idx & 2 else cut_y
    return wx, wy, ex, ey, (cut_x if idx & 1 else 0), (cut_y if idx & 2 else 0)


def mosaic_boxes(bboxes_xyxy_cls, idx, src_shape, p, cut_x, cut_y, img_size):
    """filter_truth for tile idx: rows of transform_boxes -> rows in the mosaic output (xyxy): minus the window origin,
    clip to the window, drop collapsed boxes, plus the tile's position."""
    b = np.array(bboxes_xyxy_cls, dtype=np.float64).reshape(-1, 5)
    wx, wy, ex, ey, ox, oy = tile_window(idx, mosaic_shifts(src_shape, p, cut_x, cut_y, img_size), cut_x, cut_y, img_size)
    b[:, [0, 2]] -= wx
    b[:, [1, 3]] -= wy
    b = _clip_and_drop(b, ex, ey)
    b[:, [0, 2]] += ox
    b[:, [1, 3]] += oy
    return b


def pad_labels(bboxes_xyxy_cls, max_num_labels):
    """xyxy rows -> [max_num_labels, 5] float64 (xc, yc, w, h, cls): the first rows kept, zero rows after"""
    b = np.asarray(bboxes_xyxy_cls, dtype=np.float64).reshape(-1, 5)[:max_num_labels]
    out = np.zeros((max_num_labels, 5), dtype=np.float64)
    out[:len(b), 0] = (b[:, 0] + b[:, 2]) / 2
    out[:len(b), 1] = (b[:, 1] + b[:, 3]) / 2
    out[:len(b), 2] = b[:, 2] - b[:, 0]
    out[:len(b), 3] = b[:, 3] - b[:, 1]
    out[:len(b), 4] = b[:, 4]
    return out


def sample_labels(bboxes_list, src_shapes, mp, img_size, max_num_labels):
    """padded labels of one output sample from its sources' boxes"""
    rows = []
    for idx, (bb, shp, p) in enumerate(zip(bboxes_list, src_shapes, mp.tiles)):
        b = transform_boxes(bb, shp, p, img_size)
        if len(mp.tiles) == 4:
            b = mosaic_boxes(b, idx, shp, p, mp.cut_x, mp.cut_y, img_size)
        rows.append(b)
    return pad_labels(np.concatenate(rows, axis=0), max_num_labels)


# ------------------------------------------------------------------------------------------------ training: images

def _as_device_u8(img, device):
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, 'expect uint8 HWC, 3 channels'
    if not img.is_cuda:
        img = img.to(device, non_blocking=True)
    if img.stride(2) != 1 or img.stride(1) != 3:
        img = img.contiguous()
    return img


def fill_descriptors(srcs, samples, entries, img_size, swap_rb=True):
    """Write the y4_aug_src / y4_aug_sample records of a batch.  entries: per output sample (MosaicParams, [(pointer, h, w,
    pitch), ...]); srcs / samples: ctypes arrays of AugSrc / AugSample."""
    S = int(img_size)
    t = 0
    for b, (mp, imgs) in enumerate(entries):
        n = len(imgs)
        if n not in (1, 4) or len(mp.tiles) != n:
            raise ValueError('sample %d: %d images with %d parameter records; expect 1 or 4 of each' % (b, n, len(mp.tiles)))
        samples[b].cut_x, samples[b].cut_y, samples[b].n_src, samples[b].first = int(mp.cut_x), int(mp.cut_y), n, t
        for idx, (p, (ptr, h, w, pitch)) in enumerate(zip(mp.tiles, imgs)):
            r = srcs[t]
            crop_h, crop_w = _crop_size((h, w), p)
            r.src, r.h, r.w, r.pitch, r.swap_rb = ptr, h, w, pitch, 1 if swap_rb else 0
            r.crop_left, r.crop_top, r.crop_w, r.crop_h, r.flip = int(p.crop_left), int(p.crop_top), crop_w, crop_h, int(bool(p.flip))
            r.color, r.dhue, r.dsat, r.dexp = int(bool(p.color)), float(p.dhue), float(p.dsat), float(p.dexp)
            r.win_x = r.win_y = 0
            if n == 4:
                r.win_x, r.win_y = tile_window(idx, mosaic_shifts((h, w), p, mp.cut_x, mp.cut_y, S), mp.cut_x, mp.cut_y, S)[:2]
            t += 1
    return t


def upload_batch(items, params, img_size, max_labels, device):
    """The host half of `train_batch`: sources to the device, labels in fp64, the descriptor table written in pinned memory
    and copied to the device once (asynchronously, on the current stream).  Returns what `launch_batch` needs."""
    S, B = int(img_size), len(items)
    labels = np.zeros((B, max_labels, 5), dtype=np.float64)
    keep, entries = [], []
    for b, ((imgs, boxes), mp) in enumerate(zip(items, params)):
        dev_imgs = [_as_device_u8(im, device) for im in imgs]
        keep.extend(dev_imgs)
        entries.append((mp, [(t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0))) for t in dev_imgs]))
        labels[b] = sample_labels(boxes, [t.shape[:2] for t in dev_imgs], mp, S, max_labels)
    n_table = len(keep)
    src_bytes = n_table * ctypes.sizeof(AugSrc)
    host = torch.empty(src_bytes + B * ctypes.sizeof(AugSample), dtype=torch.uint8).pin_memory()
    view = host.numpy()
    srcs = (AugSrc * n_table).from_buffer(view, 0)
    samples = (AugSample * B).from_buffer(view, src_bytes)
    fill_descriptors(srcs, samples, entries, S)
    del srcs, samples, view
    table = torch.empty(host.numel(), dtype=torch.uint8, device=device)
    table.copy_(host, non_blocking=True)
    sums = torch.empty(3 * n_table, dtype=torch.int64, device=device)
    return dict(S=S, B=B, n_table=n_table, src_bytes=src_bytes, host=host, table=table, sums=sums, sources=keep, labels=labels)


def launch_batch(plan, out):
    """The device half: the sums launch, then the gather launch, on the current stream; nothing waits for either."""
    hp, dp, nb = plan['host'].data_ptr(), plan['table'].data_ptr(), plan['src_bytes']
    check(lib().y4_augment_means_u8(dp, hp, plan['n_table'], plan['sums'].data_ptr(), _stream()), 'y4_augment_means_u8')
    check(lib().y4_augment_mosaic_u8_f32(dp, hp, plan['n_table'], dp + nb, hp + nb, plan['B'], plan['sums'].data_ptr(),
                                         out.data_ptr(), out.stride(0), out.stride(1), out.stride(2), out.stride(3),
                                         plan['S'], _stream()), 'y4_augment_mosaic_u8_f32')


def train_batch(items, img_size, cfg, params=None, rng=None, out=None):
    """items: B entries (img_list, bboxes_list) of 1 or 4 uint8 HWC BGR images (numpy arrays or tensors on any device) with
    their [K, 5] (x, y, w, h, cls) boxes -> (x [B,3,S,S] fp32 on the GPU, padded_labels [B, MAX_NUM_LABELS, 5] float64 on
    the CPU).  params: one MosaicParams per entry (drawn with `sample_train_params` and rng when None).  out: the batch to
    write into (any strides).  The sources are uploaded, ONE descriptor table goes from pinned memory to the device, then the
    sums launch and the gather launch follow on the current stream: no host synchronisation anywhere."""
    S, B = int(img_size), len(items)
    assert B >= 1
    max_labels = int(cfg['DATA']['MAX_NUM_LABELS'])
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=torch.device('cuda', torch.cuda.current_device()))
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S)
    if params is None:
        params = [sample_train_params(cfg, [im.shape[:2] for im in imgs], S, rng, [len(bb) for bb in boxes])
                  for imgs, boxes in items]
    assert len(params) == B
    with torch.cuda.device(out.device):
        plan = upload_batch(items, params, S, max_labels, out.device)
        launch_batch(plan, out)
    return out, torch.from_numpy(plan['labels'])


class Transform(object):
    """The reference's Transform (yolo/data/transform.py:359-481): same constructor, same call.  Training goes through
    `train_batch` with one sample, evaluation through `val_transform`.  Difference: the image is fp32 on the GPU (the
    reference returns float64 on the CPU); labels stay float64 on the CPU."""

    def __init__(self, cfg, is_train=True):
        self.cfg = cfg
        self.is_train = is_train
        aug = cfg['AUGMENTATION']
        self.jitter_ratio = aug['JITTER']
        self.is_flip = aug['RANDOM_HORIZONTAL_FLIP']
        self.color_jitter = aug['COLOR_DITHERING']
        self.hue, self.saturation, self.exposure = aug['HUE'], aug['SATURATION'], aug['EXPOSURE']
        self.is_mosaic = aug['IS_MOSAIC']
        self.min_offset = aug['MIN_OFFSET']
        self.max_num_labels = cfg['DATA']['MAX_NUM_LABELS']

    def __call__(self, img_list, bboxes_list, img_size):
        if self.is_train:
            assert len(img_list) == len(bboxes_list) == (4 if self.is_mosaic else 1)
            x, labels = train_batch([(img_list, bboxes_list)], img_size, self.cfg)
            return x[0], {'padded_labels': labels[0], 'img_info': []}
        assert len(img_list) == 1 and len(bboxes_list) == 1
        img, info = val_transform(img_list[0], img_size)
        b = np.array(bboxes_list[0], dtype=np.float64).reshape(-1, 5)      # (x, y, w, h, cls), scaled, then centre form
        b[:, [0, 2]] *= img_size / info[1]
        b[:, [1, 3]] *= img_size / info[0]
        b[:, 2] += b[:, 0]
        b[:, 3] += b[:, 1]
        return img, {'padded_labels': torch.from_numpy(pad_labels(b, self.max_num_labels)), 'img_info': info}
