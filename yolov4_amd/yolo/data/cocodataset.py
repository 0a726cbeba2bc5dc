# -*- coding: utf-8 -*-
"""The reference's COCO dataset (yolo/data/cocodataset.py) without cv2 and pycocotools: annotations through `json`, images
through the native JPEG decoder (yolo/data/jpeg.py), and a single-process batch loader that feeds `train()` / `validate()`.

`COCODataset` keeps the reference's constructor, attributes and `__getitem__` contract.  `COCOBatchLoader` is what a training
run uses instead of torch's DataLoader over that dataset: files are read and entropy-decoded on threads one batch ahead, the
whole batch (4 B images with mosaic) is decoded on the device in two launches and handed to `train_batch` / `val_batch`
without a copy.  No process is forked and none is started once the GPU is initialised.
"""
import json
import os.path
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .jpeg import MAX_WORKERS, decode_entropy_batch, decode_jpeg_batch, entropy_batch
from .transform import (letterbox_batch, letterbox_labels, letterbox_mode, pad_labels, sample_train_params, train_batch,
                        val_batch)
from ..model.yololayer import layer_strides


class COCODataset(object):
    """Constructor, attributes (`ids`, `class_ids`, ...) and item contract of the reference's class of this name.

    ids        image ids in the order of the annotation file's `images` list
    class_ids  the category ids, sorted; a box's class is its category's position in this list
    Boxes of an image are (x, y, w, h, class) rows in REVERSE annotation order (the reference prepends each one), without
    those whose width or height does not exceed `min_size` and those whose class is outside [0, num_classes)."""

    SPLITS = ('train', 'val')

    def __init__(self, root, name: str = 'train2017', img_size: int = 416, min_size: int = 1,
                 model_type: str = 'YOLO', is_train: bool = True, transform=None, num_classes=80):
        split = next((s for s in self.SPLITS if s in name), None)
        if split is None:
            raise ValueError('%r names neither a train nor a val split' % (name,))
        self.root, self.name, self.model_type = root, name, model_type
        self.img_size, self.min_size, self.num_classes = img_size, min_size, num_classes
        self.is_train, self.transform = is_train, transform
        self.annotation_file = os.path.join(root, 'annotations', 'instances_%s2017.json' % split)
        with open(self.annotation_file, 'r') as f:
            doc = json.load(f)
        self.ids = [im['id'] for im in doc.get('images', [])]
        self._sizes = [(im.get('height'), im.get('width')) for im in doc.get('images', [])]
        self.class_ids = sorted(c['id'] for c in doc.get('categories', []))
        self._class_of = {}
        for k, c in enumerate(self.class_ids):
            self._class_of.setdefault(c, k)                 # what class_ids.index(c) gives
        self._annos = {}
        for a in doc.get('annotations', []):
            self._annos.setdefault(a['image_id'], []).append(a['bbox'][:4] + [a['category_id']])
        self._labels = {}                                   # (index, min_size, num_classes) -> boxes, filled on first use

    def __len__(self):
        return len(self.ids)

    def img_file(self, index):
        path = os.path.join(self.root, 'images', self.name, '%012d.jpg' % self.ids[index])
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        return path

    def img_hw(self, index):
        """(height, width) of image `index` as the annotation file states them; no image is read"""
        h, w = self._sizes[index]
        if not h or not w:
            raise ValueError('image %r has no height / width in %s' % (self.ids[index], self.annotation_file))
        return int(h), int(w)

    def get_labels(self, index):
        """[K, 5] float64 rows (x, y, w, h, class) of image `index` (a fresh copy; K may be 0)"""
        key = (index, self.min_size, self.num_classes)
        rows = self._labels.get(key)
        if rows is None:
            annos = self._annos.get(self.ids[index], [])
            rows = np.array([[x, y, w, h, self._class_of[cat]] for x, y, w, h, cat in reversed(annos)
                             if w > self.min_size and h > self.min_size], dtype=np.float64).reshape(-1, 5)
            rows = rows[(rows[:, 4] >= 0) & (rows[:, 4] < self.num_classes)]
            self._labels[key] = rows
        return rows.copy()

    def get_img_and_labels(self, index=None, decode=False):
        """(image, boxes, image id) of `index`, or of a uniformly drawn image when index is None.  The image is the file's
        bytes, or with decode=True the [h, w, 3] uint8 BGR device tensor (cv2.imread's pixels)."""
        if index is None:
            index = random.randrange(len(self.ids))
        with open(self.img_file(index), 'rb') as f:
            img = f.read()
        if decode:
            img = decode_jpeg_batch([img], workers=1)[0]
        return img, self.get_labels(index), self.ids[index]

    def _drawn_with_boxes(self):
        """a randomly drawn decoded image that has at least one box, with its boxes"""
        while True:
            img, boxes, _ = self.get_img_and_labels(decode=True)
            if len(boxes):
                return img, boxes

    def __getitem__(self, index):
        """-> (input [3, S, S], target) through `transform`; target['img_info'] ends in [image id, index].  In training with a
        mosaic transform three more drawn images, each with boxes, join the indexed one.  Without a transform: (image, None)."""
        img, boxes, img_id = self.get_img_and_labels(index, decode=True)
        if self.transform is None:
            return img, None
        sources = [(img, boxes)]
        if self.is_train and self.transform.is_mosaic:
            sources += [self._drawn_with_boxes() for _ in range(3)]
        x, target = self.transform([im for im, _ in sources], [bb for _, bb in sources], self.img_size)
        labels = target['padded_labels']
        if not (torch.is_tensor(x) and torch.is_tensor(labels) and labels.dim() == 2 and len(labels) > 0
                and labels.shape[1] == 5):
            raise TypeError('the transform has to return a tensor and padded_labels of shape [n, 5]')
        cls = labels[:, 4]
        if bool(((cls < 0) | (cls >= self.num_classes)).any()):
            raise ValueError('a label class outside [0, %d)' % self.num_classes)
        target['img_info'] = list(target['img_info']) + [img_id, index]
        return x, target

    def set_img_size(self, img_size):
        self.img_size = img_size

    def get_img_size(self):
        return self.img_size


class COCOBatchLoader(object):
    """Iterable over (input, target) batches in the form `train()` and `validate()` consume.

    input   [B, 3, S, S] fp32 on the GPU, S = dataset.get_img_size() when the batch is made
    target  {'padded_labels': [B, MAX_NUM_LABELS, 5] float64 on the CPU, 'img_info': B rows}; a row is [img_id, index] when
            training and [h, w, S, S, img_id, index] when validating (what validate() reads)

    Training (dataset.is_train): mosaic by cfg['AUGMENTATION']['IS_MOSAIC'], three extra images with at least one box each
    per sample, every draw from `random.Random` seeded with (seed, epoch, batch): the same seed gives the same batches.
    shuffle permutes the images per epoch (`set_epoch`); rank / world_size take every world_size-th image of that order.
    Host work (file reads, Huffman decoding on `workers` threads, at most 16) runs one batch ahead of the device work.
    multiscale (a MultiScale, yolo/data/multiscale.py; training only): batch b of epoch e is made at
    multiscale.size_at(e, b) instead of dataset.get_img_size(); `last_img_size` is the S of the batch last yielded.

    Validation with letterbox = 'square' | 'rect' (None: the reference's stretch to S x S): the input is `letterbox_batch`'s
    [B, 3, Hc, Wc], labels are mapped onto the canvas, img_info rows are [h, w, nh, nw, img_id, index] and target['pad'] holds B
    rows of (top, left), which validate() hands to detections_to_coco.  'rect' without shuffle orders the images by h / w (from
    the annotation file; no image is read for it) so that a batch's canvas is tight."""

    def __init__(self, dataset, batch_size, cfg, shuffle=False, seed=0, workers=8, rank=0, world_size=1, fallback=None,
                 letterbox=None, multiscale=None):
        assert batch_size >= 1 and 0 <= rank < world_size
        self.letterbox = letterbox_mode(letterbox)
        if self.letterbox is not None and dataset.is_train:
            raise ValueError('letterbox is an inference option: the training pipeline stays square')
        if multiscale is not None and not dataset.is_train:
            raise ValueError('multiscale is a training option: validation runs at the size of its dataset')
        self.multiscale = multiscale
        self.last_img_size = None                           # S of the batch last yielded
        self.dataset, self.batch_size, self.cfg = dataset, int(batch_size), cfg
        self.shuffle, self.seed, self.epoch = bool(shuffle), int(seed), 0
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.rank, self.world_size, self.fallback = int(rank), int(world_size), fallback

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _order(self):
        order = list(range(len(self.dataset)))
        if self.shuffle:
            random.Random(self.seed * 1000003 + self.epoch).shuffle(order)
        elif self.letterbox == 'rect':
            aspect = [h / w for h, w in (self.dataset.img_hw(i) for i in order)]
            order.sort(key=lambda i: aspect[i])            # stable: equal aspects keep the file's order
        return order[self.rank::self.world_size]

    def __len__(self):
        return -(-len(self._order()) // self.batch_size)

    def _host_batch(self, order, b, pool):
        """file reads + the JPEG host stage of batch b: (indices, per-sample image slots, boxes, HostBatch, rng)"""
        ds = self.dataset
        rng = random.Random((self.seed * 1000003 + self.epoch) * 1000003 + b)
        indices = order[b * self.batch_size:(b + 1) * self.batch_size]
        mosaic = bool(ds.is_train and self.cfg['AUGMENTATION']['IS_MOSAIC'])
        groups, boxes = [], []
        for index in indices:
            group, bb = [index], [ds.get_labels(index)]
            if mosaic:
                misses = 0
                while len(group) < 4:
                    k = rng.randrange(len(ds))
                    lab = ds.get_labels(k)
                    if len(lab) > 0:
                        group.append(k)
                        bb.append(lab)
                    else:
                        misses += 1
                        if misses > 100 * len(ds):
                            raise RuntimeError('mosaic needs images with at least one box; found none')
            groups.append(group)
            boxes.append(bb)
        flat = [k for g in groups for k in g]

        def read(k):
            with open(ds.img_file(k), 'rb') as f:
                return f.read()
        files = list(pool.map(read, flat))
        hb = entropy_batch(files, self.workers, True, self.fallback, pool=pool)
        return indices, groups, boxes, hb, rng

    def __iter__(self):
        ds = self.dataset
        order = self._order()
        n = -(-len(order) // self.batch_size)
        if n == 0:
            return
        max_labels = int(self.cfg['DATA']['MAX_NUM_LABELS'])
        with ThreadPoolExecutor(max_workers=self.workers) as pool, ThreadPoolExecutor(max_workers=1) as ahead:
            pending = ahead.submit(self._host_batch, order, 0, pool)
            for b in range(n):
                indices, groups, boxes, hb, rng = pending.result()
                if b + 1 < n:
                    pending = ahead.submit(self._host_batch, order, b + 1, pool)
                S = int(ds.get_img_size())                  # per batch: set_img_size() between batches takes effect
                if self.multiscale is not None:
                    S = int(self.multiscale.size_at(self.epoch, b))
                pad = None
                imgs = decode_entropy_batch(hb)
                at, items = 0, []
                for g, bb in zip(groups, boxes):
                    items.append((imgs[at:at + len(g)], bb))
                    at += len(g)
                if ds.is_train:
                    params = [sample_train_params(self.cfg, [im.shape[:2] for im in il], S, rng, [len(x) for x in bl])
                              for il, bl in items]
                    x, labels = train_batch(items, S, self.cfg, params=params)
                    info = [[ds.ids[i], i] for i in indices]
                elif self.letterbox is not None:
                    G = max(layer_strides(self.cfg['MODEL'], [8, 16, 32]))
                    x, infos = letterbox_batch([il[0] for il, _ in items], S, self.letterbox, G)
                    labels = np.zeros((len(items), max_labels, 5), dtype=np.float64)
                    for k, ((_, bl), inf) in enumerate(zip(items, infos)):
                        labels[k] = pad_labels(letterbox_labels(bl[0], inf), max_labels)
                    labels = torch.from_numpy(labels)
                    info = [inf[:4] + [ds.ids[i], i] for inf, i in zip(infos, indices)]
                    pad = [inf[4:6] for inf in infos]
                else:
                    x, infos = val_batch([il[0] for il, _ in items], S)
                    labels = np.zeros((len(items), max_labels, 5), dtype=np.float64)
                    for k, ((_, bl), inf) in enumerate(zip(items, infos)):
                        bx = np.array(bl[0], dtype=np.float64).reshape(-1, 5)      # as Transform's evaluation branch
                        bx[:, [0, 2]] *= S / inf[1]
                        bx[:, [1, 3]] *= S / inf[0]
                        bx[:, 2] += bx[:, 0]
                        bx[:, 3] += bx[:, 1]
                        labels[k] = pad_labels(bx, max_labels)
                    labels = torch.from_numpy(labels)
                    info = [inf + [ds.ids[i], i] for inf, i in zip(infos, indices)]
                target = {'padded_labels': labels, 'img_info': info}
                if pad is not None:
                    target['pad'] = pad                     # letterboxed input: B rows of (top, left)
                self.last_img_size = S
                yield x, target
