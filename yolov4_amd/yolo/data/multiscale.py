# -*- coding: utf-8 -*-
"""Multi-scale training: the input size of a training batch as a pure function of (seed, epoch, batch).

Both cfg files of the reference carry AUGMENTATION.RANDOM_RESIZE: True; its rule is `(random.randint(0, 9) % 10 + 10) * 32`
every ten iterations (yolo/engine/build.py:105-107), i.e. 320 ... 608 in steps of 32, Darknet's `random=1`.  Here the draw
does not depend on what was drawn before: a resumed run gets the sizes it would have had, and several ranks agree
without talking.  Pure host code; every error is raised before any GPU work."""
import random


class MultiScale(object):
    """MultiScale(sizes) or MultiScale((lo, hi, step)): `size_at(epoch, batch)` is one of the sizes, constant within every
    run of `every` batches, drawn with random.Random seeded by (seed, epoch, batch // every) like the loader's other
    draws.  A tuple (lo, hi, step) stands for every multiple of `step` in [lo, hi]; `step` is the model's largest stride.
    A list is taken as it is; with `stride` given, each entry has to be a multiple of it.

    ValueError: a range that holds no size, lo > hi, every < 1, a size that is not a positive multiple of the stride."""

    DEFAULT = (320, 608, 32)                                   # the reference's rule
    EVERY = 10

    def __init__(self, sizes=DEFAULT, every=EVERY, seed=0, stride=None):
        if isinstance(sizes, tuple) and len(sizes) == 3:
            lo, hi, step = (int(v) for v in sizes)
            if step < 1:
                raise ValueError(f'the step of a size range must be >= 1, got {step}')
            if lo > hi:
                raise ValueError(f'the size range [{lo}, {hi}] is empty: lo > hi')
            sizes = list(range(-(-lo // step) * step, hi + 1, step))
            if not sizes or sizes[0] < 1:
                raise ValueError(f'the size range [{lo}, {hi}] holds no positive multiple of {step}')
            stride = step if stride is None else stride
        else:
            sizes = [int(s) for s in sizes]
            if not sizes:
                raise ValueError('no sizes given')
        if stride is not None and any(s < 1 or s % int(stride) for s in sizes):
            raise ValueError(f'every size must be a positive multiple of the stride {stride}, got {sizes}')
        if int(every) < 1:
            raise ValueError(f'every must be >= 1, got {every}')
        self.sizes, self.every, self.seed = tuple(sizes), int(every), int(seed)

    def size_at(self, epoch, batch):
        rng = random.Random((self.seed * 1000003 + int(epoch)) * 1000003 + int(batch) // self.every)
        return self.sizes[rng.randrange(len(self.sizes))]

    @classmethod
    def from_cfg(cls, cfg, seed=0):
        """None unless cfg['AUGMENTATION']['RANDOM_RESIZE'] is truthy.  Optional keys: RANDOM_RESIZE_RANGE [lo, hi]
        (default 320, 608) and RANDOM_RESIZE_EVERY (default 10); the step is the largest stride of cfg['MODEL']."""
        aug = cfg.get('AUGMENTATION', {})
        if not aug.get('RANDOM_RESIZE'):
            return None
        from ..model.yololayer import layer_strides
        stride = max(layer_strides(cfg['MODEL'], [8, 16, 32])) if 'MODEL' in cfg else cls.DEFAULT[2]
        lo, hi = aug.get('RANDOM_RESIZE_RANGE', cls.DEFAULT[:2])
        return cls((int(lo), int(hi), int(stride)), every=aug.get('RANDOM_RESIZE_EVERY', cls.EVERY), seed=seed)
