# -*- coding: utf-8 -*-
"""Exponential moving average of a model's weights for validation (not in the reference, which validates the live
weights): every floating-point state_dict entry, parameters and BatchNorm running statistics alike, is averaged by ONE
multi-tensor HIP launch per update (y4_ema_multi_f32 over the optimizers' 48-byte chunk records); done from Python the
same update is 430+ small launches.

    ema = ModelEMA(model)
    train_step(..., ema=ema)                 # updates after every optimizer step
    with ema.applied_to(model):
        validate(val_loader, model, ...)

Given the optimizer's guard record (FusedAdam / FusedSGD with max_grad_norm or skip_nonfinite), an update that follows a
skipped step writes nothing: decided on the device, no host sync.  The host-side `updates` counter (the decay ramp)
advances all the same, by the optimizers' step-number policy.
"""
import contextlib
import math
from collections import OrderedDict

import numpy as np
import torch

from ... import ops
from ..._lib import check, lib
from ..optim.optimizers.build import CHUNK, dense_like


def _unwrap(model):
    inner = getattr(model, 'module', None)
    return inner if isinstance(inner, torch.nn.Module) else model


class ModelEMA:
    """Holds tensors only (no copy of the module): for every state_dict entry a clone in the entry's own memory
    layout (conv weights are KRSC / channels_last; the kernel pairs elements by raw offset)."""

    def __init__(self, model, decay=0.9999, tau=2000.0):
        self.decay = float(decay)
        self.tau = float(tau)
        self.updates = 0
        self.ema = OrderedDict((k, v.detach().clone(memory_format=torch.preserve_format))
                               for k, v in _unwrap(model).state_dict().items())
        self._table = None
        self._table_key = None

    def decay_at(self, updates):
        """decay * (1 - exp(-updates / tau)): the average follows the young model closely and settles at `decay`."""
        return self.decay * (1.0 - math.exp(-updates / self.tau))

    def _pairs(self, model):
        live = _unwrap(model).state_dict()
        if list(live.keys()) != list(self.ema.keys()):
            raise ops.Y4Error('ModelEMA: the model\'s state_dict keys differ from the ones the average was built from')
        return [(k, self.ema[k], s) for k, s in live.items()]          # state_dict() hands out detached tensors

    @torch.no_grad()
    def update(self, model, guard=None):
        """One launch over all floating-point entries; integer entries (num_batches_tracked) are copied.  guard: the
        optimizer's device record, or None."""
        self.updates += 1
        one_minus_decay = 1.0 - self.decay_at(self.updates)
        rows, key, dev, ints = [], [], None, ([], [])
        for k, e, s in self._pairs(model):
            if not s.is_floating_point():
                if e.device != s.device:
                    self.ema[k] = e = e.to(s.device)
                ints[0].append(e)
                ints[1].append(s)
                continue
            if not s.is_cuda:
                raise ops.Y4Error('ModelEMA.update: tensors must live on the GPU (no CPU fallback)')
            if s.dtype != torch.float32:
                raise ops.Y4Error(f'ModelEMA.update: float32 entries only ({k} is {s.dtype})')
            if not (s.is_contiguous() or (s.dim() == 4 and s.is_contiguous(memory_format=torch.channels_last))):
                raise ops.Y4Error(f'ModelEMA.update: {k} is not dense')
            e2 = dense_like(e.to(s.device), s)                 # the model moved or changed layout since the clone
            if e2 is not e:
                self.ema[k] = e = e2
            n = s.numel()
            key.append((e.data_ptr(), s.data_ptr(), n))
            for o in range(0, n, CHUNK):
                rows.append((e.data_ptr() + 4 * o, s.data_ptr() + 4 * o, 0, 0, min(CHUNK, n - o), 0))
            dev = s.device
        if ints[0]:
            torch._foreach_copy_(ints[0], ints[1])             # copy_ of every integer entry, batched
        if not rows:
            return
        key = tuple(key)
        if key != self._table_key:
            self._table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
            self._table_key = key
        if guard is not None and (guard.dtype != torch.float64 or guard.numel() != 4 or guard.device != dev):
            raise ops.Y4Error('ModelEMA.update: guard must be the optimizer\'s record (4 doubles on the model\'s device)')
        check(lib().y4_ema_multi_f32(ops._ptr(self._table), len(rows), float(one_minus_decay), ops._ptr(guard),
                                     ops._stream()), 'ema_multi')

    def state_dict(self):
        """The model's key names with contiguous (OIHW) tensors, as checkpoints hold them, plus 'updates'."""
        sd = OrderedDict((k, v.detach().clone(memory_format=torch.contiguous_format)) for k, v in self.ema.items())
        sd['updates'] = self.updates
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        self.updates = int(sd.pop('updates'))
        if set(sd) != set(self.ema):
            missing, extra = sorted(set(self.ema) - set(sd)), sorted(set(sd) - set(self.ema))
            raise KeyError(f'ModelEMA.load_state_dict: missing {missing[:3]}, unexpected {extra[:3]}')
        for k, e in self.ema.items():
            e.copy_(sd[k])                                     # keeps e's own memory layout

    @torch.no_grad()
    def swap(self, model):
        """Exchanges live and averaged values in place; twice restores the model bit for bit.  (The inference filter
        cache revalidates on the device, so plain copies are safe.)"""
        for _, e, s in self._pairs(model):
            tmp = s.clone(memory_format=torch.preserve_format)
            s.copy_(e)
            e.copy_(tmp)

    @contextlib.contextmanager
    def applied_to(self, model):
        """with ema.applied_to(model): validate(...)  -- the model carries the averaged weights inside the block."""
        self.swap(model)
        try:
            yield model
        finally:
            self.swap(model)
