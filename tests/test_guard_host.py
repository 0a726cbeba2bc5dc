# -*- coding: utf-8 -*-
"""Host side of grad-norm clipping / non-finite step skip / ModelEMA, without a GPU: the C ABI of the five new entry
points (header == ctypes prototypes, argument errors reported before any launch), the optimizer factory's two cfg keys,
the EMA decay ramp and ModelEMA's checkpoint format."""
import math
import os
import re

import pytest
import torch

import recipe
import yolov4_amd
from yolov4_amd import _lib
from yolov4_amd.yolo.model.yolov4 import YOLOv4
from yolov4_amd.yolo.optim.optimizers.build import FusedAdam, FusedSGD, build_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('y4_grad_sumsq_multi_f32', 'y4_grad_guard_f32', 'y4_adam_multi_step_guarded_f32',
       'y4_sgd_multi_step_guarded_f32', 'y4_ema_multi_f32')
ERR_SHAPE, ERR_NULL = 1, 2
FAKE = 0x1000            # non-NULL, 8-byte aligned, never dereferenced on the host
ODD = 0x1004             # not 8-byte aligned

OPT_CFG = {'TYPE': 'ADAM', 'LR': '3e-4', 'NO_BIAS': True, 'NO_NORM': True}


def test_header_and_prototypes_agree_for_the_new_symbols():
    txt = open(os.path.join(ROOT, 'include', 'yolov4_amd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    L = yolov4_amd.lib()
    ctype = {'void*': _lib.P, 'float*': _lib.P, 'double*': _lib.P, 'int': _lib.I, 'float': _lib.F, 'double': _lib.c_double}
    for name in NEW:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, f'{name} is not declared in include/yolov4_amd.h'
        args = [re.sub(r'\bconst\b', '', a).split() for a in m.group(1).split(',')]
        types = [ctype[''.join(a[:-1])] for a in args]                  # the last word is the argument's name
        assert name in _lib.PROTOTYPES, name
        assert _lib.PROTOTYPES[name] == (_lib.I, types), name
        assert hasattr(L, name), f'{name} not exported by the library'


def test_argument_errors_are_reported_before_any_launch():
    L = yolov4_amd.lib()
    hyper = _lib.float_array([1e-3, 1.0, 0.0, 0.0])
    # y4_grad_sumsq_multi_f32(chunks, nchunks, grad_scale, partials, stream)
    assert L.y4_grad_sumsq_multi_f32(None, 4, 1.0, FAKE, None) == ERR_NULL
    assert L.y4_grad_sumsq_multi_f32(FAKE, 4, 1.0, None, None) == ERR_NULL
    assert L.y4_grad_sumsq_multi_f32(FAKE, 0, 1.0, FAKE, None) == ERR_SHAPE
    assert L.y4_grad_sumsq_multi_f32(ODD, 4, 1.0, FAKE, None) == ERR_SHAPE
    # y4_grad_guard_f32(partials, nchunks, max_norm, guard, stream)
    assert L.y4_grad_guard_f32(None, 4, 1.0, FAKE, None) == ERR_NULL
    assert L.y4_grad_guard_f32(FAKE, 4, 1.0, None, None) == ERR_NULL
    assert L.y4_grad_guard_f32(FAKE, 0, 1.0, FAKE, None) == ERR_SHAPE
    assert L.y4_grad_guard_f32(FAKE, -3, 1.0, FAKE, None) == ERR_SHAPE
    assert L.y4_grad_guard_f32(ODD, 4, 1.0, FAKE, None) == ERR_SHAPE
    assert L.y4_grad_guard_f32(FAKE, 4, 1.0, ODD, None) == ERR_SHAPE
    # guarded steps: the unguarded argument checks plus a required guard record
    adam = lambda ck, n, h, nh, g: L.y4_adam_multi_step_guarded_f32(ck, n, h, nh, 0.9, 0.999, 1e-8, 1.0, g, None)  # noqa: E731
    sgd = lambda ck, n, h, nh, g: L.y4_sgd_multi_step_guarded_f32(ck, n, h, nh, 1.0, g, None)                      # noqa: E731
    for step in (adam, sgd):
        assert step(None, 4, hyper, 1, FAKE) == ERR_NULL
        assert step(FAKE, 4, None, 1, FAKE) == ERR_NULL
        assert step(FAKE, 4, hyper, 1, None) == ERR_NULL
        assert step(FAKE, 0, hyper, 1, FAKE) == ERR_SHAPE
        assert step(FAKE, 4, hyper, 0, FAKE) == ERR_SHAPE
        assert step(FAKE, 4, hyper, 17, FAKE) == ERR_SHAPE
        assert step(ODD, 4, hyper, 1, FAKE) == ERR_SHAPE
    # y4_ema_multi_f32(chunks, nchunks, one_minus_decay, guard /* nullable */, stream)
    assert L.y4_ema_multi_f32(None, 4, 0.5, None, None) == ERR_NULL
    assert L.y4_ema_multi_f32(FAKE, 0, 0.5, None, None) == ERR_SHAPE
    assert L.y4_ema_multi_f32(ODD, 4, 0.5, None, None) == ERR_SHAPE
    assert L.y4_ema_multi_f32(FAKE, 4, 1.5, None, None) == ERR_SHAPE
    assert L.y4_ema_multi_f32(FAKE, 4, -0.25, FAKE, None) == ERR_SHAPE
    assert L.y4_ema_multi_f32(FAKE, 4, float('nan'), None, None) == ERR_SHAPE


@pytest.fixture(scope='module')
def model():
    return YOLOv4(recipe.MODEL_CFG)


def test_build_optimizer_reads_the_two_cfg_keys(model):
    cfg = dict(recipe.FULL_CFG, OPTIMIZER=dict(OPT_CFG))
    opt = build_optimizer(cfg, model)
    assert isinstance(opt, FusedAdam)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.guarded and opt.guard is None
    opt = build_optimizer(dict(cfg, OPTIMIZER=dict(OPT_CFG, CLIP_GRAD_NORM='10.0', SKIP_NONFINITE=True)), model)
    assert opt.max_grad_norm == 10.0 and opt.skip_nonfinite is True and opt.guarded
    assert opt.guard is None                                             # allocated by the first guarded step only
    with pytest.raises(yolov4_amd.Y4Error):
        opt.guard_state()
    opt = build_optimizer(dict(cfg, OPTIMIZER=dict(OPT_CFG, SKIP_NONFINITE=True)), model)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is True and opt.guarded
    sgd_cfg = dict(OPT_CFG, TYPE='SGD', MOMENTUM=0.9, DECAY=1e-5)
    opt = build_optimizer(dict(cfg, OPTIMIZER=sgd_cfg), model)
    assert isinstance(opt, FusedSGD) and not opt.guarded
    opt = build_optimizer(dict(cfg, OPTIMIZER=dict(sgd_cfg, CLIP_GRAD_NORM=2.5)), model)
    assert isinstance(opt, FusedSGD) and opt.max_grad_norm == 2.5 and opt.skip_nonfinite is False and opt.guarded
    with pytest.raises(ValueError):
        FusedAdam(model.parameters(), max_grad_norm=0.0)
    # trailing keywords: no existing positional argument moved
    assert FusedAdam(model.parameters(), 1e-3, (0.9, 0.99), 1e-6, 0.01).defaults == \
        dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.01)
    assert FusedSGD(model.parameters(), 0.1, 0.8, 1e-4).defaults == dict(lr=0.1, momentum=0.8, weight_decay=1e-4)


def test_ema_decay_ramp(model):
    from yolov4_amd.yolo.util.ema import ModelEMA
    ema = ModelEMA(model, decay=0.9999, tau=2000.0)
    for n in (1, 2000, 10 ** 6):
        assert ema.decay_at(n) == pytest.approx(0.9999 * (1.0 - math.exp(-n / 2000.0)), rel=1e-15)
    assert ema.decay_at(1) < 6e-4 and abs(ema.decay_at(2000) - 0.9999 * (1 - math.exp(-1))) < 1e-15
    assert ema.decay_at(10 ** 6) == 0.9999                                # exp(-500) is 0 in the sum
    ema = ModelEMA(model, decay=0.5, tau=10.0)
    assert ema.decay_at(10) == pytest.approx(0.5 * (1.0 - math.exp(-1.0)), rel=1e-15)
    with pytest.raises(yolov4_amd.Y4Error):                              # the update is a HIP launch: no CPU fallback
        ema.update(model)


def test_ema_state_dict_round_trip(model):
    from yolov4_amd.yolo.util.ema import ModelEMA
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 11)
    model.load_state_dict(sd)
    ema = ModelEMA(model)
    w_live = model.backbone.stage1.base.conv.weight
    w = ema.ema['backbone.stage1.base.conv.weight']
    assert w.data_ptr() != w_live.data_ptr() and w.stride() == w_live.stride()     # a clone in the entry's own (KRSC) layout
    assert w.is_contiguous(memory_format=torch.channels_last)
    ema.updates = 37
    wire = ema.state_dict()
    assert len(wire) == 649 and list(wire)[:-1] == list(model.state_dict()) and wire['updates'] == 37
    for k, v in model.state_dict().items():
        assert wire[k].is_contiguous() and wire[k].dtype == v.dtype and torch.equal(wire[k], v), k
    # into an average built from another model: values and `updates` arrive, the KRSC memory stays
    other = ModelEMA(YOLOv4(recipe.MODEL_CFG))
    assert not torch.equal(other.ema['backbone.stage1.base.conv.weight'], w)
    other.load_state_dict(wire)
    assert other.updates == 37
    for k, v in ema.ema.items():
        assert torch.equal(other.ema[k], v) and other.ema[k].stride() == v.stride(), k
    with pytest.raises(KeyError):
        other.load_state_dict({k: v for k, v in wire.items() if not k.endswith('running_var')})
