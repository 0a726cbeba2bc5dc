# -*- coding: utf-8 -*-
"""CPU-side checks of YOLOv4-tiny: the references of tests/tiny_cases.py against torch's own operators, every case reaching
the branch it is listed for, the module tree / state_dict / Darknet order of YOLOv4Tiny, the model dispatch, the head
classes' three-layer behaviour, and Darknet weights I/O.  No GPU."""
import argparse
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipe
import tiny_cases as TC
from yolov4_amd._lib import Y4Error
from yolov4_amd.yolo.model.build import build_criterion, build_model
from yolov4_amd.yolo.model.yololayer import YOLOLayer
from yolov4_amd.yolo.model.yololoss import YOLOLoss
from yolov4_amd.yolo.model.yolov4_tiny import DARKNET_ORDER, YOLOv4Tiny, default_cfg
from yolov4_amd.yolo.util.darknet_weights import load_darknet_weights, save_darknet_weights


# ------------------------------------------------------------------------------------------ pool reference
def _same(a, b):
    """bit-equal, NaNs matching NaNs (payloads are compared on the GPU against the reference itself)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(TC.bits(a)[~nan], TC.bits(b)[~nan])


@pytest.mark.parametrize('case', TC.POOL_CASES, ids=lambda c: c[0])
def test_pool_reference_is_torch_max_pool2d(case):
    name, B, H, W, C = case[:5]
    x, dy = TC.pool_input(case)
    y, code = TC.pool_ref(x)
    dx = TC.pool_bwd_ref(dy, code, H, W)
    assert y.shape == (B, H // 2, W // 2, C) and code.dtype == np.int8 and dx.shape == x.shape
    if H < 2 or W < 2:
        assert y.size == 0 and not dx.any() and not np.signbit(dx).any()
        return
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt, it = F.max_pool2d(xt, 2, 2, return_indices=True)
    yt.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    ih, iw = (it // W).numpy(), (it % W).numpy()
    ho, wo = np.arange(H // 2).reshape(1, 1, -1, 1), np.arange(W // 2).reshape(1, 1, 1, -1)
    tcode = ((ih - 2 * ho) * 2 + (iw - 2 * wo)).transpose(0, 2, 3, 1)
    assert _same(y, yt.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(code, tcode)
    assert _same(dx, xt.grad.permute(0, 2, 3, 1).numpy())
    if H % 2:
        assert not dx[:, H - 1].any()
    if W % 2:
        assert not dx[:, :, W - 1].any()


def test_pool_special_windows_reach_their_branches():
    case = [c for c in TC.POOL_CASES if c[0] == 'specials'][0]
    x, _ = TC.pool_input(case)
    y, code = TC.pool_ref(x)
    assert code[0, 0, :, 0].tolist() == [0, 0, 3, 2] and code[0, 1, :, 0].tolist() == [0, 1, 0, 2]
    assert TC.bits(y[0, 0, :, 0]).tolist()[1:] == [TC.NAN_A, TC.NAN_A, TC.NAN_B]        # the LAST NaN's payload
    assert y[0, 1, 0, 0] == -np.inf and y[0, 1, 1, 0] == np.inf and np.signbit(y[0, 1, 2, 0])
    assert {c[4] // 4 for c in TC.POOL_CASES} >= {1, 3, 5, 16}
    assert TC.laps(65 * 65 * 128) >= 2 and TC.laps(64 * 26 * 26 * 128) >= 2              # the grid-stride case; tiny's own maps too
    assert all(c[5] % 4 == 0 and c[7] % 4 == 0 and c[6] % 4 == 0 and c[8] % 4 == 0 for c in TC.POOL_CASES)


# ------------------------------------------------------------------------------------------ stem references
@pytest.mark.parametrize('case', TC.STEM_CASES + [TC.STEM_WGRAD_MULTI_SLAB], ids=str)
def test_stem_references_against_torch_fp32(case):
    c = TC.stem_input(case)
    x, w = torch.from_numpy(c['x']), torch.from_numpy(c['w']).requires_grad_(True)
    y32 = F.conv2d(x, w, stride=2, padding=1)
    y64, bound = TC.stem_fwd64(c['x'], c['w'])
    assert y64.shape == c['dy'].shape
    assert (np.abs(y32.detach().permute(0, 2, 3, 1).numpy() - y64) <= bound).all()
    z64, zb = TC.stem_fwd64(c['x'], c['w'], c['scale'], c['shift'], 1)
    z32 = F.leaky_relu(y32.detach() * x.new_tensor(c['scale']).view(1, -1, 1, 1) + x.new_tensor(c['shift']).view(1, -1, 1, 1), 0.1)
    assert (np.abs(z32.permute(0, 2, 3, 1).numpy() - z64) <= zb).all()
    (y32 * torch.from_numpy(c['dy']).permute(0, 3, 1, 2)).sum().backward()
    dw64, S = TC.stem_wgrad64(c['x'], c['dy'])
    plan = TC.wgrad_plan(*case)
    assert (np.abs(w.grad.numpy() - dw64) <= (plan['M'] + 1) * TC.U * S + TC.TINY).all()
    assert 1 <= plan['L'] <= plan['M'] and plan['blocks'] * plan['T'] >= plan['M'] and plan['P'] * (case[3] // 4) <= 256


def test_wgrad_plan_cases_reach_their_branches():
    assert TC.wgrad_plan(*TC.STEM_WGRAD_MULTI_SLAB)['blocks'] > 1
    assert all(TC.wgrad_plan(*c)['blocks'] == 1 for c in TC.STEM_CASES)
    full = TC.wgrad_plan(64, 416, 416, 32)                  # the training shape: the block cap, 3.5 MB of slabs
    assert full['blocks'] == 1024 and full['P'] == 32 and full['L'] == -(-full['T'] // 32) + 31
    assert {c[3] for c in TC.STEM_CASES} == {4, 32, 64} and {c[0] for c in TC.STEM_CASES} == {1, 3}
    assert np.array_equal(TC.krsc(np.arange(54).reshape(2, 3, 3, 3))[1, 2, 1], [27 + 7, 36 + 7, 45 + 7])


# ------------------------------------------------------------------------------------------ the model, host side
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(3)
    return YOLOv4Tiny(default_cfg())


def test_tree_parameter_count_and_darknet_order(model):
    assert sum(p.numel() for p in model.parameters()) == TC.N_PARAMS_80 == 6056606
    assert list(model.state_dict().keys()) == TC.expected_keys()
    convs = model.darknet_convs()
    assert len(convs) == 21 and len(set(map(id, convs))) == 21
    assert model.darknet_layers() == DARKNET_ORDER == TC.DARKNET_ORDER
    names = {id(m): n for n, m in model.named_modules()}
    by_layer = dict(zip(DARKNET_ORDER, (names[id(m)] for m in convs)))
    assert by_layer[0] == 'backbone.conv1' and by_layer[7] == 'backbone.block1.conv4' and by_layer[20] == 'backbone.block3.conv2'
    assert by_layer[26] == 'backbone.conv3' and by_layer[27] == 'neck.conv1' and by_layer[29] == 'head.yolo2.1'
    assert by_layer[32] == 'neck.conv2' and by_layer[36] == 'head.yolo1.1'
    assert [m.has_bn for m in convs].count(False) == 2 and all(m.act_name == 'leaky_relu' for m in convs if m.has_bn)
    assert model.head.yolo1[2].stride == 16 and model.head.yolo2[2].stride == 32
    assert model.head.yolo1[2].anchor_mask == [1, 2, 3] and model.head.yolo2[2].anchor_mask == [3, 4, 5]
    assert 3 * (416 // 16) ** 2 + 3 * (416 // 32) ** 2 == 2535


def test_default_cfg_and_dispatch(model):
    cfg = {'MODEL': default_cfg(3)}
    m = build_model(argparse.Namespace(), cfg)
    assert isinstance(m, YOLOv4Tiny) and m.head.yolo1[1].conv.out_channels == 24
    assert type(build_model(argparse.Namespace(), {'MODEL': dict(recipe.MODEL_CFG)})).__name__ == 'YOLOv4'
    with pytest.raises(ValueError):
        build_model(argparse.Namespace(), {'MODEL': dict(default_cfg(), TYPE='YOLOv5')})
    with pytest.raises(ValueError):
        YOLOv4Tiny(dict(recipe.MODEL_CFG))
    for shape in ((1, 3, 48, 64), (1, 3, 64, 80)):
        with pytest.raises(ValueError):
            model(torch.zeros(shape))
    crit = build_criterion(TC.full_cfg())
    assert len(crit.last) == 2 and crit.scale_xy == [1.0, 1.0] and crit._layer_cfg(1)['stride'] == 32
    assert crit._layer_cfg(0)['anch_mask'] == [1, 2, 3] and len(crit._layer_cfg(0)['all_anchors']) == 6


def test_three_layer_heads_behave_as_before():
    cfg = dict(recipe.MODEL_CFG)
    assert [YOLOLayer(cfg, l).stride for l in range(3)] == [8, 16, 32] == YOLOLayer.strides == YOLOLoss.strides
    crit = YOLOLoss(cfg)
    assert crit.last == [None, None, None] and crit.scale_xy == [1.0, 1.0, 1.0] and crit._layer_cfg(2)['stride'] == 32
    bad = dict(cfg, SCALE_X_Y=[1.1, 1.2])
    for make in (lambda: YOLOLayer(bad, 0), lambda: YOLOLoss(bad, box_loss='ciou')):
        with pytest.raises(ValueError) as e:
            make()
        assert str(e.value) == 'SCALE_X_Y must be one number or one per layer (3), got [1.1, 1.2]'
    two = dict(default_cfg(), SCALE_X_Y=[1.05, 1.05])
    assert YOLOLayer(two, 1).scale_xy == pytest.approx(1.05) and YOLOLoss(two, box_loss='ciou').scale_xy == pytest.approx([1.05, 1.05])
    with pytest.raises(ValueError):
        YOLOLayer(dict(default_cfg(), SCALE_X_Y=[1.05, 1.05, 1.05]), 0)


# ------------------------------------------------------------------------------------------ Darknet weights
def _filled(seed):
    m = YOLOv4Tiny(default_cfg())
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, seed)
    for k in sd:                                  # running statistics that are not the defaults
        if k.endswith('running_mean'):
            sd[k].copy_(recipe.randn(sd[k].shape, 7))
        elif k.endswith('running_var'):
            sd[k].copy_(recipe.rand(sd[k].shape, 8) + 0.5)
    m.load_state_dict(sd)
    return m


def _equal(a, b, keys=None):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in (keys or sa) if not k.endswith('num_batches_tracked'))


def test_darknet_weights_round_trip_sizes_cutoff_and_errors(tmp_path):
    a, b = _filled(11), _filled(12)
    full, part = str(tmp_path / 'tiny.weights'), str(tmp_path / 'tiny.conv.29')
    assert save_darknet_weights(a, full) == 21 and os.path.getsize(full) == 24251276
    assert save_darknet_weights(a, part, cutoff=29) == 17 and os.path.getsize(part) == 19789716
    with open(full, 'rb') as f:
        assert struct.unpack('<iiiQ', f.read(20)) == (0, 2, 5, 0)
    assert not _equal(a, b)
    assert load_darknet_weights(b, full) == 21 and _equal(a, b)
    assert b.backbone.conv1.conv.weight.is_contiguous(memory_format=torch.channels_last)
    c = _filled(12)
    before = {k: v.clone() for k, v in c.state_dict().items()}
    assert load_darknet_weights(c, part) == 17
    first17 = [n for n, m in c.named_modules() if any(m is d for d in c.darknet_convs()[:17])]
    last4 = [n for n, m in c.named_modules() if any(m is d for d in c.darknet_convs()[17:])]
    assert sorted(last4) == ['head.yolo1.0', 'head.yolo1.1', 'head.yolo2.1', 'neck.conv2']
    for k, v in c.state_dict().items():
        mine = k.rsplit('.', 2)[0]
        if k.endswith('num_batches_tracked'):
            continue
        assert torch.equal(v, a.state_dict()[k] if mine in first17 else before[k]), k
    raw = open(full, 'rb').read()
    for name, data in (('short', raw[:-4]), ('long', raw + b'\0\0\0\0'), ('header', raw[:10])):
        p = str(tmp_path / name)
        open(p, 'wb').write(data)
        d = _filled(12)
        with pytest.raises(Y4Error):
            load_darknet_weights(d, p)
        assert _equal(d, _filled(12))                    # a refused file writes nothing


def test_darknet_weights_old_header_with_4_byte_seen(tmp_path):
    m = _filled(5)
    conv = m.darknet_convs()[0]                          # 3 -> 32, 3x3, BatchNorm
    rng = np.random.RandomState(0)
    beta, gamma, mean, var = (rng.standard_normal(32).astype('<f4') for _ in range(4))
    w = rng.standard_normal((32, 3, 3, 3)).astype('<f4')
    p = str(tmp_path / 'one.weights')
    with open(p, 'wb') as f:
        f.write(struct.pack('<iiiI', 0, 1, 0, 12345))    # major * 10 + minor = 1 < 2: `seen` is 32 bits
        for a in (beta, gamma, mean, var, w):
            f.write(a.tobytes())
    assert load_darknet_weights(m, p) == 1
    assert np.array_equal(conv.norm.bias.detach().numpy(), beta) and np.array_equal(conv.norm.weight.detach().numpy(), gamma)
    assert np.array_equal(conv.norm.running_mean.numpy(), mean) and np.array_equal(conv.norm.running_var.numpy(), var)
    assert np.array_equal(conv.conv.weight.detach().numpy(), w)
    with pytest.raises(Y4Error):
        load_darknet_weights(torch.nn.Linear(2, 2), p)


# ------------------------------------------------------------------------------------------ the model cases' inputs
@pytest.mark.parametrize('case', TC.MODEL_CASES, ids=str)
def test_model_inputs_are_the_first_well_conditioned_ones(case):
    """The image of a model case is the first seed from 500 + S upwards on which the fp64 oracle has no pool tie and no
    LeakyReLU kink within COND_K x the fp32 oracle's local error (tiny_cases.MODEL_INPUT_SEEDS): it qualifies, the seeds
    before it do not."""
    B, S = case
    sd = YOLOv4Tiny(default_cfg()).state_dict()
    recipe.fill_state_dict_(sd, TC.MODEL_SEED)
    chosen = TC.MODEL_INPUT_SEEDS[S]
    assert chosen >= 500 + S
    pool, act = TC.conditioning(sd, TC.model_input(case)[0])
    print('%s seed %d: pool gap / error %.2f, |pre-activation| / error %.2f' % (case, chosen, pool, act))
    assert pool >= TC.COND_K and act >= TC.COND_K
    for seed in range(500 + S, chosen):
        pool, act = TC.conditioning(sd, TC.model_input(case, seed)[0])
        print('%s seed %d: pool gap / error %.2f, |pre-activation| / error %.2f' % (case, seed, pool, act))
        assert min(pool, act) < TC.COND_K, seed


# ------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize('case', TC.MODEL_CASES, ids=str)
def test_tiny_oracle_fp32_agrees_with_fp64(case):
    from oracle import head as H
    B, S = case
    m = YOLOv4Tiny(default_cfg())
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, TC.MODEL_SEED)
    x, labels = TC.model_input(case)
    o32, o64 = (TC.tiny_oracle(sd, x, dt, True, labels) for dt in (torch.float32, torch.float64))
    assert H.STRIDES == (8, 16, 32)                      # the patch is undone
    assert [t.shape for t in o64['logits']] == [(B, 255, S // 16, S // 16), (B, 255, S // 32, S // 32)]
    for a, b in zip(o32['logits'], o64['logits']):
        assert np.abs(a - b).max() <= 1e-4 * max(1.0, np.abs(b).max())
    assert abs(o32['loss'] - o64['loss']) <= 1e-4 * abs(o64['loss']) and o64['loss'] > 0
    assert sorted(o64['grads']) == sorted(k for k in sd if not ('running_' in k or k.endswith('num_batches_tracked')))
    for k, g in o64['grads'].items():
        assert np.abs(o32['grads'][k] - g).max() <= 1e-3 * np.abs(g).max(), k
        assert np.abs(g).max() > 0, k
    e32, e64 = (TC.tiny_oracle(sd, x, dt, False) for dt in (torch.float32, torch.float64))
    assert e64.shape == (B, 3 * (S // 16) ** 2 + 3 * (S // 32) ** 2, 85)
    assert np.abs(e32.astype(np.float64) - e64).max() <= 1e-4 * max(1.0, np.abs(e64).max())
