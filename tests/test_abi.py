# -*- coding: utf-8 -*-
"""CPU-side checks of the C-ABI boundary and the host mirror of the reference
interface: the library loads without a GPU, exports every symbol the header
declares, and the Python classes keep the reference's constructor signatures,
attribute tree and state_dict -- and fail loudly instead of falling back."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import recipe
import yolov4_amd
from yolov4_amd import _lib, ops
from yolov4_amd.darknet.darknet import ConvBNAct, CSPDownSample, CSPDownSample0, ResBlock
from yolov4_amd.yolo.model.build import build_criterion, build_model
from yolov4_amd.yolo.model.yololayer import YOLOLayer
from yolov4_amd.yolo.model.yololoss import YOLOLoss
from yolov4_amd.yolo.model.yolov4 import YOLOv4
from yolov4_amd.yolo.util import utils
from oracle import network as NW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, 'include', 'yolov4_amd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(y4_\w+)\s*\(', txt)))


def test_library_loads_and_exports_every_declared_symbol():
    L = yolov4_amd.lib()
    syms = header_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(L, s), f'{s} declared in include/yolov4_amd.h but not exported'
    assert sorted(_lib.PROTOTYPES) == syms, 'ctypes prototypes and header disagree'
    assert L.y4_version() >= 100
    assert L.y4_strerror(0) == b'ok' and b'shape' in L.y4_strerror(1)
    assert L.y4_device_count() >= 0
    assert L.y4_get_conv_mode() in (0, 1, 2, 3) and L.y4_set_conv_mode(7) == 1


def test_workspace_queries_run_on_host():
    L = yolov4_amd.lib()
    assert L.y4_conv2d_dgrad_workspace(128, 255, 3) == 128 * 9 * 256 * 6 + 64 + 4096
    assert L.y4_conv2d_fwd_workspace(128, 255, 3) == 64 + 4096 + 255 * 9 * 128 * 6
    assert L.y4_bn_workspace(1000, 64) >= 2 * 64 * 8
    assert L.y4_conv2d_wgrad_workspace(64, 76, 76, 128, 128, 3, 1) > 0
    assert L.y4_yolo_loss_workspace(4, 76, 3, 60, 80) > 4 * 3 * 76 * 76 * 4
    assert L.y4_post_nms_workspace(1000, 160) >= 1000 * (8 + 16 + 4 + 4)


def test_plane_window_query_runs_on_host():
    """y4_conv_planes_fit: the DMA kernels' 32-bit buffer windows, asked by the host before a producer writes planes."""
    L = yolov4_amd.lib()
    was = L.y4_get_conv_mode()
    try:
        L.y4_set_conv_mode(3)
        assert L.y4_conv_planes_fit(64, 76, 76, 128, 128, 3, 1, 1) == 1
        assert L.y4_conv_planes_fit(64, 152, 152, 128, 256, 3, 2, 1) == 1
        assert L.y4_conv_planes_fit(64, 76, 76, 100, 128, 3, 1, 1) == 0            # not whole K tiles
        assert L.y4_conv_planes_fit(64, 75, 76, 128, 256, 3, 2, 1) == 0            # stride 2 on an odd grid
        assert L.y4_conv_planes_fit(1, 4096, 4096, 64, 128, 3, 1, 1) == 0          # one image = 4 GiB: beyond a forward window
        assert L.y4_conv_planes_fit(1, 1024, 1024, 64, 128, 3, 1, 1) == 1
        # stride 2: the plane dgrad scatters into ONE window over the whole dx tensor (6 GiB here); forward and wgrad fit
        assert L.y4_conv_planes_fit(512, 152, 152, 128, 256, 3, 2, 1) == 0
        assert L.y4_conv_planes_fit(512, 152, 152, 128, 256, 3, 2, 0) == 1
        L.y4_set_conv_mode(0)
        assert L.y4_conv_planes_fit(64, 76, 76, 128, 128, 3, 1, 1) == 0            # no plane kernels in this mode
    finally:
        L.y4_set_conv_mode(was)


def test_null_and_shape_errors_are_reported_before_any_launch():
    L = yolov4_amd.lib()
    assert L.y4_conv2d_fwd_f32(None, 32, None, None, 32, 1, 8, 8, 32, 32, 3, 1, None, None, 0, None, 0, None, None, None, 0, None) == 2
    # Cin not a multiple of 32 -> shape error (pointers are fake but never dereferenced on the host)
    fake = 0x1000
    assert L.y4_conv2d_fwd_f32(fake, 48, fake, fake, 32, 1, 8, 8, 48, 32, 3, 1, None, None, 0, None, 0, None, None, fake, 1 << 30, None) == 1
    assert L.y4_conv2d_fwd_f32(fake, 32, fake, fake, 32, 1, 8, 8, 32, 32, 5, 1, None, None, 0, None, 0, None, None, fake, 1 << 30, None) == 1


# the status codes as include/yolov4_amd.h defines them: Y4_OK 0, Y4_ERR_SHAPE 1, Y4_ERR_NULL 2, Y4_ERR_WORKSPACE 4
# (_lib.py names only the JPEG codes ERR_FORMAT / ERR_UNSUPPORTED)
OK, SHAPE, NULL, WORKSPACE = 0, 1, 2, 4
ALL_MODES = (0, 1, 2, 3)


def _conv_entry_early_returns(L):
    """(entry, conv modes, arguments, expected status): calls of the conv entries (csrc/conv_api.hip, conv_stem.hip) that must
    return before anything is launched, behind fake device pointers.  Defaults are a valid call; each case names what it changes."""
    F, MIS = 0x1000, 0x1004
    conv = dict(B=2, H=8, W=8, Cin=64, Cout=64, k=3, s=1)

    def args(order, base, kw):
        d = dict(base, **kw)
        assert set(kw) <= set(base), kw
        return [d[n] for n in order.split()]

    fwd_o = 'x ldx w y ldy B H W Cin Cout k s scale shift act res ldr x_amax y_amax ws ws_bytes stream'
    fwd_b = dict(conv, x=F, ldx=64, w=F, y=F, ldy=64, scale=None, shift=None, act=0, res=None, ldr=0, x_amax=None, y_amax=None,
                 ws=F, ws_bytes=1 << 30, stream=None)
    bn_o = 'x ldx w y ldy B H W Cin Cout k s partials partial_bytes nparts x_amax ws ws_bytes dgf dgf_bytes stream'
    bn_b = dict(conv, x=F, ldx=64, w=F, y=F, ldy=64, partials=F, partial_bytes=1 << 30, nparts=F, x_amax=None, ws=F,
                ws_bytes=1 << 30, dgf=None, dgf_bytes=0, stream=None)
    pf_o = 'x ldx wp y ldy B H W Cin Cout k s scale shift act res ldr x_amax y_amax stream'
    pf_b = dict(conv, x=F, ldx=64, wp=F, y=F, ldy=64, scale=None, shift=None, act=0, res=None, ldr=0, x_amax=None, y_amax=None,
                stream=None)
    pr_o = 'w Cout K prepared nbytes stream'
    pr_b = dict(w=F, Cout=64, K=576, prepared=F, nbytes=1 << 30, stream=None)
    dg_o = 'dy lddy w dx lddx B H W Cin Cout k s ws ws_bytes dy_amax res ldr stream'
    dg_b = dict(conv, dy=F, lddy=64, w=F, dx=F, lddx=64, ws=F, ws_bytes=1 << 30, dy_amax=None, res=None, ldr=0, stream=None)
    wg_o = 'x ldx dy lddy dw B H W Cin Cout k s ws ws_bytes x_amax dy_amax stream'
    wg_b = dict(conv, B=4, H=38, W=38, x=F, ldx=64, dy=F, lddy=64, dw=F, ws=F, ws_bytes=1 << 30, x_amax=None, dy_amax=None,
                stream=None)                                  # a split-K shape: the slabs go through the workspace in every mode
    sf_o = 'x sxb sxc sxh sxw w y ldy B H W Cout scale shift act stats stream'
    sf_b = dict(x=F, sxb=3 * 64 * 64, sxc=64 * 64, sxh=64, sxw=1, w=F, y=F, ldy=32, B=2, H=64, W=64, Cout=32, scale=None,
                shift=None, act=0, stats=None, stream=None)
    sw_o = 'x sxb sxc sxh sxw dy lddy dw B H W Cout ws ws_bytes stream'
    sw_b = dict(x=F, sxb=3 * 64 * 64, sxc=64 * 64, sxh=64, sxw=1, dy=F, lddy=32, dw=F, B=2, H=64, W=64, Cout=32, ws=F,
                ws_bytes=1 << 30, stream=None)
    am_o = 'x ldx M C out stream'
    am_b = dict(x=F, ldx=64, M=100, C=64, out=F, stream=None)
    mg_o = 'dst src stream'
    mg_b = dict(dst=F, src=F, stream=None)

    fwd_ws = L.y4_conv2d_fwd_workspace(64, 64, 3)
    dg_ws = L.y4_conv2d_dgrad_workspace(64, 64, 3)
    bn_ws = L.y4_conv2d_bnstats_workspace(2, 8, 8, 64, 64, 3, 1)
    pr_ws = L.y4_conv2d_prepared_bytes(64, 576)
    wg_ws = L.y4_conv2d_wgrad_workspace(4, 38, 38, 64, 64, 3, 1)
    sw_ws = L.y4_conv2d_stem_wgrad_workspace(2, 64, 64, 32)
    assert wg_ws > 64 and bn_ws > 0

    split = (1, 2, 3)                                           # the modes whose forward takes a workspace
    cases = []

    def add(entry, order, base, rows):
        for modes, kw, want in rows:
            cases.append((entry, modes, args(order, base, kw), want, kw))

    add('y4_conv2d_fwd_f32', fwd_o, fwd_b, [
        (ALL_MODES, dict(x=None, k=5), NULL), (ALL_MODES, dict(w=None, B=0), NULL),
        (ALL_MODES, dict(y=None, Cin=48), NULL),
        (ALL_MODES, dict(k=5, ws_bytes=0), SHAPE), (ALL_MODES, dict(s=3, ws_bytes=0), SHAPE), (ALL_MODES, dict(Cin=48, ldx=48), SHAPE),
        (ALL_MODES, dict(Cin=32, ldx=31), SHAPE), (ALL_MODES, dict(ldy=63), SHAPE), (ALL_MODES, dict(ldx=66), SHAPE),
        (ALL_MODES, dict(x=MIS), SHAPE), (ALL_MODES, dict(res=F, ldr=63, ws_bytes=0), SHAPE),
        (ALL_MODES, dict(B=128, H=4096, W=4096, Cin=32, ldx=32, k=1, ws_bytes=0), SHAPE),        # M = 2^31
        (split, dict(ws=None), NULL), (split, dict(ws=None, ws_bytes=0), NULL),
        (split, dict(ws_bytes=fwd_ws - 1), WORKSPACE), (split, dict(ws=MIS, ws_bytes=fwd_ws - 1), WORKSPACE),
        (split, dict(ws=MIS), SHAPE)])
    add('y4_conv2d_fwd_bnstats_f32', bn_o, bn_b, [
        (ALL_MODES, dict(partials=None, k=5), NULL), (ALL_MODES, dict(nparts=None, partial_bytes=0), NULL),
        (ALL_MODES, dict(x=None, k=5), NULL),
        ((0, 1, 2), dict(dgf=F, dgf_bytes=1 << 30), SHAPE),            # a dgrad_filter outside mode 3
        ((0, 1, 2), dict(dgf=F, dgf_bytes=1 << 30, partial_bytes=0), SHAPE), ((0, 1, 2), dict(dgf=F, x=None), SHAPE),
        (ALL_MODES, dict(partial_bytes=bn_ws - 1), WORKSPACE),
        (ALL_MODES, dict(partial_bytes=bn_ws - 1, x=None), WORKSPACE),    # the partial rows are checked before the conv's operands
        (ALL_MODES, dict(k=5, partial_bytes=0, ws_bytes=0), SHAPE), (ALL_MODES, dict(Cin=48, ldx=48, partial_bytes=1 << 30), SHAPE),
        (split, dict(ws_bytes=fwd_ws - 1, partial_bytes=bn_ws), WORKSPACE), (split, dict(ws=None), NULL),
        ((3,), dict(dgf=F, dgf_bytes=dg_ws - 1), WORKSPACE), ((3,), dict(dgf=MIS, dgf_bytes=dg_ws - 1), WORKSPACE),
        ((3,), dict(dgf=MIS, dgf_bytes=dg_ws), SHAPE), ((3,), dict(dgf=F, dgf_bytes=dg_ws, ws_bytes=fwd_ws - 1), WORKSPACE)])
    add('y4_conv2d_fwd_prepared_f32', pf_o, pf_b, [
        (ALL_MODES, dict(wp=None, k=5), NULL), (ALL_MODES, dict(x=None, k=5), NULL), (ALL_MODES, dict(y=None, Cin=33), NULL),
        (ALL_MODES, dict(k=5), SHAPE), (ALL_MODES, dict(Cin=33, ldx=36), SHAPE), (ALL_MODES, dict(ldy=63), SHAPE),
        ((0, 1, 2), dict(), SHAPE),                                     # prepared filters are f16x2 planes: mode 3 only
        ((3,), dict(wp=MIS), SHAPE)])
    add('y4_conv2d_prepare_filter_f32', pr_o, pr_b, [
        (ALL_MODES, dict(w=None, K=31), NULL), (ALL_MODES, dict(prepared=None, Cout=0), NULL),
        (ALL_MODES, dict(K=31, nbytes=0), SHAPE), (ALL_MODES, dict(Cout=0, nbytes=0), SHAPE),
        (ALL_MODES, dict(nbytes=pr_ws - 1), WORKSPACE), (ALL_MODES, dict(prepared=MIS, nbytes=pr_ws - 1), WORKSPACE),
        (ALL_MODES, dict(prepared=MIS, nbytes=pr_ws), SHAPE), (ALL_MODES, dict(w=MIS), SHAPE)])
    add('y4_conv2d_dgrad_f32', dg_o, dg_b, [
        (ALL_MODES, dict(dy=None, k=5), NULL), (ALL_MODES, dict(dx=None, Cin=0), NULL), (ALL_MODES, dict(ws=None, k=5), NULL),
        ((0, 1, 2), dict(w=None), NULL), ((0, 1, 2), dict(w=None, k=5), NULL),
        ((3,), dict(w=None, k=5), SHAPE), ((3,), dict(w=None, ws_bytes=dg_ws - 1), WORKSPACE),    # w == NULL passes in mode 3
        (ALL_MODES, dict(k=5, ws_bytes=0), SHAPE), (ALL_MODES, dict(Cin=0, ws_bytes=0), SHAPE), (ALL_MODES, dict(lddy=63, ws_bytes=0), SHAPE),
        (ALL_MODES, dict(Cout=33, lddy=36), SHAPE), (ALL_MODES, dict(lddx=63), SHAPE), (ALL_MODES, dict(lddy=66), SHAPE),
        (ALL_MODES, dict(ws_bytes=dg_ws - 1), WORKSPACE), (ALL_MODES, dict(ws=MIS, ws_bytes=dg_ws - 1), WORKSPACE),
        (ALL_MODES, dict(ws=MIS, ws_bytes=dg_ws), SHAPE), (ALL_MODES, dict(dy=MIS), SHAPE)])
    add('y4_conv2d_wgrad_f32', wg_o, wg_b, [
        (ALL_MODES, dict(x=None, k=5), NULL), (ALL_MODES, dict(dy=None, Cin=0), NULL), (ALL_MODES, dict(dw=None, ws_bytes=0), NULL),
        (ALL_MODES, dict(k=5, ws_bytes=0), SHAPE), (ALL_MODES, dict(s=0, ws_bytes=0), SHAPE), (ALL_MODES, dict(Cin=30, ldx=32, ws_bytes=0), SHAPE),
        (ALL_MODES, dict(ldx=63), SHAPE), (ALL_MODES, dict(lddy=62), SHAPE), (ALL_MODES, dict(lddy=60), SHAPE), (ALL_MODES, dict(x=MIS), SHAPE),
        (ALL_MODES, dict(ws=None), NULL), (ALL_MODES, dict(ws_bytes=wg_ws - 65), WORKSPACE), (ALL_MODES, dict(ws_bytes=0), WORKSPACE),
        ((3,), dict(ws_bytes=wg_ws - 1), WORKSPACE), ((3,), dict(ws_bytes=wg_ws - 1, x_amax=F), WORKSPACE)])   # the amax words
    add('y4_conv2d_stem_fwd_f32', sf_o, sf_b, [
        (ALL_MODES, dict(x=None, Cout=33), NULL), (ALL_MODES, dict(w=None, B=0), NULL), (ALL_MODES, dict(y=None), NULL),
        (ALL_MODES, dict(Cout=33, ldy=33), SHAPE), (ALL_MODES, dict(Cout=0), SHAPE), (ALL_MODES, dict(ldy=31), SHAPE),
        (ALL_MODES, dict(B=0), SHAPE), (ALL_MODES, dict(W=-1), SHAPE),
        (ALL_MODES, dict(B=1, H=1 << 20, W=1 << 20), SHAPE)])           # 2^32 blocks
    add('y4_conv2d_stem_wgrad_f32', sw_o, sw_b, [
        (ALL_MODES, dict(ws=None, W=1), NULL), (ALL_MODES, dict(x=None, Cout=33), NULL), (ALL_MODES, dict(dw=None, ws_bytes=0), NULL),
        (ALL_MODES, dict(W=1, ws_bytes=0), SHAPE), (ALL_MODES, dict(Cout=33, ws_bytes=0), SHAPE), (ALL_MODES, dict(lddy=31, ws_bytes=0), SHAPE),
        (ALL_MODES, dict(ws_bytes=sw_ws - 1), WORKSPACE), (ALL_MODES, dict(ws_bytes=sw_ws - 1, sxw=-1), WORKSPACE),
        (ALL_MODES, dict(ws_bytes=sw_ws, sxw=-1), SHAPE), (ALL_MODES, dict(ws_bytes=sw_ws, sxb=1 << 30), SHAPE),     # 32-bit window
        (ALL_MODES, dict(ws_bytes=sw_ws, B=128, H=608, W=608, lddy=1 << 26), SHAPE)])                                   # a wave's dy rows
    add('y4_amax_f32', am_o, am_b, [
        (ALL_MODES, dict(x=None, C=0), NULL), (ALL_MODES, dict(out=None, M=-1), NULL),
        (ALL_MODES, dict(C=0), SHAPE), (ALL_MODES, dict(M=-1), SHAPE), (ALL_MODES, dict(ldx=63), SHAPE)])
    add('y4_amax_merge_u32', mg_o, mg_b, [(ALL_MODES, dict(dst=None), NULL), (ALL_MODES, dict(src=None), NULL),
                                         (ALL_MODES, dict(dst=None, src=None), NULL)])
    return cases


def test_conv_entries_report_null_then_shape_then_workspace_before_any_launch():
    """Every conv entry checks NULL operands, then shapes and pitches, then workspace sizes, in that order and before it
    launches anything; in which modes a case applies is part of the table (w == NULL for dgrad is allowed in mode 3 only, a
    dgrad_filter for the BN-statistics forward in mode 3 only, the forward takes a workspace in modes 1-3)."""
    L = yolov4_amd.lib()
    cases = _conv_entry_early_returns(L)
    assert {c[0] for c in cases} == {
        'y4_conv2d_fwd_f32', 'y4_conv2d_fwd_bnstats_f32', 'y4_conv2d_fwd_prepared_f32', 'y4_conv2d_prepare_filter_f32',
        'y4_conv2d_dgrad_f32', 'y4_conv2d_wgrad_f32', 'y4_conv2d_stem_fwd_f32', 'y4_conv2d_stem_wgrad_f32', 'y4_amax_f32',
        'y4_amax_merge_u32'}
    was = L.y4_get_conv_mode()
    try:
        assert L.y4_set_conv_mode(-1) == SHAPE and L.y4_set_conv_mode(4) == SHAPE and L.y4_get_conv_mode() == was
        for mode in ALL_MODES:
            assert L.y4_set_conv_mode(mode) == OK and L.y4_get_conv_mode() == mode
            for entry, modes, a, want, what in cases:
                if mode in modes:
                    got = getattr(L, entry)(*a)
                    assert got == want, (entry, mode, what, got, want)
    finally:
        L.y4_set_conv_mode(was)


def test_state_dict_matches_reference_tree():
    m = YOLOv4(recipe.MODEL_CFG)
    sd = m.state_dict()
    spec = NW.yolov4_state_dict_spec()
    assert list(sd.keys()) == [k for k, _ in spec]
    for k, shp in spec:
        assert tuple(sd[k].shape) == tuple(shp)
        assert sd[k].dtype == (torch.int64 if k.endswith('num_batches_tracked') else torch.float32)
    assert len(sd) == 648 and sum(p.numel() for p in m.parameters()) == 64885341
    # round trip through the reference's OIHW layout keeps KRSC memory
    m2 = YOLOv4(recipe.MODEL_CFG)
    recipe.fill_state_dict_(sd, 3)
    m2.load_state_dict({k: v.contiguous() for k, v in sd.items()})
    w = m2.backbone.stage1.base.conv.weight
    assert w.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(m2.state_dict()['backbone.stage1.base.conv.weight'], sd['backbone.stage1.base.conv.weight'])


def test_constructor_signatures_match_reference():
    assert list(inspect.signature(ConvBNAct.__init__).parameters)[1:] == \
        ['in_ch', 'out_ch', 'kernel_size', 'stride', 'bias', 'bn', 'act']
    assert list(inspect.signature(ResBlock.__init__).parameters)[1:] == ['ch', 'num_blocks', 'shortcut', 'act']
    assert list(inspect.signature(CSPDownSample0.__init__).parameters)[1:] == \
        ['in_ch', 'out_ch', 'kernel_size', 'stride', 'act']
    assert list(inspect.signature(CSPDownSample.__init__).parameters)[1:] == \
        ['in_ch', 'out_ch', 'kernel_size', 'stride', 'num_blocks', 'shortcut', 'act']
    assert list(inspect.signature(YOLOv4.__init__).parameters)[1:] == ['cfg', 'device']
    assert list(inspect.signature(YOLOLayer.__init__).parameters)[1:] == ['cfg', 'layer_no', 'device']
    assert list(inspect.signature(YOLOLoss.__init__).parameters)[1:4] == ['cfg', 'ignore_thresh', 'device']
    assert list(inspect.signature(utils.postprocess).parameters) == ['prediction', 'num_classes', 'conf_thre', 'nms_thre']
    assert list(inspect.signature(utils.nms).parameters) == ['bbox', 'thresh', 'score', 'limit']
    assert YOLOLayer.strides == [8, 16, 32] and YOLOLoss.strides == [8, 16, 32]
    with pytest.raises(ValueError):
        ConvBNAct(8, 8, 1, 1, act='gelu')
    with pytest.raises(AssertionError):
        YOLOv4(dict(recipe.MODEL_CFG, TYPE='YOLOv3'))
    c = ConvBNAct(32, 255, 1, 1, bias=True, bn=False, act='linear')
    assert sorted(c.state_dict()) == ['conv.bias', 'conv.weight']
    c = ConvBNAct(32, 64, 3, 2)
    assert sorted(c.state_dict()) == ['conv.weight', 'norm.bias', 'norm.num_batches_tracked', 'norm.running_mean',
                                      'norm.running_var', 'norm.weight']


def test_no_cpu_fallback():
    m = ConvBNAct(32, 32, 1, 1)
    with pytest.raises(yolov4_amd.Y4Error):
        m(torch.zeros(1, 32, 4, 4))
    lay = YOLOLayer(recipe.MODEL_CFG, 0).eval()
    with pytest.raises(yolov4_amd.Y4Error):
        lay(torch.zeros(1, 255, 4, 4))
    if not torch.cuda.is_available():
        with pytest.raises(yolov4_amd.Y4Error):
            utils.postprocess(torch.zeros(1, 10, 85), 80)
        with pytest.raises(yolov4_amd.Y4Error):
            utils.nms(np.zeros((3, 4), np.float32), 0.5)
    # the product package must not import the oracle
    import sys
    for name, mod in list(sys.modules.items()):
        if name.startswith('yolov4_amd') and mod is not None and getattr(mod, '__file__', None):
            src = open(mod.__file__).read()
            assert 'import oracle' not in src and 'from oracle' not in src, name


def test_build_factories():
    import argparse
    m = build_model(argparse.Namespace(channels_last=True), recipe.FULL_CFG, device=torch.device('cpu'))
    assert isinstance(m, YOLOv4)
    c = build_criterion(recipe.FULL_CFG, device=torch.device('cpu'))
    assert isinstance(c, YOLOLoss) and abs(c.ignore_thresh - 0.7) < 1e-12


def test_nhwc_pitch_helper():
    t = torch.empty((2, 64, 5, 7), memory_format=torch.channels_last)
    assert ops.nhwc_pitch(t) == 64
    assert ops.nhwc_pitch(t[:, 16:48]) == 64
    assert ops.nhwc_pitch(torch.empty(2, 64, 5, 7)) is None
    assert ops.nhwc_pitch(torch.empty((2, 64, 1, 1), memory_format=torch.channels_last)) == 64
    v, ld = ops.as_nhwc(torch.arange(2 * 6 * 3 * 3, dtype=torch.float32).reshape(2, 6, 3, 3))
    assert ld == 8 and v.shape == (2, 6, 3, 3)
    assert torch.equal(v, torch.arange(2 * 6 * 3 * 3, dtype=torch.float32).reshape(2, 6, 3, 3))
