# -*- coding: utf-8 -*-
"""The stem without its pre-BatchNorm tensor (csrc/stem_fused.hip: y0 = conv(x) re-formed inside the BatchNorm passes)
against the separate conv / BatchNorm / wgrad calls it replaces and against an fp64 reference.

Shapes: (3, 37, 41): M = 4551 ends inside a 32-pixel tile and inside a 256-pixel group (18 groups = 18 blocks), fed as
NCHW strides and as NHWC; (1, 16, 16): exactly one group; (2, 5, 7): less than one group, nearly every pixel on the halo.
Cout 32 and 16 (lanes >= Cout idle); Mish and leaky ReLU.

Bounds.  Statistics: bit-equal to the old sequence (the same partial rows, the same finalize).  z, the amax word, dgamma,
dbeta, dW: max |error| against torch-CPU float64 (conv2d -> batch_norm(training) -> activation, and its autograd) at most
1.5 x the error of the OLD sequence on the same inputs + 1e-6 max|reference|.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import recipe
import yolov4_amd
from yolov4_amd import ops
from yolov4_amd._lib import ACT_IDS, check

EPS, MOM = 1e-5, 0.1
CASES = [
    # B, H, W, nhwc, Cout, act
    (3, 37, 41, False, 32, 'mish'),
    (3, 37, 41, True, 32, 'mish'),
    (1, 16, 16, False, 32, 'mish'),
    (2, 5, 7, False, 32, 'mish'),
    (3, 37, 41, True, 16, 'mish'),
    (3, 37, 41, False, 32, 'leaky_relu'),
    (2, 5, 7, True, 16, 'leaky_relu'),
]
IDS = ['%dx%dx%d-%s-c%d-%s' % (c[0], c[1], c[2], 'nhwc' if c[3] else 'nchw', c[4], c[5]) for c in CASES]


def _dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _act64(v, act):
    return F.mish(v) if act == 'mish' else F.leaky_relu(v, 0.1)


def _word(cell):
    return float(cell.cpu().view(torch.float32)[0])


@functools.lru_cache(maxsize=None)
def run(case):
    """Old sequence, new sequence (backward twice) and the fp64 reference of one case, computed once: CPU tensors."""
    B, H, W, nhwc, Cout, act = case
    dev = _dev()
    L = yolov4_amd.lib()
    assert L.y4_get_conv_mode() == 3
    seed = 1000 + 7 * B + H + 3 * Cout
    x = recipe.randn((B, 3, H, W), seed)
    w = recipe.randn((Cout, 3, 3, 3), seed + 1, 0.3)
    gamma = 1.0 + recipe.randn((Cout,), seed + 2, 0.2)
    beta = recipe.randn((Cout,), seed + 3, 0.3)
    dz = recipe.randn((B, Cout, H, W), seed + 4)
    M = B * H * W
    ngroups = (M + 255) // 256
    xd = x.to(dev).contiguous(memory_format=torch.channels_last) if nhwc else x.to(dev)
    wd = w.to(dev).contiguous(memory_format=torch.channels_last)
    gd, bd = gamma.to(dev), beta.to(dev)
    dzd = dz.to(dev).contiguous(memory_format=torch.channels_last)
    strides = xd.stride()
    assert L.y4_stem_fused_ok(*strides, B, H, W, Cout) == 1
    out = {}

    # ---- the old sequence through the C ABI
    def stats_buffers():
        return (torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev), torch.zeros((), dtype=torch.int64, device=dev))
    y = ops.empty_nhwc(B, Cout, H, W, dev)
    part = torch.zeros(ngroups * 2 * Cout, device=dev)
    check(L.y4_conv2d_stem_fwd_f32(_p(xd), *strides, _p(wd), _p(y), ops.nhwc_pitch(y), B, H, W, Cout, None, None,
                                   ACT_IDS['linear'], _p(part), _st()), 'stem_fwd')
    mean_o, invstd_o = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    rm_o, rv_o, nbt_o = stats_buffers()
    fb = L.y4_bn_finalize_workspace(Cout)
    fws = torch.empty(fb, dtype=torch.uint8, device=dev)
    check(L.y4_bn_finalize_partials_f32(_p(part), ngroups, M, Cout, _p(mean_o), _p(invstd_o), _p(rm_o), _p(rv_o), _p(nbt_o),
                                        MOM, EPS, _p(fws), fb, _st()), 'finalize')
    cell_o = torch.zeros(1, dtype=torch.int32, device=dev)
    z_o = ops.bn_act_fwd_raw(y, mean_o, invstd_o, gd, bd, act, out_amax=cell_o)
    dy_o, dg_o, db_o = ops.bn_act_bwd_raw(dzd, y, mean_o, invstd_o, gd, bd, act)
    dw_o = ops.conv_wgrad_raw(xd, dy_o, (Cout, 3, 3, 3), 3, 1)

    # ---- the recomputing passes
    z_n = ops.empty_nhwc(B, Cout, H, W, dev)
    mean_n, invstd_n = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    rm_n, rv_n, nbt_n = stats_buffers()
    cell_n = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = L.y4_stem_bn_act_fwd_workspace(B, H, W, Cout)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    check(L.y4_stem_bn_act_fwd_f32(_p(xd), *strides, _p(wd), B, H, W, Cout, _p(gd), _p(bd), ACT_IDS[act], _p(mean_n),
                                   _p(invstd_n), _p(rm_n), _p(rv_n), _p(nbt_n), MOM, EPS, _p(z_n), ops.nhwc_pitch(z_n),
                                   _p(cell_n), _p(ws), nb, _st()), 'stem_bn_act_fwd')
    part_n = ws[:ngroups * 2 * Cout * 4].view(torch.float32)
    dw_n, dg_n, db_n = ops.stem_bn_act_bwd_raw(xd, wd, dzd, mean_n, invstd_n, gd, bd, act)
    dw_2, dg_2, db_2 = ops.stem_bn_act_bwd_raw(xd, wd, dzd, mean_n, invstd_n, gd, bd, act)
    torch.cuda.synchronize()
    for k, v in dict(part_o=part, part_n=part_n, mean_o=mean_o, mean_n=mean_n, invstd_o=invstd_o, invstd_n=invstd_n,
                     rm_o=rm_o, rm_n=rm_n, rv_o=rv_o, rv_n=rv_n, nbt_o=nbt_o, nbt_n=nbt_n, z_o=z_o, z_n=z_n,
                     dg_o=dg_o, dg_n=dg_n, dg_2=dg_2, db_o=db_o, db_n=db_n, db_2=db_2, dw_o=dw_o, dw_n=dw_n, dw_2=dw_2).items():
        out[k] = v.detach().cpu().clone()
    out['amax_o'], out['amax_n'] = _word(cell_o), _word(cell_n)

    # ---- fp64 reference
    x64 = x.double()
    w64, g64, b64 = w.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z64 = _act64(F.batch_norm(F.conv2d(x64, w64, None, 1, 1), None, None, g64, b64, True, MOM, EPS), act)
    z64.backward(dz.double())
    out.update(z_r=z64.detach(), dw_r=w64.grad, dg_r=g64.grad, db_r=b64.grad)
    return out


def _no_worse(r, name):
    ref = r[name + '_r']
    e_new = float((r[name + '_n'].double() - ref).abs().max())
    e_old = float((r[name + '_o'].double() - ref).abs().max())
    bound = 1.5 * e_old + 1e-6 * float(ref.abs().max())
    print(f'{name}: err new {e_new:.3e}  old {e_old:.3e}  bound {bound:.3e}  bit-equal to old: {torch.equal(r[name + "_n"], r[name + "_o"])}')
    assert e_new <= bound, (name, e_new, e_old, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_statistics_are_bit_equal_to_the_old_sequence(case):
    r = run(case)
    assert torch.equal(r['part_n'], r['part_o'])
    for k in ('mean', 'invstd', 'rm', 'rv', 'nbt'):
        assert torch.equal(r[k + '_n'], r[k + '_o']), k
    assert int(r['nbt_n']) == 1


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_no_worse_than_the_old_sequence_vs_fp64(case):
    r = run(case)
    _no_worse(r, 'z')
    # the word is max|z| of what was written, exactly -- as the old path's word is of its z
    assert r['amax_o'] == float(r['z_o'].abs().max())
    assert r['amax_n'] == float(r['z_n'].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_backward_no_worse_than_the_old_sequence_vs_fp64(case):
    r = run(case)
    for name in ('dg', 'db', 'dw'):
        _no_worse(r, name)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_backward_is_deterministic(case):
    r = run(case)
    for name in ('dg', 'db', 'dw'):
        assert torch.equal(r[name + '_n'], r[name + '_2']), name


def _stem_module(dev, act='mish'):
    from yolov4_amd.darknet.darknet import ConvBNAct
    torch.manual_seed(5)
    m = ConvBNAct(3, 32, 3, 1, act=act).to(dev).train()
    with torch.no_grad():
        m.norm.weight.copy_(1.0 + recipe.randn((32,), 21, 0.2).to(dev))
        m.norm.bias.copy_(recipe.randn((32,), 22, 0.3).to(dev))
    return m


@pytest.mark.gpu
def test_module_takes_the_fused_path_and_saves_no_y0():
    dev = _dev()
    m = _stem_module(dev)
    x = recipe.randn((2, 3, 19, 23), 31).to(dev)
    z = m(x)
    assert ops.last_conv_kernel().startswith('stem_bn_act_write_kernel')
    saved = z.grad_fn.saved_tensors
    assert not any(t.dim() == 4 and tuple(t.shape) == tuple(z.shape) for t in saved)      # no pre-BatchNorm tensor kept
    gz = recipe.randn(tuple(z.shape), 32).to(dev)
    z.backward(gz)              # (without y0 only the recomputing backward can produce these gradients)
    # against the fp64 reference of the same module: fp32-grade, 2e-5 of the tensor's range (sums over 874 pixels of
    # values carrying ~1e-6 relative error each; the raw conv tests use 1e-5 for a single 27-term chain)
    w64 = m.conv.weight.detach().cpu().double().requires_grad_(True)
    g64 = m.norm.weight.detach().cpu().double().requires_grad_(True)
    b64 = m.norm.bias.detach().cpu().double().requires_grad_(True)
    z64 = F.mish(F.batch_norm(F.conv2d(x.cpu().double(), w64, None, 1, 1), None, None, g64, b64, True, MOM, EPS))
    z64.backward(gz.cpu().double())
    for got, ref in ((z, z64), (m.conv.weight.grad, w64.grad), (m.norm.weight.grad, g64.grad), (m.norm.bias.grad, b64.grad)):
        err = float((got.detach().cpu().double() - ref.detach()).abs().max())
        assert err <= 2e-5 * float(ref.detach().abs().max()), (err, float(ref.detach().abs().max()))
    assert int(m.norm.num_batches_tracked) == 1


@pytest.mark.gpu
def test_module_with_input_gradient_takes_the_old_sequence():
    dev = _dev()
    m = _stem_module(dev)
    x = recipe.randn((2, 3, 19, 23), 31).to(dev).requires_grad_(True)
    ops.last_conv_kernel()
    z = m(x)
    assert not ops.last_conv_kernel().startswith('stem_bn_act')
    assert any(t.dim() == 4 and tuple(t.shape) == tuple(z.shape) for t in z.grad_fn.saved_tensors)     # y0 is there
    gz = recipe.randn(tuple(z.shape), 32).to(dev)
    z.backward(gz)
    x64 = x.detach().cpu().double().requires_grad_(True)
    z64 = F.mish(F.batch_norm(F.conv2d(x64, m.conv.weight.detach().cpu().double(), None, 1, 1), None, None,
                              m.norm.weight.detach().cpu().double(), m.norm.bias.detach().cpu().double(), True, MOM, EPS))
    z64.backward(gz.cpu().double())
    assert x.grad is not None and tuple(x.grad.shape) == tuple(x.shape)
    err = float((x.grad.cpu().double() - x64.grad).abs().max())
    assert err <= 2e-5 * float(x64.grad.abs().max()), err


def test_dispatch_predicate_runs_on_host():
    """y4_stem_fused_ok: x goes through ONE 32-bit window, z and dz through a window per group -- so bs 128 @608 (6 GB of z)
    is in, an x of more than 4 GiB or a mode without the matrix-core stem is out."""
    L = yolov4_amd.lib()
    was = L.y4_get_conv_mode()

    def nchw(B, H, W):
        return (3 * H * W, H * W, W, 1)

    def nhwc(B, H, W):
        return (3 * H * W, 1, 3 * W, 3)
    try:
        for mode in (1, 2, 3):
            L.y4_set_conv_mode(mode)
            assert L.y4_stem_fused_ok(*nchw(128, 608, 608), 128, 608, 608, 32) == 1
            assert L.y4_stem_fused_ok(*nhwc(128, 608, 608), 128, 608, 608, 32) == 1
        assert 128 * 608 * 608 * 32 * 4 > (1 << 32)                                   # z / dz beyond one window: still in
        assert L.y4_stem_fused_ok(*nchw(64, 608, 608), 64, 608, 608, 16) == 1
        assert L.y4_stem_fused_ok(*nchw(1024, 608, 608), 1024, 608, 608, 32) == 0     # x = 4.5 GB
        assert L.y4_stem_fused_ok(*nchw(2, 64, 64), 2, 64, 64, 64) == 0               # Cout > 32
        assert L.y4_stem_fused_ok(*nchw(2, 64, 64), 2, 64, 64, 30) == 0               # not a multiple of 4
        assert L.y4_stem_fused_ok(*nchw(2, 64, 4), 2, 64, 4, 32) == 0                 # W < 5 (the B-operand walk)
        assert L.y4_stem_fused_ok(3 * 64 * 64, 64 * 64, -64, 1, 2, 64, 64, 32) == 0   # negative stride
        assert L.y4_stem_fused_ok(*nchw(1, 4096, 4096), 1, 4096, 4096, 32) == 0       # H W >= 2^24
        L.y4_set_conv_mode(0)
        assert L.y4_stem_fused_ok(*nchw(64, 608, 608), 64, 608, 608, 32) == 0         # fp32 mode: the VALU stem, old sequence
    finally:
        L.y4_set_conv_mode(was)
    assert L.y4_stem_bn_act_fwd_workspace(64, 608, 608, 32) >= (64 * 608 * 608 // 256) * 2 * 32 * 4
    assert L.y4_stem_bn_act_bwd_workspace(64, 608, 608, 32) >= 4096 * 4096 + 64 * 1024 * 8
    # pointers are checked before anything is launched
    assert L.y4_stem_bn_act_fwd_f32(None, 1, 1, 1, 1, None, 1, 8, 8, 32, None, None, 2, None, None, None, None, None,
                                    0.1, 1e-5, None, 32, None, None, 0, None) == 2


def test_python_predicate_rejects_other_layers():
    x = torch.zeros(2, 3, 16, 16)
    assert not ops.stem_fused_ok(x, 32, 3, 2)
    assert not ops.stem_fused_ok(x, 32, 1, 1)
    assert not ops.stem_fused_ok(torch.zeros(2, 4, 16, 16), 32, 3, 1)
    assert ops.stem_fused_ok(x, 32, 3, 1) == (yolov4_amd.lib().y4_get_conv_mode() in (1, 2, 3))
