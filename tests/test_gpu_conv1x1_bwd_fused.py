# -*- coding: utf-8 -*-
"""The fused backward of conv 1x1 -> BatchNorm -> activation (csrc/conv1x1_bwd_fused.hip) through the C ABI, over the cases
of tests/conv1x1_bwd_cases.py (tests/test_conv1x1_bwd_cases.py shows without a GPU which branch each reaches), and through
autograd on the smallest map the route takes.  References, bounds and the plan are those of conv1x1_bwd_cases.py; every
buffer sits between guards of a NaN bit pattern no kernel produces, and every output starts out filled with it.

Beside each accepted result the tests print how far the fused result lies from the fp64 product of the UNSPLIT fp64 dy,
relative to the unfused sequence of the same library (ops.bn_act_bwd_raw -> conv_dgrad_raw / conv_wgrad_raw) on the same
inputs: rms(fused - fp64) / rms(unfused - fp64).  That ratio is a record, not a threshold: the fused kernel scales dy by a
bound of its maximum, the unfused sequence by the measured maximum, which may be a few bits finer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_cases as BC
import conv1x1_bwd_cases as FC

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
G = 32                                   # guard words (128 B) in front of and behind every device buffer
RATIO = {'dx': 0.0, 'dw': 0.0}           # largest rms ratio fused / unfused so far (printed per test)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    old, old_bf = yolov4_amd.get_conv_mode(), yolov4_amd.lib().y4_get_planes_bf16()
    yolov4_amd.set_conv_mode('f16x2')
    yield torch.device('cuda:0')
    yolov4_amd.set_conv_mode(old)
    yolov4_amd.lib().y4_set_planes_bf16(old_bf)


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import lib
    return lib(), ops._stream


class Buf(object):
    """n 32-bit words on the device between two guards; everything starts as the sentinel unless `init` is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        h = np.full(self.n + 2 * G, BC.SENT, dtype=np.uint32)
        if init is not None:
            h[G:G + self.n] = np.ascontiguousarray(init).view(np.uint32).ravel()
        self.t = torch.from_numpy(h.view(np.int32)).to(dev)

    def ptr(self, off_words=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (G + off_words))

    def get(self):
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:G] == BC.SENT).all() and (h[G + self.n:] == BC.SENT).all(), 'write outside the buffer'
        return h[G:G + self.n].copy()


def _rows(a, ld, off=0):
    """[M, C] -> [M, ld] with a at columns [off, off + C) and the sentinel everywhere else"""
    out = BC.sentinel((a.shape[0], ld))
    out[:, off:off + a.shape[1]] = a
    return out


@functools.lru_cache(maxsize=None)
def _data(i):
    c = FC.CASES[i]
    d = FC.build(c)
    r = FC.bn_ref(c, d)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d, r


def _run(dev, c, d, prepared=None, shape=None, frozen=0, misalign=0):
    """one y4_conv1x1_bn_act_bwd_fused_f32 call -> dict(rc, dx [M, Cin], dw, dgamma, dbeta, bounds, kernel); the pitch padding
    of dx and every guard are checked here"""
    from yolov4_amd import ops
    L, stream = _abi()
    M = c['M']
    Cout, Cin = shape or (c['Cout'], c['Cin'])
    dzd = Buf(dev, M * c['lddz'], _rows(d['dz'], c['lddz'], c['dz_off']))
    yd = Buf(dev, M * c['ldy'], _rows(d['y'], c['ldy']))
    xd = Buf(dev, M * c['ldx'], _rows(d['x'], c['ldx']))
    rd = Buf(dev, M * c['ldr'], _rows(d['res'], c['ldr'])) if d['res'] is not None else None
    v = [Buf(dev, c['Cout'], np.asarray(d[k], F32)) for k in ('mean', 'invstd', 'gamma', 'beta')]
    wd = Buf(dev, d['w'].size, d['w'])
    pd = Buf(dev, prepared.size, prepared) if prepared is not None else None
    xw = Buf(dev, 1, np.array([BC.amax_word(d['x'])], dtype=np.uint32))
    dxd, dwd, dg, db = Buf(dev, M * c['lddx']), Buf(dev, c['Cout'] * c['Cin']), Buf(dev, c['Cout']), Buf(dev, c['Cout'])
    bd = Buf(dev, 8, np.zeros(8, dtype=np.uint32))
    nbytes = L.y4_conv1x1_bn_act_bwd_fused_workspace(M, c['Cin'], c['Cout'])
    assert nbytes == FC.workspace(M, c['Cin'], c['Cout'])
    ws = Buf(dev, nbytes // 4)
    ops.last_conv_kernel()
    rc = L.y4_conv1x1_bn_act_bwd_fused_f32(
        dzd.ptr(c['dz_off']), c['lddz'], yd.ptr(), c['ldy'], v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), c['act'],
        dg.ptr(), db.ptr(), M, Cin, Cout, ctypes.c_void_p(xd.ptr().value + misalign), c['ldx'], xw.ptr(),
        None if prepared is not None else wd.ptr(), pd.ptr() if prepared is not None else None,
        dxd.ptr(), c['lddx'], rd.ptr() if rd is not None else None, c['ldr'], dwd.ptr(), ws.ptr(), nbytes, bd.ptr(), frozen, stream())
    torch.cuda.synchronize()
    ws.get()
    for b in [dzd, yd, xd, wd, xw] + v + ([rd] if rd is not None else []) + ([pd] if pd is not None else []):
        b.get()
    body = dxd.get().reshape(M, c['lddx'])
    if rc == 0:
        assert (body[:, c['Cin']:] == BC.SENT).all(), 'write into the pitch padding of dx'
    return dict(rc=rc, dx=np.ascontiguousarray(body[:, :c['Cin']]), dw=dwd.get().reshape(c['Cout'], c['Cin']), dgamma=dg.get(),
                dbeta=db.get(), bounds=bd.get(), kernel=ops.last_conv_kernel())


def _t4(dev, a):
    """[M, C] -> logical [1, C, 1, M] tensor over NHWC memory"""
    M, C = a.shape
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev).view(1, 1, M, C).permute(0, 3, 1, 2)


def _unfused(dev, c, d):
    """the sequence the fused call replaces, on the same inputs: (dx, dw, dgamma, dbeta) as numpy"""
    from yolov4_amd import ops
    from yolov4_amd._lib import ACT_IDS
    act = {v: k for k, v in ACT_IDS.items()}[c['act']]
    M, Cout, Cin = c['M'], c['Cout'], c['Cin']
    vec = [torch.from_numpy(np.asarray(d[k], F32)).to(dev) for k in ('mean', 'invstd', 'gamma', 'beta')]
    cell = torch.zeros(1, dtype=torch.int32, device=dev)
    dy, dgamma, dbeta = ops.bn_act_bwd_raw(_t4(dev, d['dz']), _t4(dev, d['y']), *vec, act, out_amax=cell)
    w = torch.from_numpy(d['w']).to(dev).view(Cout, 1, 1, Cin).permute(0, 3, 1, 2)
    x = _t4(dev, d['x'])
    dx = ops.conv_dgrad_raw(dy, w, (1, Cin, 1, M), 1, 1, dy_amax=cell, residual=_t4(dev, d['res']) if d['res'] is not None else None)
    dw = ops.conv_wgrad_raw(x, dy, (Cout, Cin, 1, 1), 1, 1, x_amax=ops.amax_raw(x), dy_amax=cell)
    torch.cuda.synchronize()
    return (dx.permute(0, 2, 3, 1).reshape(M, Cin).cpu().numpy(), dw.permute(0, 2, 3, 1).reshape(Cout, Cin).cpu().numpy(),
            dgamma.cpu().numpy(), dbeta.cpu().numpy())


def _rms(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.sqrt(np.mean((a[fin] - b[fin]) ** 2))) if fin.any() else 0.0


def _worst(ok, got, ref, bound):
    bad = np.argwhere(~ok)[:5]
    return [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in bad]


@pytest.mark.parametrize('i', range(len(FC.CASES)), ids=[FC.case_id(c) for c in FC.CASES])
def test_fused_against_fp64(dev, i):
    c = FC.CASES[i]
    d, r = _data(i)
    prep = FC.prepared_filter(d['w']) if c['prepared'] else None
    o = _run(dev, c, d, prepared=prep)
    assert o['rc'] == 0
    assert FC.KERNEL in o['kernel'], o['kernel']
    # the scale word: formed as the plane layers form it, at or above the true bound; poisoned by a planted Inf
    word = int(o['bounds'][5])
    if c['plant']:
        assert ((word >> 23) & 0xff) == 255 and BC.scale_exp(word) == 127
    else:
        true = BC.bwd_bound_ref64(r)
        assert true <= BC.word_value(word) <= true * 1.01 + BC.TINY, (true, BC.word_value(word))
    p = FC.products(c, d, r, word)
    dx, dw = o['dx'].view(F32), o['dw'].view(F32)
    for got, name in ((dx, 'dx'), (dw, 'dw')):
        assert not BC.is_sentinel(got).any(), name + ': an element was not written'
        ok, used = FC.judge(got, p[name], p['b_' + name])
        print('%s %s: share of the bound used %.3f' % (FC.case_id(c), name, float(used.max())))
        assert ok.all(), (name, _worst(ok, got, p[name], p['b_' + name]))
    if c['plant']:
        assert not np.isfinite(dx).any()
        assert np.where(~np.isfinite(dw).all(axis=1))[0].tolist() == sorted(ch for _, ch in d['sites'])
    # a second call gives the same bits (with the filter handed in the other way where the case has it prepared)
    o2 = _run(dev, c, d)
    assert o2['rc'] == 0
    for k in ('dx', 'dw', 'dgamma', 'dbeta', 'bounds'):
        assert np.array_equal(o[k], o2[k]), k
    # the unfused sequence on the same inputs: dgamma / dbeta bit-equal, dx / dW as a yardstick of accuracy
    udx, udw, udg, udb = _unfused(dev, c, d)
    assert np.array_equal(o['dgamma'], udg.view(np.uint32)) and np.array_equal(o['dbeta'], udb.view(np.uint32))
    if not c['plant']:
        for got, ugot, name in ((dx, udx, 'dx'), (dw, udw, 'dw')):
            ef, eu = _rms(got, p[name + '64']), _rms(ugot, p[name + '64'])
            ratio = ef / eu if eu > 0 else 0.0
            RATIO[name] = max(RATIO[name], ratio)
            print('%s %s: rms distance from fp64 fused %.3e unfused %.3e ratio %.3f (largest so far %.3f)'
                  % (FC.case_id(c), name, ef, eu, ratio, RATIO[name]))


def test_unsupported_calls_write_nothing(dev):
    c = FC.CASES[[FC.case_id(k) for k in FC.CASES].index('co64_ci64_m229')]
    d, _ = _data(FC.CASES.index(c))
    for kw in (dict(shape=(128, 64)), dict(shape=(64, 32)), dict(shape=(32, 128)), dict(frozen=1), dict(misalign=4)):
        o = _run(dev, c, d, **kw)
        assert o['rc'] == 1, kw                                              # Y4_ERR_SHAPE
        for k in ('dx', 'dw', 'dgamma', 'dbeta'):
            assert (o[k] == BC.SENT).all(), (kw, k)
        assert (o['bounds'] == 0).all()


# ------------------------------------------------------------------------------------------ through autograd
def _layer(dev, cin, cout, seed):
    from yolov4_amd.darknet.darknet import ConvBNAct
    torch.manual_seed(seed)
    m = ConvBNAct(cin, cout, 1, 1, act='mish').to(dev)
    with torch.no_grad():
        m.norm.weight.uniform_(0.5, 1.5)
        m.norm.bias.normal_(0.0, 0.5)
    return m.train()


def _grads(dev, m, x0, gz, fused, park, slots):
    """one forward / backward of the layer -> (dx, dw, dgamma, dbeta, kernel) as numpy, on the route `fused` selects"""
    from yolov4_amd import ops
    old = ops.FUSED_1X1['on']
    ops.FUSED_1X1['on'] = fused
    # backward runs on autograd's own thread and the library keeps the kernel's name per thread: ask right after each call
    names = []
    raw = {n: getattr(ops, n) for n in ('conv1x1_bn_act_bwd_fused_raw', 'conv_dgrad_raw', 'conv_wgrad_raw')}

    def spy(fn):
        def inner(*a, **kw):
            out = fn(*a, **kw)
            names.append(ops.last_conv_kernel())
            return out
        return inner
    for n, fn in raw.items():
        setattr(ops, n, spy(fn))
    try:
        for p in m.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        box = {'dres': park.clone()} if park is not None else None
        ready = []
        if slots:                                             # gradient slots as BucketedDDP hands them out: zeroed, fresh
            for p in (m.conv.weight, m.norm.weight, m.norm.bias):
                p.grad = torch.zeros_like(p)
                p._y4_grad_fresh = True
                p._y4_grad_ready = (lambda q=p: ready.append(q))
        z = m(x, dres_take=box)
        z.backward(gz)
        torch.cuda.synchronize()
        kern = ' '.join(names)
        if slots:
            assert len(ready) == 3 and not any(p._y4_grad_fresh for p in ready)
        out = (x.grad.permute(0, 2, 3, 1).cpu().numpy().astype(F64), m.conv.weight.grad.cpu().numpy().astype(F64),
               m.norm.weight.grad.cpu().numpy(), m.norm.bias.grad.cpu().numpy(), kern)
        assert box is None or 'dres' not in box
        return out
    finally:
        ops.FUSED_1X1['on'] = old
        for n, fn in raw.items():
            setattr(ops, n, fn)
        for p in m.parameters():
            for a in ('_y4_grad_fresh', '_y4_grad_ready'):
                if hasattr(p, a):
                    delattr(p, a)


@pytest.mark.parametrize('cin', [64, 128])
def test_autograd_route(dev, cin):
    """ConvBNAct(cin, 64, 1, 1) on a 2 x cin x 256 x 256 input (M = 131072: the route's threshold), switch on and off, with
    and without a parked skip gradient, with DDP-style in-place slots.  Both routes are judged by the bounds of the C ABI
    test: the fp64 reference takes the fp32 y, mean and invstd the forward pass itself computes (the same call, repeated
    here), dW whole and dx on every 37th pixel (a row of dx depends on its own row of dy alone)."""
    from yolov4_amd import ops
    m = _layer(dev, cin, 64, 7 + cin)
    g = torch.Generator(device='cpu').manual_seed(11 + cin)
    x0 = torch.randn(2, cin, 256, 256, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    gz = torch.randn(2, 64, 256, 256, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    park = (torch.randn(2, cin, 256, 256, generator=g) * 0.1).to(dev).contiguous(memory_format=torch.channels_last)
    M = 2 * 256 * 256
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, -1).cpu().numpy()
    y, mean, invstd = ops.conv_fwd_bnstats_raw(x0, m.conv.weight.detach(), 1, 1, None, None, None, 0.1, m.norm.eps, x_amax=ops.amax_raw(x0))
    c = dict(M=M, Cout=64, Cin=cin, act=BC.ACT_MISH)
    d = dict(dz=flat(gz), y=flat(y), mean=mean.cpu().numpy(), invstd=invstd.cpu().numpy(), gamma=m.norm.weight.detach().cpu().numpy(),
             beta=m.norm.bias.detach().cpu().numpy(), x=flat(x0), w=m.conv.weight.detach().permute(0, 2, 3, 1).reshape(64, cin).cpu().numpy(),
             res=None)
    r = FC.bn_ref(c, d)
    word = FC.bound_word(r)
    rows = np.arange(0, M, 37)
    for pk in (None, park):
        d['res'] = flat(pk) if pk is not None else None
        p = FC.products(c, d, r, word, rows=rows)
        for slots in (False, True):
            a = _grads(dev, m, x0, gz, True, pk, slots)
            b = _grads(dev, m, x0, gz, False, pk, slots)
            assert FC.KERNEL in a[4], a[4]
            assert FC.KERNEL not in b[4], b[4]
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])          # dgamma, dbeta: the same kernels
            what = 'cin %d park %s slots %s' % (cin, pk is not None, slots)
            for route, got in (('fused', a), ('unfused', b)):
                for name, v in (('dx', got[0].reshape(M, cin)[rows]), ('dw', got[1].reshape(64, cin))):
                    ok, used = FC.judge(v, p[name], p['b_' + name])
                    print('%s %s %s: share of the bound used %.3f, rms distance from fp64 %.3e'
                          % (what, route, name, float(used.max()), _rms(v, p[name + '64'])))
                    assert ok.all(), (what, route, name, _worst(ok, v, p[name], p['b_' + name]))
