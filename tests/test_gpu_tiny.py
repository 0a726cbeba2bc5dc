# -*- coding: utf-8 -*-
"""YOLOv4-tiny on the GPU: the kernels of csrc/tiny.hip driven through the C ABI against the references of
tests/tiny_cases.py (tests/test_tiny_cases.py checks those without a GPU), fork_half, the model against tiny_oracle in two
conv modes, and one pass through train_step / validate / detect_images / Darknet weights.

Every device buffer a kernel writes starts as a NaN bit pattern no kernel produces and sits between two guards: pitch
padding, neighbouring channel slices and the guards must still hold the pattern afterwards.

Which case reaches which branch:
  y4_maxpool2x2_s2_fwd_f32 / _bwd   test_pool: C / 4 = 1, 3, 5, 16; pitch > C on either side; channel slices at 16-byte
                                    offsets; one output; 7 x 9 (dropped row and column); 1 x 1 and 1 x 5 (no output); ties, NaN
                                    first / last / twice, +-inf, signed zeros; idx = NULL; test_pool_grid_stride: two laps;
                                    test_pool_refused_calls: every refused argument set, nothing written
  y4_conv2d_stem_s2_fwd_f32         test_stem_forward: maps 8x8, 13x9, 2x2, 1x1; B = 1, 3; Cout = 4, 32, 64; NCHW and NHWC
                                    strides; three epilogues; test_stem_dispatch: Cout = 68 and 6 stay on the direct kernel
  y4_conv2d_stem_s2_wgrad_f32       test_stem_wgrad: the same shapes and one with twelve slabs per filter element
  y4_fork_half_bwd_f32              test_fork_half (g_full only: no launch; g_hi only; both)"""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import recipe
import tiny_cases as TC

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
G = 32                                   # guard words (128 B) in front of and behind every device buffer


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import lib
    return lib(), ops._stream


class Buf(object):
    """n 32-bit words on the device between two guards; everything starts as the sentinel unless `init` is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        h = np.full(self.n + 2 * G, TC.SENT, dtype=np.uint32)
        if init is not None:
            h[G:G + self.n] = np.ascontiguousarray(init).view(np.uint32).ravel()
        self.t = torch.from_numpy(h.view(np.int32)).to(dev)

    def ptr(self, off_words=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (G + off_words))

    def get(self):
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:G] == TC.SENT).all() and (h[G + self.n:] == TC.SENT).all(), 'write outside the buffer'
        return h[G:G + self.n].copy()


class Rows(object):
    """[M, C] fp32 rows at pitch ld, `off` columns into the buffer's rows; the columns beside the slice hold the sentinel
    before the call and must hold it afterwards.  data = None: an output (all sentinel)."""

    def __init__(self, dev, M, C, ld, off=0, data=None):
        self.M, self.C, self.ld, self.off = M, C, ld, off
        h = TC.sentinel((M, ld))
        if data is not None:
            h[:, off:off + C] = np.asarray(data, F32).reshape(M, C)
        self.buf = Buf(dev, M * ld, h)

    def ptr(self):
        return self.buf.ptr(self.off)

    def get(self):
        h = self.buf.get().reshape(self.M, self.ld)
        around = np.ones(self.ld, bool)
        around[self.off:self.off + self.C] = False
        assert (h[:, around] == TC.SENT).all(), 'write into the pitch padding or a neighbouring slice'
        return h[:, self.off:self.off + self.C].copy()


def _exact(words, ref, what):
    same = np.asarray(words).reshape(-1) == TC.bits(ref).reshape(-1)
    assert same.all(), (what, 'first differing elements', np.argwhere(~same)[:5].ravel().tolist())


# ------------------------------------------------------------------------------------------ max pool
def _run_pool(dev, case):
    name, B, H, W, C, ldx, offx, ldy, offy = case
    L, stream = _abi()
    x, dy = TC.pool_input(case)
    y_ref, code_ref = TC.pool_ref(x)
    Ho, Wo = H // 2, W // 2
    Mi, Mo = B * H * W, B * Ho * Wo
    xs = Rows(dev, Mi, C, ldx, offx, x)
    ys, ys2 = Rows(dev, Mo, C, ldy, offy), Rows(dev, Mo, C, ldy, offy)
    nidx = -(-Mo * C // 4)
    idx = Buf(dev, nidx)
    assert L.y4_maxpool2x2_s2_fwd_f32(xs.ptr(), ldx, ys.ptr(), ldy, idx.ptr(), B, H, W, C, stream()) == 0
    assert L.y4_maxpool2x2_s2_fwd_f32(xs.ptr(), ldx, ys2.ptr(), ldy, None, B, H, W, C, stream()) == 0      # inference: no codes
    dys = Rows(dev, Mo, C, ldy, offy, dy)
    dxs = Rows(dev, Mi, C, ldx, offx)
    none = Mo == 0
    assert L.y4_maxpool2x2_s2_bwd_f32(None if none else dys.ptr(), ldy, None if none else idx.ptr(), dxs.ptr(), ldx, B, H, W, C,
                                      stream()) == 0
    torch.cuda.synchronize()
    _exact(ys.get(), y_ref, name + ' values')
    _exact(ys2.get(), y_ref, name + ' values without idx')
    got_code = idx.get().view(np.int8)[:Mo * C].reshape(code_ref.shape)
    assert np.array_equal(got_code, code_ref), name
    _exact(dxs.get(), TC.pool_bwd_ref(dy, code_ref, H, W), name + ' dx')
    _exact(xs.get(), x, name + ' x untouched')


@pytest.mark.parametrize('case', TC.POOL_CASES, ids=lambda c: c[0])
def test_pool(dev, case):
    _run_pool(dev, case)


def test_pool_grid_stride(dev):
    assert TC.laps(65 * 65 * 128) == 2
    _run_pool(dev, TC.POOL_GRID_STRIDE)


def test_pool_refused_calls(dev):
    L, stream = _abi()
    base = dict(B=1, H=4, W=4, C=12, ldx=12, ldy=12, x=1, y=1, x_off=0, y_off=0)
    for what, over, rc in TC.pool_rejects():
        a = dict(base, **over)
        xs, ys = Buf(dev, 16 * 16 + 8), Buf(dev, 4 * 16 + 8)
        idx = Buf(dev, 64)
        xp = ctypes.c_void_p(xs.ptr().value + a['x_off']) if a['x'] else None
        yp = ctypes.c_void_p(ys.ptr().value + a['y_off']) if a['y'] else None
        assert L.y4_maxpool2x2_s2_fwd_f32(xp, a['ldx'], yp, a['ldy'], idx.ptr(), a['B'], a['H'], a['W'], a['C'], stream()) == rc, what
        # backward with the roles swapped: dy <- "y", dx <- "x"
        assert L.y4_maxpool2x2_s2_bwd_f32(yp, a['ldy'], idx.ptr(), xp, a['ldx'], a['B'], a['H'], a['W'], a['C'], stream()) == rc, what
        torch.cuda.synchronize()
        for b in (xs, ys, idx):
            assert (b.get() == TC.SENT).all(), what
    xs, ys, idx = Buf(dev, 256), Buf(dev, 64), Buf(dev, 64)
    assert L.y4_maxpool2x2_s2_bwd_f32(ys.ptr(), 12, None, xs.ptr(), 12, 1, 4, 4, 12, stream()) == TC.ERR_NULL       # idx is needed
    assert L.y4_maxpool2x2_s2_bwd_f32(ys.ptr(), 12, ctypes.c_void_p(idx.ptr().value + 1), xs.ptr(), 12, 1, 4, 4, 12, stream()) == TC.ERR_SHAPE
    assert L.y4_maxpool2x2_s2_fwd_f32(xs.ptr(), 12, ys.ptr(), 12, ctypes.c_void_p(idx.ptr().value + 2), 1, 4, 4, 12, stream()) == TC.ERR_SHAPE
    torch.cuda.synchronize()
    assert (xs.get() == TC.SENT).all() and (ys.get() == TC.SENT).all()


# ------------------------------------------------------------------------------------------ stem
def _x_layouts(dev, x):
    """(name, device tensor, element strides b, c, h, w) for the loader's NCHW image and an NHWC one"""
    B, _, H, W = x.shape
    nchw = torch.from_numpy(x).to(dev)
    nhwc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).to(dev)
    return [('nchw', nchw, (3 * H * W, H * W, W, 1)), ('nhwc', nhwc, (H * W * 3, 1, W * 3, 3))], nhwc


@pytest.mark.parametrize('case', TC.STEM_CASES, ids=str)
def test_stem_forward(dev, case):
    B, H, W, Cout = case
    L, stream = _abi()
    c = TC.stem_input(case)
    Ho, Wo = TC.out_hw(H, W)
    M = B * Ho * Wo
    w = torch.from_numpy(TC.krsc(c['w'])).to(dev)
    scale, shift = torch.from_numpy(c['scale']).to(dev), torch.from_numpy(c['shift']).to(dev)
    layouts, nhwc = _x_layouts(dev, c['x'])
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    worst = 0.0
    for ep, (sc, sh, act) in zip(TC.STEM_EPILOGUES, ((None, None, 0), (scale, shift, 1), (None, shift, 0))):
        y64, bound = TC.stem_fwd64(c['x'], c['w'], None if sc is None else c['scale'], None if sh is None else c['shift'], act)
        gen = Rows(dev, M, Cout, Cout)
        assert L.y4_conv2d_generic_fwd_f32(P(nhwc), 3, P(w), gen.ptr(), Cout, B, H, W, 3, Cout, 3, 2, P(sc), P(sh), act, None, 0,
                                           stream()) == 0
        for name, xt, st in layouts:
            for ld, off in ((Cout, 0), (Cout + 8, 4)):
                ys = Rows(dev, M, Cout, ld, off)
                assert L.y4_conv2d_stem_s2_fwd_f32(P(xt), *st, P(w), ys.ptr(), ld, B, H, W, Cout, P(sc), P(sh), act, stream()) == 0
                torch.cuda.synchronize()
                got = ys.get()
                assert np.array_equal(got, gen.get()), (case, ep, name, ld, 'differs from y4_conv2d_generic_fwd_f32')
                err = np.abs(got.view(F32).astype(F64).reshape(y64.shape) - y64)
                assert (err <= bound).all(), (case, ep, name, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
    print('stem forward %s: largest share of the bound used %.3f' % (case, worst))


def test_stem_forward_refused_calls(dev):
    L, stream = _abi()
    x, w, y = Buf(dev, 3 * 64), Buf(dev, 27 * 68), Buf(dev, 16 * 72)
    st = (192, 64, 8, 1)
    ok = dict(x=x.ptr(), w=w.ptr(), y=y.ptr(), ldy=32, Cout=32, act=0, st=st, B=1)
    for what, over, rc in (('x NULL', dict(x=None), TC.ERR_NULL), ('w NULL', dict(w=None), TC.ERR_NULL), ('y NULL', dict(y=None), TC.ERR_NULL),
                           ('Cout > 64', dict(Cout=68, ldy=68), TC.ERR_SHAPE), ('Cout % 4', dict(Cout=6), TC.ERR_SHAPE),
                           ('ldy < Cout', dict(ldy=28), TC.ERR_SHAPE), ('ldy % 4', dict(ldy=34), TC.ERR_SHAPE),
                           ('y misaligned', dict(y=y.ptr(1)), TC.ERR_SHAPE), ('act', dict(act=4), TC.ERR_SHAPE),
                           ('negative stride', dict(st=(192, 64, -8, 1)), TC.ERR_SHAPE), ('B = 0', dict(B=0), TC.ERR_SHAPE)):
        a = dict(ok, **over)
        assert L.y4_conv2d_stem_s2_fwd_f32(a['x'], *a['st'], a['w'], a['y'], a['ldy'], a['B'], 8, 8, a['Cout'], None, None, a['act'],
                                           stream()) == rc, what
    ws = Buf(dev, 27 * 32)
    assert L.y4_conv2d_stem_s2_wgrad_workspace(1, 8, 8, 32) == 27 * 32 * 4 and L.y4_conv2d_stem_s2_wgrad_workspace(1, 8, 8, 68) == 0
    dw = Buf(dev, 27 * 32)
    for what, args, rc in (('dw NULL', (x.ptr(), *st, y.ptr(), 32, None, 1, 8, 8, 32, ws.ptr(), 27 * 32 * 4), TC.ERR_NULL),
                           ('workspace NULL', (x.ptr(), *st, y.ptr(), 32, dw.ptr(), 1, 8, 8, 32, None, 27 * 32 * 4), TC.ERR_NULL),
                           ('workspace short', (x.ptr(), *st, y.ptr(), 32, dw.ptr(), 1, 8, 8, 32, ws.ptr(), 27 * 32 * 4 - 4), TC.ERR_WORKSPACE),
                           ('lddy < Cout', (x.ptr(), *st, y.ptr(), 28, dw.ptr(), 1, 8, 8, 32, ws.ptr(), 27 * 32 * 4), TC.ERR_SHAPE),
                           ('Cout = 68', (x.ptr(), *st, y.ptr(), 68, dw.ptr(), 1, 8, 8, 68, ws.ptr(), 27 * 32 * 4), TC.ERR_SHAPE)):
        assert L.y4_conv2d_stem_s2_wgrad_f32(*args, stream()) == rc, what
    torch.cuda.synchronize()
    for b in (x, w, y, ws, dw):
        assert (b.get() == TC.SENT).all()


def test_stem_dispatch(dev, monkeypatch):
    """3 -> Cout 3x3 stride 2 through ops.conv_fwd_raw / conv_wgrad_raw: Cout = 32 takes the new kernels (the same forward
    bits as with Y4_TINY_STEM=0), Cout = 68 and 6 stay on the direct kernels whatever the switch says"""
    from yolov4_amd import ops
    L, _ = _abi()
    calls = []
    for name in ('y4_conv2d_stem_s2_fwd_f32', 'y4_conv2d_stem_s2_wgrad_f32', 'y4_conv2d_generic_fwd_f32', 'y4_conv2d_generic_wgrad_f32'):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    x = recipe.randn((2, 3, 10, 12), 5).to(dev)
    for Cout, new in ((32, True), (64, True), (68, False), (6, False)):
        w = recipe.randn((Cout, 3, 3, 3), 6).to(dev).contiguous(memory_format=torch.channels_last)
        res = {}
        for on in (True, False):
            monkeypatch.setitem(ops._TINY_STEM, 'on', on)
            assert ops.tiny_stem_shape(3, Cout, 3, 2) == (on and new)
            del calls[:]
            y = ops.conv_fwd_raw(x, w, 3, 2, act='leaky_relu')
            dw = ops.conv_wgrad_raw(x, y, tuple(w.shape), 3, 2)
            torch.cuda.synchronize()
            want = ['y4_conv2d_stem_s2_fwd_f32', 'y4_conv2d_stem_s2_wgrad_f32'] if (on and new) else \
                ['y4_conv2d_generic_fwd_f32', 'y4_conv2d_generic_wgrad_f32']
            assert calls == want, (Cout, on, calls)
            res[on] = (y.cpu(), dw.cpu())
        assert torch.equal(res[True][0], res[False][0]) and res[True][0].shape == (2, Cout, 5, 6)
        assert torch.allclose(res[True][1], res[False][1], rtol=1e-4, atol=1e-4)
    assert not ops.tiny_stem_shape(3, 32, 3, 1) and not ops.tiny_stem_shape(4, 32, 3, 2) and not ops.tiny_stem_shape(3, 32, 1, 2)


@pytest.mark.parametrize('case', TC.STEM_CASES + [TC.STEM_WGRAD_MULTI_SLAB], ids=str)
def test_stem_wgrad(dev, case):
    B, H, W, Cout = case
    L, stream = _abi()
    c = TC.stem_input(case)
    Ho, Wo = TC.out_hw(H, W)
    M = B * Ho * Wo
    plan = TC.wgrad_plan(*case)
    nbytes = L.y4_conv2d_stem_s2_wgrad_workspace(B, H, W, Cout)
    assert nbytes == plan['workspace']
    dw64, S = TC.stem_wgrad64(c['x'], c['dy'])
    dw64, S = TC.krsc(dw64), TC.krsc(S)
    bound = (plan['L'] + 1) * TC.U * S + TC.TINY
    layouts, _ = _x_layouts(dev, c['x'])
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731
    first = None
    for name, xt, st in layouts:
        for ld, off in ((Cout, 0), (Cout + 8, 4)):
            dys = Rows(dev, M, Cout, ld, off, c['dy'])
            for rep in range(2):
                ws, dw = Buf(dev, nbytes // 4), Buf(dev, Cout * 27)
                assert L.y4_conv2d_stem_s2_wgrad_f32(P(xt), *st, dys.ptr(), ld, dw.ptr(), B, H, W, Cout, ws.ptr(), nbytes, stream()) == 0
                torch.cuda.synchronize()
                ws.get()
                got = dw.get()
                first = got if first is None else first
                assert np.array_equal(got, first), (case, name, ld, rep, 'not the same bits as the first run')
            err = np.abs(got.view(F32).astype(F64).reshape(dw64.shape) - dw64)
            assert (err <= bound).all(), (case, name, float((err / bound).max()))
    print('stem wgrad %s: L = %d, %d slab(s), largest share of the bound used %.3f' % (case, plan['L'], plan['blocks'],
                                                                                     float((err / bound).max())))


# ------------------------------------------------------------------------------------------ fork_half
@pytest.mark.parametrize('which', ['full', 'hi', 'both'])
def test_fork_half(dev, which, monkeypatch):
    from yolov4_amd import ops
    L, _ = _abi()
    launches = []
    real = L.y4_fork_half_bwd_f32
    monkeypatch.setattr(L, 'y4_fork_half_bwd_f32', lambda *a: (launches.append(1), real(*a))[1])
    monkeypatch.setattr(ops, 'add_raw', lambda *a: pytest.fail('fork_half backward went through add_raw'))
    B, C, H, W = 2, 24, 5, 3
    x0 = recipe.randn((B, C, H, W), 31)
    gf, gh = recipe.randn((B, C, H, W), 32), recipe.randn((B, C // 2, H, W), 33)
    xc = x0.clone().requires_grad_(True)
    loss = 0
    if which in ('full', 'both'):
        loss = loss + (xc * gf).sum()
    if which in ('hi', 'both'):
        loss = loss + (xc[:, C // 2:] * gh).sum()
    loss.backward()
    x = x0.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    a, b = ops.fork_half(x)
    assert a.shape == x.shape and b.shape == (B, C // 2, H, W)
    assert a.data_ptr() == x.data_ptr() and b.data_ptr() == x.data_ptr() + 4 * (C // 2)      # views: no copy
    assert ops.nhwc_pitch(b) == C
    assert torch.equal(b.detach().cpu(), x0[:, C // 2:])
    loss = 0
    if which in ('full', 'both'):
        loss = loss + (a * gf.to(dev)).sum()
    if which in ('hi', 'both'):
        loss = loss + (b * gh.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert len(launches) == (0 if which == 'full' else 1)
    assert np.array_equal(TC.bits(x.grad.cpu().numpy()), TC.bits(xc.grad.numpy()))
    with torch.no_grad():
        a2, b2 = ops.fork_half(x)
    assert a2 is x and b2.data_ptr() == b.data_ptr()
    with pytest.raises(ops.Y4Error):
        ops.fork_half(torch.zeros(1, 12, 2, 2, device=dev))


def test_fork_half_refused_calls(dev):
    L, stream = _abi()
    g, h, d = Buf(dev, 64), Buf(dev, 32), Buf(dev, 64)
    ok = (g.ptr(), 16, h.ptr(), 8, d.ptr(), 16, 4, 16)
    for what, i, v, rc in (('dx NULL', 4, None, TC.ERR_NULL), ('C % 8', 7, 12, TC.ERR_SHAPE), ('M = 0', 6, 0, TC.ERR_SHAPE),
                           ('ldh < C / 2', 3, 4, TC.ERR_SHAPE), ('g_hi misaligned', 2, h.ptr(1), TC.ERR_SHAPE)):
        args = list(ok)
        args[i] = v
        assert L.y4_fork_half_bwd_f32(*args, stream()) == rc, what
    assert L.y4_fork_half_bwd_f32(None, 0, None, 0, d.ptr(), 16, 4, 16, stream()) == TC.ERR_NULL
    torch.cuda.synchronize()
    assert (d.get() == TC.SENT).all()


def test_maxpool2x2_op(dev):
    """ops.maxpool2x2 under autograd: torch's values and gradient; idx only when the input needs a gradient; into a slot"""
    from yolov4_amd import ops
    x0 = recipe.randn((2, 8, 7, 6), 41)
    xc = x0.clone().requires_grad_(True)
    yc = torch.nn.functional.max_pool2d(xc, 2, 2)
    g = recipe.randn(tuple(yc.shape), 42)
    yc.backward(g)
    x = x0.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.maxpool2x2(x)
    y.backward(g.to(dev))
    assert torch.equal(y.detach().cpu(), yc.detach()) and torch.equal(x.grad.cpu(), xc.grad)
    cb = ops.cat_buffer(y, [8, 8])
    with torch.no_grad():
        z = ops.maxpool2x2(x.detach(), out=cb.slot(1))
    assert z.data_ptr() == cb.slot(1).data_ptr() and torch.equal(cb.buf[:, 8:].cpu(), yc.detach())


# ------------------------------------------------------------------------------------------ the model
MODES = ['default', 'f32']


def _cpu_sd(model):
    return {k: v.detach().cpu().clone(memory_format=torch.contiguous_format) for k, v in model.state_dict().items()}


def _fresh(dev):
    from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
    model = YOLOv4Tiny(default_cfg())
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, TC.MODEL_SEED)
    model.load_state_dict(sd)
    return model, _cpu_sd(model)


@pytest.fixture(scope='module')
def oracle():
    """per model case, computed once: the fp32 and fp64 oracle's train step"""
    out = {}
    for case in TC.MODEL_CASES:
        from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
        sd = YOLOv4Tiny(default_cfg()).state_dict()
        recipe.fill_state_dict_(sd, TC.MODEL_SEED)
        x, labels = TC.model_input(case)
        out[case] = {dt: TC.tiny_oracle(sd, x, dt, True, labels) for dt in (torch.float32, torch.float64)}
    return out


@pytest.fixture(scope='module')
def runs(dev):
    import yolov4_amd
    from yolov4_amd import ops
    from yolov4_amd.yolo.model.build import build_criterion
    out = {}
    old = yolov4_amd.get_conv_mode()
    for case in TC.MODEL_CASES:
        B, S = case
        x, labels = TC.model_input(case)
        for mode in MODES:
            if mode != 'default':
                yolov4_amd.set_conv_mode(mode)
            try:
                r = {}
                model, sd0 = _fresh(dev)
                model = model.to(dev).train()
                crit = build_criterion(TC.full_cfg(S), device=dev)
                copies, repacks = [], []
                real_copy, real_nhwc = ops.copy_into_raw, ops.as_nhwc

                def counting_nhwc(t, *a, **k):
                    got = real_nhwc(t, *a, **k)
                    if got[0] is not t:
                        repacks.append(tuple(t.shape))
                    return got
                ops.copy_into_raw = lambda s, d: (copies.append(tuple(s.shape)), real_copy(s, d))[1]
                ops.as_nhwc = counting_nhwc
                try:
                    outs = model(x.to(dev))
                    loss = crit(outs, {'padded_labels': labels.to(dev)})
                    loss.backward()
                    torch.cuda.synchronize()
                finally:
                    ops.copy_into_raw, ops.as_nhwc = real_copy, real_nhwc
                r['copies'], r['repacks'] = copies, repacks
                r['layers'] = [(o['layer_no'], tuple(o['output'].shape), tuple(o['pred'].shape)) for o in outs]
                r['loss'] = float(loss.detach())
                r['grads'] = {k: p.grad.detach().cpu().numpy().astype(F64) for k, p in model.named_parameters()}
                # the head logits of a second, hook-free forward of the same weights and statistics
                model.load_state_dict(sd0)
                with torch.no_grad():
                    lg = model.head.logits(*model.neck(*model.backbone(x.to(dev))))
                r['logits'] = [t.cpu().numpy().astype(F64) for t in lg]
                # eval on calibrated statistics: both sides use the HIP model's running statistics
                model.load_state_dict(sd0)
                recipe.calibrate_bn_(model, recipe.randn((4, 3, S, S), 3).to(dev))
                model.eval()
                with torch.no_grad():
                    r['eval'] = model(x.to(dev)).cpu().numpy()
                sd1 = _cpu_sd(model)
                r['eval32'] = TC.tiny_oracle(sd1, x, torch.float32, False).astype(F64)
                r['eval64'] = TC.tiny_oracle(sd1, x, torch.float64, False)
                out[(case, mode)] = r
            finally:
                yolov4_amd.set_conv_mode(old)
    return out


CASE_MODES = [(c, m) for c in TC.MODEL_CASES for m in MODES]


@pytest.mark.parametrize('case, mode', CASE_MODES, ids=str)
def test_model_train_step_against_tiny_oracle(runs, oracle, case, mode):
    """error versus fp64 at most max(floor, 1.5 x the fp32 oracle's own distance from fp64): floors loss relative 1e-4,
    gradients 1e-3 of the tensor's maximum, logits absolute 1e-4 (scaled by the tensor's magnitude)

    Measured on an MI355X: logits 2e-7 .. 6e-7, loss 6e-8 .. 7e-8, gradients 1e-8 .. 1.4e-5 of the maximum in all four cases.
    The images are the first well-conditioned ones (tiny_cases.MODEL_INPUT_SEEDS): on seed 596 at S = 96, where one window of
    block 3's pool holds candidates 5.98e-6 apart (a third of the local fp32 error), the 'f32' run selected the other
    element than the fp64 oracle and backbone.block3.conv1's filter gradient came out 5.9e-2 of its maximum away -- the
    layer's dgrad, wgrad and BatchNorm backward agreeing with fp64 to 2e-6, 3e-7 and 5e-9 on the operands of that run."""
    B, S = case
    r, o32, o64 = runs[(case, mode)], oracle[case][torch.float32], oracle[case][torch.float64]
    assert r['layers'] == [(0, (B, 3, S // 16, S // 16, 85), (B, 3, S // 16, S // 16, 4)),
                           (1, (B, 3, S // 32, S // 32, 85), (B, 3, S // 32, S // 32, 4))]
    for i, (got, a, b) in enumerate(zip(r['logits'], o32['logits'], o64['logits'])):
        s = max(1.0, np.abs(b).max())
        e, ref = np.abs(got - b).max() / s, np.abs(a - b).max() / s
        print('%s %s: logits[%d] err %.2e (fp32 oracle %.2e)' % (case, mode, i, e, ref))
        assert got.shape == b.shape and TC.within(e, ref, 1e-4)
    e, ref = abs(r['loss'] - o64['loss']) / abs(o64['loss']), abs(o32['loss'] - o64['loss']) / abs(o64['loss'])
    print('%s %s: loss %.6f, rel err %.2e (fp32 oracle %.2e)' % (case, mode, r['loss'], e, ref))
    assert np.isfinite(r['loss']) and TC.within(e, ref, 1e-4)
    assert sorted(r['grads']) == sorted(o64['grads'])
    bad = []
    for k, g64 in o64['grads'].items():
        top = np.abs(g64).max()
        e, ref = np.abs(r['grads'][k] - g64).max() / top, np.abs(o32['grads'][k] - g64).max() / top
        print('%s %s: grad %s err %.2e of max (fp32 oracle %.2e)' % (case, mode, k, e, ref))
        if not (r['grads'][k].shape == g64.shape and TC.within(e, ref, 1e-3)):
            bad.append((k, e, ref))
    assert not bad, bad


@pytest.mark.parametrize('case, mode', CASE_MODES, ids=str)
def test_model_eval_against_tiny_oracle(runs, case, mode):
    B, S = case
    r = runs[(case, mode)]
    s = max(1.0, np.abs(r['eval64']).max())
    e, ref = np.abs(r['eval'] - r['eval64']).max() / s, np.abs(r['eval32'] - r['eval64']).max() / s
    print('%s %s: eval err %.2e (fp32 oracle %.2e)' % (case, mode, e, ref))
    assert r['eval'].shape == (B, 3 * (S // 16) ** 2 + 3 * (S // 32) ** 2, 85)
    assert np.isfinite(r['eval']).all() and TC.within(e, ref, 1e-4)


@pytest.mark.parametrize('case, mode', CASE_MODES, ids=str)
def test_no_copy_kernel_for_the_concats(runs, case, mode):
    """forward + backward: no y4_copy_channels_f32 launch (every concat input was produced in place) and no layout repack"""
    r = runs[(case, mode)]
    assert r['copies'] == [] and r['repacks'] == []


# ------------------------------------------------------------------------------------------ end to end at S = 64
def test_end_to_end(dev, tmp_path):
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.engine.build import train_step, validate
    from yolov4_amd.yolo.model.build import build_criterion, build_model
    from yolov4_amd.yolo.optim.optimizers.build import FusedAdam
    from yolov4_amd.yolo.util.darknet_weights import load_darknet_weights, save_darknet_weights
    S = 64
    cfg = dict(TC.full_cfg(S), TRAIN={'ACCUMULATION_STEPS': 1}, LR_SCHEDULER={'IS_WARMUP': False, 'WARMUP_EPOCH': 0})
    model = build_model(argparse.Namespace(), cfg, device=dev)
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 9)
    model.load_state_dict(sd)
    model.train()
    crit = build_criterion(cfg, device=dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    x, labels = TC.model_input((2, S))
    loss = train_step(cfg, model, crit, opt, x, {'padded_labels': labels}, device=dev)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    for k, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k + ' did not move'
        assert bool(torch.isfinite(p).all()), k
    recipe.calibrate_bn_(model, recipe.randn((4, 3, S, S), 3).to(dev))
    info = torch.tensor([[48., 64., S, S, 17., 0.], [33., 50., S, S, 42., 0.]])
    loader = [(recipe.rand((2, 3, S, S), 4 + i), {'img_info': info}) for i in range(2)]
    validate(loader, model, 0.05, 0.4, device=dev)
    for rec in validate.records:
        assert rec['image_id'] in (17, 42) and len(rec['bbox']) == 4 and np.isfinite(rec['bbox']).all() and np.isfinite(rec['score'])
    img = (recipe.rand((48, 64, 3), 6) * 255).to(torch.uint8).to(dev)
    res = detect_images(model, cfg, [img, img], conf_thre=0.05, encode=False, batch=2)
    assert len(res) == 2 and res[0]['image'].shape == (48, 64, 3) and res[0]['detections'].shape[1] == 7
    assert np.array_equal(res[0]['detections'], res[1]['detections'])
    # Darknet weights: saved and loaded into a fresh model, the eval output is the same in every bit
    path = str(tmp_path / 'tiny.weights')
    assert save_darknet_weights(model, path) == 21
    other = build_model(argparse.Namespace(), cfg, device=dev)
    assert load_darknet_weights(other, path) == 21
    model.eval(), other.eval()
    with torch.no_grad():
        a, b = model(x.to(dev)), other(x.to(dev))
    assert a.shape == (2, 3 * 16 + 3 * 4, 85) and np.array_equal(TC.bits(a.cpu().numpy()), TC.bits(b.cpu().numpy()))
