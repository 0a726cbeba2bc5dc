# -*- coding: utf-8 -*-
"""The plane conv kernels of csrc/conv_planes.hip -- the forward tile kernel in its three shapes, the bf16 streaming 1x1
kernel, dgrad (stride 1, and the four parity classes of stride 2), wgrad with its split-K plan, and the two split kernels --
each driven through the C ABI at the sizes where the host picks another kernel or a kernel takes another branch: row
counts around one tile, column counts that are no multiple of the tile, pitched results, a bias, a pitched skip operand,
bf16 results, 131072 rows (the streaming threshold) and 1025 tiles on 512 persistent blocks.

The operands are built on the host (tests/conv_cases.py) exactly as the kernels read them, the references are fp64 sums
over the decoded operands, and every element is judged by its own bound; tests/test_conv_cases.py shows, without a GPU,
that every case reaches the branch it is listed for.  Every output buffer is filled with a NaN bit pattern no kernel
produces: pitch padding, the rows behind M, the second half of bf16 result rows and a guard around every buffer must
still hold it afterwards.  The kernel name is asserted after each call."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import bn_cases as BC
import conv_cases as CC

pytestmark = pytest.mark.gpu
F32 = np.float32
G = 32                                   # guard words (128 B) in front of and behind every device buffer
USED = {}                                # group -> largest share of its bound used so far (printed per test)
MODE_IDS = {'f16x2': (3, 0), 'bf16': (2, 0), 'hybrid': (3, 1)}      # conv mode, y4_set_planes_bf16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    v = os.environ.get('Y4_BF_STREAM')
    assert v is None or int(v) != 0, 'Y4_BF_STREAM=0 switches the bf16 streaming kernel off for the whole process: unset it'
    assert os.environ.get('Y4_PLANES_SMALL') is None and os.environ.get('Y4_BF_WGRAD_2CU') is None, 'experiment switches are set'
    return torch.device('cuda:0')


@pytest.fixture()
def mode(dev):
    """set_mode('f16x2' | 'bf16' | 'hybrid'); the conv mode and the plane flag are restored afterwards"""
    L = _abi()[0]
    old = (L.y4_get_conv_mode(), L.y4_get_planes_bf16())

    def set_mode(name):
        m, flag = MODE_IDS[name]
        assert L.y4_set_conv_mode(m) == 0 and L.y4_set_planes_bf16(flag) == 0
        return CC.is_bf(name)
    yield set_mode
    L.y4_set_conv_mode(old[0])
    L.y4_set_planes_bf16(old[1])


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import lib
    return lib(), ops._stream, ops.last_conv_kernel


class Buf(object):
    """n 32-bit words on the device between two guards; everything starts as the sentinel unless `init` is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        if init is None:
            self.t = torch.full((self.n + 2 * G,), BC.SENT, dtype=torch.int32, device=dev)
        else:
            h = np.full(self.n + 2 * G, BC.SENT, dtype=np.uint32)
            h[G:G + self.n] = np.ascontiguousarray(init).view(np.uint32).ravel()
            self.t = torch.from_numpy(h.view(np.int32)).to(dev)

    def ptr(self, off_bytes=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * G + off_bytes)

    def get(self):
        """the body as uint32 words; the guards must be untouched"""
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:G] == BC.SENT).all() and (h[G + self.n:] == BC.SENT).all(), 'write outside the buffer'
        return h[G:G + self.n].copy()


def _f32(words):
    return np.ascontiguousarray(words).view(F32)


def _note(group, used, what=''):
    """print the share of its bound a check used and keep the group's maximum"""
    m = float(np.max(used)) if np.size(used) else 0.0
    USED[group] = max(USED.get(group, 0.0), m)
    print('%s %s: share of the bound used %.3g; group maximum so far %.3g' % (group, what, m, USED[group]))


def _worst(ok, got, r, bf, ybf=False):
    bound = CC.conv_bound(r, bf, ybf)[0]
    got = np.asarray(got).reshape(r['y'].shape)
    return [(tuple(i), float(got[tuple(i)]), float(r['y'][tuple(i)]), float(np.broadcast_to(bound, r['y'].shape)[tuple(i)]))
            for i in np.argwhere(~ok)[:5]]


def _word(dev, word):
    return Buf(dev, 1, np.array([word], dtype=np.uint32)) if word is not None else None


def _p(buf):
    return buf.ptr() if buf is not None else None


def _rows(body, M, ld, width, what):
    """the first `width` words of the first M rows of a sentinel-filled [rows, ld] buffer; the rest must hold the sentinel"""
    body = body.reshape(-1, ld)
    assert (body[M:] == BC.SENT).all(), what + ': write behind row M'
    assert (body[:M, width:] == BC.SENT).all(), what + ': write into the pitch padding / the second half of a bf16 row'
    return np.ascontiguousarray(body[:M, :width])


# ------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=1)
def _fwd_inputs(B, H, W, Cin, Cout, k, s, bf, bias):
    seed = CC.seed_of(B, H, W, Cin, Cout, k, s)
    x = CC.make_values(B * H * W, Cin, seed, spread=2)
    w = CC.make_filter(Cout, k, Cin, seed + 1)
    b = CC.make_values(1, Cout, seed + 2, spread=10)[0] if bias else None
    xa = CC.act_planes(x, bf)
    r = CC.fwd_ref(xa['dec'].reshape(B, H, W, Cin), w, k, s, bf, b)
    return xa, w, b, r


def _run_fwd(dev, c, xa, w, bias, dgrad_filter=None, y_off=0, bias_off=0, ws_short=0, ldy=None, partials=None, y_bf16=None):
    """one y4_conv2d_fwd_planes_f32 call of case c -> dict(rc, kernel, y [M, Cout] as stored (fp32 values), nparts, part)"""
    L, stream, last = _abi()
    bf = CC.is_bf(c['mode'])
    B, H, W, Cin, Cout, k, s = (c[t] for t in ('B', 'H', 'W', 'Cin', 'Cout', 'k', 's'))
    M = CC.fwd_dims(c)[0]
    ldy = c['Cout'] + c['ldy_pad'] if ldy is None else ldy
    partials = c['partials'] if partials is None else partials
    y_bf16 = c['y_bf16'] if y_bf16 is None else y_bf16
    xd = Buf(dev, xa['words'].size, xa['words'])
    wd = Buf(dev, w.size, w)
    bd = Buf(dev, Cout, bias) if bias is not None else None
    yd = Buf(dev, (M + 2) * max(ldy, Cout))
    ad = _word(dev, xa['word'])
    nws = L.y4_conv2d_fwd_workspace(Cin, Cout, k)
    assert nws == CC.fwd_workspace(Cin, Cout, k)
    ws = Buf(dev, CC.cdiv(nws, 4))
    pwords = CC.cdiv(M, 128) * 2 * Cout
    pd = Buf(dev, pwords) if partials else None
    n = ctypes.c_longlong(-1)
    rc = L.y4_conv2d_fwd_planes_f32(xd.ptr(), wd.ptr(), yd.ptr(y_off), ldy, B, H, W, Cin, Cout, k, s, _p(pd), 4 * pwords if partials else 0,
                                    ctypes.byref(n), _p(ad), ws.ptr(), nws - ws_short, _p(dgrad_filter),
                                    4 * dgrad_filter.n if dgrad_filter is not None else 0, 1 if y_bf16 else 0,
                                    bd.ptr(bias_off) if bd is not None else None, stream())
    torch.cuda.synchronize()
    ws.get()
    out = dict(rc=rc, kernel=last(), nparts=n.value, raw=yd.get())
    if rc == 0:
        what = CC.case_id(c)
        if y_bf16:
            body = _rows(out['raw'], M, ldy, Cout // 2, what)
            out['y'] = BC.bf16_to_f32(body.view(np.uint16).reshape(M, Cout))
        else:
            out['y'] = _f32(_rows(out['raw'], M, ldy, Cout, what))
        if partials:
            p = pd.get()
            assert (p[n.value * 2 * Cout:] == BC.SENT).all(), what + ': write behind the last partial row'
            out['part'] = _f32(p[:n.value * 2 * Cout]).reshape(n.value, 2, Cout)
    return out


def _check_fwd(dev, c):
    bf = CC.is_bf(c['mode'])
    xa, w, b, r = _fwd_inputs(c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['k'], c['s'], bf, c['bias'])
    assert CC.left_out(r, bf, c['y_bf16']) <= CC.LEFT_OUT_CAP
    name, nparts, rows = CC.fwd_kernel(c)
    o = _run_fwd(dev, c, xa, w, b)
    what = CC.case_id(c)
    assert o['rc'] == 0, what
    group = 'fwd.%s.%s%s' % ('bf16' if bf else 'f16x2', c['want'], '.ybf' if c['y_bf16'] else '')
    ok, used = CC.conv_accept(o['y'], r, bf, c['y_bf16'])
    _note(group, used, what)
    assert ok.all(), (what, o['kernel'], _worst(ok, o['y'], r, bf, c['y_bf16']))
    assert o['kernel'] == name and CC.tag(name) == c['want'], (what, o['kernel'], name)
    assert o['nparts'] == nparts, (what, o['nparts'], nparts)
    if c['partials']:
        ok, used = CC.colsum_accept(o['part'], o['y'], rows)
        _note(group + '.colsum', used, what)
        assert ok.all(), (what, np.argwhere(~ok)[:5])
    return o


@pytest.mark.parametrize('m', ('f16x2', 'bf16'))
def test_forward_rows_and_columns_against_the_128_row_tile(dev, mode, m):
    """1x1, Cin = 64: M in {1, 127, 128, 129, 257} x N in {4, 36, 128, 132, 192}; the pitch (Cout, Cout + 4), the partial
    rows, a bias and (bf16) a bf16 result take turns over the grid"""
    mode(m)
    for c in CC.FWD_GRID[m]:
        _check_fwd(dev, c)


@pytest.mark.parametrize('c', CC.FWD_CASES, ids=CC.case_id)
def test_forward_tile_shapes(dev, mode, c, monkeypatch):
    """the 256-row shape by natural dispatch (32769 rows, K > 256), bf16 256 x 256 forced and natural, 3 x 3 at stride 1 and 2
    on odd and even maps whose tiles span images, the hybrid mode"""
    mode(c['mode'])
    if c['bf_tile']:
        monkeypatch.setenv('Y4_BF_TILE', str(c['bf_tile']))
    _check_fwd(dev, c)


@pytest.mark.parametrize('c', CC.STREAM_CASES, ids=CC.case_id)
def test_forward_streaming_kernel_and_its_threshold(dev, mode, c):
    """131071 rows stay on the tile kernel, 131072 stream; 131072 + 37 rows are 1025 tiles on 512 persistent blocks (three
    tiles on one block, two on the others, the last tile 37 rows); Cs in {64, 128}, NT = 1, 2, 4; fp32 and bf16 results with
    partial rows (one per block).  A BIAS (one row for every pixel) is not a skip operand the streaming epilogue can
    address: such a call must come back with the bias added -- from the tile kernel."""
    mode(c['mode'])
    _check_fwd(dev, c)


def test_forward_pitch_changes_no_arithmetic_and_bf16_result_is_rne_of_the_fp32_result(dev, mode):
    for m, Cin in (('f16x2', 32), ('bf16', 64)):
        bf = mode(m)
        c = CC._fc('pitch', m, 3, 7, 9, Cin, 64, 3, 1, 'tile128x128', partials=True)
        xa, w, _, r = _fwd_inputs(3, 7, 9, Cin, 64, 3, 1, bf, False)
        a = _run_fwd(dev, c, xa, w, None)
        b = _run_fwd(dev, c, xa, w, None, ldy=64 + 4, partials=False)
        assert a['rc'] == 0 and b['rc'] == 0 and np.array_equal(a['y'].view(np.uint32), b['y'].view(np.uint32))
        if bf:
            y = _run_fwd(dev, c, xa, w, None, y_bf16=True)
            assert y['rc'] == 0 and np.array_equal(BC.bf16_rne(y['y']), BC.bf16_rne(a['y']))
            assert np.array_equal(y['y'], BC.bf16_to_f32(BC.bf16_rne(a['y'])))


def test_forward_refused_calls_leave_the_result_alone(dev, mode):
    """bias with partial rows, bias with a bf16 result, a misaligned y / bias, a workspace one byte short, ldy < Cout: the
    documented status, and y still holds the sentinel"""
    for m, Cin in (('f16x2', 32), ('bf16', 64)):
        bf = mode(m)
        c = CC._fc('refused', m, 1, 3, 5, Cin, 64, 1, 1, 'tile128x128')
        xa, w, b, r = _fwd_inputs(1, 3, 5, Cin, 64, 1, 1, bf, True)
        for kw, want in ((dict(partials=True), BC.ERR_SHAPE), (dict(y_bf16=True), BC.ERR_SHAPE), (dict(y_off=4), BC.ERR_SHAPE),
                         (dict(bias_off=2), BC.ERR_SHAPE), (dict(ws_short=1), BC.ERR_WORKSPACE), (dict(ldy=60), BC.ERR_SHAPE),
                         (dict(ldy=66), BC.ERR_SHAPE)):
            o = _run_fwd(dev, c, xa, w, b, **kw)
            assert o['rc'] == want, (m, kw, o['rc'])
            assert (o['raw'] == BC.SENT).all(), (m, kw)
        o = _run_fwd(dev, c, xa, w, b)                                   # the same call, valid
        assert o['rc'] == 0
        ok, _ = CC.conv_accept(o['y'], r, bf)
        assert ok.all()
        if not bf:                                                       # f16x2 planes without their amax word
            xa2 = dict(xa, word=None)
            o = _run_fwd(dev, c, xa2, w, b)
            assert o['rc'] == BC.ERR_NULL and (o['raw'] == BC.SENT).all()


@pytest.mark.parametrize('m', ('f16x2', 'bf16'))
def test_forward_nonfinite_input_stays_inside_its_receptive_field(dev, mode, m):
    """one NaN and one +Inf in x (3 x 3, stride 1): the outputs whose window contains one are non-finite.  bf16: every other
    output meets its bound.  f16x2: a non-finite tensor poisons its amax word (the scale falls back to 1), so only `finite
    elsewhere` is asserted"""
    bf = mode(m)
    B, H, W, Cin, Cout, k = 2, 6, 7, 64, 36, 3
    seed = CC.seed_of(B, H, W, 99)
    x = CC.make_values(B * H * W, Cin, seed, spread=2).reshape(B, H, W, Cin)
    w = CC.make_filter(Cout, k, Cin, seed + 1, spread=2)
    sites = ((0, 2, 3, 5, np.nan), (1, 5, 0, 40, np.inf))
    hit = np.zeros((B, H, W), dtype=bool)
    clean = x.copy()
    for b, h, ww, ch, val in sites:
        x[b, h, ww, ch] = val
        clean[b, h, ww, ch] = 0
        hit[b, max(h - 1, 0):h + 2, max(ww - 1, 0):ww + 2] = True
    if bf:
        xa = CC.act_bf16(x.reshape(-1, Cin))
    else:
        xa = CC.act_f16x2(x.reshape(-1, Cin), word=0x7fc00000)
    c = CC._fc('nonfinite', m, B, H, W, Cin, Cout, k, 1, 'tile128x128')
    o = _run_fwd(dev, c, xa, w, None)
    assert o['rc'] == 0
    y = o['y'].reshape(B, H, W, Cout)
    assert not np.isfinite(y[hit]).any() and np.isfinite(y[~hit]).all()
    if bf:
        r = CC.fwd_ref(CC.act_bf16(clean.reshape(-1, Cin))['dec'].reshape(B, H, W, Cin), w, k, 1, True)
        ok, used = CC.conv_accept(y, r, True)
        _note('fwd.bf16.nonfinite', used[~hit])
        assert ok[~hit].all()


# ------------------------------------------------------------------------------------------ dgrad
@functools.lru_cache(maxsize=1)
def _dgrad_inputs(B, H, W, Cin, Cout, k, s, bf, res):
    seed = CC.seed_of(B, H, W, Cin, Cout, k, s, 7)
    Ho, Wo = CC.out_hw(H, W, k, s)
    dy = CC.make_values(B * Ho * Wo, Cout, seed, spread=2)
    w = CC.make_filter(Cout, k, Cin, seed + 1, axis=3)
    rs = CC.make_values(B * H * W, Cin, seed + 2, spread=10) if res else None
    da = CC.act_planes(dy, bf)
    r = CC.dgrad_ref(da['dec'].reshape(B, Ho, Wo, Cout), w, k, s, H, W, bf, rs.reshape(B, H, W, Cin) if res else None)
    return da, w, rs, r


def _run_dgrad(dev, c, da, w, res, prepared=None, ws_short=0):
    L, stream, last = _abi()
    B, H, W, Cin, Cout, k, s = (c[t] for t in ('B', 'H', 'W', 'Cin', 'Cout', 'k', 's'))
    M = B * H * W
    lddx, ldr = Cin + c['lddx_pad'], Cin + c['ldr_pad']
    dyd = Buf(dev, da['words'].size, da['words'])
    wd = Buf(dev, w.size, w) if prepared is None else None
    rd = Buf(dev, M * ldr, BC.pad_rows(res, ldr)) if res is not None else None
    dxd = Buf(dev, (M + 2) * lddx)
    ad = _word(dev, da['word'])
    nws = L.y4_conv2d_dgrad_workspace(Cin, Cout, k)
    assert nws == CC.dgrad_workspace(Cin, Cout, k)
    ws = Buf(dev, CC.cdiv(nws, 4)) if prepared is None else prepared
    rc = L.y4_conv2d_dgrad_planes_f32(dyd.ptr(), _p(wd), dxd.ptr(), lddx, B, H, W, Cin, Cout, k, s, ws.ptr(), nws - ws_short, _p(ad),
                                      _p(rd), ldr if res is not None else 0, stream())
    torch.cuda.synchronize()
    ws.get()
    out = dict(rc=rc, kernel=last(), raw=dxd.get())
    if rc == 0:
        out['dx'] = _f32(_rows(out['raw'], M, lddx, Cin, CC.case_id(c)))
    return out


@pytest.mark.parametrize('c', CC.DGRAD_CASES, ids=CC.case_id)
def test_dgrad(dev, mode, c):
    """stride 1 with and without a skip operand at pitches ldr > Cin, lddx > Cin, on the 128-row, the 256-row and (bf16, 131072
    rows and more) the streaming kernel; stride 2: the four parity classes on a map of one pixel per class, on 4 x 6 and on
    class grids of two ragged tiles by two column tiles"""
    bf = mode(c['mode'])
    da, w, rs, r = _dgrad_inputs(c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['k'], c['s'], bf, c['res'])
    assert CC.left_out(r, bf) <= CC.LEFT_OUT_CAP
    o = _run_dgrad(dev, c, da, w, rs)
    what = CC.case_id(c)
    assert o['rc'] == 0, what
    assert o['kernel'] == CC.dgrad_kernel(c) and CC.tag(o['kernel']) == c['want'], (what, o['kernel'])
    ok, used = CC.conv_accept(o['dx'], r, bf)
    _note('dgrad.%s.%s' % ('bf16' if bf else 'f16x2', c['want']), used, what)
    assert ok.all(), (what, _worst(ok, o['dx'], r, bf))
    if c['name'] in ('k3', 's2-4x6'):                                    # a workspace one byte short; a residual at stride 2
        o = _run_dgrad(dev, c, da, w, rs, ws_short=1)
        assert o['rc'] == BC.ERR_WORKSPACE and (o['raw'] == BC.SENT).all()
    if c['name'] == 's2-4x6':
        o = _run_dgrad(dev, c, da, w, np.zeros((c['B'] * c['H'] * c['W'], c['Cin']), F32))
        assert o['rc'] == BC.ERR_SHAPE and (o['raw'] == BC.SENT).all()


@pytest.mark.parametrize('m', ('f16x2', 'bf16'))
@pytest.mark.parametrize('s', (1, 2))
def test_dgrad_on_the_filter_the_forward_call_prepared(dev, mode, m, s):
    """w == NULL with the workspace filled by y4_conv2d_fwd_planes_f32 (dgrad_filter): bit-equal to the call that splits the
    filter itself, and under the bound"""
    bf = mode(m)
    L = _abi()[0]
    c = CC._dc('prepared', m, 2, 4, 6, 64, 64, 3, s, '')
    da, w, _, r = _dgrad_inputs(2, 4, 6, 64, 64, 3, s, bf, False)
    own = _run_dgrad(dev, c, da, w, None)
    fc = CC._fc('prepare', m, 1, 2, 2, 64, 64, 3, s, '')
    xa = CC.act_planes(CC.make_values(4, 64, 5), bf)
    prep = Buf(dev, CC.cdiv(L.y4_conv2d_dgrad_workspace(64, 64, 3), 4))
    f = _run_fwd(dev, fc, xa, w, None, dgrad_filter=prep)
    assert f['rc'] == 0
    o = _run_dgrad(dev, c, da, w, None, prepared=prep)
    assert own['rc'] == 0 and o['rc'] == 0 and o['kernel'] == own['kernel']
    assert np.array_equal(o['dx'].view(np.uint32), own['dx'].view(np.uint32))
    ok, used = CC.conv_accept(o['dx'], r, bf)
    _note('dgrad.prepared', used, '%s stride %d' % (m, s))
    assert ok.all()


# ------------------------------------------------------------------------------------------ wgrad
def _run_wgrad(dev, c, xa, da, ws_short=0):
    L, stream, last = _abi()
    B, H, W, Cin, Cout, k, s = (c[t] for t in ('B', 'H', 'W', 'Cin', 'Cout', 'k', 's'))
    xd = Buf(dev, xa['words'].size, xa['words'])
    dyd = Buf(dev, da['words'].size, da['words'])
    dwd = Buf(dev, Cout * k * k * Cin)
    nws = L.y4_conv2d_wgrad_planes_workspace(B, H, W, Cin, Cout, k, s)
    if not c['tile']:
        assert nws == CC.wgrad_workspace(B, H, W, Cin, Cout, k, s)
    ws = Buf(dev, CC.cdiv(nws, 4))
    xw, dw_ = _word(dev, xa['word']), _word(dev, da['word'])
    rc = L.y4_conv2d_wgrad_planes_f32(xd.ptr(), dyd.ptr(), dwd.ptr(), B, H, W, Cin, Cout, k, s, ws.ptr(), nws - ws_short,
                                      _p(xw), _p(dw_), stream())
    torch.cuda.synchronize()
    ws.get()
    return dict(rc=rc, kernel=last(), dw=dwd.get())


@pytest.mark.parametrize('c', CC.WGRAD_CASES, ids=CC.case_id)
def test_wgrad(dev, mode, c, monkeypatch):
    """one split and several, J = k k Cin over one and two 256-wide j tiles, Cout = 32, 255 (dy rows padded to 256 channels
    with zeros) and 256, stride 2, the 256-row bf16 tile forced; the second run is bit-identical; a workspace one byte short
    of the slabs is refused"""
    bf = mode(c['mode'])
    if c['tile']:
        monkeypatch.setenv('Y4_BF_WGRAD_TILE', str(c['tile']))
    B, H, W, Cin, Cout, k, s = (c[t] for t in ('B', 'H', 'W', 'Cin', 'Cout', 'k', 's'))
    Ho, Wo = CC.out_hw(H, W, k, s)
    seed = CC.seed_of(B, H, W, Cin, Cout, k, s, 11)
    q = 64 if bf else 32
    ldc = CC.cdiv(Cout, q) * q
    xa = CC.act_planes(CC.make_values(B * H * W, Cin, seed, spread=2), bf)
    da = CC.act_planes(CC.make_values(B * Ho * Wo, ldc, seed + 1, spread=10), bf, c_valid=Cout)
    tn, ntn, ntj, splits, per = CC.wgrad_case_plan(c)
    r = CC.wgrad_ref(xa['dec'].reshape(B, H, W, Cin), da['dec'][:, :Cout].reshape(B, Ho, Wo, Cout), k, s, splits)
    assert CC.left_out(r, bf) <= CC.LEFT_OUT_CAP
    o = _run_wgrad(dev, c, xa, da)
    what = CC.case_id(c)
    assert o['rc'] == 0, what
    assert o['kernel'] == CC.wgrad_name(tn, bf, s), (what, o['kernel'])
    dw = _f32(o['dw']).reshape(Cout, k, k, Cin)
    ok, used = CC.conv_accept(dw, r, bf)
    _note('wgrad.%s' % ('bf16' if bf else 'f16x2'), used, what + ' splits %d' % splits)
    assert ok.all(), (what, _worst(ok, dw, r, bf))
    assert np.array_equal(_run_wgrad(dev, c, xa, da)['dw'], o['dw']), what
    if splits > 1:
        o = _run_wgrad(dev, c, xa, da, ws_short=65)
        assert o['rc'] == BC.ERR_WORKSPACE and (o['dw'] == BC.SENT).all()


# ------------------------------------------------------------------------------------------ the split kernels
@pytest.mark.parametrize('m', ('f16x2', 'bf16'))
def test_split_kernels_write_the_bytes_of_the_host_builder(dev, mode, m):
    """y4_planes_split_f32 and y4_planes_split_into_f32 (a channel slice of a wider pre-split row, pad channels past c_valid
    written as zeros whatever the source holds there): bit for bit the rows of conv_cases.act_planes, the neighbouring
    slices, the second half of dense bf16 rows and the source's pitch padding untouched"""
    bf = mode(m)
    L, stream, _ = _abi()
    for M, C, ldx, ldp, off, cv in CC.SPLIT_CASES:
        a = CC.make_values(M, C, CC.seed_of(M, C, ldx), spread=10)
        word = BC.amax_word(a * F32(1.7))                                # the scale of a bound above the maximum
        src = BC.pad_rows(a, ldx)
        src[:, cv:C] = BC.sentinel((M, C - cv))                          # pad channels of the source: never used
        want = CC.act_planes(a, bf, ld=ldp or C, off=off, c_valid=cv, **({} if bf else dict(word=word)))
        xd = Buf(dev, M * ldx, src)
        od = Buf(dev, M * (ldp or C))
        ad = _word(dev, None if bf else word)
        if ldp:
            rc = L.y4_planes_split_into_f32(xd.ptr(), ldx, M, C, _p(ad), od.ptr((2 if bf else 4) * off), ldp, cv, stream())
        else:
            rc = L.y4_planes_split_f32(xd.ptr(), ldx, M, C, _p(ad), od.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, (M, C, ldp)
        got = od.get().reshape(M, ldp or C)
        same = got == want['words']
        assert same.all(), ((M, C, ldx, ldp, off, cv), np.argwhere(~same)[:5])
    od = Buf(dev, 64 * 64)
    xd = Buf(dev, 64 * 64, CC.make_values(64, 64, 1))
    ad = _word(dev, 0x40000000)
    assert L.y4_planes_split_f32(xd.ptr(), 60, 64, 64, _p(ad), od.ptr(), stream()) == BC.ERR_SHAPE
    assert L.y4_planes_split_into_f32(xd.ptr(), 64, 64, 64, _p(ad), od.ptr(64), 64, 64, stream()) == BC.ERR_SHAPE
    assert L.y4_planes_split_into_f32(xd.ptr(), 64, 64, 64, _p(ad), od.ptr(), 64, 65, stream()) == BC.ERR_SHAPE
    torch.cuda.synchronize()
    assert (od.get() == BC.SENT).all()
