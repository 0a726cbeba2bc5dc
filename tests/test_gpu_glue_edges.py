# -*- coding: utf-8 -*-
"""The glue kernels of csrc/pointwise.hip -- channel copy, add, the stride-1 max pool and its backward, the x2 and the
general nearest upsample with their adjoints, the flat activations -- and the operand-maximum kernels of
csrc/conv_f16x2.hip, each driven through the C ABI at the sizes where the host or a kernel takes another path: C / 4 that is
no power of two, pitch > C and channel slices of wider buffers, grids over their cap (the grid-stride loops), the scalar
paths of the activation and amax kernels, windows larger than the image, ties / NaN / infinities in the pool,
accumulate = 1, and every argument set the host code refuses.

References, acceptance criteria and case lists are tests/glue_cases.py; tests/test_glue_cases.py shows without a GPU that
every case reaches the branch it is listed for.  Every output buffer starts as a NaN bit pattern no kernel produces:
pitch padding, neighbouring channel slices and a guard in front of and behind every buffer must still hold it.

Which case reaches which branch (refused argument sets: glue_cases.REJECTS, one test_refused_calls case per entry point):
  y4_copy_channels_f32, y4_add_f32      one lap: test_copy_and_add (C / 4 = 1, 2, 3, 5, 9, 16; M = 1, 2, 255, 257; three
                                        pitches; out = a, out = b, a = b); grid-stride: test_copy_and_add_grid_stride
  y4_maxpool_s1_fwd_f32 / _bwd_f32      test_maxpool (ks 1 .. 11, windows larger than the image, idx and idx = NULL,
                                        accumulate 0 and 1, own and reference codes); grid-stride: test_maxpool_grid_stride
  y4_upsample2x_fwd_f32 / _bwd_f32      test_upsample2x; grid-stride: test_upsample2x_grid_stride
  y4_upsample_nearest_fwd_f32 / _bwd    integer_factor = 0: test_upsample_nearest; = 1: test_upsample_nearest_integer_factor;
                                        grid-stride: test_upsample_nearest_grid_stride
  y4_act_fwd_f32 / y4_act_bwd_f32       vector body + scalar tail: offsets (0, 0, 0) of test_act; scalar path: the other
                                        offsets; grid-stride: test_act_grid_stride
  y4_amax_f32                           vector and strided kernel, M = 0: test_amax; capped grid: test_amax_capped_grid
  y4_amax_merge_u32                     test_amax_merge

Largest share of each bound used on an MI355X (every test prints its own): maxpool_bwd 1.000 and upsample_nearest_bwd 1.000
(two addends: one rounding, which is the whole bound), upsample2x_bwd 0.637, mish forward 0.374, mish backward 0.258; everything
else is bit-exact.  The slowest test, test_maxpool_grid_stride, takes 0.9 s."""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as GC

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
G = 32                                   # guard words (128 B) in front of and behind every device buffer
USED = {}                                # group -> largest share of its bound used so far (printed per test)


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


def _sync():
    torch.cuda.synchronize()


class Buf(object):
    """n 32-bit words on the device between two guards; everything starts as the sentinel unless `init` is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        if init is None:
            self.t = torch.full((self.n + 2 * G,), GC.SENT, dtype=torch.int32, device=dev)
        else:
            h = np.full(self.n + 2 * G, GC.SENT, dtype=np.uint32)
            h[G:G + self.n] = np.ascontiguousarray(init).view(np.uint32).ravel()
            self.t = torch.from_numpy(h.view(np.int32)).to(dev)

    def ptr(self, off_words=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (G + off_words))

    def get(self):
        """the body as uint32 words; the guards must be untouched"""
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:G] == GC.SENT).all() and (h[G + self.n:] == GC.SENT).all(), 'write outside the buffer'
        return h[G:G + self.n].copy()


class Rows(object):
    """[M, C] fp32 rows at pitch ld, starting `off` columns into the buffer's rows: the columns beside the slice hold the
    sentinel before the call and must hold it afterwards.  data = None: an output (all sentinel)."""

    def __init__(self, dev, M, C, pitch, data=None):
        self.M, self.C, (self.ld, self.off) = M, C, pitch
        h = GC.sentinel((M, self.ld))
        if data is not None:
            h[:, self.off:self.off + C] = np.asarray(data, F32).reshape(M, C)
        self.buf = Buf(dev, M * self.ld, h)

    def ptr(self):
        return self.buf.ptr(self.off)

    def get(self):
        """the slice as uint32 [M, C]; everything around it untouched"""
        h = self.buf.get().reshape(self.M, self.ld)
        around = np.ones(self.ld, bool)
        around[self.off:self.off + self.C] = False
        assert (h[:, around] == GC.SENT).all(), 'write into the pitch padding or a neighbouring slice'
        return h[:, self.off:self.off + self.C].copy()


def _f32(words):
    return np.ascontiguousarray(words).view(F32)


def _note(group, used, what=''):
    """print the share of its bound a check used and keep the group's maximum"""
    used = np.asarray(used, F64)
    m = float(np.max(used)) if used.size else 0.0
    USED[group] = max(USED.get(group, 0.0), m)
    print('%s %s: share of the bound used %.3f; group maximum so far %.3f' % (group, what, m, USED[group]))


def _worst(ok, got, ref):
    bad = np.argwhere(~np.asarray(ok))[:5]
    return [(tuple(i), float(np.asarray(got)[tuple(i)]), float(np.asarray(ref)[tuple(i)])) for i in bad]


def _exact(got_words, ref, what):
    same = np.asarray(got_words).reshape(-1) == GC.bits(ref).reshape(-1)
    assert same.all(), (what, 'first differing elements', np.argwhere(~same)[:5].ravel().tolist())


def _pitch(C, i):
    return GC.pitches(C)[i % 3]


# ------------------------------------------------------------------------------------------ copy, add
def _add_input(M, C, seed):
    rng = np.random.RandomState(seed)
    a, b = rng.standard_normal((M, C)).astype(F32), (rng.standard_normal((M, C)) * 1e-3).astype(F32)
    sp_a = np.array([np.inf, -np.inf, 2.0 ** -149, -0.0, 1.5, GC.FLT_MAX, 2.0 ** -126], F32)
    sp_b = np.array([1.0, -2.0, 2.0 ** -149, 0.0, -1.5, GC.FLT_MAX, -2.0 ** -127], F32)
    n = min(sp_a.size, M * C)
    a.reshape(-1)[:n], b.reshape(-1)[:n] = sp_a[:n], sp_b[:n]
    if M * C > 8:
        a.reshape(-1)[-1] = GC.f32_from_bits(GC.NAN_A)                  # one NaN operand: its payload comes through
        b.reshape(-1)[-2] = GC.f32_from_bits(GC.NAN_B)
    return a, b


def _copy(dev, x, ps, pd):
    L, stream = _abi()
    M, C = x.shape
    src, dst = Rows(dev, M, C, ps, x), Rows(dev, M, C, pd)
    rc = L.y4_copy_channels_f32(src.ptr(), src.ld, dst.ptr(), dst.ld, M, C, stream())
    _sync()
    assert rc == 0
    _exact(src.get(), x, 'source changed')
    return dst.get()


def _add(dev, a, b, pa, pb, po, alias=None):
    """alias: None, 'a' (out is a's buffer), 'b', or 'ab' (a and b are one buffer, out separate)"""
    L, stream = _abi()
    M, C = a.shape
    ra = Rows(dev, M, C, pa, a)
    rb = ra if alias == 'ab' else Rows(dev, M, C, pb, b)
    ro = ra if alias == 'a' else rb if alias == 'b' else Rows(dev, M, C, po)
    rc = L.y4_add_f32(ra.ptr(), ra.ld, rb.ptr(), rb.ld, ro.ptr(), ro.ld, M, C, stream())
    _sync()
    assert rc == 0
    for r in (ra, rb):
        if r is not ro:
            r.get()
    return ro.get()


@pytest.mark.parametrize('C', GC.CHANNELS)
def test_copy_and_add(dev, C):
    """y4_copy_channels_f32 and y4_add_f32, bit for bit, over the row counts and every pair of pitches (dense, a slice in
    the middle of a wider buffer, a slice at its start); add with out aliasing a, aliasing b, and a == b"""
    for M in GC.ROWS:
        a, b = _add_input(M, C, M + C)
        with np.errstate(over='ignore', invalid='ignore'):
            want = a + b
            twice = a + a
        for i in range(3):
            for j in range(3):
                _exact(_copy(dev, a, _pitch(C, i), _pitch(C, j)), a, 'copy C%d M%d %d->%d' % (C, M, i, j))
            _exact(_add(dev, a, b, _pitch(C, i), _pitch(C, i + 1), _pitch(C, i + 2)), want, 'add C%d M%d %d' % (C, M, i))
            _exact(_add(dev, a, b, _pitch(C, i), _pitch(C, i + 1), None, alias='a'), want, 'add into a')
            _exact(_add(dev, a, b, _pitch(C, i + 1), _pitch(C, i), None, alias='b'), want, 'add into b')
            _exact(_add(dev, a, a, _pitch(C, i), None, _pitch(C, i + 1), alias='ab'), twice, 'a + a')


def test_copy_and_add_grid_stride(dev):
    C, M = GC.BIG_ROWS
    assert GC.laps(M * (C // 4)) == 2
    a, b = _add_input(M, C, 1)
    _exact(_copy(dev, a, _pitch(C, 0), _pitch(C, 2)), a, 'copy, two laps')
    with np.errstate(over='ignore', invalid='ignore'):
        _exact(_add(dev, a, b, _pitch(C, 0), _pitch(C, 0), _pitch(C, 0)), a + b, 'add, two laps')


# ------------------------------------------------------------------------------------------ max pool
def _pool_fwd(dev, x, ks, px, py, with_idx=True):
    L, stream = _abi()
    B, H, W, C = x.shape
    M = B * H * W
    rx, ry = Rows(dev, M, C, px, x), Rows(dev, M, C, py)
    idx = Buf(dev, M * C // 4) if with_idx else None
    rc = L.y4_maxpool_s1_fwd_f32(rx.ptr(), rx.ld, ry.ptr(), ry.ld, idx.ptr() if idx else None, B, H, W, C, ks, stream())
    _sync()
    assert rc == 0
    rx.get()
    return ry.get().reshape(x.shape), idx.get().view(np.int8).reshape(x.shape) if idx else None


def _pool_bwd(dev, dy, code, ks, pdy, pdx, old=None):
    L, stream = _abi()
    B, H, W, C = dy.shape
    M = B * H * W
    rdy, rdx = Rows(dev, M, C, pdy, dy), Rows(dev, M, C, pdx, old)
    idx = Buf(dev, M * C // 4, np.ascontiguousarray(code, dtype=np.int8).view(np.uint32))
    rc = L.y4_maxpool_s1_bwd_f32(rdy.ptr(), rdy.ld, idx.ptr(), rdx.ptr(), rdx.ld, 1 if old is not None else 0, B, H, W, C, ks,
                                 stream())
    _sync()
    assert rc == 0
    rdy.get()
    idx.get()
    return rdx.get().reshape(dy.shape)


def _check_pool(dev, x, ks, i, what, twice=True):
    C = x.shape[3]
    y_ref, code_ref = GC.maxpool_ref(x, ks)
    y, code = _pool_fwd(dev, x, ks, _pitch(C, i), _pitch(C, i + 1))
    _exact(y, y_ref, what + ' values')
    assert np.array_equal(code, code_ref), (what, 'codes', np.argwhere(code != code_ref)[:5].tolist())
    y2, none = _pool_fwd(dev, x, ks, _pitch(C, i + 1), _pitch(C, i), with_idx=False)      # idx = NULL: the inference path
    assert none is None
    _exact(y2, y_ref, what + ' values, idx = NULL')
    rng = np.random.RandomState(ks + i)
    dy, old = rng.standard_normal(x.shape).astype(F32), rng.standard_normal(x.shape).astype(F32)
    for acc in (None, old):
        dx_ref, sa, k = GC.maxpool_bwd_ref(dy, code_ref, ks, acc)
        runs = [_pool_bwd(dev, dy, c, ks, _pitch(C, i + 2), _pitch(C, i), acc) for c in ((code, code_ref, code) if twice else (code,))]
        assert all(np.array_equal(runs[0], r) for r in runs[1:]), (what, 'the backward sum is not reproducible')
        got = _f32(runs[0])
        ok, used = GC.sum_accept(got, dx_ref, sa, k)
        _note('maxpool_bwd', used, '%s accumulate=%d' % (what, acc is not None))
        assert ok.all(), (what, acc is not None, _worst(ok, got, dx_ref))


@pytest.mark.parametrize('ks', GC.POOL_KS)
def test_maxpool(dev, ks):
    """forward values and int8 codes bit for bit (ties, two NaNs in a window, a window of -inf, +inf; windows larger than
    the image), with and without idx; backward with accumulate 0 and 1, on the kernel's own codes and on the
    reference's, twice with equal bits"""
    i = 0
    for H, W in GC.POOL_IMAGES:
        for B in GC.POOL_BATCH:
            for C in (GC.CHANNELS if (H, W) == GC.POOL_IMAGES[-1] and B == 3 else (4, 12)):
                i += 1
                _check_pool(dev, GC.make_pool_input(B, H, W, C, ks * 100 + i), ks, i, 'ks%d B%d %dx%d C%d' % (ks, B, H, W, C))


def test_maxpool_grid_stride(dev):
    B, H, W, C = GC.BIG_IMAGE
    assert GC.laps(B * H * W * (C // 4)) == 2
    _check_pool(dev, GC.make_pool_input(B, H, W, C, 7), 3, 0, 'two laps', twice=False)


# ------------------------------------------------------------------------------------------ upsample
def _image_call(dev, fn, x, out_shape, px, po, *tail):
    """fn(x, ldx, out, ldo, B, H, W, ...tail, stream) on NHWC images -> out words in out_shape"""
    _, stream = _abi()
    B, H, W, C = x.shape
    rx = Rows(dev, B * H * W, C, px, x)
    ro = Rows(dev, int(np.prod(out_shape[:3])), C, po)
    rc = fn(rx.ptr(), rx.ld, ro.ptr(), ro.ld, *(tuple(tail) + (stream(),)))
    _sync()
    assert rc == 0
    rx.get()
    return ro.get().reshape(out_shape)


def _check_up2(dev, B, H, W, C, i, what):
    L, _ = _abi()
    rng = np.random.RandomState(H * 7 + W + C)
    x = rng.standard_normal((B, H, W, C)).astype(F32)
    x.reshape(-1)[0] = GC.f32_from_bits(GC.NAN_A)
    y = _image_call(dev, L.y4_upsample2x_fwd_f32, x, (B, 2 * H, 2 * W, C), _pitch(C, i), _pitch(C, i + 1), B, H, W, C)
    _exact(y, GC.upsample2x_ref(x), what + ' forward')
    dy = rng.standard_normal((B, 2 * H, 2 * W, C)).astype(F32)
    dx_ref, sa = GC.upsample2x_bwd_ref(dy)
    runs = [_image_call(dev, L.y4_upsample2x_bwd_f32, dy, (B, H, W, C), _pitch(C, i + 2), _pitch(C, i), B, H, W, C) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]), (what, 'the adjoint is not reproducible')
    ok, used = GC.sum_accept(_f32(runs[0]), dx_ref, sa, 4)
    _note('upsample2x_bwd', used, what)
    assert ok.all(), (what, _worst(ok, _f32(runs[0]), dx_ref))


@pytest.mark.parametrize('H,W', GC.UP2_IMAGES)
def test_upsample2x(dev, H, W):
    i = 0
    for B in GC.UP2_BATCH:
        for C in GC.CHANNELS:
            i += 1
            _check_up2(dev, B, H, W, C, i, 'B%d %dx%d C%d' % (B, H, W, C))


def test_upsample2x_grid_stride(dev):
    L, _ = _abi()
    B, H, W, C = GC.BIG_HALF
    assert GC.laps(B * 4 * H * W * (C // 4)) == 2
    x = np.random.RandomState(5).standard_normal((B, H, W, C)).astype(F32)
    y = _image_call(dev, L.y4_upsample2x_fwd_f32, x, (B, 2 * H, 2 * W, C), _pitch(C, 0), _pitch(C, 0), B, H, W, C)
    _exact(y, GC.upsample2x_ref(x), 'forward, two laps')
    B, H, W, C = GC.BIG_IMAGE
    assert GC.laps(B * H * W * (C // 4)) == 2
    dy = np.random.RandomState(6).standard_normal((B, 2 * H, 2 * W, C)).astype(F32)
    dx_ref, sa = GC.upsample2x_bwd_ref(dy)
    got = _f32(_image_call(dev, L.y4_upsample2x_bwd_f32, dy, (B, H, W, C), _pitch(C, 0), _pitch(C, 0), B, H, W, C))
    ok, used = GC.sum_accept(got, dx_ref, sa, 4)
    _note('upsample2x_bwd', used, 'two laps')
    assert ok.all(), _worst(ok, got, dx_ref)


def _check_nearest(dev, B, H, W, Ho, Wo, C, factor, i, what, twice=True):
    L, _ = _abi()
    rng = np.random.RandomState(H * 31 + Wo + C)
    x = rng.standard_normal((B, H, W, C)).astype(F32)
    x.reshape(-1)[-1] = GC.f32_from_bits(GC.NAN_B)
    y = _image_call(dev, L.y4_upsample_nearest_fwd_f32, x, (B, Ho, Wo, C), _pitch(C, i), _pitch(C, i + 1), B, H, W, Ho, Wo, C,
                    1 if factor else 0)
    _exact(y, GC.nearest_ref(x, Ho, Wo, factor), what + ' forward')
    dy = rng.standard_normal((B, Ho, Wo, C)).astype(F32)
    dx_ref, sa, k = GC.nearest_bwd_ref(dy, H, W, factor)
    runs = [_image_call(dev, L.y4_upsample_nearest_bwd_f32, dy, (B, H, W, C), _pitch(C, i + 2), _pitch(C, i), B, H, W, Ho, Wo, C,
                        1 if factor else 0) for _ in range(2 if twice else 1)]
    assert all(np.array_equal(runs[0], r) for r in runs[1:]), (what, 'the adjoint is not reproducible')
    got = _f32(runs[0])
    ok, used = GC.sum_accept(got, dx_ref, sa, k)
    _note('upsample_nearest_bwd', used, '%s (blocks of up to %d)' % (what, int(k.max())))
    assert ok.all(), (what, _worst(ok, got, dx_ref))
    return x, y


@pytest.mark.parametrize('size', GC.NEAREST_SIZES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_upsample_nearest(dev, size):
    """F.interpolate(size=..., mode='nearest') in ATen's fp32 index arithmetic and its adjoint: identity, x2, a
    non-integer ratio, different ratios per axis, downsampling (source pixels without destinations: exactly 0), 1 -> 17,
    17 -> 1, a block of 1366 rows, and a pair where the fp32 map differs from the rational one"""
    (H, W), (Ho, Wo) = size
    i = 0
    for B in (1, 2):
        for C in (4, 12, 20) if Ho < 100 else (4,):
            i += 1
            x, y = _check_nearest(dev, B, H, W, Ho, Wo, C, False, i, 'B%d C%d' % (B, C))
            if (H, W) == (Ho, Wo):
                _exact(y, x, 'identity')


@pytest.mark.parametrize('case', GC.NEAREST_FACTORS, ids=lambda c: '%dx%d-by-%dx%d' % (c[0] + c[1]))
def test_upsample_nearest_integer_factor(dev, case):
    (H, W), (fh, fw) = case
    i = 0
    for B in (1, 2):
        for C in (4, 12, 36):
            i += 1
            _check_nearest(dev, B, H, W, H * fh, W * fw, C, True, i, 'B%d C%d factor' % (B, C))


def test_upsample_nearest_grid_stride(dev):
    (B, H, W, C), (Ho, Wo) = GC.BIG_NEAREST_FWD
    assert GC.laps(B * Ho * Wo * (C // 4)) == 2
    L, _ = _abi()
    x = np.random.RandomState(8).standard_normal((B, H, W, C)).astype(F32)
    y = _image_call(dev, L.y4_upsample_nearest_fwd_f32, x, (B, Ho, Wo, C), _pitch(C, 0), _pitch(C, 0), B, H, W, Ho, Wo, C, 0)
    _exact(y, GC.nearest_ref(x, Ho, Wo), 'forward, two laps')
    (B, H, W, C), (Ho, Wo) = GC.BIG_NEAREST_BWD
    assert GC.laps(B * H * W * (C // 4)) == 2
    dy = np.random.RandomState(9).standard_normal((B, Ho, Wo, C)).astype(F32)
    dx_ref, sa, k = GC.nearest_bwd_ref(dy, H, W)
    got = _f32(_image_call(dev, L.y4_upsample_nearest_bwd_f32, dy, (B, H, W, C), _pitch(C, 0), _pitch(C, 0), B, H, W, Ho, Wo, C, 0))
    ok, used = GC.sum_accept(got, dx_ref, sa, k)
    _note('upsample_nearest_bwd', used, 'two laps')
    assert ok.all(), _worst(ok, got, dx_ref)


# ------------------------------------------------------------------------------------------ activations
def _flat(dev, a, off):
    """n floats starting `off` floats after a 16-B boundary (the guard is 128 B)"""
    n = np.size(a)
    h = GC.sentinel((n + 4,))
    h[off:off + n] = a
    return Buf(dev, n + 4, h)


def _flat_out(buf, n, off):
    h = buf.get()
    assert (h[:off] == GC.SENT).all() and (h[off + n:] == GC.SENT).all(), 'write outside the tensor'
    return h[off:off + n]


def _act_call(dev, x, dy, act, offs):
    """(y, dx) words of y4_act_fwd_f32 / y4_act_bwd_f32 with x, dy and the output offset by offs floats"""
    L, stream = _abi()
    n = x.size
    ox, ody, oo = offs
    bx, bdy, by, bdx = _flat(dev, x, ox), _flat(dev, dy, ody), Buf(dev, n + 4), Buf(dev, n + 4)
    rc = L.y4_act_fwd_f32(bx.ptr(ox), by.ptr(oo), n, act, stream())
    rc2 = L.y4_act_bwd_f32(bx.ptr(ox), bdy.ptr(ody), bdx.ptr(oo), n, act, stream())
    _sync()
    assert rc == 0 and rc2 == 0
    assert np.array_equal(_flat_out(bx, n, ox), GC.bits(x)) and np.array_equal(_flat_out(bdy, n, ody), GC.bits(dy))
    return _flat_out(by, n, oo), _flat_out(bdx, n, oo)


def _check_act(dev, n, act, offs, what):
    x, dy = GC.make_act_input(n, n % 97)
    y, dx = _act_call(dev, x, dy, act, offs)
    name = GC.ACT_NAMES[act]
    with np.errstate(invalid='ignore', over='ignore'):
        ok, used = GC.act_fwd_accept(_f32(y), x, act)
        _note(name + '.fwd', used, what)
        assert ok.all(), (what, 'forward (index, got, x)', _worst(ok, _f32(y), x))
        ok, used = GC.act_bwd_accept(_f32(dx), x, dy, act)
        _note(name + '.bwd', used, what)
        assert ok.all(), (what, 'backward (index, got, x)', _worst(ok, _f32(dx), x), dy[~ok][:5])
    return x, dy, _f32(y), _f32(dx)


@pytest.mark.parametrize('act', GC.ACTS, ids=GC.ACT_NAMES.get)
def test_act(dev, act):
    """y4_act_fwd_f32 / y4_act_bwd_f32 over the sizes around one vector and one block, all pointers aligned (vector body +
    scalar tail) and x, dy, the output one float off in turn (the scalar path), on the grid through zeros, denormals,
    the clamp at 20, the exponent's range, FLT_MAX, infinities and NaN, with dy = 0 at the large-x points"""
    for n in GC.ACT_SIZES:
        for offs in GC.ACT_OFFSETS:
            x, dy, y, dx = _check_act(dev, n, act, offs, 'n%d offsets%s' % (n, offs))
    if act == GC.ACT_MISH:                                            # the derivative far above the clamp, as computed
        x, dy = np.array([1e17, 1e22, 1e17, 1e22], F32), np.array([1.0, 1.0, 0.0, 0.0], F32)
        _, dx = _act_call(dev, x, dy, act, (0, 0, 0))
        print("mish'(1e17), mish'(1e22) with dy = 1: %r; with dy = 0: %r" % (_f32(dx)[:2].tolist(), _f32(dx)[2:].tolist()))


@pytest.mark.parametrize('act', GC.ACTS, ids=GC.ACT_NAMES.get)
def test_act_grid_stride(dev, act):
    assert GC.act_plan(GC.BIG_ACT, True)[1:] == (2, 3)
    _check_act(dev, GC.BIG_ACT, act, (0, 0, 0), 'two laps')


# ------------------------------------------------------------------------------------------ amax
def _amax(dev, x, C, off, M=None):
    L, stream = _abi()
    rows, ld = x.shape
    h = GC.sentinel((x.size + 4,))
    h[off:off + x.size] = x.reshape(-1)
    xb = Buf(dev, x.size + 4, h)
    word = Buf(dev, 1, np.array([0x7f000000], np.uint32))                # overwritten, not folded into
    rc = L.y4_amax_f32(xb.ptr(off), ld, rows if M is None else M, C, word.ptr(), stream())
    _sync()
    assert rc == 0
    assert np.array_equal(xb.get(), GC.bits(h))
    return int(word.get()[0])


def test_amax(dev):
    """y4_amax_f32 on the vector and the strided kernel: pad columns holding 3e38 and NaN patterns do not count, the
    maximum is found in the first element, the last row's last valid channel and the middle, as a negative number;
    zeros, -0.0, denormals, only inf / NaN; the word is overwritten; M = 0 leaves 0"""
    for name, x, C, off, kind in GC.amax_cases():
        M, ld = x.shape
        assert GC.amax_plan(16 + 4 * off, ld, M, C)[0] == kind
        got = _amax(dev, x, C, off)
        assert got == GC.amax_ref(x, C), (name, hex(got), hex(GC.amax_ref(x, C)))
    name, x, C, off, _ = GC.amax_cases()[0]
    assert _amax(dev, x, C, off, M=0) == 0


@pytest.mark.parametrize('M,C,ld', GC.BIG_AMAX)
def test_amax_capped_grid(dev, M, C, ld):
    assert GC.amax_plan(16, ld, M, C)[1:] == (GC.AMAX_CAP, 5)
    x = np.random.RandomState(M % 1000).standard_normal((M, ld)).astype(F32)
    x[M - 1, C - 1] = F32(-1234.5)
    assert _amax(dev, x, C, 0) == GC.bits(F32(1234.5))
    x[M - 1, C - 1] = F32(0.5)
    assert _amax(dev, x, C, 0) == GC.amax_ref(x, C)


def test_amax_merge(dev):
    L, stream = _abi()
    for d, s in GC.MERGE_CASES:
        dst, src = Buf(dev, 1, np.array([d], np.uint32)), Buf(dev, 1, np.array([s], np.uint32))
        assert L.y4_amax_merge_u32(dst.ptr(), src.ptr(), stream()) == 0
        _sync()
        assert int(dst.get()[0]) == GC.merge_ref(d, s) and int(src.get()[0]) == s


# ------------------------------------------------------------------------------------------ refused calls
def _reject_call(L, stream, entry, a, p):
    """the call of `entry` with the argument set a; p(name) is the operand's pointer (None when the set nulls it)"""
    ld = lambda n: a['ld_' + n]                                          # noqa: E731
    B, H, W, C = a['B'], a['H'], a['W'], a['C']
    if entry == 'copy':
        return L.y4_copy_channels_f32(p('src'), ld('src'), p('dst'), ld('dst'), a['M'], C, stream())
    if entry == 'add':
        return L.y4_add_f32(p('a'), ld('a'), p('b'), ld('b'), p('out'), ld('out'), a['M'], C, stream())
    if entry == 'maxpool_fwd':
        return L.y4_maxpool_s1_fwd_f32(p('x'), ld('x'), p('y'), ld('y'), p('idx'), B, H, W, C, a['ks'], stream())
    if entry == 'maxpool_bwd':
        return L.y4_maxpool_s1_bwd_f32(p('dy'), ld('dy'), p('idx'), p('dx'), ld('dx'), a['accumulate'], B, H, W, C, a['ks'], stream())
    if entry == 'upsample2x_fwd':
        return L.y4_upsample2x_fwd_f32(p('x'), ld('x'), p('y'), ld('y'), B, H, W, C, stream())
    if entry == 'upsample2x_bwd':
        return L.y4_upsample2x_bwd_f32(p('dy'), ld('dy'), p('dx'), ld('dx'), B, H, W, C, stream())
    if entry == 'nearest_fwd':
        return L.y4_upsample_nearest_fwd_f32(p('x'), ld('x'), p('y'), ld('y'), B, H, W, a['Ho'], a['Wo'], C, a['integer_factor'], stream())
    if entry == 'nearest_bwd':
        return L.y4_upsample_nearest_bwd_f32(p('dy'), ld('dy'), p('dx'), ld('dx'), B, H, W, a['Ho'], a['Wo'], C, a['integer_factor'], stream())
    if entry == 'act_fwd':
        return L.y4_act_fwd_f32(p('x'), p('y'), a['n'], a['act'], stream())
    if entry == 'act_bwd':
        return L.y4_act_bwd_f32(p('x'), p('dy'), p('dx'), a['n'], a['act'], stream())
    if entry == 'amax':
        return L.y4_amax_f32(p('x'), ld('x'), a['M'], C, p('word'), stream())
    assert entry == 'merge'
    return L.y4_amax_merge_u32(p('dst'), p('src'), stream())


@pytest.mark.parametrize('entry', sorted(GC.REJECTS))
def test_refused_calls(dev, entry):
    """every argument set the host code refuses before a launch returns its code and writes nothing: inputs, outputs and
    the amax word still hold the sentinel"""
    L, stream = _abi()
    for name, over, want in GC.REJECTS[entry]:
        a = GC.reject_args(entry, over)
        assert GC.mirror_rc(entry, a) == want != 0
        bufs = {}

        def p(n):
            if a.get('null_' + n):
                return None
            bufs.setdefault(n, Buf(dev, 1024))
            return bufs[n].ptr(a.get('off_' + n, 0))

        rc = _reject_call(L, stream, entry, a, p)
        _sync()
        assert rc == want, (entry, name, rc)
        for n, b in bufs.items():
            assert (b.get() == GC.SENT).all(), (entry, name, n)
