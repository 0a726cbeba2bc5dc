# -*- coding: utf-8 -*-
"""tests/glue_cases.py checked without a GPU: every listed case reaches the branch of csrc/pointwise.hip /
csrc/conv_f16x2.hip it is listed for (through the mirror of the host dispatch), the references agree with torch on the CPU,
every acceptance function accepts the fp32-rounded reference on every listed input, and every one rejects planted faults."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as GC

F32, F64 = np.float32, np.float64
BASE = 1 << 20                            # a 16-B aligned stand-in for a device address


# ------------------------------------------------------------------------------------------ branch coverage
def test_channels_and_rows():
    assert {C: C // 4 for C in GC.CHANNELS} == {4: 1, 8: 2, 12: 3, 20: 5, 36: 9, 64: 16}
    assert all(GC.CHANNEL_TABLE[C][0] == C // 4 for C in GC.CHANNELS)
    pow2 = [C for C in GC.CHANNELS if (C // 4) & (C // 4 - 1) == 0]
    assert pow2 == [4, 8, 64]
    for C in GC.CHANNELS:
        assert [ld - C for ld, _ in GC.pitches(C)] == [0, 8, 4]
        for ld, off in GC.pitches(C):
            assert GC.vec_ok(BASE + 4 * off, ld, C) and off + C <= ld
        for M in GC.ROWS:                                   # the small cases: one lap, the last block ragged or one thread
            assert GC.laps(M * (C // 4)) == 1
    assert GC.grid_for(1) == 1 and GC.grid_for(255 * 3) == 3 and GC.grid_for(257) == 2 and GC.grid_for(0) == 1


def test_grid_stride_cases():
    full = GC.GRID_CAP * GC.PW_THREADS
    C, M = GC.BIG_ROWS
    totals = {'copy/add': M * (C // 4)}
    B, H, W, C = GC.BIG_IMAGE
    totals['pool, upsample2x_bwd'] = B * H * W * (C // 4)
    B, H, W, C = GC.BIG_HALF
    totals['upsample2x_fwd'] = B * 4 * H * W * (C // 4)
    (B, H, W, C), (Ho, Wo) = GC.BIG_NEAREST_FWD
    totals['nearest_fwd'] = B * Ho * Wo * (C // 4)
    (B, H, W, C), (Ho, Wo) = GC.BIG_NEAREST_BWD
    totals['nearest_bwd'] = B * H * W * (C // 4)
    assert Ho * Wo * C * 4 <= 17 << 20
    for name, t in totals.items():
        assert full < t < full + full // 128 and t % 256, name     # just above the cap, ragged last block
        assert GC.grid_for(t) == GC.GRID_CAP and GC.laps(t) == 2, name
        assert t * 16 <= 17 << 20, name                            # about 16 MB
    grid, vlaps, tail = GC.act_plan(GC.BIG_ACT, True)
    assert (grid, vlaps, tail) == (GC.GRID_CAP, 2, 3) and GC.BIG_ACT * 4 <= 17 << 20
    (M1, C1, ld1), (M2, C2, ld2) = GC.BIG_AMAX
    assert GC.amax_plan(BASE, ld1, M1, C1) == ('vector', GC.AMAX_CAP, 5) and M1 * ((C1 + 3) // 4) > 1024 * 1024
    assert GC.amax_plan(BASE, ld2, M2, C2) == ('strided', GC.AMAX_CAP, 5) and M2 * C2 > 1024 * 1024


def test_act_paths():
    for n in GC.ACT_SIZES:
        grid, vlaps, tail = GC.act_plan(n, True)
        assert grid == -(-((n + 3) // 4) // 256) and tail == n % 4 and vlaps == (1 if n >= 4 else 0)
        assert GC.act_plan(n, False) == (grid, 0, n)
    assert sorted(n % 4 for n in GC.ACT_SIZES) == [0, 0, 1, 1, 1, 3, 3, 3]
    # the scalar loop strides over the grid: at n = 1025 two blocks of 256 threads take 1025 elements in three trips
    assert GC.act_plan(1025, False)[0] == 2
    assert GC.ACT_OFFSETS[0] == (0, 0, 0) and all(sum(o) == 1 for o in GC.ACT_OFFSETS[1:])
    x, dy = GC.make_act_input(1023, 1)
    assert set(GC.bits(GC.ACT_GRID)) <= set(GC.bits(x))
    big = np.isin(x, GC.ACT_LARGE_X) & (dy == 0)
    assert big.sum() >= GC.ACT_LARGE_X.size                          # dy = 0 at the large-x points
    seen = set()
    for n in GC.ACT_SIZES[:5]:
        seen |= set(GC.bits(GC.make_act_input(n, n)[0]))
    assert len(seen) >= 15


def test_pool_cases():
    for ks in (9, 11):
        for H, W in GC.POOL_IMAGES[:3]:
            assert H - 1 <= ks // 2 and W - 1 <= ks // 2             # every window covers the whole image
        H, W = GC.POOL_IMAGES[3]
        assert H > ks and W > ks
    x = GC.make_pool_input(1, 12, 13, 4, 0)
    for ks in GC.POOL_KS:
        y, code = GC.maxpool_ref(x, ks)
        p = ks // 2
        assert np.isneginf(y[0, min(p, 11), min(p, 12), 1]) if ks <= 11 else True
        assert code[0, 0, 0, 1] == p * ks + p                        # all -inf: the first valid tap of a corner window
        if ks >= 3:                                                  # the window of (0, 0) holds both NaNs: the last wins
            assert GC.bits(y[0, 0, 0, 2]) == GC.NAN_B and GC.bits(y[0, 1, 1, 2]) == GC.NAN_B
            assert code[0, 0, 0, 2] == (p + 1) * ks + p + 1
        assert np.isposinf(y[0, 11, 12, 3])
        fin = np.isfinite(y)
        assert code.min() >= 0 and code.max() <= ks * ks - 1 <= 127
        # ties: most windows of ks >= 3 hold their maximum more than once
        if ks >= 3:
            yy, cc = GC.maxpool_ref(GC.make_pool_finite(1, 12, 13, 4, 0), ks)
            _, last = _pool_variant(GC.make_pool_finite(1, 12, 13, 4, 0), ks, ties_last=True)
            assert (cc != last).mean() > 0.5
        assert fin.any()


def test_nearest_cases():
    assert GC.fp32_map_differs(64)[0] == GC.ROUNDING_PAIR == (14, 46)
    assert ((14, 3), (46, 5)) in GC.NEAREST_SIZES
    hs = GC.nearest_index(3, 4099)
    assert np.bincount(hs).tolist() == [1367, 1366, 1366]           # the block of source 2 starts 2733 destinations in
    assert np.bincount(GC.nearest_index(10, 7), minlength=10).min() == 0    # downsampling: sources without destinations
    assert np.bincount(GC.nearest_index(17, 1), minlength=17).tolist() == [1] + [0] * 16
    assert np.array_equal(GC.nearest_index(9, 9), np.arange(9))
    assert np.array_equal(GC.nearest_index(19, 38), np.arange(38) // 2)
    assert len(set(np.bincount(GC.nearest_index(38, 75)))) == 2     # blocks of 1 and 2
    for (H, W), (fh, fw) in GC.NEAREST_FACTORS:
        assert np.array_equal(GC.nearest_index(H, H * fh, True), np.arange(H * fh) // fh)
    assert [f for _, f in GC.NEAREST_FACTORS] == [(1, 1), (2, 3), (4, 1)]


def test_amax_cases():
    kinds = {}
    for name, x, C, off, kind in GC.amax_cases():
        M, ld = x.shape
        assert GC.amax_plan(BASE + 4 * off, ld, M, C)[0] == kind, name
        assert GC.rc_amax(BASE, BASE, ld, M, C) == 0
        kinds.setdefault(kind, []).append(name)
        pad = x[:, C:]
        assert (pad.size or name == 'strided C6 ld6') and ((pad == GC.PAD_HUGE) | GC.is_sentinel(pad)).all(), name
        assert GC.amax_ref(x, C) < GC.bits(GC.PAD_HUGE)
    # the strided kernel three ways
    assert any('ld%4' in n for n in kinds['strided']) and any('base+1' in n for n in kinds['strided'])
    assert 'strided C6 ld6' in kinds['strided'] and GC.amax_plan(BASE, 6, 9, 6)[0] == 'strided'
    assert GC.amax_plan(BASE, 8, 0, 5) == ('none', 0, 0)
    words = {n: GC.amax_ref(x, C) for n, x, C, _, _ in GC.amax_cases()}
    assert words['vector C5 first'] == GC.bits(F32(55.5)) and words['vector C5 middle'] == GC.bits(F32(77.25))
    assert words['vector zeros'] == 0 and words['strided -0.0'] == 0 and words['vector denormals'] == 5
    assert words['vector inf'] == 0 and words['strided nan'] == 0


@pytest.mark.parametrize('entry', sorted(GC.REJECTS))
def test_rejections_follow_from_the_host_code(entry):
    assert GC.mirror_rc(entry, GC.reject_args(entry, {})) == 0       # the base call is valid
    names = [n for n, _, _ in GC.REJECTS[entry]]
    assert len(set(names)) == len(names)
    for name, over, rc in GC.REJECTS[entry]:
        assert rc in (GC.ERR_SHAPE, GC.ERR_NULL)
        assert GC.mirror_rc(entry, GC.reject_args(entry, over)) == rc, (entry, name)


# ------------------------------------------------------------------------------------------ references against torch
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _nhwc(t):
    return np.transpose(t.detach().numpy(), (0, 2, 3, 1))


@pytest.mark.parametrize('ks', GC.POOL_KS)
def test_maxpool_reference_against_torch(ks):
    for H, W in GC.POOL_IMAGES:
        for B in GC.POOL_BATCH:
            x = GC.make_pool_input(B, H, W, 8, ks + H)
            y, _ = GC.maxpool_ref(x, ks)
            ty = _nhwc(F.max_pool2d(_nchw(x), ks, 1, ks // 2))
            assert np.array_equal(y, ty, equal_nan=True), (H, W, B)
            xf = GC.make_pool_finite(B, H, W, 8, ks + W)
            xf[0, :11, :11, 1] = -np.inf                             # no NaN, but a window of -inf
            y, code = GC.maxpool_ref(xf, ks)
            ty, ti = F.max_pool2d(_nchw(xf), ks, 1, ks // 2, return_indices=True)
            assert np.array_equal(y, _nhwc(ty)) and np.array_equal(GC.code_to_flat(code, ks), _nhwc(ti)), (H, W, B)
            # backward: torch scatters dy to the recorded index
            dy = np.random.RandomState(ks).randint(-8, 9, xf.shape).astype(F32)      # small integers: every sum is exact
            t = _nchw(xf).requires_grad_(True)
            F.max_pool2d(t, ks, 1, ks // 2).backward(_nchw(dy))
            dx, sa, k = GC.maxpool_bwd_ref(dy, code, ks)
            assert np.array_equal(dx, _nhwc(t.grad)) and (k <= ks * ks).all() and (sa >= np.abs(dx)).all()
            old = np.ones(xf.shape, F32)
            dx1, _, k1 = GC.maxpool_bwd_ref(dy, code, ks, old)
            assert np.array_equal(dx1, dx + 1) and np.array_equal(k1, k + 1)


def test_upsample_references_against_torch():
    rng = np.random.RandomState(3)
    for (H, W), (Ho, Wo) in GC.NEAREST_SIZES:
        x = rng.standard_normal((2, H, W, 4)).astype(F32)
        t = _nchw(x).requires_grad_(True)
        ty = F.interpolate(t, size=(Ho, Wo), mode='nearest')
        assert np.array_equal(GC.nearest_ref(x, Ho, Wo), _nhwc(ty)), ((H, W), (Ho, Wo))
        dy = rng.randint(-8, 9, (2, Ho, Wo, 4)).astype(F32)          # small integers: torch's fp32 sums are exact
        ty.backward(_nchw(dy))
        dx, sa, k = GC.nearest_bwd_ref(dy, H, W)
        assert np.array_equal(dx, _nhwc(t.grad)), ((H, W), (Ho, Wo))
        assert k.sum() == 2 * Ho * Wo * 4 and (sa >= np.abs(dx)).all()
    for (H, W), (fh, fw) in GC.NEAREST_FACTORS:
        x = rng.standard_normal((2, H, W, 4)).astype(F32)
        want = torch.from_numpy(x).repeat_interleave(fh, dim=1).repeat_interleave(fw, dim=2).numpy()
        assert np.array_equal(GC.nearest_ref(x, H * fh, W * fw, True), want)
        dy = rng.randint(-8, 9, want.shape).astype(F32)
        dx, _, k = GC.nearest_bwd_ref(dy, H, W, True)
        assert np.array_equal(dx, dy.astype(F64).reshape(2, H, fh, W, fw, 4).sum(axis=(2, 4))) and (k == fh * fw).all()
    for H, W in GC.UP2_IMAGES:
        x = rng.standard_normal((2, H, W, 4)).astype(F32)
        want = torch.from_numpy(x).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).numpy()
        assert np.array_equal(GC.upsample2x_ref(x), want)
        assert np.array_equal(GC.upsample2x_ref(x), GC.nearest_ref(x, 2 * H, 2 * W))
        dy = rng.randint(-8, 9, want.shape).astype(F32)
        dx, sa = GC.upsample2x_bwd_ref(dy)
        assert np.array_equal(dx, GC.nearest_bwd_ref(dy, H, W)[0]) and (sa >= np.abs(dx)).all()


def _torch_act(act):
    return {GC.ACT_LINEAR: torch.nn.Identity(), GC.ACT_LEAKY: torch.nn.LeakyReLU(0.1), GC.ACT_MISH: torch.nn.Mish(),
            GC.ACT_RELU: torch.nn.ReLU()}[act]


@pytest.mark.parametrize('act', GC.ACTS, ids=GC.ACT_NAMES.get)
def test_activation_references_against_torch(act):
    """in double, over the grid and the bulk: values and autograd to 1e-12 of the element (of the sum of the derivative's
    absolute addends); NaN and infinities where torch has them, except mish'(+inf), where the reference takes the limit"""
    x, dy = GC.make_act_input(4096, 5)
    x64, dy64 = x.astype(F64), dy.astype(F64)
    t = torch.from_numpy(x64).requires_grad_(True)
    ty = _torch_act(act)(t)
    ty.backward(torch.from_numpy(dy64))
    want, wgrad = ty.detach().numpy(), t.grad.numpy()
    ref = GC.act_ref64(x64, act)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(ref), nan)
    with np.errstate(invalid='ignore'):
        assert np.all((np.abs(ref - want) <= 1e-12 * np.abs(want)) | nan | (ref == want))
    if act == GC.ACT_MISH:
        d, A = GC.mish_grad_ref64(x64)
        assert np.isnan(want[np.isneginf(x64)]).all() and np.isnan(wgrad[np.isneginf(x64)]).all()
        assert (want[np.isposinf(x64)] == np.inf).all()
        assert (d[np.isposinf(x64)] == 1.0).all() and (d[(x64 >= 50) & np.isfinite(x64)] == 1.0).all()
        assert GC.act_grad_ref64(np.array([1e17, 1e22, GC.FLT_MAX]), act).tolist() == [1.0, 1.0, 1.0]
    else:
        d, A = GC.act_grad_ref64(x64, act), 1.0
    g = dy64 * d
    # left out: mish'(+inf) (the limit here, inf * 0 in torch); relu' and leaky' at NaN (0 and 0.1 here, as `x > 0` reads)
    skip = np.isposinf(x64) if act == GC.ACT_MISH else np.isnan(x64)
    nan = np.isnan(wgrad)
    assert np.array_equal(np.isnan(g)[~skip], nan[~skip])
    with np.errstate(invalid='ignore'):
        close = (np.abs(g - wgrad) <= 1e-12 * np.abs(A * dy64)) | (g == wgrad)
    assert np.all(close | nan | skip)
    if act != GC.ACT_MISH:                                           # the fp32 forms against torch in float
        t = torch.from_numpy(x).requires_grad_(True)
        ty = _torch_act(act)(t)
        ty.backward(torch.from_numpy(dy))
        assert np.array_equal(GC.act_f32(x, act), ty.detach().numpy(), equal_nan=True)
        xn = ~np.isnan(x)
        assert np.array_equal(GC.act_grad_f32(x, dy, act)[xn], t.grad.numpy()[xn], equal_nan=True)
        nanx = np.array([np.nan], F32)
        want = {GC.ACT_LINEAR: 1.5, GC.ACT_RELU: 0.0, GC.ACT_LEAKY: float(F32(1.5) * F32(0.1))}[act]
        assert float(GC.act_grad_f32(nanx, np.array([1.5], F32), act)[0]) == want
        assert np.isnan(GC.act_f32(nanx, act)[0])


# ------------------------------------------------------------------------------------------ the rounded reference passes
@functools.lru_cache(maxsize=None)
def _act_input(n):
    x, dy = GC.make_act_input(n, n % 97)
    x.setflags(write=False)
    dy.setflags(write=False)
    return x, dy


@pytest.mark.parametrize('n', GC.ACT_SIZES + (4099, GC.BIG_ACT))
def test_mish_bounds_hold_for_the_rounded_reference(n):
    x, dy = _act_input(n)
    with np.errstate(invalid='ignore', over='ignore'):
        ref, bound = GC.mish_fwd_ref(x)
        ok, used = GC.mish_fwd_accept(ref.astype(F32), x)
        assert ok.all() and used.max() <= 1.0
        ref, bound = GC.mish_bwd_ref(x, dy)
        ok, used = GC.mish_bwd_accept(ref.astype(F32), x, dy)
        assert ok.all() and used.max() <= 1.0
    for act in (GC.ACT_LINEAR, GC.ACT_LEAKY, GC.ACT_RELU):
        assert GC.act_fwd_accept(GC.act_f32(x, act), x, act)[0].all()
        assert GC.act_bwd_accept(GC.act_grad_f32(x, dy, act), x, dy, act)[0].all()


def test_sum_bounds_hold_for_the_rounded_reference():
    rng = np.random.RandomState(9)
    for (H, W), (Ho, Wo) in GC.NEAREST_SIZES:
        dy = rng.standard_normal((2, Ho, Wo, 4)).astype(F32)
        dx, sa, k = GC.nearest_bwd_ref(dy, H, W)
        ok, used = GC.sum_accept(dx.astype(F32), dx, sa, k)
        assert ok.all() and used.max() <= 1.0
        assert (dx[k == 0] == 0).all()
    for (H, W), (fh, fw) in GC.NEAREST_FACTORS:
        dy = rng.standard_normal((2, H * fh, W * fw, 4)).astype(F32)
        dx, sa, k = GC.nearest_bwd_ref(dy, H, W, True)
        assert GC.sum_accept(dx.astype(F32), dx, sa, k)[0].all()
    for shape in [(2, 2 * H, 2 * W, 4) for H, W in GC.UP2_IMAGES] + [(1, 2 * GC.BIG_IMAGE[1], 2 * GC.BIG_IMAGE[2], 4)]:
        dy = rng.standard_normal(shape).astype(F32)
        dx, sa = GC.upsample2x_bwd_ref(dy)
        assert GC.sum_accept(dx.astype(F32), dx, sa, 4)[0].all()
    for ks in GC.POOL_KS:
        for H, W in GC.POOL_IMAGES:
            x = GC.make_pool_input(3, H, W, 4, ks)
            _, code = GC.maxpool_ref(x, ks)
            dy = rng.standard_normal(x.shape).astype(F32)
            for old in (None, rng.standard_normal(x.shape).astype(F32)):
                dx, sa, k = GC.maxpool_bwd_ref(dy, code, ks, old)
                assert GC.sum_accept(dx.astype(F32), dx, sa, k)[0].all()
                assert k.max() <= ks * ks + (old is not None)
                none = k == (old is not None)                        # inputs no output selected
                assert np.array_equal(dx[none], (old[none].astype(F64) if old is not None else np.zeros(none.sum())))


# ------------------------------------------------------------------------------------------ planted faults
def _pool_variant(x, ks, ties_last=False, skip_nan=False):
    """the pool with one rule of ATen's replaced: `>=` instead of `>`, or a NaN that does not replace the maximum"""
    B, H, W, C = x.shape
    p = ks // 2
    best = np.full(x.shape, -np.inf, dtype=F32)
    code = np.full(x.shape, -1, dtype=np.int8)
    for r in range(ks):
        for q in range(ks):
            dh, dw = r - p, q - p
            h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
            if h0 >= h1 or w0 >= w1:
                continue
            v = x[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
            b, c = best[:, h0:h1, w0:w1], code[:, h0:h1, w0:w1]
            c[c < 0] = r * ks + q
            with np.errstate(invalid='ignore'):
                take = (v >= b) if ties_last else (v > b)
                if not skip_nan:
                    take |= np.isnan(v)
            b[take] = v[take]
            c[take] = r * ks + q
    return best, code


def test_bit_exact_checks_reject_planted_faults():
    rng = np.random.RandomState(1)
    M, C, ld = 7, 12, 20
    x = rng.standard_normal((M, C)).astype(F32)
    want = GC.pad_rows(x, ld)
    assert GC.same_bits(want, want).all()
    dropped = want.copy()
    dropped[M - 1, :C] = GC.sentinel((C,))                           # the last row never written
    assert not GC.same_bits(dropped, want).all()
    off = GC.sentinel((M + 1, ld))                                   # every row written one pitch further
    off[1:, :C] = x
    assert not GC.same_bits(off[:M], want).all() and not GC.is_sentinel(off[M]).all()
    neg0 = np.array([-0.0], F32)                                     # +0 for -0 is a different word
    assert not GC.same_bits(neg0, np.array([0.0], F32)).all()
    # the pool: ties to the last maximum, a NaN that loses against the running maximum
    xp = GC.make_pool_input(1, 12, 13, 4, 2)
    for ks in (3, 5, 11):
        y, code = GC.maxpool_ref(xp, ks)
        y2, code2 = _pool_variant(xp, ks, ties_last=True)
        assert not np.array_equal(code, code2)
        y3, _ = _pool_variant(xp, ks, skip_nan=True)
        assert not GC.same_bits(y3, y).all()
    # amax: a pad column or an infinity that counts
    for name, xa, Ca, _, _ in GC.amax_cases():
        assert GC.amax_ref(xa, xa.shape[1]) != GC.amax_ref(xa, Ca) or xa.shape[1] == Ca, name
    xi = np.array([[1.0, -np.inf, 2.0, np.nan]], F32)
    assert GC.amax_ref(xi, 4) == GC.bits(F32(2.0)) != int((GC.bits(xi) & 0x7fffffff)[GC.bits(xi) & 0x7fffffff <= 0x7f800000].max())
    assert GC.merge_ref(3, 5) == 5 and GC.merge_ref(5, 0) == 5


def _moved(ref, bound, times=8.0):
    """every finite element moved by `times` of its own bound (+ as many TINY)"""
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(ref), ref + times * (bound + GC.TINY), ref)


def test_bounds_reject_planted_faults():
    rng = np.random.RandomState(2)
    # x2 adjoint without one of its four terms
    dy = rng.standard_normal((2, 6, 4, 4)).astype(F32)
    dx, sa = GC.upsample2x_bwd_ref(dy)
    three = dx - dy.astype(F64)[:, 1::2, 1::2]
    assert not GC.sum_accept(three.astype(F32), dx, sa, 4)[0].any()
    assert not GC.sum_accept(_moved(dx, GC.sum_bound(sa, 4)), dx, sa, 4)[0].any()
    # nearest adjoint: the last source row dropped; a source pixel without destinations that is not exactly 0
    dy = rng.standard_normal((1, 7, 5, 4)).astype(F32)
    dx, sa, k = GC.nearest_bwd_ref(dy, 10, 10)
    got = dx.astype(F32)
    assert GC.sum_accept(got, dx, sa, k)[0].all()
    bad = got.copy()
    bad[:, -1] = 0
    assert not GC.sum_accept(bad, dx, sa, k)[0][:, -1][k[:, -1] > 0].any()
    bad = got.copy()
    bad[k == 0] = F32(1e-30)
    assert not GC.sum_accept(bad, dx, sa, k)[0][k == 0].any()
    assert not GC.sum_accept(_moved(dx, GC.sum_bound(sa, k)), dx, sa, k)[0][k >= 2].any()
    one = (k == 1) & (dx != 0)                                       # one addend: no rounding, one ulp off is refused
    assert one.any() and not GC.sum_accept(np.nextafter(got, F32(np.inf)), dx, sa, k)[0][one].any()
    # pool backward with accumulate: the old value lost
    x = GC.make_pool_finite(1, 6, 6, 4, 0)
    _, code = GC.maxpool_ref(x, 3)
    dyp, old = rng.standard_normal(x.shape).astype(F32), rng.standard_normal(x.shape).astype(F32)
    dx, sa, k = GC.maxpool_bwd_ref(dyp, code, 3, old)
    dx0 = GC.maxpool_bwd_ref(dyp, code, 3)[0]
    assert not GC.sum_accept(dx0.astype(F32), dx, sa, k)[0].any()
    # mish'(1e17) = 2.7, a zero gradient turned NaN at 1e22, a NaN input answered with 1
    x = np.array([1e17, 1e22, np.nan, 1e17], F32)
    dyv = np.array([1.0, 0.0, 1.0, 0.0], F32)
    assert GC.mish_bwd_accept(np.array([1.0, 0.0, np.nan, 0.0], F32), x, dyv)[0].all()
    assert GC.mish_bwd_accept(np.array([2.7, np.nan, 1.0, 0.0], F32), x, dyv)[0].tolist() == [False, False, False, True]
    assert not GC.mish_fwd_accept(np.array([np.inf], F32), np.array([GC.FLT_MAX], F32))[0].any()
    assert not GC.mish_fwd_accept(np.array([0.0], F32), np.array([np.nan], F32))[0].any()
    # an element moved by 8 of its own bounds
    xs, dys = GC.make_act_input(2048, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        ref, bound = GC.mish_fwd_ref(xs)
        assert not GC.mish_fwd_accept(_moved(ref, bound), xs)[0][np.isfinite(ref)].any()
        ref, bound = GC.mish_bwd_ref(xs, dys)
        assert not GC.mish_bwd_accept(_moved(ref, bound), xs, dys)[0][np.isfinite(ref)].any()
    for act in (GC.ACT_LINEAR, GC.ACT_LEAKY, GC.ACT_RELU):           # the bit-exact activations: one ulp is enough
        fin = np.isfinite(xs) & (xs != 0)
        y = GC.act_f32(xs, act)
        with np.errstate(over='ignore'):
            assert not GC.act_fwd_accept(np.nextafter(y, F32(np.inf)), xs, act)[0][fin & (y != 0)].any()
