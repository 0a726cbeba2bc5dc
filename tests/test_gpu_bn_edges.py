# -*- coding: utf-8 -*-
"""The BatchNorm family of csrc/pointwise.hip -- statistics, the two-stage folds, finalize, the analytic plane bound, apply
+ activation (+ skip) in its five output forms, the two backward passes, the bias gradient and the eval fold -- each driven
through the C ABI at the sizes where the host picks another thread map or a kernel takes another branch: channel counts
whose C / 4 is no power of two, row counts around one trip of 4 rpb rows, a grid over its cap, nrows = 5.

The references, formats and acceptance criteria are tests/bn_cases.py (fp64, from the definitions); tests/test_bn_cases.py
shows, without a GPU, that every case used here reaches the branch it is listed for.  Every output buffer is filled with a
NaN bit pattern no kernel produces before the call: pitch padding, neighbouring channel slices, the second half of bf16
rows and a guard behind every buffer must still hold it afterwards."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_cases as BC

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
G = 32                                   # guard words (128 B) in front of and behind every device buffer
USED = {}                                # group -> largest share of its allowance used so far (printed per test)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import check, lib
    return lib(), ops._ptr, ops._stream, check


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

    def ptr(self, off_words=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (G + off_words))

    def get(self):
        """the body as uint32 words; the guards must be untouched"""
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:G] == BC.SENT).all() and (h[G + self.n:] == BC.SENT).all(), 'write outside the buffer'
        return h[G:G + self.n].copy()


def _f32(words):
    return np.ascontiguousarray(words).view(F32)


def _note(group, used, allowed, what=''):
    """print the constant a check needed (share of the bound used, scaled to the allowance) and keep the group's maximum"""
    m = float(np.max(used)) if np.size(used) else 0.0
    USED[group] = max(USED.get(group, 0.0), m)
    print('%s %s: constant needed %.3f (allowed %.1f); group maximum so far %.3f'
          % (group, what, m * allowed, allowed, USED[group] * allowed))


def _worst(ok, got, ref, bound):
    bad = np.argwhere(~ok)[:5]
    bound = np.broadcast_to(bound, np.shape(ref))
    return [(tuple(i), float(np.asarray(got)[tuple(i)]), float(np.asarray(ref)[tuple(i)]), float(bound[tuple(i)])) for i in bad]


@functools.lru_cache(maxsize=64)
def _case(M, C):
    case = BC.make_case(M, C)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=64)
def _apply_ref(M, C, act, res):
    c = _case(M, C)
    return BC.apply_ref64(c['y'], c['mean'], c['invstd'], c['gamma'], c['beta'], act, c['res'] if res else None)


@functools.lru_cache(maxsize=64)
def _bwd_ref(M, C, act, frozen):
    c = _case(M, C)
    return BC.bwd_ref64(c['dz'], c['y'], c['mean'], c['invstd'], c['gamma'], c['beta'], act, frozen)


def _vec(dev, a):
    return Buf(dev, np.size(a), np.asarray(a, dtype=F32))


# ------------------------------------------------------------------------------------------ statistics
def _run_stats(dev, y, ld, running, ws_short=0):
    """y4_bn_stats_f32 on y [M, C] at pitch ld -> (rc, mean, invstd, running mean, running var, counter)"""
    L, _, stream, _ = _abi()
    M, C = y.shape
    nbytes = L.y4_bn_workspace(M, C)
    assert nbytes == BC.bn_workspace(M, C) and nbytes % 4 == 0
    yd = Buf(dev, M * ld, BC.pad_rows(y, ld))
    ws = Buf(dev, nbytes // 4)
    mean, invstd = Buf(dev, C), Buf(dev, C)
    rm0, rv0 = np.linspace(-1, 1, C).astype(F32), np.linspace(0.5, 2, C).astype(F32)
    rm, rv = (_vec(dev, rm0), _vec(dev, rv0)) if running else (None, None)
    nbt = Buf(dev, 2, np.array([41], dtype=np.int64)) if running else None
    rc = L.y4_bn_stats_f32(yd.ptr(), ld, M, C, mean.ptr(), invstd.ptr(), rm.ptr() if running else None,
                           rv.ptr() if running else None, nbt.ptr() if running else None, BC.MOMENTUM, BC.EPS, ws.ptr(),
                           nbytes - ws_short, stream())
    torch.cuda.synchronize()
    ws.get()
    out = dict(rc=rc, mean=mean.get(), invstd=invstd.get(), rm0=rm0, rv0=rv0)
    if running:
        out.update(rm=_f32(rm.get()), rv=_f32(rv.get()), nbt=int(nbt.get().view(np.int64)[0]))
    return out


def _check_stats(o, st, what, running):
    assert o['rc'] == 0
    mean, invstd = _f32(o['mean']), _f32(o['invstd'])
    ok, used = BC.mean_accept(mean, st)
    _note('stats.mean', used, 1.0, what)
    assert ok.all(), _worst(ok, mean, st['mean'], st['dmean'])
    ok, used = BC.invstd_accept(invstd, st)
    _note('stats.invstd', used, 1.0, what)
    assert ok.all(), _worst(ok, invstd, st['invstd'], st['dvar'])
    if running:
        nm, bm, nv, bv = BC.running_ref64(st, o['rm0'], o['rv0'])
        ok, used = BC.judge(o['rm'], nm, bm)
        _note('stats.running_mean', used, BC.RUN_CONST, what)
        assert ok.all(), _worst(ok, o['rm'], nm, bm)
        ok, used = BC.judge(o['rv'], nv, bv)
        _note('stats.running_var', used, BC.RUN_CONST, what)
        assert ok.all(), _worst(ok, o['rv'], nv, bv)
        assert o['nbt'] == 42


@pytest.mark.parametrize('C', BC.CHANNELS)
def test_stats(dev, C):
    """y4_bn_stats_f32 over the M list at both pitches, with and without the running buffers: mean, invstd and the running
    statistics under the bounds of bn_cases.stats_ref64 (channels with |mean| / std of 0, 10 and 1000 and constant
    channels), the counter up by exactly 1, a second call bit-identical, a workspace one byte short refused."""
    for M in BC.m_list(C):
        case = _case(M, C)
        for ld in (C, C + 8):
            for running in (True, False):
                o = _run_stats(dev, case['y'], ld, running)
                _check_stats(o, case['stats'], 'C%d M%d ld%d' % (C, M, ld), running)
                if ld == C and running:
                    first = o
                else:
                    assert np.array_equal(o['mean'], first['mean']) and np.array_equal(o['invstd'], first['invstd'])
        if M == 1:                                                     # the mean of one row is that row
            assert np.array_equal(_f32(first['mean']), case['y'][0])
        cc = case['props']['const']
        if cc:                                                         # constant channels: the variance clamps at >= 0
            assert np.isfinite(_f32(first['invstd'])[cc]).all()
            assert (_f32(first['invstd'])[cc] <= F32(1.0 / np.sqrt(F64(F32(BC.EPS))) * (1 + 2.0 ** -22))).all()
        o = _run_stats(dev, case['y'], C, True, ws_short=1)
        assert o['rc'] == BC.ERR_WORKSPACE and (o['mean'] == BC.SENT).all() and o['nbt'] == 41


@pytest.mark.parametrize('C,M', BC.LARGE)
def test_stats_large(dev, C, M):
    case = _case(M, C)
    o = _run_stats(dev, case['y'], C, True)
    _check_stats(o, case['stats'], 'C%d M%d' % (C, M), True)
    o2 = _run_stats(dev, case['y'], C, False)
    assert np.array_equal(o['mean'], o2['mean']) and np.array_equal(o['invstd'], o2['invstd'])


# ------------------------------------------------------------------------------------------ finalize from partial rows
@pytest.mark.parametrize('C', BC.FOLD_CHANNELS)
def test_finalize_partials(dev, C):
    """y4_bn_finalize_partials_f32 on synthetic partial rows with a mean 300 standard deviations from 0: every addition
    of the kernels is fp64, so mean and invstd carry one fp32 rounding; a sum held in fp32 anywhere, a dropped partial row
    or a dropped fp64 row is far outside."""
    L, _, stream, _ = _abi()
    nbytes = L.y4_bn_finalize_workspace(C)
    assert nbytes == BC.bn_finalize_workspace(C)
    for nparts in BC.FOLD_NPARTS:
        part, M = BC.make_partials(nparts, C, nparts + C)
        r = BC.partials_ref64(part, M)
        pd = torch.from_numpy(part).to(dev)
        outs = []
        for rep in range(2):
            ws = Buf(dev, nbytes // 4)
            mean, invstd = Buf(dev, C), Buf(dev, C)
            rm, rv = _vec(dev, np.zeros(C)), _vec(dev, np.ones(C))
            nbt = Buf(dev, 2, np.array([7], dtype=np.int64))
            rc = L.y4_bn_finalize_partials_f32(ctypes.c_void_p(pd.data_ptr()), nparts, M, C, mean.ptr(), invstd.ptr(), rm.ptr(),
                                               rv.ptr(), nbt.ptr(), BC.MOMENTUM, BC.EPS, ws.ptr(), nbytes, stream())
            torch.cuda.synchronize()
            assert rc == 0
            ws.get()
            outs.append((mean.get(), invstd.get(), rm.get(), rv.get()))
            assert int(nbt.get().view(np.int64)[0]) == 8
        assert all(np.array_equal(a, b) for a, b in zip(*outs))
        what = 'C%d nparts%d nb%d' % (C, nparts, BC.fold_plan(nparts, C)[0])
        mean, invstd = _f32(outs[0][0]), _f32(outs[0][1])
        ok, used = BC.mean_accept(mean, r)
        _note('finalize.mean', used, 1.0, what)
        assert ok.all(), (what, _worst(ok, mean, r['mean'], r['dmean']))
        ok, used = BC.invstd_accept(invstd, r)
        _note('finalize.invstd', used, 1.0, what)
        assert ok.all(), (what, _worst(ok, invstd, r['invstd'], r['dvar']))
        nm, bm, nv, bv = BC.running_ref64(r, np.zeros(C), np.ones(C))
        ok, _ = BC.judge(_f32(outs[0][2]), nm, bm)
        assert ok.all(), what
        ok, _ = BC.judge(_f32(outs[0][3]), nv, bv)
        assert ok.all(), what
    ws = Buf(dev, nbytes // 4)
    mean = Buf(dev, C)
    assert L.y4_bn_finalize_partials_f32(ctypes.c_void_p(pd.data_ptr()), 1, 64, C, mean.ptr(), mean.ptr(), None, None, None,
                                         BC.MOMENTUM, BC.EPS, ws.ptr(), nbytes - 1, stream()) == BC.ERR_WORKSPACE


# ------------------------------------------------------------------------------------------ plane bound
@pytest.mark.parametrize('C', BC.BOUND_CHANNELS)
def test_planes_bound(dev, C):
    """y4_bn_planes_bound_f32 bit-equal to the fp32 evaluation in the kernel's operation order; floor_word: the larger
    word wins and a poisoned (Inf / NaN) word stays poisoned"""
    L, _, stream, _ = _abi()
    rng = np.random.RandomState(C)
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.randint(0, 2, C) > 0, 1, -1)).astype(F32)
    beta = rng.standard_normal(C).astype(F32)
    gamma[C - 1] = F32(-1.75)                                           # the maximum sits in the last channel
    gd, bd = _vec(dev, gamma), _vec(dev, beta)
    for M in (1, 2, 361, 369664):
        plain = BC.planes_bound_f32(gamma, beta, M)
        for floor in (None, 0, plain - 1, plain + 1, 0x7f800000, 0x7fc00000):
            out = Buf(dev, 1)
            fl = Buf(dev, 1, np.array([floor], dtype=np.uint32)) if floor is not None else None
            rc = L.y4_bn_planes_bound_f32(gd.ptr(), bd.ptr(), C, M, fl.ptr() if fl else None, out.ptr(), stream())
            torch.cuda.synchronize()
            assert rc == 0
            got = int(out.get()[0])
            assert got == BC.planes_bound_f32(gamma, beta, M, None, floor), (M, floor, hex(got))
            assert got == (plain if floor is None else max(plain, floor))
    g2 = gamma.copy()
    g2[C // 2] = np.inf
    out = Buf(dev, 1)
    assert L.y4_bn_planes_bound_f32(_vec(dev, g2).ptr(), bd.ptr(), C, 100, None, out.ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert int(out.get()[0]) == 0x7f800000


# ------------------------------------------------------------------------------------------ apply
def _run_apply(dev, y, stats, gamma, beta, act, res=None, ldy=None, ldr=None, ldz=None, off=0, word=0, z_planes=0,
               res_word=None, twin=False, store=True, ybf=False):
    """One y4_bn_act_fwd_f32 call.  z is the channel slice [off, off + C) of a sentinel-filled [M, ldz] tensor; everything
    outside the slice must still hold the sentinel.  Returns dict(rc, z = the slice's raw words [M, C], word, twin)."""
    L, _, stream, _ = _abi()
    M, C = y.shape
    ldy, ldr, ldz = ldy or C, ldr or C, ldz or C
    assert ldz >= off + C
    yd = Buf(dev, M * ldy, BC.bf16_rows(y, ldy) if ybf else BC.pad_rows(y, ldy))
    rd = Buf(dev, M * ldr, BC.pad_rows(res, ldr)) if res is not None else None
    zd = Buf(dev, M * ldz) if store else None
    wd = Buf(dev, 1, np.array([word], dtype=np.uint32))
    rw = Buf(dev, 1, np.array([res_word], dtype=np.uint32)) if res_word is not None else None
    td = Buf(dev, M * C) if twin else None
    v = [_vec(dev, t) for t in (stats[0], stats[1], gamma, beta)]
    rc = L.y4_bn_act_fwd_f32(yd.ptr(), ldy, v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), act, rd.ptr() if rd else None, ldr,
                             zd.ptr(off) if store else None, ldz, M, C, wd.ptr(), z_planes + (16 if ybf else 0),
                             rw.ptr() if rw else None, td.ptr() if twin else None, stream())
    torch.cuda.synchronize()
    out = dict(rc=rc, word=int(wd.get()[0]))
    if store:
        body = zd.get().reshape(M, ldz)
        assert (body[:, :off] == BC.SENT).all() and (body[:, off + C:] == BC.SENT).all(), 'write outside the channel slice'
        out['z'] = np.ascontiguousarray(body[:, off:off + C])
    if twin:
        out['twin'] = td.get().reshape(M, C)
    return out


def _check_z(z, r, act, group, what):
    ok, used = BC.apply_accept(z, r, act)
    _note(group, used, BC.APPLY_CONST if act != BC.ACT_MISH else BC.MISH_CONST, what)
    assert ok.all(), (what, _worst(ok, z, r['z'], BC.apply_bound(r, act)))


PITCHES = (('dense', 0, 0, 0, 0), ('padded', 8, 8, 8, 4), ('mixed', 8, 0, 8, 0))     # name, ldy - C, ldr - C, ldz - C, slice offset


@pytest.mark.parametrize('act', BC.ACTS, ids=BC.ACT_NAMES.get)
@pytest.mark.parametrize('C', BC.CHANNELS)
def test_apply(dev, C, act):
    """y4_bn_act_fwd_f32, fp32 output, with and without the residual, dense and padded pitches with z a channel slice of a
    wider tensor: every element under bn_cases.apply_accept; *out_amax bit-equal to max|finite z| of the stored z, a larger
    pre-seeded word survives, the measure-only call (z == NULL) leaves the same word."""
    for M in BC.m_list(C):
        c = _case(M, C)
        st = (c['mean'], c['invstd'])
        for res in (False, True):
            r = _apply_ref(M, C, act, res)
            first = None
            for name, py, pr, pz, off in PITCHES:
                o = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], act, c['res'] if res else None, C + py, C + pr, C + pz, off)
                assert o['rc'] == 0
                z = _f32(o['z'])
                _check_z(z, r, act, 'apply.' + BC.ACT_NAMES[act], 'C%d M%d res%d %s' % (C, M, res, name))
                assert o['word'] == BC.amax_word(z)
                if first is None:
                    first = o
                else:                                                   # the pitch changes no arithmetic
                    assert np.array_equal(o['z'], first['z'])
            big = first['word'] + 12345
            o = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], act, c['res'] if res else None, word=big)
            assert o['word'] == big and np.array_equal(o['z'], first['z'])
            o = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], act, c['res'] if res else None, store=False)
            assert o['rc'] == 0 and o['word'] == first['word']


@pytest.mark.parametrize('act', BC.ACTS, ids=BC.ACT_NAMES.get)
def test_apply_nonfinite(dev, act):
    """a NaN, a +Inf and a -Inf in y come out as the fp64 reference has them (NaN stays NaN through every activation,
    ReLU included) at those elements only; the amax word is the maximum of the finite results"""
    for C, M in ((36, 289), (1028, 10), (4, 1)):
        c = _case(M, C)
        y, sites = BC.plant_nonfinite(c['y'])
        for res in (None, c['res']):
            with np.errstate(invalid='ignore', over='ignore'):
                r = BC.apply_ref64(y, c['mean'], c['invstd'], c['gamma'], c['beta'], act, res)
            o = _run_apply(dev, y, (c['mean'], c['invstd']), c['gamma'], c['beta'], act, res)
            z = _f32(o['z'])
            special = ~np.isfinite(y)
            assert special.sum() == 3
            for m, ch, name in sites:
                if name == 'nan':
                    assert np.isnan(z[m, ch]), (act, name)
                else:
                    assert np.isnan(z[m, ch]) == np.isnan(r['z'][m, ch]) and (np.isnan(z[m, ch]) or z[m, ch] == r['z'][m, ch]), (act, name, z[m, ch], r['z'][m, ch])
            assert np.isfinite(z[~special]).all()
            rr = {k: np.where(special, 0.0, v) for k, v in r.items()}
            ok, _ = BC.apply_accept(np.where(special, 0.0, z), rr, act)
            assert ok.all()
            assert o['word'] == BC.amax_word(z)


@pytest.mark.parametrize('C', BC.PLANE_CHANNELS)
def test_apply_planes(dev, C):
    """The plane forms of y4_bn_act_fwd_f32: z_planes 1 (f16x2 at the scale of a given word), 2 (the same at the analytic
    bound) and 3 (bf16), into z itself -- dense, and as a 128-byte aligned slice of a wider pre-split tensor -- and into
    planes_twin beside an fp32 z.  With a twin the planes / bf16 rows are bit-equal to the numpy split / RNE of the
    call's own fp32 z; without one the decoded planes meet the fp32 criterion plus the format's own term."""
    for M in BC.m_list(C):
        c = _case(M, C)
        st = (c['mean'], c['invstd'])
        rword = BC.amax_word(c['res'])
        for k, (form, twin, sl) in enumerate((f, t, s) for f in (1, 2, 3) for t, s in ((False, False), (True, False), (False, True))):
            act = BC.ACTS[(k + M) % 4]
            res = (k + M // 2) % 2 == 1
            r = _apply_ref(M, C, act, res)
            what = 'C%d M%d planes%d twin%d slice%d %s res%d' % (C, M, form, twin, sl, BC.ACT_NAMES[act], res)
            given = BC.amax_word((np.abs(r['z']).max() * 1.001).astype(F32)) if form == 1 else 0x12345
            ldz, off = (C + 64, 32) if sl else ((C + 8, 4) if twin else (C, 0))
            o = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], act, c['res'] if res else None, C + 8, C + 8, ldz, off, word=given,
                           z_planes=form, res_word=rword if res else None, twin=twin)
            assert o['rc'] == 0, what
            bound = BC.apply_bound(r, act)
            if form == 2:
                word = BC.planes_bound_f32(c['gamma'], c['beta'], M, rword if res else None)
                assert o['word'] == word and BC.word_value(word) >= np.abs(r['z']).max(), what
            else:
                word = given
                assert o['word'] == given, what
            rows = o['twin'] if twin else o['z']
            if twin:
                z = _f32(o['z'])
                _check_z(z, r, act, 'apply.planes', what)
            if form == 3:
                h = rows.view(np.uint16).reshape(M, 2 * C)
                assert (h[:, C:] == np.array([BC.SENT], np.uint32).view(np.uint16)[np.arange(C) % 2]).all(), what
                if twin:
                    assert np.array_equal(h[:, :C], BC.bf16_rne(z)), what
                else:
                    ok, used = BC.judge(BC.bf16_to_f32(h[:, :C]), r['z'], bound * (1 + 2.0 ** -8) + BC.bf16_error(np.abs(r['z'])))
                    assert ok.all(), what
                continue
            hi, lo = BC.planes_unpack(rows.view(np.uint16).reshape(M, 2 * C))
            assert np.isfinite(hi.astype(F32)).all() and np.isfinite(lo.astype(F32)).all(), what
            if twin:
                eh, el = BC.split_f16x2(z, word)
                same = (hi.view(np.uint16) == eh.view(np.uint16)) & (lo.view(np.uint16) == el.view(np.uint16))
                assert same.all(), (what, np.argwhere(~same)[:5])
            else:
                ps = F64(BC.scale_of(word))
                ok, used = BC.judge(BC.planes_decode(hi, lo, word), r['z'], bound * (1 + 2.0 ** -21) + BC.split_error(np.abs(r['z']) * ps) / ps)
                _note('apply.planes_decoded', used, 1.0, what)
                assert ok.all(), what


@pytest.mark.parametrize('C', (12, 36, 96, 1028))
def test_apply_bf16_input(dev, C):
    """z_planes + 16: y given as bf16 rows (the second half of every row poisoned) gives bit-identical results to the
    fp32-input call on the same bf16-representable values"""
    for M in BC.m_list(C):
        c = _case(M, C)
        y = BC.bf16_to_f32(BC.bf16_rne(c['y']))
        st = (c['mean'], c['invstd'])
        forms = ((0, False), (3, True), (1, True)) if C % 32 == 0 else ((0, False),)
        for form, twin in forms:
            for act, res in ((BC.ACT_MISH, c['res']), (BC.ACT_LEAKY, None)):
                kw = dict(ldy=C + 8, ldz=C + 8, off=4, z_planes=form, twin=twin, word=0x42000000 if form == 1 else 0)
                a = _run_apply(dev, y, st, c['gamma'], c['beta'], act, res, **kw)
                b = _run_apply(dev, y, st, c['gamma'], c['beta'], act, res, ybf=True, **kw)
                assert a['rc'] == 0 and b['rc'] == 0
                assert np.array_equal(a['z'], b['z']) and a['word'] == b['word']
                if twin:
                    assert np.array_equal(a['twin'], b['twin'])
                r = BC.apply_ref64(y, c['mean'], c['invstd'], c['gamma'], c['beta'], act, res)
                _check_z(_f32(b['z']), r, act, 'apply.bf16_input', 'C%d M%d form%d' % (C, M, form))


def test_apply_refused_call_leaves_the_word(dev):
    """z_planes == 2 with ldy < C: Y4_ERR_SHAPE, and *out_amax is untouched (the bound kernel is launched only after
    every check); the same call with a valid pitch writes the bound"""
    L, _, stream, _ = _abi()
    M, C = 8, 32
    c = _case(M, C)
    bufs = [_vec(dev, t) for t in (c['mean'], c['invstd'], c['gamma'], c['beta'])]
    yd = Buf(dev, M * C, c['y'])
    for ldy, want_rc in ((C - 4, BC.ERR_SHAPE), (C, 0)):
        zd, wd = Buf(dev, M * C), Buf(dev, 1, np.array([0x2a], dtype=np.uint32))
        rc = L.y4_bn_act_fwd_f32(yd.ptr(), ldy, bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(), bufs[3].ptr(), BC.ACT_MISH, None, C,
                                 zd.ptr(), C, M, C, wd.ptr(), 2, None, None, stream())
        torch.cuda.synchronize()
        assert rc == want_rc
        if want_rc:
            assert int(wd.get()[0]) == 0x2a and (zd.get() == BC.SENT).all()
        else:
            assert int(wd.get()[0]) == BC.planes_bound_f32(c['gamma'], c['beta'], M)


@pytest.mark.parametrize('C,M', BC.LARGE)
def test_apply_large(dev, C, M):
    """the grid at its cap (the second lap of the `tb += step` loop), the tensor ending inside a trip: fp32 with the
    residual, and planes at the analytic bound beside an fp32 twin"""
    c = _case(M, C)
    st = (c['mean'], c['invstd'])
    r = _apply_ref(M, C, BC.ACT_MISH, True)
    o = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], BC.ACT_MISH, c['res'], ldz=C + 8, off=4)
    z = _f32(o['z'])
    _check_z(z, r, BC.ACT_MISH, 'apply.large', 'C%d M%d' % (C, M))
    assert o['word'] == BC.amax_word(z)
    rword = BC.amax_word(c['res'])
    o2 = _run_apply(dev, c['y'], st, c['gamma'], c['beta'], BC.ACT_MISH, c['res'], z_planes=2, res_word=rword, twin=True)
    assert np.array_equal(o2['z'], o['z'])
    assert o2['word'] == BC.planes_bound_f32(c['gamma'], c['beta'], M, rword)
    hi, lo = BC.planes_unpack(o2['twin'].view(np.uint16).reshape(M, 2 * C))
    eh, el = BC.split_f16x2(z, o2['word'])
    assert np.array_equal(hi.view(np.uint16), eh.view(np.uint16)) and np.array_equal(lo.view(np.uint16), el.view(np.uint16))


# ------------------------------------------------------------------------------------------ backward
def _run_bwd(dev, c, act, y=None, lddz=None, ldy=None, lddy=None, alias=False, flags=0, planes=False, twin=False, word=0):
    """One y4_bn_act_bwd_f32 call -> dict(rc, dy = raw words [M, C], dgamma, dbeta, word, bounds, twin)"""
    L, _, stream, _ = _abi()
    M, C = c['M'], c['C']
    y = c['y'] if y is None else y
    lddz, ldy, lddy = lddz or C, ldy or C, lddy or C
    if alias:
        lddy = lddz
    dzd = Buf(dev, M * lddz, BC.pad_rows(c['dz'], lddz))
    yd = Buf(dev, M * ldy, BC.bf16_rows(y, ldy) if flags & 4 else BC.pad_rows(y, ldy))
    dyd = dzd if alias else Buf(dev, M * lddy)
    v = [_vec(dev, t) for t in (c['mean'], c['invstd'], c['gamma'], c['beta'])]
    dg, db = Buf(dev, C), Buf(dev, C)
    nbytes = L.y4_bn_workspace(M, C)
    ws = Buf(dev, nbytes // 4)
    wd = Buf(dev, 1, np.array([word], dtype=np.uint32))
    bd = Buf(dev, 8, np.zeros(8, dtype=np.uint32)) if planes else None
    td = Buf(dev, M * C) if twin else None
    rc = L.y4_bn_act_bwd_f32(dzd.ptr(), lddz, yd.ptr(), ldy, v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), act, dyd.ptr(), lddy,
                             dg.ptr(), db.ptr(), M, C, ws.ptr(), nbytes, wd.ptr(), bd.ptr() if planes else None,
                             td.ptr() if twin else None, flags, stream())
    torch.cuda.synchronize()
    ws.get()
    body = dyd.get().reshape(M, lddy)
    if rc == 0:
        assert (body[:, C:] == BC.SENT).all(), 'write into the pitch padding'
    out = dict(rc=rc, dy=np.ascontiguousarray(body[:, :C]), dgamma=dg.get(), dbeta=db.get(), word=int(wd.get()[0]))
    if planes:
        out['bounds'] = bd.get()
    if twin:
        out['twin'] = td.get().reshape(M, C)
    return out


def _check_bwd(o, r, act, what, dy=True):
    for key, bk in (('dbeta', 'b_dbeta'), ('dgamma', 'b_dgamma')) + ((('dy', 'b_dy'),) if dy else ()):
        got = _f32(o[key])
        ok, used = BC.judge(got, r[key], r[bk])
        _note('bwd.%s.%s' % (key, BC.ACT_NAMES[act]), used, 1.0, what)
        assert ok.all(), (what, key, _worst(ok, got, r[key], r[bk]))


def _same(a, b, keys=('dy', 'dgamma', 'dbeta', 'word')):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize('act', BC.ACTS, ids=BC.ACT_NAMES.get)
@pytest.mark.parametrize('C', BC.CHANNELS)
def test_backward(dev, C, act):
    """y4_bn_act_bwd_f32 over the M list: dgamma, dbeta and dy under the bounds of bn_cases.bwd_ref64 with lddz != lddy,
    out_amax bit-equal to max|finite dy| of the stored dy, a second call bit-identical, dy aliasing dz, frozen statistics,
    y as bf16 rows; and where C is a whole number of 32-channel tiles dy as bf16 and as f16x2 planes, with and without
    the fp32 twin."""
    for M in BC.m_list(C):
        c = _case(M, C)
        r = _bwd_ref(M, C, act, False)
        what = 'C%d M%d' % (C, M)
        o = _run_bwd(dev, c, act, lddz=C + 8, ldy=C + 8, lddy=C)
        assert o['rc'] == 0
        _check_bwd(o, r, act, what)
        assert o['word'] == BC.amax_word(_f32(o['dy']))
        assert _same(o, _run_bwd(dev, c, act, lddz=C + 8, ldy=C + 8, lddy=C)), what
        assert _same(o, _run_bwd(dev, c, act, lddz=C, ldy=C, lddy=C + 8)), what
        assert _same(o, _run_bwd(dev, c, act, lddz=C + 8, alias=True)), what
        big = o['word'] + 999
        assert _run_bwd(dev, c, act, word=big)['word'] == big
        f = _run_bwd(dev, c, act, lddz=C + 8, lddy=C, flags=1)
        assert f['rc'] == 0
        _check_bwd(f, _bwd_ref(M, C, act, True), act, what + ' frozen')
        assert np.array_equal(f['dgamma'], o['dgamma']) and np.array_equal(f['dbeta'], o['dbeta'])
        assert f['word'] == BC.amax_word(_f32(f['dy']))
        yb = BC.bf16_to_f32(BC.bf16_rne(c['y']))                        # bit 2: y as bf16 rows
        a = _run_bwd(dev, c, act, y=yb, ldy=C + 8)
        b = _run_bwd(dev, c, act, y=yb, ldy=C + 8, flags=4)
        assert a['rc'] == 0 and b['rc'] == 0 and _same(a, b), what
        _check_bwd(b, BC.bwd_ref64(c['dz'], yb, c['mean'], c['invstd'], c['gamma'], c['beta'], act), act, what + ' bf16 y')
        if C % 32:
            continue
        # bit 1: dy as bf16.  With the twin dy stays fp32 (+ its maximum) and the twin holds RNE(dy)
        t = _run_bwd(dev, c, act, lddz=C + 8, lddy=C + 8, flags=2, twin=True)
        assert t['rc'] == 0 and _same(o, t), what
        h = t['twin'].view(np.uint16).reshape(M, 2 * C)
        half = np.array([BC.SENT], np.uint32).view(np.uint16)[np.arange(C) % 2]
        assert np.array_equal(h[:, :C], BC.bf16_rne(_f32(t['dy']))) and (h[:, C:] == half).all(), what
        n = _run_bwd(dev, c, act, lddz=C + 8, flags=2, word=77)
        assert n['rc'] == 0 and n['word'] == 77 and np.array_equal(n['dgamma'], o['dgamma'])
        h = n['dy'].view(np.uint16).reshape(M, 2 * C)
        assert (h[:, C:] == half).all(), what
        ok, _ = BC.judge(BC.bf16_to_f32(h[:, :C]), r['dy'], r['b_dy'] * (1 + 2.0 ** -8) + BC.bf16_error(np.abs(r['dy'])))
        assert ok.all(), what
        assert np.array_equal(h[:, :C], BC.bf16_rne(_f32(o['dy']))), what
        # f16x2 planes at the derived bound
        true_max = float(np.abs(_f32(o['dy'])).max())
        for twin in (True, False):
            p = _run_bwd(dev, c, act, lddz=C + 8, lddy=C + 8 if twin else C, planes=True, twin=twin, word=77)
            assert p['rc'] == 0 and p['word'] == 77, what
            assert np.array_equal(p['dgamma'], o['dgamma']) and np.array_equal(p['dbeta'], o['dbeta'])
            w = [BC.word_value(x) for x in p['bounds'][:6]]
            assert w[5] >= true_max and np.isfinite(w[5]), (what, w)
            # the maxima the bound is made of, each rounded up by 1.0001: never below the true maximum ...
            assert w[0] >= np.abs(r['g']).max() * (1 - 2.0 ** -12) and w[1] >= np.abs(r['xh']).max() * (1 - 2.0 ** -20), (what, w)
            gi = np.abs(c['gamma'].astype(F64) * c['invstd'].astype(F64)).max()
            k1 = np.abs(_f32(o['dbeta']).astype(F64) / M).max()
            k2 = np.abs(_f32(o['dgamma']).astype(F64) / M).max()
            for got, true in ((w[2], gi), (w[3], k1), (w[4], k2), (w[5], w[2] * (w[0] + w[3] + w[1] * w[4]))):
                assert true * 1.00005 - BC.TINY <= got <= true * 1.00015 + BC.TINY, (what, got, true)
            rows = p['twin'] if twin else p['dy']
            hi, lo = BC.planes_unpack(rows.view(np.uint16).reshape(M, 2 * C))
            assert np.isfinite(hi.astype(F32)).all() and np.isfinite(lo.astype(F32)).all(), what
            if twin:
                assert np.array_equal(p['dy'], o['dy']), what
            eh, el = BC.split_f16x2(_f32(o['dy']), int(p['bounds'][5]))
            same = (hi.view(np.uint16) == eh.view(np.uint16)) & (lo.view(np.uint16) == el.view(np.uint16))
            assert same.all(), (what, twin, np.argwhere(~same)[:5])
            assert _same(p, _run_bwd(dev, c, act, lddz=C + 8, lddy=C + 8 if twin else C, planes=True, twin=twin, word=77),
                         ('dy', 'dgamma', 'dbeta', 'bounds')), what


@pytest.mark.parametrize('C,M', BC.LARGE)
def test_backward_large(dev, C, M):
    """nrows = 5 (a four-row trip and a single row per block, the tensor ending inside a trip), the apply grid at its cap"""
    c = _case(M, C)
    r = _bwd_ref(M, C, BC.ACT_MISH, False)
    o = _run_bwd(dev, c, BC.ACT_MISH, lddy=C + 8)
    assert o['rc'] == 0
    _check_bwd(o, r, BC.ACT_MISH, 'C%d M%d' % (C, M))
    assert o['word'] == BC.amax_word(_f32(o['dy']))
    p = _run_bwd(dev, c, BC.ACT_MISH, planes=True, twin=True)
    assert p['rc'] == 0 and np.array_equal(p['dy'], o['dy']) and np.array_equal(p['dgamma'], o['dgamma'])
    assert BC.word_value(p['bounds'][5]) >= np.abs(_f32(o['dy'])).max()
    hi, lo = BC.planes_unpack(p['twin'].view(np.uint16).reshape(M, 2 * C))
    eh, el = BC.split_f16x2(_f32(o['dy']), int(p['bounds'][5]))
    assert np.array_equal(hi.view(np.uint16), eh.view(np.uint16)) and np.array_equal(lo.view(np.uint16), el.view(np.uint16))


def test_backward_refusals(dev):
    c = _case(33, 32)
    assert _run_bwd(dev, c, BC.ACT_MISH, flags=1, planes=True)['rc'] == BC.ERR_SHAPE          # no plane bound with frozen statistics
    assert _run_bwd(dev, c, BC.ACT_MISH, flags=2, lddy=40)['rc'] == BC.ERR_SHAPE              # bf16 dy needs dense rows
    assert _run_bwd(dev, _case(5, 36), BC.ACT_MISH, flags=2)['rc'] == BC.ERR_SHAPE            # ... and whole 32-channel tiles


# ------------------------------------------------------------------------------------------ bias gradient, eval fold
@pytest.mark.parametrize('C', BC.BIAS_CHANNELS)
def test_bias_grad(dev, C):
    L, _, stream, _ = _abi()
    rng = np.random.RandomState(C)
    for M in BC.BIAS_ROWS:
        ld = C + 3
        x = (rng.standard_normal((M, C)) + 0.5).astype(F32)
        s, b = BC.bias_grad_ref64(x)
        nbytes = L.y4_bias_grad_workspace(M, C)
        assert nbytes == BC.colsum_rows(M) * C * 4
        xd = Buf(dev, M * ld, BC.pad_rows(x, ld))
        outs = []
        for rep in range(2):
            ws, out = Buf(dev, nbytes // 4), Buf(dev, C)
            assert L.y4_bias_grad_f32(xd.ptr(), ld, M, C, out.ptr(), ws.ptr(), nbytes, stream()) == 0
            torch.cuda.synchronize()
            ws.get()
            outs.append(out.get())
        assert np.array_equal(outs[0], outs[1])
        ok, used = BC.judge(_f32(outs[0]), s, b)
        _note('bias_grad', used, 1.0, 'C%d M%d' % (C, M))
        assert ok.all(), _worst(ok, _f32(outs[0]), s, b)
        out = Buf(dev, C)
        assert L.y4_bias_grad_f32(xd.ptr(), ld, M, C, out.ptr(), ws.ptr(), nbytes - 1, stream()) == BC.ERR_WORKSPACE
        assert L.y4_bias_grad_f32(xd.ptr(), C - 1, M, C, out.ptr(), ws.ptr(), nbytes, stream()) == BC.ERR_SHAPE
        torch.cuda.synchronize()
        assert (out.get() == BC.SENT).all()


@pytest.mark.parametrize('C', BC.FOLD_EVAL_CHANNELS)
def test_bn_fold(dev, C):
    L, _, stream, _ = _abi()
    rng = np.random.RandomState(C + 5)
    gamma, beta = BC.make_params(C, C)
    rm, rv = rng.standard_normal(C).astype(F32), rng.uniform(0.0, 2.0, C).astype(F32)
    rv[0] = 0.0
    s, bs, sh, bsh = BC.fold_ref64(gamma, beta, rm, rv)
    v = [_vec(dev, t) for t in (gamma, beta, rm, rv)]
    scale, shift = Buf(dev, C), Buf(dev, C)
    assert L.y4_bn_fold_f32(v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), BC.EPS, scale.ptr(), shift.ptr(), C, stream()) == 0
    torch.cuda.synchronize()
    ok, used = BC.judge(_f32(scale.get()), s, bs)
    _note('fold.scale', used, BC.FOLD_CONST, 'C%d' % C)
    assert ok.all()
    ok, used = BC.judge(_f32(shift.get()), sh, bsh)
    _note('fold.shift', used, BC.FOLD_CONST, 'C%d' % C)
    assert ok.all()
