# -*- coding: utf-8 -*-
"""References, operand builders, seeded inputs, case lists and acceptance criteria for the direct tests of the plane conv
kernels of csrc/conv_planes.hip (tests/test_conv_cases.py checks them on the CPU, tests/test_gpu_conv_planes_edges.py feeds
them to the kernels through the C ABI).

Four parts, numpy only, on top of tests/bn_cases.py (formats, judge, the sentinel):
  * a mirror of the HOST dispatch (which kernel a call reaches, under the name y4_last_conv_kernel reports; partial rows;
    the parity classes of the stride-2 dgrad; the split-K plan of wgrad): it lets a case STATE its branch and supplies the
    chain lengths of the bounds; it is never the reference of a value;
  * operand builders: f16x2 planes and bf16 rows exactly as the kernels read them, with the values they decode to;
  * fp64 references from the definition, all tensors NHWC / KRSC: y[b, ho, wo, n] = sum_{r, q, c} x[b, ho s + r - pad,
    wo s + q - pad, c] w[n, r, q, c], its adjoint in x (dgrad), its gradient in w (wgrad), each with the companion
    S = the same sum over |x| |w|;
  * acceptance functions, per element (u = 2^-24):
        2 (K + 1) u S            K fp32 additions inside and between the MFMAs (which need not round to nearest: 2)
      + 2^-21 S                  f16x2 only: the lo * lo product never formed (2^-22) and the recombination's two roundings
      + split of the filter      f16x2 only, where the library splits the fp32 filter itself: bn_cases.split_error
      + u (|v| + |r|)            the rounding of the sum with a skip operand or bias r
      + half a bf16 ulp          bf16 results
      + TINY
"""
import numpy as np

import bn_cases as BC

F32, F64, U, TINY = BC.F32, BC.F64, BC.U, BC.TINY
ACC_CONST = 2.0                          # the MFMA's internal summation need not round to nearest


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, k, stride):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------------------------------ host dispatch mirror
def _b(v):
    return 'true' if v else 'false'


def tile_name(bm, bn, wm, wn, bf, yb=False, dg2=False):
    return 'conv_planes_mfma<%d, %d, %d, %d, %s, %s, %s>' % (bm, bn, wm, wn, _b(bf), _b(yb), _b(dg2))


def stream_name(Cs, N, yb):
    """KS = Cs / 16, NT = ceil(N / 32) rounded up to 1, 2 or 4, four waves"""
    nt = cdiv(N, 32)
    return 'conv1x1_stream_bf16<%d, %d, 4, %s>' % (Cs // 16, nt if nt <= 2 else 4, _b(yb))


def wgrad_name(tn, bf, stride):
    return 'wgrad_planes_mfma<%d, 256, %s, %d>' % (tn, _b(bf), stride)


def planes_small(M, N, K):
    """(small, quant): the 128-row two-blocks-per-CU shape for short K, or where 256-row tiles quantise badly on 256 CUs"""
    nt = cdiv(N, 128)
    b256, b128 = cdiv(M, 256) * nt, cdiv(M, 128) * nt
    c256 = cdiv(b256, 256) * 2
    tail = b128 % 512
    c128 = (b128 // 512) * 2 + (0 if tail == 0 else (1 if tail <= 256 else 2))
    quant = c128 * 1.08 < c256
    return K <= 256 or quant, quant


def stream_ok(M, N, Cs, k, stride, y_bf16=False, res=False, bias=False):
    """eligibility of the bf16 streaming 1x1 kernel (Y4_BF_STREAM unset); a bias (one row added to every pixel) goes to
    the tile kernel"""
    if k != 1 or stride != 1 or Cs not in (64, 128) or N > 128 or N < 1:
        return False
    if y_bf16 and (res or bias or N % 2):
        return False
    if bias:
        return False
    return M >= 131072


def bf_big(M, N, bf_tile=0):
    mt = cdiv(M, 256)
    r256, r128 = cdiv(mt * cdiv(N, 256), 256), cdiv(mt * cdiv(N, 128), 256)
    return bf_tile == 2 or (bf_tile == 0 and N > 128 and r256 * 2.0 <= r128 * 1.25)


def planes_conv_kernel(bf, M, N, Cs, k, stride=1, y_bf16=False, res=False, bias=False, bf_tile=0):
    """(kernel name, nparts, rows behind one partial row) of y4::planes_conv"""
    K = k * k * Cs
    small, _ = planes_small(M, N, K)
    if bf and stream_ok(M, N, Cs, k, stride, y_bf16, res, bias):
        tiles = cdiv(M, 128)
        grid = min(tiles, 512)
        return stream_name(Cs, N, y_bf16), grid, cdiv(tiles, grid) * 128
    if bf:
        big = bf_big(M, N, bf_tile)
        if small and not big:
            return tile_name(128, 128, 2, 2, True, y_bf16), cdiv(M, 128), 128
        return (tile_name(256, 256, 2, 4, True, y_bf16) if big else tile_name(256, 128, 4, 2, True, y_bf16)), cdiv(M, 256), 256
    if small:
        return tile_name(128, 128, 2, 2, False), cdiv(M, 128), 128
    return tile_name(256, 128, 4, 2, False), cdiv(M, 256), 256


def nparts(bf, M, N, Cs, k, stride=1, y_bf16=False, bf_tile=0):
    return planes_conv_kernel(bf, M, N, Cs, k, stride, y_bf16, bf_tile=bf_tile)[1]


def tag(name):
    """short name of a kernel's branch"""
    if name.startswith('conv1x1_stream_bf16'):
        return 'stream'
    if name.startswith('wgrad'):
        return 'wgrad' + name[len('wgrad_planes_mfma<'):].split(',')[0]
    a = name[len('conv_planes_mfma<'):-1].split(', ')
    t = 'tile%sx%s' % (a[0], a[1])
    return t + ('.dg2' if a[6] == 'true' else '')


def dgrad_s2_classes():
    """launch order of planes_dgrad_s2 (heaviest class first): [(ph, pw, [(dh, dw, slot)])]"""
    out = []
    for c in (3, 2, 1, 0):
        ph, pw = c >> 1, c & 1
        taps = [((ph + 1 - r) // 2, (pw + 1 - q) // 2, r * 3 + q) for r in range(3) for q in range(3)
                if (ph + 1 - r) % 2 == 0 and (pw + 1 - q) % 2 == 0]
        out.append((ph, pw, taps))
    return out


def dgrad_s2_kernel(bf):
    return tile_name(256, 128, 4, 2, bf, False, True)


def wgrad_tn(Cout, bf, wgrad_tile=0):
    if not bf:
        return 128
    if wgrad_tile == 128 or (wgrad_tile == 256 and Cout >= 256):
        return wgrad_tile
    return 128


def wgrad_plan(M, Cin, Cout, k, tn, bf):
    """(ntn, ntj, splits, steps per split) of y4::planes_wgrad_plan; M: pixels of the dy grid"""
    cap = 512 if (bf and tn == 128) else 256
    J = k * k * Cin
    ntn, ntj = cdiv(Cout, tn), cdiv(J, 256)
    tiles = ntn * ntj
    steps = cdiv(M, 32)
    best, bs = -1, 1
    for s in range(1, cap + 1):
        per = cdiv(steps, s)
        if s > 1 and per < 12:
            break
        cost = cdiv(tiles * s, cap) * (per + 6)
        if best < 0 or cost < best:
            best, bs = cost, s
    per = cdiv(steps, bs)
    return ntn, ntj, cdiv(steps, per), per


def wgrad_workspace(B, H, W, Cin, Cout, k, stride):
    """y4_conv2d_wgrad_planes_workspace (H, W: the x grid): the larger of the two modes' slab sets, + 64"""
    if min(B, H, W, Cin, Cout, k) <= 0 or stride not in (1, 2):
        return 0
    if stride == 2:
        H, W = (H + 1) // 2, (W + 1) // 2
    most = 0
    for bf in (False, True):
        splits = wgrad_plan(B * H * W, Cin, Cout, k, wgrad_tn(Cout, bf), bf)[2]
        most = max(most, splits * Cout * k * k * Cin * 4 if splits > 1 else 0)
    return most + 64


def fwd_workspace(Cin, Cout, k):
    return 64 + 4096 + Cout * k * k * Cin * 6


def dgrad_workspace(Cin, Cout, k):
    return Cin * k * k * cdiv(Cout, 32) * 32 * 6 + 64 + 4096


def conv_window_ok(B, Hs, Ws, Cs, N, k, stride, bf):
    Hd, Wd = out_hw(Hs, Ws, k, stride)
    if Hd <= 0 or Wd <= 0 or B * Hd * Wd >= 2 ** 31:
        return False
    img = Hs * Ws * Cs * 4
    wb = N * k * k * Cs * (2 if bf else 4)
    return img * (256 // (Hd * Wd) + 2) < 0xfffffff0 and wb < 0xfffffff0


# ------------------------------------------------------------------------------------------ seeded values
def make_values(rows, C, seed, spread=0, lo=0.5, hi=2.0):
    """[rows, C] fp32, |v| uniform in [lo, hi) with a random sign, channel c scaled by 2^(spread ((c % 3) - 1)): with
    spread = 10 the channels differ in scale by 2^+-10, and no element is small enough to leave the normal range of an
    fp16 piece under the tensor's scale (the smallest is 2^-23 of the largest)."""
    rng = np.random.RandomState(seed % (2 ** 31))
    v = rng.uniform(lo, hi, (rows, C)) * np.where(rng.randint(0, 2, (rows, C)) > 0, 1.0, -1.0)
    return (v * 2.0 ** (spread * ((np.arange(C) % 3) - 1.0))).astype(F32)


def make_filter(Cout, k, Cin, seed, spread=10, axis=0):
    """[Cout, k, k, Cin] fp32 of magnitude ~ 1 / sqrt(K); axis 0: output channel n scaled by 2^(spread ((n % 3) - 1)) (the
    columns of a forward result then differ by 2^+-spread), axis 3: input channel c (the columns of a dgrad result)"""
    K = k * k * Cin
    w = make_values(Cout, K, seed, 0).astype(F64).reshape(Cout, k, k, Cin) / np.sqrt(K)
    n = Cout if axis == 0 else Cin
    sc = 2.0 ** (spread * ((np.arange(n) % 3) - 1.0))
    w = w * (sc[:, None, None, None] if axis == 0 else sc[None, None, None, :])
    return w.astype(F32)


def seed_of(*dims):
    s = 17
    for d in dims:
        s = (s * 1000003 + int(d)) % 2147483629
    return s


# ------------------------------------------------------------------------------------------ operand builders
def zero_pads(a, c_valid):
    a = np.array(a, dtype=F32)
    a[:, c_valid:] = 0
    return a


def place(payload16, ld, byte_off=0):
    """16-bit payload rows [M, n] at byte `byte_off` of sentinel-filled rows of ld 32-bit words"""
    M, n = payload16.shape
    out = BC.sentinel((M, ld))
    h = out.view(np.uint16).reshape(M, 2 * ld)
    assert byte_off % 2 == 0 and byte_off // 2 + n <= 2 * ld
    h[:, byte_off // 2:byte_off // 2 + n] = payload16
    return out.view(np.uint32)


def act_f16x2(a, word=None, ld=None, off=0, c_valid=None):
    """f16x2 activation planes of a [M, C]: rows [C / 32][hi 32 x fp16 | lo 32 x fp16] under the scale of `word` (default:
    the word of max|a|), as channels [off, off + C) of rows of ld channels (4 bytes per channel), channels >= c_valid zero.
    -> dict(words [M, ld] uint32, word, dec [M, C] fp64: what the planes stand for)"""
    a = np.asarray(a, dtype=F32)
    if c_valid is not None:
        a = zero_pads(a, c_valid)
    M, C = a.shape
    word = BC.amax_word(a) if word is None else int(word)
    hi, lo = BC.split_f16x2(a, word)
    ld = C if ld is None else ld
    assert off % 32 == 0 and ld % 32 == 0 and off + C <= ld
    return dict(words=place(BC.planes_pack(hi, lo), ld, 4 * off), word=word, dec=BC.planes_decode(hi, lo, word), hi=hi, lo=lo)


def act_bf16(a, ld=None, off=0, c_valid=None):
    """bf16 rows of a [M, C]: C bf16 values (RNE) from byte 2 off of rows of ld channels (4 bytes per channel; a dense row
    keeps its second half poisoned).  -> dict(words, word = None, dec)"""
    a = np.asarray(a, dtype=F32)
    if c_valid is not None:
        a = zero_pads(a, c_valid)
    M, C = a.shape
    h = BC.bf16_rne(a)
    ld = C if ld is None else ld
    assert off % 64 == 0 and off + C <= ld
    return dict(words=place(h, ld, 2 * off), word=None, dec=BC.bf16_to_f32(h).astype(F64))


def act_planes(a, bf, **kw):
    return act_bf16(a, **kw) if bf else act_f16x2(a, **kw)


def filter_seen(w, bf):
    """(the filter values the reference uses, the bound of what the kernel's own copy may differ by, elementwise).
    bf16: the library rounds to nearest even -- decoded exactly, no term.  f16x2: the library splits the fp32 filter under
    the scale of max|w|; the reference keeps w and the split error (bn_cases.split_error, in units of the scale) is a term."""
    w = np.asarray(w, dtype=F32)
    if bf:
        return BC.bf16_to_f32(BC.bf16_rne(w)).astype(F64), None
    s = F64(BC.scale_of(BC.amax_word(w)))
    return w.astype(F64), BC.split_error(np.abs(w.astype(F64)) * s) / s


# ------------------------------------------------------------------------------------------ fp64 references
def _taps(k, skip_tap=None):
    return [(r, q) for r in range(k) for q in range(k) if (r, q) != skip_tap]


def conv_fwd64(x, w, k, stride, skip_tap=None):
    """x [B, H, W, Cin], w [Cout, k, k, Cin] -> y [B, Ho, Wo, Cout], same padding (k - 1) / 2, fp64"""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, H, W, Cin = x.shape
    pad = (k - 1) // 2
    Ho, Wo = out_hw(H, W, k, stride)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    y = np.zeros((B, Ho, Wo, w.shape[0]))
    for r, q in _taps(k, skip_tap):
        patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, q:q + stride * (Wo - 1) + 1:stride, :]
        y += patch.reshape(-1, Cin).dot(w[:, r, q, :].T).reshape(y.shape)
    return y


def conv_dgrad64(dy, w, k, stride, H, W, skip_tap=None):
    """the adjoint of conv_fwd64 in x: dy [B, Ho, Wo, Cout] -> dx [B, H, W, Cin]"""
    dy, w = np.asarray(dy, F64), np.asarray(w, F64)
    B, Ho, Wo, Cout = dy.shape
    Cin = w.shape[3]
    pad = (k - 1) // 2
    assert (Ho, Wo) == out_hw(H, W, k, stride)
    Hp, Wp = max(H + 2 * pad, stride * (Ho - 1) + k), max(W + 2 * pad, stride * (Wo - 1) + k)
    dxp = np.zeros((B, Hp, Wp, Cin))
    for r, q in _taps(k, skip_tap):
        dxp[:, r:r + stride * (Ho - 1) + 1:stride, q:q + stride * (Wo - 1) + 1:stride, :] += \
            dy.reshape(-1, Cout).dot(w[:, r, q, :]).reshape(B, Ho, Wo, Cin)
    return dxp[:, pad:pad + H, pad:pad + W, :].copy()


def conv_wgrad64(x, dy, k, stride, skip_tap=None):
    """the gradient of conv_fwd64 in w: x [B, H, W, Cin], dy [B, Ho, Wo, Cout] -> dw [Cout, k, k, Cin]"""
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    pad = (k - 1) // 2
    assert (Ho, Wo) == out_hw(H, W, k, stride)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    dw = np.zeros((Cout, k, k, Cin))
    for r, q in _taps(k, skip_tap):
        patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, q:q + stride * (Wo - 1) + 1:stride, :]
        dw[:, r, q, :] = dy.reshape(-1, Cout).T.dot(patch.reshape(-1, Cin))
    return dw


def fwd_ref(xdec, w, k, stride, bf, bias=None):
    """forward reference on the decoded activation xdec [B, H, W, Cin] and the fp32 filter w.
    -> dict(v: the conv, y: v + bias, S, K, wsplit (f16x2: the filter-split term), r: the bias or None)"""
    wv, dw = filter_seen(w, bf)
    v = conv_fwd64(xdec, wv, k, stride)
    S = conv_fwd64(np.abs(xdec), np.abs(wv), k, stride)
    out = dict(v=v, S=S, K=k * k * xdec.shape[3], r=None, y=v, wsplit=None)
    if dw is not None:
        out['wsplit'] = conv_fwd64(np.abs(xdec), dw, k, stride)
    if bias is not None:
        out['r'] = np.broadcast_to(np.asarray(bias, F64), v.shape)
        out['y'] = v + out['r']
    return out


def dgrad_ref(dydec, w, k, stride, H, W, bf, res=None):
    """dgrad reference; K per element: the taps that reach it times Cout (stride 2: (1 + h % 2) (1 + w % 2) taps)"""
    wv, dw = filter_seen(w, bf)
    v = conv_dgrad64(dydec, wv, k, stride, H, W)
    S = conv_dgrad64(np.abs(dydec), np.abs(wv), k, stride, H, W)
    Cout = dydec.shape[3]
    if stride == 2:
        K = ((1 + np.arange(H) % 2)[:, None] * (1 + np.arange(W) % 2)[None, :] * Cout)[None, :, :, None]
    else:
        K = k * k * Cout
    out = dict(v=v, S=S, K=K, r=None, y=v, wsplit=None)
    if dw is not None:
        out['wsplit'] = conv_dgrad64(np.abs(dydec), dw, k, stride, H, W)
    if res is not None:
        out['r'] = np.asarray(res, F64)
        out['y'] = v + out['r']
    return out


def wgrad_ref(xdec, dydec, k, stride, splits):
    """wgrad reference: both operands arrive split (no filter term); K = the pixels of the dy grid + the slab additions"""
    v = conv_wgrad64(xdec, dydec, k, stride)
    S = conv_wgrad64(np.abs(xdec), np.abs(dydec), k, stride)
    M = dydec.shape[0] * dydec.shape[1] * dydec.shape[2]
    return dict(v=v, y=v, S=S, K=M + splits, r=None, wsplit=None)


# ------------------------------------------------------------------------------------------ acceptance
def bf16_half_ulp(z_abs):
    """half a bf16 ulp (8-bit significand) of |z|: 2^(floor(log2 |z|) - 8), between 2^-9 |z| and 2^-8 |z|"""
    z = np.asarray(z_abs, F64)
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(np.where(z > 0, z, 1.0)))
    return np.where(z > 0, 2.0 ** (e - 8), 0.0)


def conv_bound(r, bf, y_bf16=False):
    """the elementwise bound of a result against r['y'], and its addends by name"""
    t = dict(acc=ACC_CONST * (np.asarray(r['K'], F64) + 1.0) * U * r['S'])
    if not bf:
        t['lolo'] = 2.0 ** -21 * r['S']
        if r['wsplit'] is not None:
            t['wsplit'] = r['wsplit']
    if r['r'] is not None:
        t['skip'] = U * (np.abs(r['v']) + np.abs(r['r']))
    b = sum(t.values())
    if y_bf16:
        t['bf16'] = bf16_half_ulp(np.abs(r['y']) + b)
        b = b + t['bf16']
    return b, t


def conv_accept(got, r, bf, y_bf16=False):
    """(ok, used) per element, bn_cases.judge under conv_bound"""
    b, _ = conv_bound(r, bf, y_bf16)
    return BC.judge(np.asarray(got).reshape(r['y'].shape), r['y'], b)


def left_out(r, bf, y_bf16=False):
    """share of the elements judged by the floor alone (bn_cases.left_out): a case may leave out at most LEFT_OUT_CAP"""
    b, _ = conv_bound(r, bf, y_bf16)
    return BC.left_out(r['y'], b)


LEFT_OUT_CAP = 0.01


def colsum_accept(part, stored, rows):
    """partial rows [nparts, 2, N] (sum y, sum y^2 of the rows behind each, fp32) against the fp64 column sums of the
    values the GPU itself stored [M, N]: every partial is an fp32 sum of at most `rows` terms, their sum is taken here in
    fp64 -> |sum - ref| <= rows u sum|y|; the squares carry one more rounding each -> (rows + 1) u sum y^2"""
    part = np.asarray(part, F64)
    y = np.asarray(stored, F64)
    s, ss = part[:, 0].sum(axis=0), part[:, 1].sum(axis=0)
    ok1, u1 = BC.judge(s, y.sum(axis=0), rows * U * np.abs(y).sum(axis=0))
    ok2, u2 = BC.judge(ss, (y * y).sum(axis=0), (rows + 1) * U * (y * y).sum(axis=0))
    return ok1 & ok2, np.maximum(u1, u2)


# ------------------------------------------------------------------------------------------ emulations (CPU self-test)
def emulate_f16x2(xa, wa, k, stride, drop=None):
    """what the f16x2 kernel computes from the pieces, in fp64: (hi hi + (hi lo + lo hi) / 2048) / (s_x s_w); drop='lohi':
    without the lo_x hi_w product.  xa: act_f16x2 dict reshaped by the caller ([B, H, W, C] pieces), wa: the same for w"""
    hx, lx, hw, lw = (np.asarray(t, F64) for t in (xa['hi'], xa['lo'], wa['hi'], wa['lo']))
    acc0 = conv_fwd64(hx, hw, k, stride)
    acc1 = conv_fwd64(hx, lw, k, stride)
    if drop != 'lohi':
        acc1 = acc1 + conv_fwd64(lx, hw, k, stride)
    return (acc0 + acc1 / 2048.0) / (F64(BC.scale_of(xa['word'])) * F64(BC.scale_of(wa['word'])))


def emulate_f32(xdec, wv, k, stride):
    """the same operands, products and sums in float32, taps and channels in the reverse order"""
    x = np.asarray(xdec, F32)[..., ::-1]
    w = np.asarray(wv, F32)[..., ::-1]
    B, H, W, Cin = x.shape
    pad = (k - 1) // 2
    Ho, Wo = out_hw(H, W, k, stride)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    y = np.zeros((B, Ho, Wo, w.shape[0]), dtype=F32)
    for r, q in reversed(_taps(k)):
        patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, q:q + stride * (Wo - 1) + 1:stride, :]
        acc = np.zeros((B * Ho * Wo, w.shape[0]), dtype=F32)
        for c0 in range(0, Cin, 16):
            acc = (acc + patch.reshape(-1, Cin)[:, c0:c0 + 16].dot(w[:, r, q, c0:c0 + 16].T)).astype(F32)
        y = (y + acc.reshape(y.shape)).astype(F32)
    return y


# ------------------------------------------------------------------------------------------ case lists
STREAM_MIN = 131072


def _fc(name, mode, B, H, W, Cin, Cout, k, s, want, **opt):
    c = dict(name=name, mode=mode, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, want=want, ldy_pad=0, partials=False, bias=False,
             y_bf16=False, bf_tile=0)
    c.update(opt)
    return c


TILE_M = (1, 127, 128, 129, 257)
TILE_N = (4, 36, 128, 132, 192)


def _grid_cases(mode):
    """M x N against the 128-row tile (1x1, Cin = 64): pitch, partials, bias and bf16 result take turns"""
    out = []
    for i, (M, N) in enumerate((M, N) for M in TILE_M for N in TILE_N):
        bias = i % 3 == 0
        ybf = mode == 'bf16' and N % 32 == 0 and i % 3 == 1
        out.append(_fc('grid-M%d-N%d' % (M, N), mode, 1, 1, M, 64, N, 1, 1, 'tile128x128', ldy_pad=4 * (i % 2), bias=bias,
                       partials=not bias and (ybf or i % 3 == 2), y_bf16=ybf))
    return out


FWD_GRID = {'f16x2': _grid_cases('f16x2'), 'bf16': _grid_cases('bf16')}

FWD_CASES = [
    # the 256-row shape by natural dispatch: b128 = 257 blocks, K > 256
    _fc('rows256', 'f16x2', 1, 1, 32769, 288, 36, 1, 1, 'tile256x128', ldy_pad=4, partials=True),
    _fc('rows256-bias', 'f16x2', 1, 1, 32769, 288, 4, 1, 1, 'tile256x128', bias=True),
    _fc('rows256', 'bf16', 1, 1, 32769, 320, 96, 1, 1, 'tile256x128', partials=True, y_bf16=True),
    _fc('rows256-bias', 'bf16', 1, 1, 32769, 320, 36, 1, 1, 'tile256x128', ldy_pad=4, bias=True),
    # bf16 256 x 256: forced on a ragged two-tile map, and by natural dispatch (N > 128, 129 row tiles)
    _fc('big-forced', 'bf16', 1, 1, 257, 64, 192, 1, 1, 'tile256x256', ldy_pad=4, partials=True, bf_tile=2),
    _fc('big-forced-ybf', 'bf16', 1, 1, 257, 64, 192, 1, 1, 'tile256x256', partials=True, y_bf16=True, bf_tile=2),
    _fc('big-forced-bias', 'bf16', 1, 1, 129, 64, 132, 1, 1, 'tile256x256', bias=True, bf_tile=2),
    _fc('big-natural', 'bf16', 1, 1, 32769, 64, 192, 1, 1, 'tile256x256', partials=True),
    # 3 x 3, stride 1 and 2, odd and even maps, tiles that span images
    _fc('k3-odd', 'f16x2', 3, 7, 9, 32, 36, 3, 1, 'tile128x128', ldy_pad=4, partials=True),
    _fc('k3-even', 'f16x2', 3, 8, 6, 32, 36, 3, 1, 'tile128x128', bias=True),
    _fc('k3s2-odd', 'f16x2', 3, 7, 9, 32, 36, 3, 2, 'tile128x128', partials=True),
    _fc('k3s2-even', 'f16x2', 3, 8, 6, 64, 132, 3, 2, 'tile128x128', ldy_pad=4),
    _fc('k3-rows256', 'f16x2', 5, 82, 81, 32, 36, 3, 1, 'tile256x128', partials=True),
    _fc('k3-odd', 'bf16', 3, 7, 9, 64, 36, 3, 1, 'tile128x128', ldy_pad=4, partials=True),
    _fc('k3-even', 'bf16', 3, 8, 6, 64, 64, 3, 1, 'tile128x128', partials=True, y_bf16=True),
    _fc('k3s2-odd', 'bf16', 3, 7, 9, 64, 36, 3, 2, 'tile128x128', bias=True),
    _fc('k3s2-even', 'bf16', 3, 8, 6, 64, 132, 3, 2, 'tile128x128', partials=True),
    _fc('k3-rows256', 'bf16', 5, 82, 81, 64, 32, 3, 1, 'tile256x128', partials=True, y_bf16=True),
    # the hybrid (bf16 planes under conv mode 3) reaches the bf16 kernels
    _fc('hybrid', 'hybrid', 3, 7, 9, 64, 36, 3, 1, 'tile128x128', partials=True),
]

STREAM_CASES = [
    _fc('under', 'bf16', 1, 1, STREAM_MIN - 1, 64, 64, 1, 1, 'tile128x128', partials=True),
    _fc('K128-N4', 'bf16', 1, 1, STREAM_MIN, 128, 4, 1, 1, 'stream', ldy_pad=4, partials=True),
    _fc('K64-N32-ybf', 'bf16', 1, 1, STREAM_MIN, 64, 32, 1, 1, 'stream', partials=True, y_bf16=True),
    _fc('K128-N36', 'bf16', 1, 1, STREAM_MIN + 37, 128, 36, 1, 1, 'stream', ldy_pad=4, partials=True),
    _fc('K128-N64-ybf', 'bf16', 1, 1, STREAM_MIN + 37, 128, 64, 1, 1, 'stream', partials=True, y_bf16=True),
    _fc('K64-N128', 'bf16', 1, 1, STREAM_MIN + 37, 64, 128, 1, 1, 'stream'),
    _fc('K128-N128-ybf', 'bf16', 1, 1, STREAM_MIN, 128, 128, 1, 1, 'stream', partials=True, y_bf16=True),
    _fc('hybrid-K64-N36', 'hybrid', 1, 1, STREAM_MIN, 64, 36, 1, 1, 'stream', partials=True),
    # a bias is one row for every pixel: the streaming epilogue has no such window, the call goes to the tile kernel
    _fc('bias-K64-N36', 'bf16', 1, 1, STREAM_MIN + 37, 64, 36, 1, 1, 'tile128x128', bias=True),
    _fc('bias-K128-N128', 'bf16', 1, 1, STREAM_MIN, 128, 128, 1, 1, 'tile128x128', ldy_pad=4, bias=True),
]


def _dc(name, mode, B, H, W, Cin, Cout, k, s, want, **opt):
    """dgrad: H, W the dx (input) grid"""
    c = dict(name=name, mode=mode, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, want=want, lddx_pad=0, res=False, ldr_pad=0)
    c.update(opt)
    return c


DGRAD_CASES = [
    _dc('k3', 'f16x2', 2, 5, 7, 36, 64, 3, 1, 'tile128x128'),
    _dc('k3-res', 'f16x2', 2, 5, 7, 36, 64, 3, 1, 'tile128x128', res=True, ldr_pad=4, lddx_pad=8),
    _dc('k1-res', 'f16x2', 1, 1, 129, 132, 32, 1, 1, 'tile128x128', res=True),
    _dc('rows256-res', 'f16x2', 1, 1, 32769, 36, 288, 1, 1, 'tile256x128', res=True, ldr_pad=4),
    _dc('k3', 'bf16', 2, 5, 7, 36, 64, 3, 1, 'tile128x128', lddx_pad=4),
    _dc('k3-res', 'bf16', 2, 5, 7, 132, 64, 3, 1, 'tile128x128', res=True, ldr_pad=4, lddx_pad=8),
    _dc('rows256-res', 'bf16', 1, 1, 32769, 36, 320, 1, 1, 'tile256x128', res=True, ldr_pad=4),
    _dc('stream-res', 'bf16', 1, 1, STREAM_MIN + 37, 36, 64, 1, 1, 'stream', res=True, ldr_pad=4, lddx_pad=4),
    _dc('stream', 'bf16', 1, 1, STREAM_MIN, 128, 128, 1, 1, 'stream'),
    _dc('hybrid-res', 'hybrid', 2, 5, 7, 36, 64, 3, 1, 'tile128x128', res=True, ldr_pad=4),
    # stride 2: the parity classes on a map of one pixel per class, on 4 x 6, and on ragged two-tile class grids
    _dc('s2-2x2', 'f16x2', 1, 2, 2, 36, 32, 3, 2, 'tile256x128.dg2'),
    _dc('s2-4x6', 'f16x2', 2, 4, 6, 36, 32, 3, 2, 'tile256x128.dg2', lddx_pad=4),
    _dc('s2-ragged', 'f16x2', 3, 22, 26, 132, 32, 3, 2, 'tile256x128.dg2'),
    _dc('s2-2x2', 'bf16', 1, 2, 2, 36, 64, 3, 2, 'tile256x128.dg2'),
    _dc('s2-4x6', 'bf16', 2, 4, 6, 36, 64, 3, 2, 'tile256x128.dg2', lddx_pad=4),
    _dc('s2-ragged', 'bf16', 3, 22, 26, 132, 64, 3, 2, 'tile256x128.dg2'),
]


def _wc(name, mode, B, H, W, Cin, Cout, k, s, splits, **opt):
    """wgrad: H, W the x grid; splits: (== 1) or (> 1) as the case is listed"""
    c = dict(name=name, mode=mode, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, many=splits, tile=0, want_tn=128)
    c.update(opt)
    return c


WGRAD_CASES = [
    _wc('one-split', 'f16x2', 1, 5, 7, 32, 32, 3, 1, False),                   # J = 288: two j tiles
    _wc('splits', 'f16x2', 2, 21, 23, 32, 255, 3, 1, True),                    # Cout 255: dy rows hold 256 channels
    _wc('splits-k1', 'f16x2', 1, 1, 1000, 64, 256, 1, 1, True),
    _wc('s2', 'f16x2', 2, 40, 44, 32, 32, 3, 2, True),
    _wc('one-split', 'bf16', 1, 5, 7, 64, 32, 3, 1, False),                    # J = 576: three j tiles, the last a quarter full
    _wc('splits', 'bf16', 2, 21, 23, 64, 255, 3, 1, True),
    _wc('splits-256', 'bf16', 1, 1, 1000, 64, 256, 1, 1, True, tile=256, want_tn=256),
    _wc('s2', 'bf16', 2, 40, 44, 64, 32, 3, 2, True),
    _wc('s2-256', 'bf16', 1, 6, 10, 64, 256, 3, 2, False, tile=256, want_tn=256),
    _wc('hybrid', 'hybrid', 2, 21, 23, 64, 32, 3, 1, True),
]

SPLIT_CASES = [
    # M, C, ldx, ld_planes, off, c_valid  (ld_planes 0: y4_planes_split_f32, dense)
    (1, 64, 64, 0, 0, 64),
    (257, 128, 132, 0, 0, 128),
    (1025, 64, 64, 0, 0, 64),
    (5, 64, 64, 192, 64, 64),
    (131, 128, 136, 320, 128, 100),
    (1030, 64, 68, 64, 0, 61),
]


def case_id(c):
    return '%s-%s' % (c['mode'], c['name'])


def is_bf(mode):
    return mode in ('bf16', 'hybrid')


def fwd_dims(c):
    Ho, Wo = out_hw(c['H'], c['W'], c['k'], c['s'])
    return c['B'] * Ho * Wo, c['Cout'], c['Cin']


def fwd_kernel(c):
    M, N, Cs = fwd_dims(c)
    return planes_conv_kernel(is_bf(c['mode']), M, N, Cs, c['k'], c['s'], c['y_bf16'], False, c['bias'], c['bf_tile'])


def dgrad_kernel(c):
    if c['s'] == 2:
        return dgrad_s2_kernel(is_bf(c['mode']))
    return planes_conv_kernel(is_bf(c['mode']), c['B'] * c['H'] * c['W'], c['Cin'], c['Cout'], c['k'], 1, False, c['res'], False)[0]


def wgrad_case_plan(c):
    bf = is_bf(c['mode'])
    Ho, Wo = out_hw(c['H'], c['W'], c['k'], c['s'])
    tn = wgrad_tn(c['Cout'], bf, c['tile'])
    return (tn,) + wgrad_plan(c['B'] * Ho * Wo, c['Cin'], c['Cout'], c['k'], tn, bf)
