# -*- coding: utf-8 -*-
"""References, operand formats, seeded inputs and acceptance criteria for the direct tests of the BatchNorm family of
csrc/pointwise.hip (tests/test_bn_cases.py checks them on the CPU, tests/test_gpu_bn_edges.py feeds them to the kernels).

Four parts, numpy only:
  * a mirror of the HOST dispatch (row_map, stat_rows, the fold plan, grids, workspace sizes): it lets a case STATE which
    branch it reaches and supplies the chain lengths of the error bounds; it is never the reference of a value;
  * fp64 references written from the definitions (two-pass variance, Mish as x tanh(log1p(exp x)));
  * the operand formats the sweeps emit (f16x2 planes, bf16 rows, the analytic plane bound) as bit-exact numpy code;
  * acceptance functions.  Every one is elementwise, |got - ref| <= bound, the bound built from the fp64 reference's
    own intermediate values and expanded into its addends; u = 2^-24 is the unit roundoff of fp32.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126                       # smallest normal fp32: a result flushed to zero is off by less than this
SENT = 0x7fa5c3e1                        # a NaN bit pattern no kernel produces
ACT_LINEAR, ACT_LEAKY, ACT_MISH, ACT_RELU = 0, 1, 2, 3
ACTS = (ACT_LINEAR, ACT_LEAKY, ACT_MISH, ACT_RELU)
ACT_NAMES = {ACT_LINEAR: 'linear', ACT_LEAKY: 'leaky', ACT_MISH: 'mish', ACT_RELU: 'relu'}
ERR_SHAPE, ERR_NULL, ERR_WORKSPACE = 1, 2, 4
EPS = 1e-5
MOMENTUM = 0.03

# ------------------------------------------------------------------------------------------ host dispatch mirror
PW_THREADS = 256
PW_UNROLL = 4
FOLD_BLOCKS = 256
STAT_ROWS_MAX = 128
GRID_CAP = 4096


def row_map(C):
    """(tpr, rpb): threads per row = the largest power of two <= min(C / 4, 256); rows per block iteration"""
    tpr = min(C // 4, PW_THREADS)
    p = 1
    while p * 2 <= tpr:
        p *= 2
    return p, PW_THREADS // p


def channel_passes(C):
    """(passes of the channel loop, active threads per row in the last one)"""
    tpr, _ = row_map(C)
    n = -(-C // (tpr * 4))
    return n, C // 4 - (n - 1) * tpr


def stat_rows(M, rpb):
    return int(min(max(M // (rpb * 4096), 4), STAT_ROWS_MAX))


def bn_blocks(M, C):
    _, rpb = row_map(C)
    rows = rpb * stat_rows(M, rpb)
    return -(-M // rows)


def fold_plan(nparts, C):
    """(blocks, per, cw, rg_n) of fold_partials: blocks = nb, the number of fp64 rows the finalize kernels add"""
    want = (nparts + 15) // 16
    blocks = max(min(want, FOLD_BLOCKS), 1)
    per = -(-nparts // blocks)
    blocks = max(-(-nparts // per), 1)
    cw = 32
    while cw < 2 * C and cw < PW_THREADS:
        cw *= 2
    return blocks, per, cw, PW_THREADS // cw


def fold_unrolled(nparts, C):
    """does the 8-way unrolled loop of fold_partials_kernel start (in the first block, row group 0)?"""
    _, per, _, rg_n = fold_plan(nparts, C)
    return 7 * rg_n < min(per, nparts)


def rows32_unrolled(nb):
    """(groups g of fold_rows32 that enter the `r + 56 < nb` loop, groups with rows left for the tail loop)"""
    main = [g for g in range(8) if g + 56 < nb]
    tail = []
    for g in range(8):
        r = g
        while r + 56 < nb:
            r += 64
        if r < nb:
            tail.append(g)
    return main, tail


def apply_grid(M, C):
    _, rpb = row_map(C)
    return min(-(-M // (PW_UNROLL * rpb)), GRID_CAP)


def apply_laps(M, C):
    """trips of the busiest block of the apply sweeps (the `tb += step` loop)"""
    _, rpb = row_map(C)
    trips = -(-M // (PW_UNROLL * rpb))
    return -(-trips // apply_grid(M, C))


def bn_finalize_workspace(C):
    return (1 + FOLD_BLOCKS) * 2 * C * 8 if C > 0 else 0


def bn_workspace(M, C):
    if M <= 0 or C <= 0:
        return 0
    return bn_finalize_workspace(C) + bn_blocks(M, C) * 2 * C * 4


def bn_loads_nt(C):
    return C >= 64


def colsum_rows(M):
    return int(min(M, 1024))


def sum_chain(M, C):
    """fp32 additions behind one channel sum of the statistics / backward reduce: nrows per thread + rpb in the block"""
    _, rpb = row_map(C)
    return stat_rows(M, rpb) + rpb


# ------------------------------------------------------------------------------------------ case lists
# C: (c4, tpr, rpb, what it reaches)
CHANNEL_TABLE = {
    4: (1, 1, 256, ''),
    8: (2, 2, 128, ''),
    12: (3, 2, 128, 'second channel pass with one active quad'),
    32: (8, 8, 32, ''),
    36: (9, 8, 32, 'remainder pass, one quad; C % 32 != 0 in finalize'),
    64: (16, 16, 16, 'first nt size'),
    96: (24, 16, 16, 'half-full second pass, with planes'),
    160: (40, 32, 8, ''),
    1024: (256, 256, 1, ''),
    1028: (257, 256, 1, 'second pass, one thread'),
    2048: (512, 256, 1, 'two full passes'),
}
CHANNELS = tuple(CHANNEL_TABLE)
PLANE_CHANNELS = (32, 96, 160, 1024)
# (C, M): nrows = 5 and an apply grid over the cap (second lap); the grid cap at rpb = 4
LARGE = ((1024, 20483), (256, 65537 + 3))
FOLD_NPARTS = (1, 15, 16, 17, 16 * 57, 16 * 64, 16 * 65, 4096, 4097, 70001)
FOLD_CHANNELS = (4, 36, 128, 1028)
FOLD_NB = (1, 57, 64, 65, 256)
BOUND_CHANNELS = (1, 255, 256, 257, 1028)
BIAS_CHANNELS = (1, 3, 255, 256)
BIAS_ROWS = (1, 1023, 1024, 1025, 5003)
FOLD_EVAL_CHANNELS = (1, 255, 1028)


def m_list(C):
    """row counts around one trip T = 4 rpb of the sweeps"""
    _, rpb = row_map(C)
    T = PW_UNROLL * rpb
    return (1, T - 1, T, T + 1, 2 * T + rpb + 1)


# ------------------------------------------------------------------------------------------ formats
def sentinel(shape):
    return np.full(shape, SENT, dtype=np.uint32).view(F32)


def is_sentinel(a):
    return np.ascontiguousarray(a).view(np.uint32) == SENT


def pad_rows(a, ld):
    """[M, C] -> [M, ld] with the pitch padding holding the sentinel"""
    a = np.asarray(a, dtype=F32)
    out = sentinel((a.shape[0], ld))
    out[:, :a.shape[1]] = a
    return out


def scale_exp(word):
    """biased exponent of the power-of-two scale the f16x2 split applies for an amax word (f16x2_scale_exp)"""
    e8 = (int(word) >> 23) & 0xff
    se = 268 - e8
    if e8 in (0, 255):
        se = 127
    return min(max(se, 2), 252)


def scale_of(word):
    return np.array([scale_exp(word) << 23], dtype=np.uint32).view(F32)[0]


def split_f16x2(z, word):
    """(hi, lo) fp16 pieces of fp32 values at the scale the word implies: t = z * 2^k, hi = f16(t),
    lo = f16((t - f32(hi)) * 2048), every step rounded to nearest even as the hardware conversions are"""
    with np.errstate(over='ignore', invalid='ignore'):
        t = (np.asarray(z, dtype=F32) * scale_of(word)).astype(F32)
        hi = t.astype(np.float16)
        lo = ((t - hi.astype(F32)).astype(F32) * F32(2048.0)).astype(F32).astype(np.float16)
    return hi, lo


def planes_pack(hi, lo):
    """[M, C] hi / lo -> [M, 2C] fp16 words of a plane row: per 32-channel tile [64 B hi | 64 B lo]"""
    M, C = hi.shape
    assert C % 32 == 0
    out = np.empty((M, C // 32, 2, 32), dtype=np.uint16)
    out[:, :, 0] = np.ascontiguousarray(hi).view(np.uint16).reshape(M, C // 32, 32)
    out[:, :, 1] = np.ascontiguousarray(lo).view(np.uint16).reshape(M, C // 32, 32)
    return out.reshape(M, 2 * C)


def planes_unpack(words):
    """inverse of planes_pack: (hi, lo) as fp16 [M, C]"""
    M, n = words.shape
    w = np.ascontiguousarray(words, dtype=np.uint16).reshape(M, n // 64, 2, 32)
    hi = np.ascontiguousarray(w[:, :, 0]).reshape(M, n // 2).view(np.float16)
    lo = np.ascontiguousarray(w[:, :, 1]).reshape(M, n // 2).view(np.float16)
    return hi, lo


def planes_decode(hi, lo, word):
    """the value a plane pair stands for, in fp64"""
    return (hi.astype(F64) + lo.astype(F64) / 2048.0) / F64(scale_of(word))


def split_error(t_abs):
    """bound of |hi + lo / 2048 - t| in scaled units (t = z * 2^k)"""
    return 2.0 ** -22 * t_abs + 2.0 ** -36


def bf16_rne(z):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; finite values only"""
    b = np.ascontiguousarray(z, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_error(z_abs):
    """bound of |bf16(z) - z|: round to nearest with an 8-bit significand is off by at most 2^-8 |z| (normal range)"""
    return 2.0 ** -8 * z_abs


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_rows(a, ld):
    """[M, C] bf16-representable fp32 values -> [M, ld] fp32-sized rows: C bf16 values in the first half of the row, the
    rest of the row poisoned with the sentinel"""
    a = np.asarray(a, dtype=F32)
    M, C = a.shape
    out = sentinel((M, ld))
    h = out.view(np.uint16).reshape(M, 2 * ld)
    h[:, :C] = bf16_rne(a)
    return out


def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 operands: the product is exact in fp64 and the fp64 sum is rounded once more, which
    differs from a fused fp32 operation only on a tie of the second rounding"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def planes_bound_f32(gamma, beta, M, res_word=None, floor_word=None):
    """The amax word of bn_planes_bound_kernel, in its operation order: max_c fma(sqrt(M - 1), |gamma_c|, |beta_c|),
    times 1.0001f, plus fma(res_amax, 1.0001f, .); the larger bit pattern of it and floor_word."""
    s = np.sqrt(F32(M - 1 if M > 1 else 1), dtype=F32)
    m = F32(max(0.0, float(np.max(_fma32(s, np.abs(np.asarray(gamma, F32)), np.abs(np.asarray(beta, F32)))))))
    with np.errstate(over='ignore', invalid='ignore'):
        b = F32(m * F32(1.0001))
        if res_word is not None:
            b = _fma32(np.array([res_word], np.uint32).view(F32)[0], F32(1.0001), b)
    w = int(np.array([b], dtype=F32).view(np.uint32)[0])
    if floor_word is not None and int(floor_word) > w:
        w = int(floor_word)
    return w


def word_value(word):
    return float(np.array([word], dtype=np.uint32).view(F32)[0])


def amax_word(z):
    """bit pattern of max|finite z| (0 when there is none): what the sweeps fold into *out_amax"""
    b = np.ascontiguousarray(z, dtype=F32).view(np.uint32) & 0x7fffffff
    b = b[b < 0x7f800000]
    return int(b.max()) if b.size else 0


# ------------------------------------------------------------------------------------------ fp64 references
def mish64(x):
    with np.errstate(over='ignore'):
        return x * np.tanh(np.log1p(np.exp(x)))


def mish_grad64(x, parts=False):
    """d/dx [x tanh(softplus x)] = t + x (1 - t^2) sigmoid(x), 1 - t^2 = 1 / cosh^2(softplus x); parts: also the sum of
    the absolute values of the two addends"""
    with np.errstate(over='ignore'):
        sp = np.log1p(np.exp(x))
        t = np.tanh(sp)
        sech2 = 1.0 / np.cosh(sp) ** 2
        sg = 1.0 / (1.0 + np.exp(-x))
    d = t + x * sech2 * sg
    return (d, np.abs(t) + np.abs(x * sech2 * sg)) if parts else d


def act64(v, act):
    if act == ACT_LEAKY:
        return np.where(v > 0, v, 0.1 * v)
    if act == ACT_MISH:
        return mish64(v)
    if act == ACT_RELU:
        return np.where(v < 0, 0.0, v)
    return v.copy()


def act_grad64(v, act):
    if act == ACT_LEAKY:
        return np.where(v > 0, 1.0, 0.1)
    if act == ACT_MISH:
        return mish_grad64(v)
    if act == ACT_RELU:
        return np.where(v > 0, 1.0, 0.0)
    return np.ones_like(v)


def colsum64(x):
    """(column sums, column sums of |x|) of an fp32 [M, C] array, accumulated in fp64"""
    x = np.asarray(x)
    return x.sum(axis=0, dtype=F64), np.abs(x).sum(axis=0, dtype=F64)


def stats_ref64(y, C=None, eps=EPS, chain=None):
    """Batch statistics of y [M, C] (fp32 values) in fp64, two-pass variance, with the bounds the kernel's fp32 partial
    sums allow: sums of `chain` fp32 additions each (everything after is fp64), so
        |sum y - s| <= chain u sum|y|,  |sum y^2 - ss| <= chain u sum y^2   (the square is fused into the add)
        dmean = that / M,  dvar = that / M + 2 |mean| dmean + dmean^2      (var = ss / M - mean^2)."""
    y = np.asarray(y, dtype=F64)
    M = y.shape[0]
    chain = sum_chain(M, y.shape[1]) if chain is None else chain
    mean = y.mean(axis=0)
    var = ((y - mean) ** 2).mean(axis=0)
    sa = np.abs(y).sum(axis=0)
    sq = (y * y).sum(axis=0)
    dmean = chain * U * sa / M
    dvar = chain * U * sq / M + 2.0 * np.abs(mean) * dmean + dmean ** 2
    e = F64(F32(eps))
    return dict(M=M, mean=mean, var=var, invstd=1.0 / np.sqrt(var + e), eps=e, dmean=dmean, dvar=dvar,
                unbiased=var * M / (M - 1) if M > 1 else var.copy())


def running_ref64(r, rmean, rvar, momentum=MOMENTUM):
    """running-stat update in fp64: (new mean, its bound, new var, its bound).  The kernel evaluates
    (1 - m) * old + m * new in fp32: RUN_CONST * 2^-23 * (sum of |addends|) plus the propagated statistic bound."""
    m = F64(F32(momentum))
    k = r['M'] / (r['M'] - 1.0) if r['M'] > 1 else 1.0
    rm, rv = np.asarray(rmean, F64), np.asarray(rvar, F64)
    new_m = (1.0 - m) * rm + m * r['mean']
    new_v = (1.0 - m) * rv + m * r['unbiased']
    bm = RUN_CONST * 2.0 ** -23 * (np.abs((1.0 - m) * rm) + np.abs(m * r['mean'])) + m * r['dmean']
    bv = RUN_CONST * 2.0 ** -23 * (np.abs((1.0 - m) * rv) + np.abs(m * r['unbiased'])) + m * r['dvar'] * k
    return new_m, bm, new_v, bv


def apply_ref64(y, mean, invstd, gamma, beta, act, res=None):
    """z = act(gamma xhat + beta) (+ res) in fp64 on the fp32 operands the kernel receives.
    Returns dict(z, v (pre-activation), actv, S = |y a| + |mean a| + |beta| (+ |res|), a = gamma invstd)."""
    y = np.asarray(y, F64)
    mean, invstd, gamma, beta = (np.asarray(t, F64) for t in (mean, invstd, gamma, beta))
    a = gamma * invstd
    v = (y - mean) * a + beta
    actv = act64(v, act)
    z = actv.copy()
    S = np.abs(y * a) + np.abs(mean * a) + np.abs(beta)
    if res is not None:
        z = z + np.asarray(res, F64)
        S = S + np.abs(np.asarray(res, F64))
    return dict(z=z, v=v, actv=actv, S=S)


def bwd_ref64(dz, y, mean, invstd, gamma, beta, act, frozen=False, chain=None):
    """Backward of z = act(gamma xhat + beta) in fp64 on the fp32 operands: dbeta = sum g, dgamma = sum g xhat,
    dy = gamma invstd (g - k1 - xhat k2), k1 = dbeta / M, k2 = dgamma / M (both 0 with frozen statistics), g = dz act'(v).

    Error model of the kernels (u = 2^-24), every term from the reference's own values:
      xhat: two roundings; v = fma(gamma, xhat, beta):      dv <= 4 u (|gamma xhat| + |beta|)
      act': mish  (|v| + MISH_GRAD_CONST) 2^-23 A, A the sum of the absolute addends of the derivative, plus dv (|mish''| <= 1);
            leaky / relu exact, except that an element with |v| <= 2 dv may take the other side of the kink
      Eg  = bound of g:   |dz| (that) + u |g|
      sums: chain u sum|terms| + sum of the per-term bounds (Eg, resp. Eg |xhat| + 3 u |g xhat|) + one final rounding
      dy:  DY_CONST 2^-23 S, S = |gi| (|g| + |k1| + |xhat k2|), + |gi| (Eg + dk1 + |xhat| dk2)."""
    dz, y = np.asarray(dz, F64), np.asarray(y, F64)
    mean, invstd, gamma, beta = (np.asarray(t, F64) for t in (mean, invstd, gamma, beta))
    M, C = y.shape
    chain = sum_chain(M, C) if chain is None else chain
    xh = (y - mean) * invstd
    v = gamma * xh + beta
    dv = 4.0 * U * (np.abs(gamma * xh) + np.abs(beta))
    if act == ACT_MISH:
        d, A = mish_grad64(v, parts=True)
        ed = (np.abs(v) + MISH_GRAD_CONST) * 2.0 ** -23 * A + dv
    else:
        d = act_grad64(v, act)
        jump = {ACT_LEAKY: 0.9, ACT_RELU: 1.0}.get(act, 0.0)
        ed = np.where(np.abs(v) <= 2.0 * dv, jump, 0.0)
    g = dz * d
    Eg = np.abs(dz) * ed + U * np.abs(g)
    gx = g * xh
    Egx = Eg * np.abs(xh) + 3.0 * U * np.abs(gx)
    sg, sgx = g.sum(axis=0), gx.sum(axis=0)
    b_sg = chain * U * np.abs(g).sum(axis=0) + Eg.sum(axis=0)
    b_sgx = chain * U * np.abs(gx).sum(axis=0) + Egx.sum(axis=0)
    if frozen:
        k1, k2, dk1, dk2 = (np.zeros(C) for _ in range(4))
    else:
        k1, k2 = sg / M, sgx / M
        dk1, dk2 = b_sg / M + U * np.abs(k1), b_sgx / M + U * np.abs(k2)
    gi = gamma * invstd
    dy = gi * (g - k1 - xh * k2)
    S = np.abs(gi) * (np.abs(g) + np.abs(k1) + np.abs(xh * k2))
    b_dy = DY_CONST * 2.0 ** -23 * S + np.abs(gi) * (Eg + dk1 + np.abs(xh) * dk2)
    return dict(dbeta=sg, dgamma=sgx, b_dbeta=b_sg + U * np.abs(sg), b_dgamma=b_sgx + U * np.abs(sgx), dy=dy, S=S, b_dy=b_dy,
                g=g, xh=xh, v=v, k1=k1, k2=k2, gi=gi)


def bwd_bound_ref64(r):
    """the true value of the bound the plane backward derives: max|gi| (max|g| + max|k1| + max|xhat| max|k2|)"""
    return float(np.abs(r['gi']).max() * (np.abs(r['g']).max() + np.abs(r['k1']).max() + np.abs(r['xh']).max() * np.abs(r['k2']).max()))


def bias_grad_ref64(x):
    """column sums and their bound: block r adds rows r, r + R, ... (ceil(M / R) fp32 additions), the rest is fp64"""
    M = x.shape[0]
    chain = -(-M // colsum_rows(M))
    s, sa = colsum64(x)
    return s, chain * U * sa + U * np.abs(s)


def fold_ref64(gamma, beta, rm, rv, eps=EPS):
    """eval fold: scale = gamma / sqrt(rv + eps), shift = beta - rm scale, with FOLD_CONST 2^-23 (sum of |addends|)"""
    gamma, beta, rm, rv = (np.asarray(t, F64) for t in (gamma, beta, rm, rv))
    s = gamma / np.sqrt(rv + F64(F32(eps)))
    sh = beta - rm * s
    return s, FOLD_CONST * 2.0 ** -23 * np.abs(s), sh, FOLD_CONST * 2.0 ** -23 * (np.abs(beta) + np.abs(rm * s))


def partials_ref64(part, M, eps=EPS):
    """statistics from partial rows [nparts, 2, C] (fp32), every addition in fp64.  The kernel adds the same numbers in
    fp64 in another order: n 2^-53 sum|terms| bounds either sum; var = ss / M - mean^2 cancels, so the bound is kept in
    absolute terms."""
    n = part.shape[0]
    s, sa = colsum64(part[:, 0])
    ss, ssa = colsum64(part[:, 1])
    mean = s / M
    var = np.maximum(ss / M - mean * mean, 0.0)
    dmean = (n + 8) * 2.0 ** -53 * sa / M
    dvar = (n + 8) * 2.0 ** -53 * ssa / M + 2.0 * np.abs(mean) * dmean + 4.0 * 2.0 ** -53 * mean * mean
    e = F64(F32(eps))
    return dict(M=M, mean=mean, var=var, invstd=1.0 / np.sqrt(var + e), eps=e, dmean=dmean, dvar=dvar,
                unbiased=var * M / (M - 1) if M > 1 else var.copy())


# ------------------------------------------------------------------------------------------ acceptance
# Allowances, with the largest constant needed on an MI355X over the cases of tests/test_gpu_bn_edges.py (each test prints
# its own).  A case that needs more than its allowance shows a wrong kernel or a wrong derivation: the number stays.
APPLY_CONST = 4.0            # roundings of a, b, the multiply-add and the skip add, in units of 2^-23 S: 1.24 needed
MISH_CONST = 8.0             # the activation's own error, (|v| + 8) 2^-23 |mish(v)|: as head_cases.decode_accept; 1.22 needed
MISH_GRAD_CONST = 16.0       # the same for the derivative: as the decode backward; dy uses 0.11 of its bound
DY_CONST = 4.0               # linear / leaky / relu: dy uses 0.33 of its bound, dgamma / dbeta 0.41 of theirs
RUN_CONST = 4.0              # 1.21 needed
FOLD_CONST = 4.0             # 1.01 needed


def judge(got, ref, bound):
    """(ok, used): ok where |got - ref| <= bound or <= TINY and got is no NaN; used = |got - ref| / bound, the share of
    the allowance an element needs (0 where the error is 0, inf where a zero bound is exceeded by more than TINY)"""
    got = np.asarray(got, dtype=F64)
    ref = np.asarray(ref, dtype=F64)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), ref.shape)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got - ref)
        ok = (err <= bound) | (err <= TINY)
        used = np.where(err <= TINY, 0.0, err / bound)
    ok &= ~np.isnan(got)
    used = np.where(np.isnan(got), np.inf, used)
    return ok, used


def left_out(ref, bound):
    """share of the elements whose (non-zero) reference and bound both lie under TINY: the only elements that are judged
    by the flush-to-zero floor alone.  (An exact zero with a zero bound is judged strictly: the result must be 0.)"""
    ref = np.asarray(ref, F64)
    bound = np.broadcast_to(np.asarray(bound, F64), ref.shape)
    return float(np.mean((bound < TINY) & (ref != 0) & (np.abs(ref) < TINY)))


def apply_bound(r, act):
    b = APPLY_CONST * 2.0 ** -23 * r['S']
    if act == ACT_MISH:
        b = b + (np.abs(r['v']) + MISH_CONST) * 2.0 ** -23 * np.abs(r['actv'])
    return b


def apply_accept(got, r, act):
    return judge(got, r['z'], apply_bound(r, act))


def mean_accept(got, r):
    return judge(got, r['mean'], r['dmean'] + U * np.abs(r['mean']))


def invstd_accept(got, r):
    """invstd = (var + eps)^-1/2 is monotone in var: the result must lie between its values at var + dvar and at
    max(var - dvar, 0) (the kernel clamps a negative variance to 0), widened by one rounding"""
    got = np.asarray(got, F64)
    lo = 1.0 / np.sqrt(r['var'] + r['dvar'] + r['eps']) * (1.0 - 2.0 * U)
    hi = 1.0 / np.sqrt(np.maximum(r['var'] - r['dvar'], 0.0) + r['eps']) * (1.0 + 2.0 * U)
    ok = (got >= lo) & (got <= hi)
    with np.errstate(invalid='ignore', divide='ignore'):
        used = np.where(got >= r['invstd'], (got - r['invstd']) / (hi - r['invstd']), (r['invstd'] - got) / (r['invstd'] - lo))
    return ok, np.where(np.isnan(got), np.inf, used)


# ------------------------------------------------------------------------------------------ seeded builders
RATIOS = (0.0, 10.0, 1000.0)             # |mean| / std of channel c: RATIOS[c % 3]


def const_channels(C):
    """channels that hold one value in every row (batch variance 0: the var < 0 clamp)"""
    return [c for c in range(C) if c % 7 == 3]


def make_y(M, C, seed, ratios=RATIOS):
    """y [M, C] fp32: N(mean_c, std_c) columns with |mean_c| / std_c = ratios[c % len], constant columns at c % 7 == 3"""
    rng = np.random.RandomState(seed)
    std = rng.uniform(0.5, 2.0, C)
    sign = np.where(rng.randint(0, 2, C) > 0, 1.0, -1.0)
    ratio = np.array([ratios[c % len(ratios)] for c in range(C)])
    mu = ratio * std * sign
    y = (rng.standard_normal((M, C)) * std + mu).astype(F32)
    cc = const_channels(C)
    for c in cc:
        y[:, c] = F32(1.1) * F32(1 + c % 5) * F32(sign[c])
    return y, dict(ratio=ratio, const=cc, std=std, mean=mu)


def make_params(C, seed):
    """(gamma, beta) fp32: |gamma| in [0.5, 1.5) with both signs, beta ~ N(0, 0.5)"""
    rng = np.random.RandomState(seed + 1000)
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.randint(0, 2, C) > 0, 1.0, -1.0)).astype(F32)
    beta = (rng.standard_normal(C) * 0.5).astype(F32)
    return gamma, beta


def make_grad(M, C, seed):
    return np.random.RandomState(seed + 2000).standard_normal((M, C)).astype(F32)


def make_res(M, C, seed):
    return np.random.RandomState(seed + 3000).standard_normal((M, C)).astype(F32)


def make_case(M, C, seed=None, ratios=RATIOS):
    """Everything a sweep over an [M, C] tensor needs: y, gamma, beta, dz, res and the fp32 statistics of y (the fp64
    batch statistics rounded once), plus the properties the case exists for."""
    seed = (M * 31 + C) % 100003 if seed is None else seed
    y, props = make_y(M, C, seed, ratios)
    gamma, beta = make_params(C, seed)
    st = stats_ref64(y)
    tpr, rpb = row_map(C)
    props.update(tpr=tpr, rpb=rpb, nrows=stat_rows(M, rpb), blocks=bn_blocks(M, C), grid=apply_grid(M, C),
                 laps=apply_laps(M, C), passes=channel_passes(C), nt=bn_loads_nt(C),
                 last_trip_rows=M % (PW_UNROLL * rpb))
    return dict(M=M, C=C, y=y, gamma=gamma, beta=beta, dz=make_grad(M, C, seed), res=make_res(M, C, seed),
                mean=st['mean'].astype(F32), invstd=st['invstd'].astype(F32), stats=st, props=props)


NONFINITE = (('nan', np.nan), ('+inf', np.inf), ('-inf', -np.inf))


def plant_nonfinite(y):
    """copy of y with a NaN, a +Inf and a -Inf in three different rows and channels: (y, [(row, channel, name)])"""
    y = np.array(y, dtype=F32)
    M, C = y.shape
    sites = []
    for k, (name, val) in enumerate(NONFINITE):
        m, c = divmod((M * C // 2 + k * (C + 1)) % (M * C), C)
        y[m, c] = val
        sites.append((m, c, name))
    return y, sites


def make_partials(nparts, C, seed, rows=64, mu=300.0):
    """Partial rows [nparts, 2, C] (fp32) of a tensor of M = nparts * rows pixels whose channels have mean +-mu and unit
    variance: sum y and sum y^2 of `rows` pixels each.  At mu = 300 the variance is 1e-5 of sum y^2 / M, so a sum held
    in fp32 anywhere misses it.  More than 4099 rows repeat the first 4099."""
    rng = np.random.RandomState(seed)
    n = min(nparts, 4099)
    sign = np.where(rng.randint(0, 2, C) > 0, 1.0, -1.0)
    e = rng.standard_normal((n, C)) * np.sqrt(rows)             # sum of the deviations of a block's pixels
    q = rows + rng.standard_normal((n, C)) * np.sqrt(2.0 * rows)  # sum of their squares
    part = np.empty((n, 2, C), dtype=F32)
    part[:, 0] = rows * mu * sign + e
    part[:, 1] = rows * mu * mu + 2.0 * mu * sign * e + q
    if nparts > n:
        part = np.resize(part, (nparts, 2, C))
    return part, nparts * rows
