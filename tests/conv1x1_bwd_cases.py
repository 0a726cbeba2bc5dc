# -*- coding: utf-8 -*-
"""Cases, fp64 references and acceptance bounds of the fused backward of conv 1x1 -> BatchNorm -> activation
(csrc/conv1x1_bwd_fused.hip), built from what the project already has: bn_cases.bwd_ref64 for dy and the bound words,
bn_cases.split_f16x2 / planes_decode for what the kernel's dy operand stands for under the scale word it reports, and
conv_cases.conv_dgrad64 / conv_wgrad64 / conv_bound for the two products.

What the kernel cannot show is its dy: it lives in registers.  The reference therefore rounds the fp64 dy to fp32, splits it
under the kernel's word and propagates, beside conv_bound, the distance the kernel's own operand may have from that:
    E_dy = b_dy (bwd_ref64: the error of the fp32 expression) + u |dy| (the rounding of the reference itself)
           + 2 split_error((|dy| + b_dy) s) / s (one split each side)
through the products with the absolute value of the other operand."""
import numpy as np

import bn_cases as BC
import conv_cases as CC

F32, F64 = np.float32, np.float64
SHAPES = ((64, 64), (32, 64), (64, 128))           # (Cout, Cin) the kernel takes
CHUNK = 32                                         # pixels per K step
RESIDENT = 512                                     # blocks the launch aims at: two on each of 256 CUs
MIN_ROWS = 131072                                  # the route's threshold in ops.ConvBNActFn.backward
KERNEL = 'conv1x1_bn_act_bwd_fused_f16x2'


def plan(M, Cout):
    """the host's split of M rows: chunks of 32, `per` chunks per block, only blocks that get a chunk are launched"""
    chunks = -(-M // CHUNK)
    per = max(1, -(-chunks // RESIDENT))
    blocks = -(-chunks // per)
    return dict(chunks=chunks, per=per, blocks=blocks, last=chunks - (blocks - 1) * per, tail_rows=M - (chunks - 1) * CHUNK,
                slabs=blocks * (2 if Cout == 32 else 1), empty_slots=max(0, RESIDENT - blocks))


def dgrad_workspace(Cin, Cout):
    return Cin * ((Cout + 31) // 32 * 32) * 6 + 64 + 4096


def workspace(M, Cin, Cout):
    a = lambda n: (n + 255) // 256 * 256
    return a(BC.bn_workspace(M, Cout)) + a(dgrad_workspace(Cin, Cout)) + 256 + plan(M, Cout)['slabs'] * Cout * Cin * 4


def _c(name, Cout, Cin, M, act=BC.ACT_MISH, res=False, lddz=None, dz_off=0, ldy=None, ldx=None, lddx=None, ldr=None,
       plant=False, prepared=False, want=()):
    return dict(name=name, Cout=Cout, Cin=Cin, M=M, act=act, res=res, lddz=lddz or Cout, dz_off=dz_off, ldy=ldy or Cout,
                ldx=ldx or Cin, lddx=lddx or Cin, ldr=ldr or Cin, plant=plant, prepared=prepared, want=tuple(want))


BIG = 39979                                        # 1250 chunks: 3 per block, 417 blocks, the last with 2, the last chunk with 11 rows
CASES = []
for _co, _ci in SHAPES:
    for _m, _w in ((1, 'one_row'), (31, 'short_chunk'), (32, 'whole_chunk'), (33, 'second_chunk'), (32 * 7 + 5, 'fewer_chunks_than_slots')):
        CASES.append(_c('m%d' % _m, _co, _ci, _m, res=bool(_m & 1), want=(_w,)))
    CASES.append(_c('big', _co, _ci, BIG, res=_co == 64, want=('short_last_block', 'many_blocks')))
CASES += [
    _c('slice', 64, 64, 229, lddz=128, dz_off=64, want=('dz_slice',)),
    _c('pitches', 64, 64, 229, res=True, ldy=72, ldx=68, lddx=76, ldr=80, want=('pitches',)),
    _c('pitches', 64, 128, 229, res=True, ldx=136, lddx=132, ldr=140, want=('pitches',)),
    _c('pitches_nores', 32, 64, 229, ldx=72, lddx=68, want=('pitches',)),
    _c('prepared', 64, 64, 229, res=True, prepared=True, want=('prepared',)),
    _c('prepared', 64, 128, 229, prepared=True, want=('prepared',)),
    _c('planted', 64, 64, 229, res=True, plant=True, want=('nonfinite',)),
    _c('planted', 32, 64, 229, plant=True, want=('nonfinite',)),
]
for _a in (BC.ACT_LINEAR, BC.ACT_LEAKY, BC.ACT_RELU):
    CASES.append(_c(BC.ACT_NAMES[_a], 64, 64, 229, act=_a, res=True, want=('act',)))
    CASES.append(_c(BC.ACT_NAMES[_a], 64, 128, 97, act=_a, want=('act',)))
    CASES.append(_c(BC.ACT_NAMES[_a], 32, 64, 97, act=_a, res=True, want=('act',)))


def case_id(c):
    return 'co%d_ci%d_%s' % (c['Cout'], c['Cin'], c['name'])


def reaches(c):
    """the branches a case reaches, from the host's plan and the case's own numbers"""
    p = plan(c['M'], c['Cout'])
    got = set()
    if c['M'] == 1:
        got.add('one_row')
    if p['chunks'] == 1 and c['M'] < CHUNK:
        got.add('short_chunk')
    if c['M'] % CHUNK == 0:
        got.add('whole_chunk')
    if p['chunks'] == 2:
        got.add('second_chunk')
    if p['empty_slots'] > 0 and p['chunks'] > 2:
        got.add('fewer_chunks_than_slots')
    if p['per'] > 1 and p['last'] < p['per']:
        got.add('short_last_block')
    if p['blocks'] > 256:
        got.add('many_blocks')
    if c['lddz'] == 128 and c['dz_off'] == 64:
        got.add('dz_slice')
    if c['ldx'] > c['Cin'] and c['lddx'] > c['Cin'] and (not c['res'] or c['ldr'] != c['lddx']):
        got.add('pitches')
    if c['prepared']:
        got.add('prepared')
    if c['plant']:
        got.add('nonfinite')
    if c['act'] != BC.ACT_MISH:
        got.add('act')
    return got


PLANT = ((0.37, 5, np.nan), (0.71, 9, np.inf))      # (row as a share of M, channel, value) written into dz


def build(c):
    """the operands of a case: bn_cases.make_case over [M, Cout] (y, dz, gamma, beta, statistics), x and the skip operand
    from conv_cases.make_values, the filter from conv_cases.make_filter (input channels differing by 2^+-4)"""
    M, Cout, Cin = c['M'], c['Cout'], c['Cin']
    seed = CC.seed_of(M, Cout, Cin, c['act'])
    b = BC.make_case(M, Cout, seed % 100003)
    dz = np.array(b['dz'], dtype=F32)
    sites = []
    if c['plant']:
        for share, ch, val in PLANT:
            m = int(share * M)
            dz[m, ch] = val
            sites.append((m, ch))
    x = CC.make_values(M, Cin, seed + 1, spread=2)
    w = CC.make_filter(Cout, 1, Cin, seed + 2, spread=4, axis=3).reshape(Cout, Cin)
    res = CC.make_values(M, Cin, seed + 3, lo=0.01, hi=0.05) if c['res'] else None
    return dict(dz=dz, y=b['y'], mean=b['mean'], invstd=b['invstd'], gamma=b['gamma'], beta=b['beta'], x=x, w=w, res=res, sites=sites)


def bn_ref(c, d):
    with np.errstate(invalid='ignore', over='ignore'):
        return BC.bwd_ref64(d['dz'], d['y'], d['mean'], d['invstd'], d['gamma'], d['beta'], c['act'])


def bound_word(r):
    """a word the kernel's bound may not fall below: the true bound of bn_cases.bwd_bound_ref64 (the kernel's, formed from
    rounded maxima times 1.0001 twice, lies at or a little above it).  The CPU test splits under this word."""
    with np.errstate(invalid='ignore'):
        v = np.array([BC.bwd_bound_ref64(r)], dtype=F32)
    return int(v.view(np.uint32)[0])


def products(c, d, r, word, rows=None):
    """references of dx and dW for the dy operand split under `word`, with their elementwise bounds.  rows: dx only for
    these pixels (a row of dx depends on its own row of dy alone; dW always sums all rows).
    -> dict(dx, b_dx, dw, b_dw, dg, wg: the conv_cases reference dicts, dx64 / dw64: the products of the unsplit fp64 dy)"""
    M, Cout, Cin = c['M'], c['Cout'], c['Cin']
    s = F64(BC.scale_of(word))
    rows = np.arange(M) if rows is None else np.asarray(rows)
    R = len(rows)
    with np.errstate(invalid='ignore', over='ignore'):
        dy32 = r['dy'].astype(F32)
        hi, lo = BC.split_f16x2(dy32, word)
        dydec = BC.planes_decode(hi, lo, word)
        e_dy = r['b_dy'] + BC.U * np.abs(r['dy']) + 2.0 * BC.split_error((np.abs(r['dy']) + r['b_dy']) * s) / s
        xa = CC.act_f16x2(d['x'])
        w4 = d['w'].reshape(Cout, 1, 1, Cin)
        dy4, x4, e4 = dydec.reshape(1, 1, M, Cout), xa['dec'].reshape(1, 1, M, Cin), e_dy.reshape(1, 1, M, Cout)
        res = None if d['res'] is None else np.asarray(d['res'])[rows].reshape(1, 1, R, Cin)
        dg = CC.dgrad_ref(dydec[rows].reshape(1, 1, R, Cout), w4, 1, 1, 1, R, False, res=res)
        b_dx = CC.conv_bound(dg, False)[0] + CC.conv_dgrad64(e_dy[rows].reshape(1, 1, R, Cout), np.abs(w4.astype(F64)), 1, 1, 1, R)
        wg = CC.wgrad_ref(x4, dy4, 1, 1, plan(M, Cout)['slabs'])
        b_dw = CC.conv_bound(wg, False)[0] + CC.conv_wgrad64(np.abs(x4), e4, 1, 1)
        dx64 = CC.conv_dgrad64(r['dy'][rows].reshape(1, 1, R, Cout), w4, 1, 1, 1, R)
        if res is not None:
            dx64 = dx64 + res
        dw64 = CC.conv_wgrad64(np.asarray(d['x']).reshape(1, 1, M, Cin), r['dy'].reshape(1, 1, M, Cout), 1, 1)
    return dict(dx=dg['y'].reshape(R, Cin), b_dx=b_dx.reshape(R, Cin), dw=wg['y'].reshape(Cout, Cin), b_dw=b_dw.reshape(Cout, Cin),
                dg=dg, wg=wg, dx64=dx64.reshape(R, Cin), dw64=dw64.reshape(Cout, Cin))


def judge(got, ref, bound):
    """bn_cases.judge where the reference is finite; where it is not (a planted NaN / Inf), the result must not be finite
    either.  -> (ok, used)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    fin = np.isfinite(ref) & np.isfinite(np.broadcast_to(bound, ref.shape))
    ok, used = BC.judge(np.where(fin, got, 0.0), np.where(fin, ref, 0.0), np.where(fin, bound, 0.0))
    return np.where(fin, ok, ~np.isfinite(got)), np.where(fin, used, 0.0)


def prepared_filter(w):
    """the transposed split filter as the forward call leaves it for the backward pass (y4_conv2d_dgrad_workspace layout):
    rows [Cin] of [Cout / 32][32 hi | 32 lo] fp16 words under the scale of max|w|, the maximum word behind 6 bytes per element"""
    Cout, Cin = w.shape
    word = BC.amax_word(w)
    hi, lo = BC.split_f16x2(np.ascontiguousarray(w.T), word)
    buf = np.zeros(dgrad_workspace(Cin, Cout) // 4, dtype=np.uint32)
    buf.view(np.uint16)[:Cin * Cout * 2] = BC.planes_pack(hi, lo).ravel()
    buf[Cin * Cout * 6 // 4] = word
    return buf
