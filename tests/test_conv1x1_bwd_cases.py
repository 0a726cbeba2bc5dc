# -*- coding: utf-8 -*-
"""Without a GPU: every case of tests/conv1x1_bwd_cases.py reaches the branch it is listed for, the host-side plan restated
there has the properties the cases rely on, the fp64 reference alone judges (almost) every element by its bound rather than by
the flush-to-zero floor, an emulation of the kernel's arithmetic from the split pieces is accepted by the bounds while a
kernel that dropped the lo pieces of dy is not, and the compiled kernel uses neither scratch nor spills."""
import os
import sys

import numpy as np
import pytest

import bn_cases as BC
import conv_cases as CC
import conv1x1_bwd_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from kernel_resources import kernel_resources  # noqa: E402

F32, F64 = np.float32, np.float64
SMALL = [c for c in FC.CASES if c['M'] <= 256]


@pytest.mark.parametrize('c', FC.CASES, ids=FC.case_id)
def test_case_reaches_its_branch(c):
    got = FC.reaches(c)
    assert set(c['want']) <= got, (c['want'], got)
    assert (c['Cout'], c['Cin']) in FC.SHAPES
    assert c['lddz'] >= c['dz_off'] + c['Cout'] and all(c[k] % 4 == 0 for k in ('lddz', 'dz_off', 'ldy', 'ldx', 'lddx', 'ldr'))


def test_every_listed_property_has_a_case():
    seen = set()
    for c in FC.CASES:
        seen |= set(c['want'])
    assert seen == {'one_row', 'short_chunk', 'whole_chunk', 'second_chunk', 'fewer_chunks_than_slots', 'short_last_block',
                    'many_blocks', 'dz_slice', 'pitches', 'prepared', 'nonfinite', 'act'}
    for shape in FC.SHAPES:
        for act in BC.ACTS:
            assert any((c['Cout'], c['Cin']) == shape and c['act'] == act for c in FC.CASES), (shape, act)
        assert any((c['Cout'], c['Cin']) == shape and c['res'] for c in FC.CASES)
        assert any((c['Cout'], c['Cin']) == shape and not c['res'] for c in FC.CASES)


@pytest.mark.parametrize('M', [1, 31, 32, 33, 229, 16384, 16385, FC.BIG, FC.MIN_ROWS, 1478656, 5914624])
def test_plan(M):
    for Cout in (32, 64):
        p = FC.plan(M, Cout)
        assert 1 <= p['blocks'] <= FC.RESIDENT and 1 <= p['last'] <= p['per']            # no block without a chunk
        assert (p['blocks'] - 1) * p['per'] + p['last'] == p['chunks'] == -(-M // 32)
        assert 1 <= p['tail_rows'] <= 32
        assert p['slabs'] == p['blocks'] * (2 if Cout == 32 else 1)
        assert FC.workspace(M, 64, Cout) % 4 == 0


@pytest.mark.parametrize('c', SMALL, ids=FC.case_id)
def test_reference_is_judged_by_its_bounds(c):
    d = FC.build(c)
    r = FC.bn_ref(c, d)
    word = FC.bound_word(r)
    if c['plant']:
        assert ((word >> 23) & 0xff) == 255 and BC.scale_exp(word) == 127       # poisoned: scale 1
    p = FC.products(c, d, r, word)
    for name in ('dx', 'dw'):
        ref, b = p[name], p['b_' + name]
        fin = np.isfinite(ref)
        assert not fin.any() or BC.left_out(ref[fin], b[fin]) <= CC.LEFT_OUT_CAP, name
        if not c['plant']:
            assert fin.all() and (b > 0).all()
            # the bound is an error bound, not a licence: a small share of the result's own scale (a single row is all
            # cancellation: g - k1 = 0)
            if c['M'] >= 97:
                assert np.median(b / np.maximum(np.abs(ref), 1e-300)) < 1e-3, name
    if c['plant']:
        chans = sorted(ch for _, ch in d['sites'])
        assert not np.isfinite(p['dx']).any()                                    # every pixel sums over the poisoned channels
        bad_rows = np.where(~np.isfinite(p['dw']).all(axis=1))[0].tolist()
        assert bad_rows == chans


def _emulate(c, d, r, word, drop_lo=False):
    """the kernel's arithmetic from the pieces, in fp64: dy (fp32 expression of the reference, rounded) split under `word`, x
    under its maximum, the filter under its own; (hi hi + (hi lo + lo hi) / 2048) / (s s')"""
    M, Cout, Cin = c['M'], c['Cout'], c['Cin']
    hd, ld = (t.astype(F64) for t in BC.split_f16x2(r['dy'].astype(F32), word))
    if drop_lo:
        ld = np.zeros_like(ld)
    xw, ww = BC.amax_word(d['x']), BC.amax_word(d['w'])
    hx, lx = (t.astype(F64) for t in BC.split_f16x2(d['x'], xw))
    hw, lw = (t.astype(F64) for t in BC.split_f16x2(d['w'], ww))
    sd, sx, sw = (F64(BC.scale_of(t)) for t in (word, xw, ww))
    dx = (hd.dot(hw) + (hd.dot(lw) + ld.dot(hw)) / 2048.0) / (sd * sw)
    if d['res'] is not None:
        dx = dx + d['res']
    dw = (hd.T.dot(hx) + (hd.T.dot(lx) + ld.T.dot(hx)) / 2048.0) / (sd * sx)
    return dx, dw


@pytest.mark.parametrize('c', [c for c in SMALL if not c['plant'] and c['M'] >= 97], ids=FC.case_id)
def test_bounds_accept_the_arithmetic_and_refuse_a_dropped_piece(c):
    d = FC.build(c)
    r = FC.bn_ref(c, d)
    word = FC.bound_word(r)
    p = FC.products(c, d, r, word)
    dx, dw = _emulate(c, d, r, word)
    for got, name in ((dx, 'dx'), (dw, 'dw')):
        ok, used = FC.judge(got, p[name], p['b_' + name])
        assert ok.all(), (name, float(used.max()))
    dx, dw = _emulate(c, d, r, word, drop_lo=True)
    assert not FC.judge(dx, p['dx'], p['b_dx'])[0].all()
    assert not FC.judge(dw, p['dw'], p['b_dw'])[0].all()


def test_prepared_filter_layout():
    w = CC.make_filter(64, 1, 128, 5, spread=4, axis=3).reshape(64, 128)
    buf = FC.prepared_filter(w)
    assert buf.nbytes == FC.dgrad_workspace(128, 64)
    word = int(buf[128 * 64 * 6 // 4])
    assert word == BC.amax_word(w)
    h = buf.view(np.uint16)[:128 * 64 * 2].reshape(128, 2, 2, 32)                 # [c][tile][hi / lo][32 n]
    hi, lo = BC.split_f16x2(w, word)
    assert (h[17, 1, 0].view(np.float16) == hi[32:64, 17]).all() and (h[17, 1, 1].view(np.float16) == lo[32:64, 17]).all()


def test_kernel_has_no_scratch_and_two_waves_per_simd():
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'conv1x1_bwd_fused.hip'))
    mine = [x for x in rows if FC.KERNEL in x['name']]
    assert len(mine) == len(FC.SHAPES) * len(BC.ACTS) * 2, [x['name'] for x in rows]
    bad = [(x['name'].split('(')[0], x['scratch'], x['vgpr_spill'], x['sgpr_spill'], x['occupancy']) for x in mine
           if x['scratch'] != 0 or x['vgpr_spill'] != 0 or x['sgpr_spill'] != 0 or x['occupancy'] < 2]
    assert not bad, bad
