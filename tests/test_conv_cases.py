# -*- coding: utf-8 -*-
"""tests/conv_cases.py without a GPU: every case of tests/test_gpu_conv_planes_edges.py reaches the branch it is listed
for (by the mirror of the host dispatch), the fp64 references are torch's double convolutions, the operand builders
round-trip, an fp32 evaluation in another order is accepted, and a reference with one tap, one channel, the bias, the last
row or column or the lo * hi product missing is rejected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import conv_cases as CC

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------ the mirror and the case lists
def test_forward_cases_reach_their_branches():
    seen = set()
    for c in CC.FWD_GRID['f16x2'] + CC.FWD_GRID['bf16'] + CC.FWD_CASES + CC.STREAM_CASES:
        name, nparts, rows = CC.fwd_kernel(c)
        assert CC.tag(name) == c['want'], (CC.case_id(c), name)
        bf = CC.is_bf(c['mode'])
        assert (', true, ' in name or 'stream' in name) == bf
        assert not (c['bias'] and (c['partials'] or c['y_bf16']))
        assert not c['y_bf16'] or (bf and c['Cout'] % 32 == 0)
        assert c['Cin'] % (64 if bf else 32) == 0 and c['Cout'] % 4 == 0
        M, N, Cs = CC.fwd_dims(c)
        assert CC.conv_window_ok(c['B'], c['H'], c['W'], Cs, N, c['k'], c['s'], bf)
        assert nparts <= CC.cdiv(M, 128)                                 # the size the ABI asks of the partial buffer
        seen.add((bf, c['want'], c['y_bf16'], c['bias'], c['partials'], c['ldy_pad'] > 0))
    for bf in (False, True):
        for want in ('tile128x128', 'tile256x128'):
            assert any(s[0] == bf and s[1] == want and s[3] for s in seen), (bf, want, 'bias')
            assert any(s[0] == bf and s[1] == want and s[4] for s in seen), (bf, want, 'partials')
            assert any(s[0] == bf and s[1] == want and s[5] for s in seen), (bf, want, 'pitch')
    for want in ('tile128x128', 'tile256x128', 'tile256x256', 'stream'):
        assert any(s[0] and s[1] == want and s[2] for s in seen), (want, 'bf16 result')
    grid = {(c['W'], c['Cout']) for c in CC.FWD_GRID['bf16']}
    assert grid == {(M, N) for M in (1, 127, 128, 129, 257) for N in (4, 36, 128, 132, 192)}


def test_streaming_cases_cover_the_template_arguments_and_the_tile_rounds():
    names = {CC.fwd_kernel(c)[0] for c in CC.STREAM_CASES} | {CC.dgrad_kernel(c) for c in CC.DGRAD_CASES}
    for ks in (4, 8):
        for nt in (1, 2, 4):
            assert any(n.startswith('conv1x1_stream_bf16<%d, %d, 4' % (ks, nt)) for n in names), (ks, nt)
    assert CC.stream_name(64, 4, False) == 'conv1x1_stream_bf16<4, 1, 4, false>'
    assert CC.stream_name(128, 96, True) == 'conv1x1_stream_bf16<8, 4, 4, true>'
    # 131071 rows do not stream; 131072 do; 131072 + 37 rows are 1025 tiles on 512 blocks: one block takes 3, the others 2
    assert not CC.stream_ok(131071, 64, 64, 1, 1) and CC.stream_ok(131072, 64, 64, 1, 1)
    name, grid, rows = CC.planes_conv_kernel(True, 131072 + 37, 36, 128, 1)
    assert grid == 512 and CC.cdiv(131072 + 37, 128) == 1025 and rows == 384
    assert {len(range(b, 1025, 512)) for b in range(512)} == {2, 3}
    # what keeps a call off the streaming kernel: 3 x 3, stride 2, other channel counts, wide N, a bf16 result with a skip
    # operand or an odd N, and a bias
    assert not CC.stream_ok(1 << 18, 64, 64, 3, 1) and not CC.stream_ok(1 << 18, 64, 64, 1, 2)
    assert not CC.stream_ok(1 << 18, 64, 192, 1, 1) and not CC.stream_ok(1 << 18, 132, 64, 1, 1)
    assert not CC.stream_ok(1 << 18, 64, 64, 1, 1, y_bf16=True, res=True) and CC.stream_ok(1 << 18, 64, 64, 1, 1, res=True)
    assert not CC.stream_ok(1 << 18, 64, 64, 1, 1, bias=True)


def test_small_and_big_rules():
    # short K: always the 128-row shape; long K: 256 rows unless the grid quantises badly
    assert CC.planes_small(10 ** 6, 128, 256) == (True, False)
    assert CC.planes_small(32768, 128, 288) == (True, True)              # 256 blocks of 128 rows: one round
    assert CC.planes_small(32769, 128, 288) == (False, False)            # the smallest natural 256-row case
    assert CC.planes_small(65537, 128, 288) == (True, True)              # 513 blocks: 3 units against 4
    assert not CC.bf_big(257, 192) and CC.bf_big(257, 192, 2) and not CC.bf_big(32769, 192, 1) and CC.bf_big(32769, 192)
    assert not CC.bf_big(32769, 128)
    assert CC.nparts(False, 257, 36, 64, 1) == 3 and CC.nparts(False, 32769, 36, 288, 1) == 129
    assert CC.nparts(True, 131072 + 37, 36, 64, 1) == 512 and CC.nparts(True, 131072 + 37, 192, 64, 1) == 513


def test_dgrad_cases_and_parity_classes():
    for c in CC.DGRAD_CASES:
        assert CC.tag(CC.dgrad_kernel(c)) == c['want'], CC.case_id(c)
        bf = CC.is_bf(c['mode'])
        assert c['Cout'] % (64 if bf else 32) == 0 and c['Cin'] % 4 == 0
        assert not (c['s'] == 2 and (c['res'] or c['H'] % 2 or c['W'] % 2 or c['k'] != 3))
    cl = CC.dgrad_s2_classes()
    assert [(ph, pw) for ph, pw, _ in cl] == [(1, 1), (1, 0), (0, 1), (0, 0)]
    assert [len(t) for _, _, t in cl] == [4, 2, 2, 1]
    assert sorted(s for _, _, t in cl for _, _, s in t) == list(range(9))       # every filter tap in exactly one class
    # dx pixel (2 hc + ph, 2 wc + pw) receives tap (r, q) from dy pixel (hc + dh, wc + dw): 2 (hc + dh) + r - 1 = 2 hc + ph
    for ph, pw, taps in cl:
        for dh, dw, slot in taps:
            r, q = divmod(slot, 3)
            assert 2 * dh + r - 1 == ph and 2 * dw + q - 1 == pw
    ragged = [c for c in CC.DGRAD_CASES if c['name'] == 's2-ragged'][0]
    M = ragged['B'] * ragged['H'] * ragged['W'] // 4
    assert 256 < M < 512 and M % 256 and 128 < ragged['Cin'] < 256


def test_wgrad_cases_and_plan():
    for c in CC.WGRAD_CASES:
        tn, ntn, ntj, splits, per = CC.wgrad_case_plan(c)
        assert tn == c['want_tn'] and (splits > 1) == c['many'], (CC.case_id(c), splits)
        Ho, Wo = CC.out_hw(c['H'], c['W'], c['k'], c['s'])
        steps = CC.cdiv(c['B'] * Ho * Wo, 32)
        assert (splits - 1) * per < steps <= splits * per
        assert ntj == CC.cdiv(c['k'] * c['k'] * c['Cin'], 256)
    assert any(CC.wgrad_case_plan(c)[2] > 1 for c in CC.WGRAD_CASES) and any(CC.wgrad_case_plan(c)[2] == 1 for c in CC.WGRAD_CASES)
    assert {c['Cout'] for c in CC.WGRAD_CASES} >= {32, 255, 256}
    assert any(c['k'] * c['k'] * c['Cin'] > 256 for c in CC.WGRAD_CASES)
    # the plan of a large layer: 128 -> 128 3 x 3 at 76^2, batch 8
    ntn, ntj, splits, per = CC.wgrad_plan(8 * 76 * 76, 128, 128, 3, 128, False)
    assert (ntn, ntj) == (1, 5) and splits * ntn * ntj <= 256 and splits * per >= CC.cdiv(8 * 76 * 76, 32)
    assert CC.wgrad_workspace(1, 5, 7, 32, 32, 3, 1) == 64
    assert CC.wgrad_workspace(2, 21, 23, 32, 255, 3, 1) == 64 + max(
        CC.wgrad_plan(966, 32, 255, 3, 128, bf)[2] for bf in (False, True)) * 255 * 288 * 4
    assert CC.wgrad_name(128, False, 1) == 'wgrad_planes_mfma<128, 256, false, 1>'
    assert CC.wgrad_name(256, True, 2) == 'wgrad_planes_mfma<256, 256, true, 2>'


def test_window_rule():
    assert CC.conv_window_ok(1, 1, 131109, 128, 128, 1, 1, True)
    assert not CC.conv_window_ok(1, 4096, 4096, 64, 64, 1, 1, False)      # one image of 4 GiB
    assert not CC.conv_window_ok(1 << 20, 64, 64, 32, 32, 1, 1, False)    # 2^32 pixels
    assert CC.conv_window_ok(64, 2, 2, 32, 32, 3, 1, False) and not CC.conv_window_ok(1, 0, 5, 32, 32, 1, 1, False)


# ------------------------------------------------------------------------------------------ references against torch
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64))).permute(0, 3, 1, 2)


def _close(a, b):
    return float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max())


@pytest.mark.parametrize('k,s,H,W', [(1, 1, 3, 5), (3, 1, 7, 9), (3, 1, 8, 6), (3, 2, 7, 9), (3, 2, 8, 6), (3, 2, 2, 2), (1, 2, 6, 4)])
def test_references_are_the_double_convolutions_of_torch(k, s, H, W):
    B, Cin, Cout = 2, 5, 7
    rng = np.random.RandomState(k * 100 + s * 10 + H)
    x = rng.standard_normal((B, H, W, Cin))
    w = rng.standard_normal((Cout, k, k, Cin))
    Ho, Wo = CC.out_hw(H, W, k, s)
    dy = rng.standard_normal((B, Ho, Wo, Cout))
    pad = (k - 1) // 2
    wt = torch.from_numpy(w).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(_nchw(x), wt, None, s, pad).permute(0, 2, 3, 1).numpy()
    assert y.shape == (B, Ho, Wo, Cout) and _close(CC.conv_fwd64(x, w, k, s), y)
    dx = torch.nn.grad.conv2d_input((B, Cin, H, W), wt, _nchw(dy).contiguous(), s, pad).permute(0, 2, 3, 1).numpy()
    assert _close(CC.conv_dgrad64(dy, w, k, s, H, W), dx)
    dw = torch.nn.grad.conv2d_weight(_nchw(x).contiguous(), (Cout, Cin, k, k), _nchw(dy).contiguous(), s, pad).permute(0, 2, 3, 1).numpy()
    assert _close(CC.conv_wgrad64(x, dy, k, s), dw)
    # the adjoint identity <conv(x), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)>
    a = float((CC.conv_fwd64(x, w, k, s) * dy).sum())
    assert abs(a - float((x * CC.conv_dgrad64(dy, w, k, s, H, W)).sum())) <= 1e-11 * abs(a)
    assert abs(a - float((w * CC.conv_wgrad64(x, dy, k, s)).sum())) <= 1e-11 * abs(a)
    # the companions are the same sums over absolute values
    assert (CC.conv_fwd64(np.abs(x), np.abs(w), k, s) >= np.abs(CC.conv_fwd64(x, w, k, s)) * (1 - 1e-12)).all()


# ------------------------------------------------------------------------------------------ builders
def test_values_have_the_scales_they_are_built_for():
    v = CC.make_values(64, 96, 3, spread=10)
    top = np.abs(v).max(axis=0)
    assert (top[0::3] < 2.0 ** -9).all() and (top[1::3] >= 0.5).all() and (top[1::3] < 2).all() and (top[2::3] >= 2.0 ** 9).all()
    assert np.abs(v).min() >= 2.0 ** -11 and (np.sign(v) != 0).all() and (v < 0).any() and (v > 0).any()
    assert np.array_equal(v, CC.make_values(64, 96, 3, spread=10))
    w = CC.make_filter(36, 3, 32, 5, axis=0)
    assert w.shape == (36, 3, 3, 32) and np.abs(w[0]).max() < 2.0 ** -9 and np.abs(w[2]).min() > 2.0 ** 4
    w = CC.make_filter(36, 3, 33, 5, axis=3)
    assert np.abs(w[..., 0]).max() < 2.0 ** -9 and np.abs(w[..., 2]).min() > 2.0 ** 4


def test_f16x2_planes_round_trip():
    a = CC.make_values(37, 96, 11, spread=10)
    p = CC.act_f16x2(a)
    assert p['word'] == BC.amax_word(a) and p['words'].shape == (37, 96) and p['words'].dtype == np.uint32
    assert (np.abs(p['dec'] - a.astype(F64)) <= 2.0 ** -22 * np.abs(a)).all()
    hi, lo = BC.planes_unpack(p['words'].view(np.uint16).reshape(37, 192))
    assert np.array_equal(hi.view(np.uint16), p['hi'].view(np.uint16)) and np.array_equal(lo.view(np.uint16), p['lo'].view(np.uint16))
    # the layout, spelled out: channel c of pixel m sits at half-word (c / 32) 64 + c % 32 (hi) and + 32 (lo)
    h = p['words'].view(np.uint16).reshape(37, 192)
    for c in (0, 31, 32, 95):
        assert np.array_equal(h[:, (c // 32) * 64 + c % 32], p['hi'][:, c].view(np.uint16))
        assert np.array_equal(h[:, (c // 32) * 64 + 32 + c % 32], p['lo'][:, c].view(np.uint16))
    # a channel slice of a wider row, pad channels zero
    q = CC.act_f16x2(a, ld=192, off=64, c_valid=70)
    assert q['words'].shape == (37, 192)
    assert (q['words'][:, :64] == BC.SENT).all() and (q['words'][:, 160:] == BC.SENT).all()
    assert (q['dec'][:, 70:] == 0).all() and (q['dec'][:, :70] != 0).all()
    hq, lq = BC.planes_unpack(q['words'][:, 64:160].copy().view(np.uint16).reshape(37, 192))
    assert (hq[:, 70:].view(np.uint16) == 0).all() and (lq[:, 70:].view(np.uint16) == 0).all()
    assert q['word'] == BC.amax_word(a[:, :70])


def test_bf16_rows_are_torch_bfloat16():
    a = CC.make_values(37, 128, 12, spread=10)
    p = CC.act_bf16(a)
    t = torch.from_numpy(a).bfloat16()
    assert np.array_equal(p['dec'], t.double().numpy())
    h = p['words'].view(np.uint16).reshape(37, 256)
    assert np.array_equal(h[:, :128].astype(np.int32), t.view(torch.int16).numpy().astype(np.int32) & 0xffff)
    assert (p['words'][:, 64:] == BC.SENT).all()                         # the second half of a dense row is never written
    q = CC.act_bf16(a, ld=320, off=128, c_valid=100)
    hq = q['words'].view(np.uint16).reshape(37, 640)
    assert np.array_equal(hq[:, 128:228], h[:, :100]) and (hq[:, 228:256] == 0).all()
    assert (q['words'][:, :64] == BC.SENT).all() and (q['words'][:, 128:] == BC.SENT).all()
    assert (q['dec'][:, 100:] == 0).all()


def test_filter_seen():
    w = CC.make_filter(36, 3, 32, 9)
    v, d = CC.filter_seen(w, True)
    assert d is None and np.array_equal(v, torch.from_numpy(w).bfloat16().double().numpy())
    v, d = CC.filter_seen(w, False)
    assert np.array_equal(v, w.astype(F64))
    p = CC.act_f16x2(w.reshape(36, -1))                                  # the split the library applies: within its bound
    assert (np.abs(p['dec'].reshape(w.shape) - v) <= d).all() and (d <= 2.0 ** -21 * np.abs(v)).all()


# ------------------------------------------------------------------------------------------ acceptance
def _small_case(bf, k, s, bias=True, seed=1):
    B, H, W, Cin, Cout = 2, 5, 6, 64, 36
    x = CC.make_values(B * H * W, Cin, seed, spread=2)
    w = CC.make_filter(Cout, k, Cin, seed + 1)
    xa = CC.act_planes(x, bf)
    b = CC.make_values(1, Cout, seed + 2, spread=10)[0] if bias else None
    r = CC.fwd_ref(xa['dec'].reshape(B, H, W, Cin), w, k, s, bf, b)
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x=x, w=w, xa=xa, bias=b, r=r)


@pytest.mark.parametrize('bf', (False, True), ids=('f16x2', 'bf16'))
@pytest.mark.parametrize('k,s', ((1, 1), (3, 1), (3, 2)))
def test_an_fp32_evaluation_in_another_order_is_accepted(bf, k, s):
    c = _small_case(bf, k, s)
    r = c['r']
    assert CC.left_out(r, bf) <= CC.LEFT_OUT_CAP
    wv = CC.filter_seen(c['w'], bf)[0]
    if not bf:                                                           # the filter as the library's split decodes it
        wv = CC.act_f16x2(c['w'].reshape(c['Cout'], -1))['dec'].reshape(c['w'].shape)
    got = CC.emulate_f32(c['xa']['dec'].reshape(c['B'], c['H'], c['W'], c['Cin']), wv, k, s)
    got = (got + c['bias'].astype(F32)).astype(F32)
    ok, used = CC.conv_accept(got, r, bf)
    assert ok.all() and used.max() < 1.0, used.max()
    # ... and rounded to bf16, under the bf16 criterion only
    gb = BC.bf16_to_f32(BC.bf16_rne(got))
    ok, _ = CC.conv_accept(gb, r, bf, y_bf16=True)
    assert ok.all()
    if k == 1:                                                           # (K = 64: the fp32 bound is far under a bf16 ulp)
        ok, _ = CC.conv_accept(gb, r, bf)
        assert ok.mean() < 0.5
    # the exact f16x2 arithmetic (three products per element, in fp64) is accepted too
    if not bf:
        xa = dict(c['xa'], hi=c['xa']['hi'].reshape(c['B'], c['H'], c['W'], c['Cin']), lo=c['xa']['lo'].reshape(c['B'], c['H'], c['W'], c['Cin']))
        wa = CC.act_f16x2(c['w'].reshape(c['Cout'], -1))
        wa = dict(wa, hi=wa['hi'].reshape(c['w'].shape), lo=wa['lo'].reshape(c['w'].shape))
        ok, used = CC.conv_accept(CC.emulate_f16x2(xa, wa, k, s) + c['bias'], r, False)
        assert ok.all() and used.max() < 0.5
        # mutation: the lo_x * hi_w product dropped -- an error of 2^-12 |x w| per term with random signs, sqrt(K) of them
        # deep, against an accumulation term that grows with K^2: rejected at K = 64, under the bound at K = 576
        ok, _ = CC.conv_accept(CC.emulate_f16x2(xa, wa, k, s, drop='lohi') + c['bias'], r, False)
        if k == 1:
            assert ok.mean() < 0.5


@pytest.mark.parametrize('bf', (False, True), ids=('f16x2', 'bf16'))
def test_mutated_references_are_rejected(bf):
    k, s = 3, 1
    c = _small_case(bf, k, s)
    r, B, H, W, Cin = c['r'], c['B'], c['H'], c['W'], c['Cin']
    xd = c['xa']['dec'].reshape(B, H, W, Cin)
    wv = CC.filter_seen(c['w'], bf)[0]
    ok, _ = CC.conv_accept(r['y'], r, bf)
    assert ok.all()
    # one tap dropped: every output that has the tap inside the map
    for tap in ((0, 0), (1, 1), (2, 1)):
        ok, _ = CC.conv_accept(CC.conv_fwd64(xd, wv, k, s, skip_tap=tap) + c['bias'], r, bf)
        assert ok.mean() < 0.35, tap
    # one channel of one K tile dropped: every output
    for ch in (0, 33, Cin - 1):
        x2 = xd.copy()
        x2[..., ch] = 0
        ok, _ = CC.conv_accept(CC.conv_fwd64(x2, wv, k, s) + c['bias'], r, bf)
        assert ok.mean() < 0.1, ch                                        # (a few sums cancel to under the bound)
    # ... in one tap only
    w2 = wv.copy()
    w2[:, 2, 2, 5] = 0
    ok, _ = CC.conv_accept(CC.conv_fwd64(xd, w2, k, s) + c['bias'], r, bf)
    assert ok.mean() < 0.5
    # the bias dropped: every output, the columns of small scale included
    ok, _ = CC.conv_accept(r['v'], r, bf)
    assert not ok.any()
    # the last row / the last column not computed (zero, or left as it was)
    for fill in (0.0, np.nan):
        g = r['y'].copy()
        g.reshape(-1, c['Cout'])[-1, :] = fill
        ok, _ = CC.conv_accept(g, r, bf)
        assert ok.reshape(-1, c['Cout'])[-1].mean() < 0.1 and ok.reshape(-1, c['Cout'])[:-1].all()
        g = r['y'].copy()
        g[..., -1] = fill
        ok, _ = CC.conv_accept(g, r, bf)
        assert ok[..., -1].mean() < 0.1 and ok[..., :-1].all()      # (an element that happens to be 0 within its bound)
    # an error of 3 % of the element in a column 2^-20 of the largest: far inside a whole-tensor criterion, rejected here
    col = int(np.argmin(np.abs(r['y']).max(axis=(0, 1, 2))))
    g = r['y'].copy()
    g[..., col] *= 1 + 2.0 ** -5
    assert np.abs(g - r['y']).max() < 2e-6 * np.abs(r['y']).max()
    ok, _ = CC.conv_accept(g, r, bf)
    assert ok[..., col].mean() < 0.2 and np.delete(ok, col, axis=3).all()


def test_dgrad_and_wgrad_bounds_reject_a_dropped_tap_and_a_dropped_pixel():
    B, H, W, Cin, Cout, k = 2, 6, 8, 36, 32, 3
    for bf in (False, True):
        for s in (1, 2):
            Ho, Wo = CC.out_hw(H, W, k, s)
            dy = CC.act_planes(CC.make_values(B * Ho * Wo, 64, 5), bf)['dec'].reshape(B, Ho, Wo, 64)
            w = CC.make_filter(64, k, Cin, 6, axis=3)
            res = CC.make_values(B * H * W, Cin, 7, spread=10).reshape(B, H, W, Cin) if s == 1 else None
            r = CC.dgrad_ref(dy, w, k, s, H, W, bf, res)
            assert CC.left_out(r, bf) <= CC.LEFT_OUT_CAP
            ok, _ = CC.conv_accept(r['y'], r, bf)
            assert ok.all()
            wv = CC.filter_seen(w, bf)[0]
            g = CC.conv_dgrad64(dy, wv, k, s, H, W, skip_tap=(0, 2)) + (r['r'] if s == 1 else 0.0)
            ok, _ = CC.conv_accept(g, r, bf)
            if s == 2:                                                   # tap (0, 2) belongs to parity class (1, 1) alone
                assert ok[:, 0::2].all() and ok[:, :, 0::2].all() and not ok[:, 1:-1:2, 1:-1:2].any()
            else:
                assert ok.mean() < 0.4
            if s == 2:                                                   # one parity class skipped: a quarter of dx missing
                g = r['y'].copy()
                g[:, 1::2, 0::2] = 0
                ok, _ = CC.conv_accept(g, r, bf)
                assert not ok[:, 1::2, 0::2].any()
            x = CC.act_planes(CC.make_values(B * H * W, 64, 8), bf)['dec'].reshape(B, H, W, 64)
            dyw = CC.act_planes(CC.make_values(B * Ho * Wo, 32, 9, spread=10), bf)['dec'].reshape(B, Ho, Wo, 32)
            rw = CC.wgrad_ref(x, dyw, k, s, 2)
            assert rw['v'].shape == (32, 3, 3, 64) and CC.left_out(rw, bf) <= CC.LEFT_OUT_CAP
            ok, _ = CC.conv_accept(rw['y'], rw, bf)
            assert ok.all()
            d2 = dyw.copy()
            d2[-1, -1, -1] = 0                                           # the last pixel dropped (a split that ends early)
            ok, _ = CC.conv_accept(CC.conv_wgrad64(x, d2, k, s), rw, bf)
            assert not ok[:, :2, :2].any()                               # every tap that reads the pixel inside the map


def test_bf16_half_ulp_and_column_sums():
    z = np.array([1.0, 1.5, 1.9999, 2.0, 0.75, 3e-5, 0.0])
    h = CC.bf16_half_ulp(z)
    assert np.array_equal(h[:5], [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9]) and h[6] == 0
    assert (h[:6] > 2.0 ** -9 * z[:6] * (1 - 1e-12)).all() and (h[:6] <= 2.0 ** -8 * z[:6]).all()
    v = np.random.RandomState(4).uniform(0.5, 2, 4096).astype(F32)       # RNE never moves a value by more than that
    assert (np.abs(BC.bf16_to_f32(BC.bf16_rne(v)).astype(F64) - v) <= CC.bf16_half_ulp(v)).all()
    y = CC.make_values(300, 36, 2, spread=10)
    part = np.zeros((3, 2, 36), dtype=F32)
    for i in range(3):
        blk = y[128 * i:128 * (i + 1)]
        for row in blk:                                                  # sequential fp32 sums
            part[i, 0] = part[i, 0] + row
            part[i, 1] = part[i, 1] + row * row
    ok, used = CC.colsum_accept(part, y, 128)
    assert ok.all() and used.max() < 0.5
    part[1, 0, 3] -= y[200, 3]                                           # one row missing from one column
    ok, _ = CC.colsum_accept(part, y, 128)
    assert not ok[3] and ok[:3].all() and ok[4:].all()


def test_no_case_leaves_an_element_to_the_floor():
    """Every operand value of every GPU case is at least 2^-11 in magnitude with a filter entry of at least
    2^-11 / sqrt(K) (conv_cases.make_values, make_filter), and every output has the centre tap inside the map: S >= 2^-22 /
    sqrt(K), so the accumulation term alone is far above TINY and no element is judged by the floor (left_out = 0 <= 1 %),
    however the signed sum cancels.  (The GPU tests assert left_out on the references they compute.)"""
    cases = CC.FWD_GRID['f16x2'] + CC.FWD_GRID['bf16'] + CC.FWD_CASES + CC.STREAM_CASES + CC.DGRAD_CASES + CC.WGRAD_CASES
    for c in cases:
        K = c['k'] * c['k'] * max(c['Cin'], c['Cout'])
        assert 2 * CC.ACC_CONST * CC.U * 2.0 ** -22 / np.sqrt(K) > 2.0 ** 60 * CC.TINY, CC.case_id(c)
    for spread in (0, 2, 10):
        assert np.abs(CC.make_values(50, 9, 1, spread)).min() >= 2.0 ** -11
    assert np.abs(CC.make_filter(9, 3, 7, 1)).min() >= 2.0 ** -11 / np.sqrt(63)
    assert CC.LEFT_OUT_CAP == 0.01


def test_split_cases_are_well_formed():
    for M, C, ldx, ldp, off, cv in CC.SPLIT_CASES:
        assert C % 64 == 0 and ldx >= C and ldx % 4 == 0 and 0 < cv <= C
        assert ldp == 0 or (ldp % 32 == 0 and off % 64 == 0 and off + C <= ldp)
    assert any(cv < C for _, C, _, _, _, cv in CC.SPLIT_CASES) and any(ldp > C for _, C, _, ldp, _, _ in CC.SPLIT_CASES)
