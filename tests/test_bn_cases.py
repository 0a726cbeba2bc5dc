# -*- coding: utf-8 -*-
"""tests/bn_cases.py checked without a GPU: every case reaches the branch of csrc/pointwise.hip it is listed for (through
the mirror of the host dispatch), the fp64 references agree with torch's BatchNorm2d and activations in double and their
autograd, the numpy operand formats have the precision they claim, and every acceptance function accepts the rounded
reference and rejects a dropped row and an element moved by 8 of its own bounds."""
import functools

import numpy as np
import pytest
import torch

import bn_cases as BC

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------ branch coverage
@pytest.mark.parametrize('C', BC.CHANNELS)
def test_row_map_table(C):
    c4, tpr, rpb, _ = BC.CHANNEL_TABLE[C]
    assert C // 4 == c4 and BC.row_map(C) == (tpr, rpb) and tpr * rpb == 256
    T = 4 * rpb
    assert BC.m_list(C) == (1, T - 1, T, T + 1, 2 * T + rpb + 1)
    # every M runs nrows = 4, one block per 4 rpb rows; the last trip is ragged for all but M = T
    for M in BC.m_list(C):
        assert BC.stat_rows(M, rpb) == 4 and BC.bn_blocks(M, C) == -(-M // T) == BC.apply_grid(M, C)
        assert BC.apply_laps(M, C) == 1
    assert [M % T for M in BC.m_list(C)] == [1 % T, T - 1, 0, 1, rpb + 1]
    assert BC.bn_loads_nt(C) == (C >= 64)


def test_channel_passes():
    want = {4: (1, 1), 8: (1, 2), 12: (2, 1), 32: (1, 8), 36: (2, 1), 64: (1, 16), 96: (2, 8), 160: (2, 8),
            1024: (1, 256), 1028: (2, 1), 2048: (2, 256)}
    assert {C: BC.channel_passes(C) for C in BC.CHANNELS} == want
    # C % 32 != 0: the last block of the finalize kernels has idle columns
    assert 36 % 32 and 1028 % 32 and 12 % 32
    # the plane forms need whole 32-channel tiles; 96 and 160 run them through a half / quarter full second pass
    assert all(C % 32 == 0 and C in BC.CHANNELS for C in BC.PLANE_CHANNELS)
    assert not BC.bn_loads_nt(32) and BC.bn_loads_nt(96)


def test_large_cases():
    (C1, M1), (C2, M2) = BC.LARGE
    assert (C1, M1) == (1024, 20483) and BC.row_map(C1) == (256, 1)
    assert BC.stat_rows(M1, 1) == 5                          # one four-row trip + one single row in the backward reduce
    assert (M1 % 5) and M1 % 4                               # the tensor ends inside a block and inside a trip
    assert -(-M1 // 4) > BC.GRID_CAP and BC.apply_grid(M1, C1) == BC.GRID_CAP and BC.apply_laps(M1, C1) == 2
    assert (C2, M2) == (256, 65540) and BC.row_map(C2) == (64, 4)
    assert -(-M2 // 16) == BC.GRID_CAP + 1 and BC.apply_grid(M2, C2) == BC.GRID_CAP and BC.apply_laps(M2, C2) == 2
    assert BC.stat_rows(M2, 4) == 4
    # C = 4 cannot reach the unrolled fold through the statistics of a tensor of practical size: nrows grows with M, so
    # M = 1024 * 16384 + 5 rows make 4097 partial rows (per = 17 < 64); the branch is reached through the partial-row
    # entry point instead (test_fold_plans)
    assert BC.bn_blocks(1024 * 16384 + 5, 4) == 4097 and not BC.fold_unrolled(4097, 4)


def test_workspace_sizes():
    for C in BC.CHANNELS:
        assert BC.bn_finalize_workspace(C) == 257 * 2 * C * 8
        for M in BC.m_list(C):
            assert BC.bn_workspace(M, C) == 257 * 2 * C * 8 + BC.bn_blocks(M, C) * 2 * C * 4
    assert BC.bn_workspace(0, 4) == 0 and BC.bn_finalize_workspace(0) == 0


def test_fold_plans():
    nb = {n: BC.fold_plan(n, 4)[0] for n in BC.FOLD_NPARTS}
    assert nb == {1: 1, 15: 1, 16: 1, 17: 2, 912: 57, 1024: 64, 1040: 65, 4096: 256, 4097: 241, 70001: 256}
    assert set(BC.FOLD_NB) <= set(nb.values())
    # both sides of the `r + 56 < nb` loop of fold_rows32: not entered, entered by group 0 only, by all groups without
    # a tail, by all groups with a tail row for group 0, four rounds
    assert BC.rows32_unrolled(1) == ([], [0]) and BC.rows32_unrolled(2) == ([], [0, 1])
    assert BC.rows32_unrolled(57) == ([0], list(range(1, 8)))
    assert BC.rows32_unrolled(64) == (list(range(8)), [])
    assert BC.rows32_unrolled(65) == (list(range(8)), [0])
    assert BC.rows32_unrolled(256) == (list(range(8)), [])
    # column widths and row groups; per grows above 16 only past 256 blocks
    assert [BC.fold_plan(16, C)[2:] for C in BC.FOLD_CHANNELS] == [(32, 8), (128, 2), (256, 1), (256, 1)]
    assert BC.fold_plan(4096, 4)[1] == 16 and BC.fold_plan(4097, 4)[1] == 17 and BC.fold_plan(70001, 4)[1] == 274
    # the 8-way unrolled loop of fold_partials_kernel: at cw = 32 only from per >= 57 on
    assert not BC.fold_unrolled(4097, 4) and BC.fold_unrolled(70001, 4)
    assert not BC.fold_unrolled(1, 36) and BC.fold_unrolled(15, 36)
    assert not BC.fold_unrolled(1, 128) and BC.fold_unrolled(15, 128) and BC.fold_unrolled(17, 1028)
    # the statistics of the large cases reach the unrolled loop too (cw = 256)
    for C, M in BC.LARGE:
        assert BC.fold_unrolled(BC.bn_blocks(M, C), C)


def test_bias_grad_chain():
    assert [BC.colsum_rows(M) for M in BC.BIAS_ROWS] == [1, 1023, 1024, 1024, 1024]
    assert [-(-M // BC.colsum_rows(M)) for M in BC.BIAS_ROWS] == [1, 1, 1, 2, 5]


# ------------------------------------------------------------------------------------------ references vs torch
def _rel_ok(a, b, scale, tol=1e-12):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= tol * np.maximum(np.abs(scale), 1e-300))


def _torch_act(act):
    return {BC.ACT_LINEAR: torch.nn.Identity(), BC.ACT_LEAKY: torch.nn.LeakyReLU(0.1), BC.ACT_MISH: torch.nn.Mish(),
            BC.ACT_RELU: torch.nn.ReLU()}[act]


@pytest.mark.parametrize('act', BC.ACTS, ids=BC.ACT_NAMES.get)
@pytest.mark.parametrize('M,C', [(5, 4), (37, 12), (130, 36)])
def test_references_against_torch(M, C, act):
    """batch and frozen statistics: forward, running statistics, dgamma, dbeta, dy to 1e-12, relative to the element (to
    the sum of the absolute addends where the expression cancels: the variance, dy, the sums)"""
    case = BC.make_case(M, C, ratios=(0.0, 10.0))
    st = case['stats']
    y, dz, res = (case[k].astype(F64) for k in ('y', 'dz', 'res'))
    rm0, rv0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
    for frozen in (False, True):
        bn = torch.nn.BatchNorm2d(C, eps=float(F32(BC.EPS)), momentum=float(F32(BC.MOMENTUM))).double()
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(case['gamma'].astype(F64)))
            bn.bias.copy_(torch.from_numpy(case['beta'].astype(F64)))
            bn.running_mean.copy_(torch.from_numpy(rm0))
            bn.running_var.copy_(torch.from_numpy(rv0))
        bn.train(not frozen)
        mean, var = (rm0, rv0) if frozen else (st['mean'], st['var'])
        invstd = 1.0 / np.sqrt(var + st['eps'])
        x = torch.from_numpy(y.T.reshape(1, C, M, 1).copy()).requires_grad_(True)
        r_t = torch.from_numpy(res.T.reshape(1, C, M, 1).copy())
        z = _torch_act(act)(bn(x)) + r_t
        z.backward(torch.from_numpy(dz.T.reshape(1, C, M, 1).copy()))
        f = BC.apply_ref64(y, mean, invstd, case['gamma'], case['beta'], act, res)
        assert _rel_ok(f['z'], z.detach().numpy()[0, :, :, 0].T, f['S'])
        b = BC.bwd_ref64(dz, y, mean, invstd, case['gamma'], case['beta'], act, frozen)
        assert _rel_ok(b['dbeta'], bn.bias.grad.numpy(), np.abs(b['g']).sum(0))
        assert _rel_ok(b['dgamma'], bn.weight.grad.numpy(), np.abs(b['g'] * b['xh']).sum(0))
        assert _rel_ok(b['dy'], x.grad.numpy()[0, :, :, 0].T, b['S'])
        if not frozen:
            nm, _, nv, _ = BC.running_ref64(st, rm0, rv0)
            assert _rel_ok(nm, bn.running_mean.numpy(), np.abs(rm0) + np.abs(st['mean']))
            assert _rel_ok(nv, bn.running_var.numpy(), nv)
            t = torch.from_numpy(y)
            assert _rel_ok(st['mean'], t.mean(0).numpy(), np.abs(y).mean(0))
            assert _rel_ok(st['var'], t.var(0, unbiased=False).numpy(), (y * y).mean(0))
            assert _rel_ok(st['unbiased'], t.var(0, unbiased=True).numpy(), (y * y).mean(0))


def test_activations_against_torch():
    v = np.concatenate([np.linspace(-60, 60, 4801), [-1e3, -100.0, -20.0, 20.0, 100.0, 1e3, 0.0, -1.1924]])
    for act in BC.ACTS:
        t = torch.from_numpy(v.copy()).requires_grad_(True)
        out = _torch_act(act)(t)
        out.sum().backward()
        assert _rel_ok(BC.act64(v, act), out.detach().numpy(), np.abs(v) + 1e-300), act
        d = BC.act_grad64(v, act)
        scale = BC.mish_grad64(v, parts=True)[1] if act == BC.ACT_MISH else np.ones_like(v)
        assert _rel_ok(d, t.grad.numpy(), scale), act


def test_stats_m1_rule():
    """M = 1: variance 0, invstd = eps^-1/2, and the running variance takes the biased value (no M / (M - 1))"""
    case = BC.make_case(1, 12)
    st = case['stats']
    assert (st['var'] == 0).all() and (st['unbiased'] == 0).all()
    assert np.allclose(st['invstd'], 1.0 / np.sqrt(F64(F32(BC.EPS))), rtol=1e-15)
    _, _, nv, _ = BC.running_ref64(st, np.zeros(12), np.ones(12))
    assert np.allclose(nv, 1.0 - F64(F32(BC.MOMENTUM)), rtol=1e-15)


def test_partials_reference():
    for nparts in (1, 17, 5000):
        part, M = BC.make_partials(nparts, 36, 3)
        assert part.shape == (nparts, 2, 36) and part.dtype == F32 and M == nparts * 64
        r = BC.partials_ref64(part, M)
        assert np.all(np.abs(np.abs(r['mean']) - 300.0) < 2.0) and np.all((r['var'] > 0.2) & (r['var'] < 3.0))
        # the bound sees a sum kept in fp32: one fp32 rounding of sum y^2 / M is far outside it
        assert np.all(2.0 ** -24 * 9e4 > 1e3 * r['dvar'])


# ------------------------------------------------------------------------------------------ formats
def test_split_reconstructs():
    rng = np.random.RandomState(5)
    z = (rng.standard_normal(200000) * np.exp(rng.uniform(-12, 3, 200000))).astype(F32)
    for word in (BC.amax_word(z), BC.amax_word(z * F32(300.0)), 0x7f800000, 0):
        hi, lo = BC.split_f16x2(z, word)
        assert np.isfinite(hi.astype(F32)).all() and np.isfinite(lo.astype(F32)).all()
        t = z.astype(F64) * F64(BC.scale_of(word))
        assert np.all(np.abs(hi.astype(F64) + lo.astype(F64) / 2048.0 - t) <= BC.split_error(np.abs(t)))
        assert np.all(np.abs(BC.planes_decode(hi, lo, word) - z) <= BC.split_error(np.abs(t)) / F64(BC.scale_of(word)))
    # the scale puts the maximum just under the fp16 range: |t| < 2^15 for |z| <= the word
    w = BC.amax_word(z)
    assert 2.0 ** 13 <= float(np.abs(z).max()) * float(BC.scale_of(w)) < 2.0 ** 15


def test_scale_exp_rules():
    assert BC.scale_exp(0) == 127 and BC.scale_exp(0x7f800000) == 127 and BC.scale_exp(0x7fc00000) == 127
    assert BC.scale_exp(0x3f800000) == 268 - 127 and BC.scale_exp(1 << 23) == 252 and BC.scale_exp(10 << 23) == 252
    assert BC.scale_exp(254 << 23) == 14 and BC.scale_exp(16 << 23) == 252 and BC.scale_exp(17 << 23) == 251


def test_plane_layout_and_bf16():
    hi = (np.arange(3 * 64).reshape(3, 64) % 100).astype(np.float16)
    lo = -hi
    w = BC.planes_pack(hi, lo)
    assert w.shape == (3, 128)
    for c in (0, 1, 31, 32, 63):                  # bytes of a pixel row: tile c / 32 at 128 B, hi at 2 (c % 32), lo 64 B on
        assert w[1, (c // 32) * 64 + c % 32] == hi.view(np.uint16)[1, c] and w[1, (c // 32) * 64 + 32 + c % 32] == lo.view(np.uint16)[1, c]
    h2, l2 = BC.planes_unpack(w)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
    # bf16: ties to even, against torch
    z = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 65504.0, 1e-40, 1.0039062], dtype=F32)
    want = torch.from_numpy(z).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(BC.bf16_rne(z), want)
    rng = np.random.RandomState(2)
    z = rng.standard_normal(100000).astype(F32)
    assert np.array_equal(BC.bf16_rne(z), torch.from_numpy(z).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.all(np.abs(BC.bf16_to_f32(BC.bf16_rne(z)).astype(F64) - z) <= BC.bf16_error(np.abs(z.astype(F64))))
    assert np.any(np.abs(BC.bf16_to_f32(BC.bf16_rne(z)).astype(F64) - z) > 0.45 * BC.bf16_error(np.abs(z.astype(F64))))
    rows = BC.bf16_rows(BC.bf16_to_f32(BC.bf16_rne(z[:24])).reshape(2, 12), 16)
    assert BC.is_sentinel(rows[:, 6:]).all() and np.array_equal(rows.view(np.uint16).reshape(2, 32)[:, :12].ravel(), BC.bf16_rne(z[:24]))


@functools.lru_cache(maxsize=None)
def _case(M, C):
    return BC.make_case(M, C)


GRID = [(M, C) for C in BC.CHANNELS for M in BC.m_list(C)]


@pytest.mark.parametrize('C', BC.CHANNELS)
def test_analytic_bound_dominates(C):
    """the plane bound is at least max|z| of every built case, every activation, with and without the residual"""
    for M in BC.m_list(C):
        case = _case(M, C)
        rw = BC.amax_word(case['res'])
        for act in BC.ACTS:
            for res in (None, case['res']):
                z = BC.apply_ref64(case['y'], case['mean'], case['invstd'], case['gamma'], case['beta'], act, res)['z']
                w = BC.planes_bound_f32(case['gamma'], case['beta'], M, rw if res is not None else None)
                assert BC.word_value(w) >= np.abs(z).max() * (1 + 2.0 ** -22), (M, act)
    assert BC.planes_bound_f32([1.0], [0.0], 5, None, 0x7f800000) == 0x7f800000
    assert BC.planes_bound_f32([np.inf], [0.0], 5, None, 0x3f800000) == 0x7f800000


# ------------------------------------------------------------------------------------------ self-acceptance
def _moved(ref, bound, idx, k=8.0):
    out = np.array(ref, dtype=F64)
    out[idx] += k * max(float(np.broadcast_to(bound, out.shape)[idx]), BC.TINY)
    return out


@pytest.mark.parametrize('C', BC.CHANNELS)
def test_self_acceptance_statistics(C):
    for M in BC.m_list(C):
        case = _case(M, C)
        st = case['stats']
        ok, used = BC.mean_accept(st['mean'].astype(F32), st)
        assert ok.all() and used.max() <= 1.0
        assert BC.invstd_accept(st['invstd'].astype(F32), st)[0].all()
        assert BC.left_out(st['mean'], st['dmean'] + BC.U * np.abs(st['mean'])) <= 0.01
        c = 0                                                   # a |mean| / std = 0 channel
        assert not BC.mean_accept(_moved(st['mean'], st['dmean'] + BC.U * np.abs(st['mean']), c), st)[0][c]
        if M > 4:                                               # one row dropped from the sums
            y = case['y'].astype(F64)[:-1]
            m2 = y.sum(0) / M
            v2 = (y * y).sum(0) / M - m2 * m2
            assert not BC.mean_accept(m2, st)[0].all()
            assert not BC.invstd_accept(1.0 / np.sqrt(np.maximum(v2, 0) + st['eps']), st)[0].all()
        rm0, rv0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
        nm, bm, nv, bv = BC.running_ref64(st, rm0, rv0)
        assert BC.judge(nm.astype(F32), nm, bm)[0].all() and BC.judge(nv.astype(F32), nv, bv)[0].all()
        assert not BC.judge(_moved(nm, bm, c), nm, bm)[0][c] and not BC.judge(_moved(nv, bv, c), nv, bv)[0][c]


@pytest.mark.parametrize('act', BC.ACTS, ids=BC.ACT_NAMES.get)
@pytest.mark.parametrize('C', BC.CHANNELS)
def test_self_acceptance_apply_and_backward(C, act):
    for M in BC.m_list(C):
        case = _case(M, C)
        a = (case['y'], case['mean'], case['invstd'], case['gamma'], case['beta'], act)
        for res in (None, case['res']):
            r = BC.apply_ref64(*a, res)
            ok, used = BC.apply_accept(r['z'].astype(F32), r, act)
            assert ok.all() and used.max() <= 1.0
            bound = BC.apply_bound(r, act)
            assert BC.left_out(r['z'], bound) <= 0.01
            idx = (M // 2, C // 2)
            assert not BC.apply_accept(_moved(r['z'], bound, idx), r, act)[0][idx]
        for frozen in (False, True):
            b = BC.bwd_ref64(case['dz'], *a, frozen)
            for key, bk in (('dy', 'b_dy'), ('dbeta', 'b_dbeta'), ('dgamma', 'b_dgamma')):
                ok, used = BC.judge(b[key].astype(F32), b[key], b[bk])
                assert ok.all() and used.max() <= 1.0, (M, key)
                assert BC.left_out(b[key], b[bk]) <= 0.01
                idx = (M // 2, C // 2) if key == 'dy' else (C // 2,)
                assert not BC.judge(_moved(b[key], b[bk], idx), b[key], b[bk])[0][idx]
            if M > 4 and not frozen:                            # one row dropped from the sums
                g = b['g'][:-1]
                assert not BC.judge(g.sum(0), b['dbeta'], b['b_dbeta'])[0].all()
                assert not BC.judge((g * b['xh'][:-1]).sum(0), b['dgamma'], b['b_dgamma'])[0].all()


@pytest.mark.parametrize('C,M', BC.LARGE)
def test_self_acceptance_large(C, M):
    """the large cases, with the activation the GPU tests run them at"""
    case = BC.make_case(M, C)
    st = case['stats']
    assert BC.mean_accept(st['mean'].astype(F32), st)[0].all() and BC.invstd_accept(st['invstd'].astype(F32), st)[0].all()
    a = (case['y'], case['mean'], case['invstd'], case['gamma'], case['beta'], BC.ACT_MISH)
    r = BC.apply_ref64(*a, case['res'])
    bound = BC.apply_bound(r, BC.ACT_MISH)
    assert BC.apply_accept(r['z'].astype(F32), r, BC.ACT_MISH)[0].all() and BC.left_out(r['z'], bound) <= 0.01
    w = BC.planes_bound_f32(case['gamma'], case['beta'], M, BC.amax_word(case['res']))
    assert BC.word_value(w) >= np.abs(r['z']).max()
    del r, bound
    b = BC.bwd_ref64(case['dz'], *a)
    for key, bk in (('dy', 'b_dy'), ('dbeta', 'b_dbeta'), ('dgamma', 'b_dgamma')):
        assert BC.judge(b[key].astype(F32), b[key], b[bk])[0].all() and BC.left_out(b[key], b[bk]) <= 0.01
    g = b['g'][:-1]
    assert not BC.judge(g.sum(0), b['dbeta'], b['b_dbeta'])[0].all()


def test_self_acceptance_sums_and_fold():
    rng = np.random.RandomState(9)
    for C in BC.BIAS_CHANNELS:
        for M in BC.BIAS_ROWS:
            x = rng.standard_normal((M, C)).astype(F32)
            s, b = BC.bias_grad_ref64(x)
            assert BC.judge(s.astype(F32), s, b)[0].all() and BC.left_out(s, b) <= 0.01
            assert not BC.judge(_moved(s, b, (0,)), s, b)[0][0]
            if M > 1:
                assert not BC.judge(x[:-1].sum(0, dtype=F64), s, b)[0].all()
    for C in BC.FOLD_EVAL_CHANNELS:
        g, be = BC.make_params(C, 4)
        rm, rv = rng.standard_normal(C).astype(F32), rng.uniform(0.0, 2.0, C).astype(F32)
        s, bs, sh, bsh = BC.fold_ref64(g, be, rm, rv)
        assert BC.judge(s.astype(F32), s, bs)[0].all() and BC.judge(sh.astype(F32), sh, bsh)[0].all()
        assert not BC.judge(_moved(s, bs, (0,)), s, bs)[0][0] and not BC.judge(_moved(sh, bsh, (0,)), sh, bsh)[0][0]
    for nparts in (1, 17, 1040):
        part, M = BC.make_partials(nparts, 36, nparts)
        r = BC.partials_ref64(part, M)
        assert BC.mean_accept(r['mean'].astype(F32), r)[0].all() and BC.invstd_accept(r['invstd'].astype(F32), r)[0].all()
        assert BC.left_out(r['mean'], r['dmean'] + BC.U * np.abs(r['mean'])) <= 0.01
        if nparts > 1:                                         # a partial row dropped; the sums held in fp32
            r2 = BC.partials_ref64(part[:-1], M)
            assert not BC.mean_accept(r2['mean'], r)[0].any() and not BC.invstd_accept(r2['invstd'], r)[0].any()
            s32, ss32 = part[:, 0].sum(0, dtype=F32).astype(F64), np.add.accumulate(part[:, 1], axis=0, dtype=F32)[-1].astype(F64)
            v32 = np.maximum(ss32 / M - (s32 / M) ** 2, 0)
            assert not BC.invstd_accept(1.0 / np.sqrt(v32 + r['eps']), r)[0].all()


# ------------------------------------------------------------------------------------------ non-finite builders
def test_nonfinite_builder():
    for M, C in ((1, 4), (5, 12), (131, 36), (10, 2048)):
        y = BC.make_case(M, C)['y']
        y2, sites = BC.plant_nonfinite(y)
        assert len(sites) == 3 and len({(m, c) for m, c, _ in sites}) == 3
        bad = ~np.isfinite(y2)
        assert bad.sum() == 3 and np.isfinite(y).all()
        for m, c, name in sites:
            assert (name == 'nan' and np.isnan(y2[m, c])) or (name == '+inf' and y2[m, c] == np.inf) or (name == '-inf' and y2[m, c] == -np.inf)
        assert np.array_equal(y2[~bad], y[~bad])


def test_sentinel_helpers():
    a = BC.pad_rows(np.ones((3, 4), F32), 12)
    assert np.isnan(a[:, 4:]).all() and BC.is_sentinel(a[:, 4:]).all() and not BC.is_sentinel(a[:, :4]).any()
    cc = BC.const_channels(36)
    y = BC.make_case(40, 36)['y']
    assert cc == [3, 10, 17, 24, 31] and all((y[:, c] == y[0, c]).all() for c in cc) and (y[:, 0] != y[0, 0]).any()
