# -*- coding: utf-8 -*-
"""CPU side of the classifier tests: every case of tests/classifier_cases.py reaches the launcher branch it is named for,
torch's own fp32 arithmetic passes every acceptance rule (so the rules ask nothing an fp32 implementation cannot give),
the seven entry points report NULL / shape errors from the host, tests/golden/classifier.npz (written from the
reference's CSPDarknet53) pins the composed oracle bit for bit, and a classifier checkpoint feeds the detector."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_cases as CC
import recipe
import yolov4_amd
from yolov4_amd.darknet.darknet import Backbone, CSPDarknet53
from yolov4_amd.darknet.loss import CrossEntropyLoss, accuracy
from yolov4_amd.darknet.train import adjust_learning_rate
from yolov4_amd.yolo.model.yolov4 import YOLOv4

FAKE = 0x1000            # never dereferenced on the host


# ------------------------------------------------------------------ branches
@pytest.mark.parametrize('case', CC.POOL_CASES, ids=str)
def test_pool_case_reaches_its_branch(case):
    B, HW, C, ld = case
    path = CC.pool_path(C, ld, ld)
    assert path == CC.POOL_BRANCH[case]
    gx, gy = CC.pool_fwd_grid(B, C, path)
    assert gy == B and gx * 64 * (4 if path == 'vec4' else 1) >= C
    assert 1 <= CC.pool_bwd_blocks(B, HW, C, path) <= 8192


def test_pool_cases_cover_the_launcher():
    paths = {CC.POOL_BRANCH[c] for c in CC.POOL_CASES}
    assert paths == {'vec4', 'scalar'}
    assert any(ld > C for _, _, C, ld in CC.POOL_CASES)                               # a pitch wider than the row
    assert any(CC.pool_fwd_grid(B, C, CC.POOL_BRANCH[(B, HW, C, ld)])[0] > 1 for B, HW, C, ld in CC.POOL_CASES)   # > 1 channel block
    assert any(HW % 4 for _, HW, _, _ in CC.POOL_CASES) and any(HW < 4 for _, HW, _, _ in CC.POOL_CASES)         # uneven pixel groups
    assert CC.pool_path(40, 48, 48, aligned=False) == 'scalar' and CC.pool_path(40, 42, 48) == 'scalar'


@pytest.mark.parametrize('case', CC.LINEAR_CASES, ids=str)
def test_linear_case_reaches_its_branch(case):
    M, K, N, ldx, ldy = case
    assert CC.linear_grids(M, K, N) == CC.LINEAR_BRANCH[case]


def test_linear_cases_cover_the_tile_edges():
    g = CC.LINEAR_BRANCH[(130, 96, 257, 96, 257)]
    for name in ('fwd', 'dx', 'dw'):
        assert all(v > 1 for v in g[name])                                            # several tiles in all three dimensions
    assert 130 % 64 and 257 % 64 and 257 % 32 and 130 % 32                            # with ragged last tiles
    assert any(ldx > K and ldy > N for _, K, N, ldx, ldy in CC.LINEAR_CASES)


def test_row_kernels_sweep_counts():
    assert [CC.row_sweeps(n) for n in CC.CE_NS] == [1, 1, 1, 4, 4]
    assert [CC.row_sweeps(n) for n in CC.TOPK_NS] == [1, 1, 1, 4]
    assert 1000 % 256 and 1003 % 256 and 1003 % 4                                     # a ragged last step, an unaligned row


# ------------------------------------------------------------------ torch's fp32 passes the rules
@pytest.mark.parametrize('case', CC.POOL_CASES, ids=str)
def test_torch_fp32_passes_pool_rules(case):
    B, HW, C, ld = case
    c = CC.pool_case(case)
    x = torch.from_numpy(c['x'][..., :C].copy())
    ok, frac = CC.pool_fwd_accept(x.mean(1).numpy(), c['y64'], c['absmean'], HW)
    assert ok.all() and frac <= 1.0
    dx = (torch.from_numpy(c['dy'][:, None, :C].copy()) / HW).expand(B, HW, C).numpy()
    ok, _ = CC.pool_bwd_accept(dx, c['dx64'])
    assert ok.all()
    assert CC.is_sentinel(c['x'][..., C:]).all() and not np.isnan(c['x'][..., :C]).any()


@pytest.mark.parametrize('case', CC.LINEAR_CASES, ids=str)
def test_torch_fp32_passes_linear_rules(case):
    M, K, N, ldx, ldy = case
    c = CC.linear_case(case)
    x = torch.from_numpy(c['x'][:, :K].copy()).requires_grad_(True)
    w = torch.from_numpy(c['w'].copy()).requires_grad_(True)
    b = torch.from_numpy(c['bias'].copy()).requires_grad_(True)
    y = F.linear(x, w, b)
    y.backward(torch.from_numpy(c['dy'][:, :N].copy()))
    for got, ref, ab, L in ((y.detach(), c['y64'], c['y_abs'], K), (x.grad, c['dx64'], c['dx_abs'], N),
                            (w.grad, c['dw64'], c['dw_abs'], M), (b.grad, c['db64'], c['db_abs'], M)):
        ok, frac = CC.linear_accept(got.numpy(), ref, ab, L)
        assert ok.all() and frac <= 0.5


@pytest.mark.parametrize('N', CC.CE_NS)
def test_torch_fp32_passes_ce_rules(N):
    c = CC.ce_case(N)
    z = torch.from_numpy(c['z'].copy()).requires_grad_(True)
    t = torch.from_numpy(c['t'].copy())
    rows = F.cross_entropy(z, t, label_smoothing=CC.SMOOTHING, reduction='none')
    mean = F.cross_entropy(z, t, label_smoothing=CC.SMOOTHING)
    (mean * CC.CE_GSCALE).backward()
    ok, frac = CC.ce_row_accept(rows.detach().numpy(), c)
    assert ok.all() and frac <= 0.25
    ok, frac = CC.ce_mean_accept(float(mean.detach()), c)
    assert ok and frac <= 0.25
    ok, frac = CC.ce_grad_accept(z.grad.numpy(), c)
    assert ok.all() and frac <= 1.0
    assert c['counted'] == 5 and c['row64'][3] == 0.0 and (c['grad64'][3] == 0.0).all()
    assert c['z'][0].max() == 80.0 and c['z'][1].min() == -90.0 and np.abs(c['z'][2] - 30.0).max() <= 1.01e-3


def test_all_ignored_batch_reference():
    c = CC.ce_case(37, all_ignored=True)
    assert c['counted'] == 0 and np.isnan(c['mean64']) and (c['grad64'] == 0.0).all() and (c['row64'] == 0.0).all()
    z, t = torch.from_numpy(c['z'].copy()), torch.from_numpy(c['t'].copy())
    assert torch.isnan(F.cross_entropy(z, t, label_smoothing=CC.SMOOTHING))           # torch's mean over nothing
    assert CC.ce_mean_accept(float('nan'), c)[0] and not CC.ce_mean_accept(0.0, c)[0]


@pytest.mark.parametrize('N', CC.TOPK_NS)
def test_rank_rule_and_planted_rows(N):
    c = CC.topk_case(N)
    z, t, rank = c['z'], c['t'], c['rank']
    assert rank[2] == N and rank[3] == N                                              # the NaN row, the -100 row
    if N >= 5:
        assert rank[0] == 1 and rank[1] == 0                                          # tie below the label counts, above does not
    if N >= 37:
        assert rank[4] == 2 and rank[5] == 6
    # on the rows without ties, NaN or ignored labels torch.topk agrees with the rule
    plain = [b for b in range(CC.TOPK_B) if b not in (0, 1, 2, 3)]
    zt, tt = torch.from_numpy(z[plain].copy()), torch.from_numpy(t[plain].copy())
    for k in (1, 5):
        kk = min(k, N)
        hit = (zt.topk(kk, 1).indices == tt[:, None]).any(1).numpy()
        assert np.array_equal(hit, rank[plain] < k)
    assert np.array_equal(CC.correct_rule(rank, (1, 5)), [int((rank < 1).sum()), int((rank < 5).sum())])


# ------------------------------------------------------------------ host-side errors of the seven entry points
def test_null_and_shape_errors_come_from_the_host():
    L = yolov4_amd.lib()
    OK_, SHAPE, NULL = 0, 1, 2
    assert L.y4_avgpool_global_fwd_f32(None, 8, FAKE, 8, 1, 4, 8, None) == NULL
    assert L.y4_avgpool_global_fwd_f32(FAKE, 8, None, 8, 1, 4, 8, None) == NULL
    assert L.y4_avgpool_global_fwd_f32(FAKE, 7, FAKE, 8, 1, 4, 8, None) == SHAPE          # pitch < C
    assert L.y4_avgpool_global_fwd_f32(FAKE, 8, FAKE, 8, 1, 0, 8, None) == SHAPE
    assert L.y4_avgpool_global_bwd_f32(None, 8, FAKE, 8, 1, 4, 8, None) == NULL
    assert L.y4_avgpool_global_bwd_f32(FAKE, 8, FAKE, 7, 1, 4, 8, None) == SHAPE
    assert L.y4_avgpool_global_bwd_f32(FAKE, 8, FAKE, 8, 0, 4, 8, None) == SHAPE
    assert L.y4_linear_fwd_f32(FAKE, 8, None, None, FAKE, 4, 2, 8, 4, None) == NULL
    assert L.y4_linear_fwd_f32(FAKE, 7, FAKE, None, FAKE, 4, 2, 8, 4, None) == SHAPE      # ldx < K
    assert L.y4_linear_fwd_f32(FAKE, 8, FAKE, None, FAKE, 3, 2, 8, 4, None) == SHAPE      # ldy < N
    assert L.y4_linear_fwd_f32(FAKE, 8, FAKE, None, FAKE, 4, 2, 0, 4, None) == SHAPE
    assert L.y4_linear_bwd_f32(FAKE, 8, FAKE, FAKE, 4, None, 8, None, None, 2, 8, 4, None) == NULL   # nothing asked for
    assert L.y4_linear_bwd_f32(FAKE, 8, FAKE, None, 4, FAKE, 8, FAKE, FAKE, 2, 8, 4, None) == NULL   # no dy
    assert L.y4_linear_bwd_f32(FAKE, 8, None, FAKE, 4, FAKE, 8, None, None, 2, 8, 4, None) == NULL   # dx needs w
    assert L.y4_linear_bwd_f32(None, 8, FAKE, FAKE, 4, None, 8, FAKE, None, 2, 8, 4, None) == NULL   # dw needs x
    assert L.y4_linear_bwd_f32(FAKE, 8, FAKE, FAKE, 3, FAKE, 8, None, None, 2, 8, 4, None) == SHAPE  # lddy < N
    assert L.y4_linear_bwd_f32(FAKE, 8, FAKE, FAKE, 4, FAKE, 7, None, None, 2, 8, 4, None) == SHAPE  # lddx < K
    assert L.y4_ce_smooth_fwd_f32(FAKE, 4, None, 2, 4, 0.1, FAKE, FAKE, None) == NULL
    assert L.y4_ce_smooth_fwd_f32(FAKE, 4, FAKE, 2, 4, 0.1, FAKE, None, None) == NULL
    assert L.y4_ce_smooth_fwd_f32(FAKE, 3, FAKE, 2, 4, 0.1, FAKE, FAKE, None) == SHAPE
    assert L.y4_ce_smooth_fwd_f32(FAKE, 4, FAKE, 2, 4, 1.5, FAKE, FAKE, None) == SHAPE
    assert L.y4_ce_smooth_fwd_f32(FAKE, 4, FAKE, 2, 4, float('nan'), FAKE, FAKE, None) == SHAPE
    assert L.y4_ce_smooth_bwd_f32(FAKE, 4, FAKE, FAKE, None, FAKE, 4, 2, 4, 0.1, None) == NULL
    assert L.y4_ce_smooth_bwd_f32(FAKE, 4, FAKE, None, FAKE, FAKE, 4, 2, 4, 0.1, None) == NULL
    assert L.y4_ce_smooth_bwd_f32(FAKE, 4, FAKE, FAKE, FAKE, FAKE, 3, 2, 4, 0.1, None) == SHAPE
    assert L.y4_ce_smooth_bwd_f32(FAKE, 4, FAKE, FAKE, FAKE, FAKE, 4, 0, 4, 0.1, None) == SHAPE
    ks = yolov4_amd._lib.int_array([1, 5])
    assert L.y4_topk_correct_f32(FAKE, 4, FAKE, 2, 4, ks, 2, None, None, None) == NULL
    assert L.y4_topk_correct_f32(FAKE, 4, FAKE, 2, 4, None, 2, FAKE, None, None) == NULL
    assert L.y4_topk_correct_f32(FAKE, 4, FAKE, 2, 4, ks, 9, FAKE, None, None) == SHAPE
    assert L.y4_topk_correct_f32(FAKE, 4, FAKE, 2, 4, ks, 0, FAKE, None, None) == SHAPE
    assert L.y4_topk_correct_f32(FAKE, 3, FAKE, 2, 4, ks, 2, FAKE, None, None) == SHAPE
    assert OK_ == 0


# ------------------------------------------------------------------ Python layer, without a GPU
def test_module_tree_and_no_cpu_fallback():
    m = CSPDarknet53(CC.MODEL_CLASSES)
    assert isinstance(m.backbone, Backbone) and isinstance(m.pool, torch.nn.AdaptiveAvgPool2d) and isinstance(m.classifier, torch.nn.Linear)
    assert [n for n, _ in m.backbone.named_children()] == ['stem', 'stage1', 'stage2', 'stage3', 'stage4', 'stage5']
    assert tuple(CSPDarknet53().classifier.weight.shape) == (1000, 1024)
    with pytest.raises(yolov4_amd.Y4Error):
        m.pool(torch.zeros(1, 8, 2, 2))
    with pytest.raises(yolov4_amd.Y4Error):
        m.classifier(torch.zeros(1, 1024))
    crit = CrossEntropyLoss(label_smoothing=0.1)
    with pytest.raises(yolov4_amd.Y4Error):
        crit(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(yolov4_amd.Y4Error):
        accuracy(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), topk=(1, 5))
    for bad in (dict(weight=torch.ones(5)), dict(reduction='sum'), dict(reduction='none'), dict(ignore_index=0)):
        with pytest.raises(yolov4_amd.Y4Error):
            CrossEntropyLoss(label_smoothing=0.1, **bad)


def test_adjust_learning_rate_follows_the_schedule():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 0, 1, 100), 0.1 * 2 / 500)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 4, 100, 100), 0.1 * 501 / 500)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 5, 1, 100), 0.1)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 60, 1, 100), 0.01)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 90, 1, 100), 0.001)
    assert math.isclose(adjust_learning_rate(opt, 0.1, 110, 1, 100), 0.0001) and math.isclose(opt.param_groups[0]['lr'], 0.0001)


def test_train_step_call_order_on_a_cpu_toy():
    """train_step is plain Python over any model / criterion / optimizer: forward, loss, zero_grad, backward, step"""
    from yolov4_amd.darknet.train import train_step
    torch.manual_seed(0)
    model = torch.nn.Linear(4, 3)
    w0, b0 = model.weight.detach().clone(), model.bias.detach().clone()
    model.weight.grad = torch.full_like(model.weight, 7.0)                                # stale: must be cleared, not added to
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    x, t = torch.randn(5, 4), torch.tensor([0, 2, 1, 1, 0])
    out, loss = train_step(model, torch.nn.CrossEntropyLoss(label_smoothing=0.1), opt, x, t)
    ref = torch.nn.Linear(4, 3)
    ref.load_state_dict({'weight': w0, 'bias': b0})
    ref_out = ref(x)
    ref_loss = F.cross_entropy(ref_out, t, label_smoothing=0.1)
    ref_loss.backward()
    assert torch.equal(out, ref_out) and torch.equal(loss, ref_loss)
    assert torch.allclose(model.weight, w0 - 0.5 * ref.weight.grad) and torch.allclose(model.bias, b0 - 0.5 * ref.bias.grad)


# ------------------------------------------------------------------ golden: the reference's CSPDarknet53 pins the composed oracle
def test_state_dict_keys_and_shapes_match_the_reference(golden):
    g = golden('classifier')
    sd = CSPDarknet53(CC.MODEL_CLASSES).state_dict()
    assert len(sd) == 434 and list(sd.keys()) == [str(k) for k in g['keys']]
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g['shapes']]
    assert list(sd.keys())[-2:] == ['classifier.weight', 'classifier.bias']
    assert tuple(sd['classifier.weight'].shape) == (37, 1024) and tuple(sd['classifier.bias'].shape) == (37,)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'classifier.npz')) < 1000000


def _filled_sd():
    # (plain contiguous tensors: the module keeps conv weights in channels_last memory, which changes the CPU conv algorithm)
    sd = {k: v.clone(memory_format=torch.contiguous_format) for k, v in CSPDarknet53(CC.MODEL_CLASSES).state_dict().items()}
    CC.fill_classifier_(sd, CC.MODEL_SEED)
    return sd


@pytest.mark.parametrize('step', range(len(CC.MODEL_STEPS)))
def test_composed_oracle_equals_the_reference_bit_for_bit(golden, step):
    """The fixture is the fp32 result of the reference's CSPDarknet53 on the machine that wrote it.  Where this machine rounds
    fp32 as that one did (CC.cpu_fingerprint, at the generator's thread count) the composed oracle must reproduce logits, loss,
    gradients and running statistics bit for bit.  On a CPU that reorders fp32 sums differently the same comparison would
    test the CPU, so there the rule of tests/test_oracle_golden.py applies: each difference at most the larger of smoke()'s
    floor and 4x the oracle's own fp32-to-fp64 distance measured here.  The fp64 results are compared closely everywhere."""
    g = golden('classifier')
    x, target = CC.model_input(step)
    was = torch.get_num_threads()
    torch.set_num_threads(CC.GOLDEN_THREADS)       # the generator's setting (tests/golden/make_golden_classifier.py)
    try:
        same_rounding = CC.cpu_fingerprint() == str(g['fingerprint'])
        net, logits, loss = CC.oracle_train_step(_filled_sd(), x, target, torch.float32)
        net64, logits64, loss64 = CC.oracle_train_step(_filled_sd(), x, target, torch.float64)
    finally:
        torch.set_num_threads(was)
    print('this machine rounds fp32 as the fixture\'s did: %s' % same_rounding)

    def check(name, a, b, a64, floor_abs=0.0, floor_of_max=0.0):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, name
        if same_rounding:
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), name
        else:
            a64 = np.asarray(a64, np.float64)
            e32 = np.abs(a.astype(np.float64) - a64).max()
            bound = max(floor_abs, floor_of_max * np.abs(a64).max(), 4 * e32)
            assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= bound, (name, e32, bound)
    check('logits', logits.numpy(), g[f'logits32_{step}'], logits64.numpy(), floor_abs=1e-4)
    check('loss', loss.numpy().reshape(1), g[f'loss32_{step}'].reshape(1), loss64.numpy().reshape(1), floor_of_max=1e-4)
    for k in CC.GRAD_KEYS:
        check(k, net.p[k].grad.numpy(), g[f'grad32_{step}_{k}'], net64.p[k].grad.numpy(), floor_of_max=1e-3)
    for k in CC.STAT_KEYS:
        check(k, net.p[k].numpy(), g[f'stat32_{step}_{k}'], net64.p[k].numpy(), floor_abs=1e-5, floor_of_max=1e-4)
    np.testing.assert_allclose(logits64.numpy(), g[f'logits64_{step}'], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(float(loss64), float(g[f'loss64_{step}']), rtol=1e-10)
    for k in CC.GRAD_KEYS:
        ref = g[f'grad64_{step}_{k}']
        tol = 2.0 ** -23 if ref.dtype == np.float32 else 1e-9
        np.testing.assert_allclose(net64.p[k].grad.numpy(), ref, rtol=tol, atol=tol * np.abs(ref).max())
    for k in CC.STAT_KEYS:
        np.testing.assert_allclose(net64.p[k].numpy(), g[f'stat64_{step}_{k}'], rtol=1e-9, atol=1e-11)


def test_fixture_was_written_where_bit_for_bit_was_checked(golden):
    """the digest is recorded, and on the machine that wrote the fixture the bit-for-bit branch above is the one that ran"""
    fp = str(golden('classifier')['fingerprint'])
    assert len(fp) == 64 and int(fp, 16) >= 0


# ------------------------------------------------------------------ checkpoint hand-off to the detector
def test_classifier_checkpoint_feeds_the_detector(tmp_path):
    m = CSPDarknet53(CC.MODEL_CLASSES)
    sd = m.state_dict()
    CC.fill_classifier_(sd, 5)
    m.load_state_dict(sd)
    path = os.path.join(str(tmp_path), 'model_best.pth.tar')
    torch.save({'state_dict': {'module.' + k: v for k, v in m.state_dict().items()}}, path)
    det = YOLOv4(dict(recipe.MODEL_CFG, BACKBONE_PRETRAINED=path))
    want = {k[len('backbone.'):]: v for k, v in m.state_dict().items() if k.startswith('backbone.')}
    got = det.backbone.state_dict()
    assert list(got.keys()) == list(want.keys()) and len(want) == 432
    for k, v in want.items():
        assert torch.equal(got[k], v), k


# ------------------------------------------------------------------ compiled kernels
def test_no_classifier_kernel_uses_scratch():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(root, 'yolov4_amd', 'csrc', 'classifier.hip'), ())
    names = ' '.join(r['name'] for r in rows)
    for k in ('avgpool_fwd_kernel', 'avgpool_bwd_kernel', 'gemm_nt_kernel', 'colsum_kernel', 'ce_fwd_rows_kernel', 'ce_mean_kernel',
              'ce_bwd_kernel', 'topk_rows_kernel'):
        assert k in names, k
    bad = [(r['name'], r['scratch'], r['vgpr_spill']) for r in rows if r['scratch'] != 0 or r['vgpr_spill'] != 0]
    assert not bad, bad
