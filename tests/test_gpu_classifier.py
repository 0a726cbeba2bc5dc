# -*- coding: utf-8 -*-
"""The classifier kernels of csrc/classifier.hip driven through the C ABI against the fp64 references and acceptance
rules of tests/classifier_cases.py (tests/test_classifier_cases.py shows without a GPU that every case reaches the branch
it is named for and that torch's own fp32 passes the same rules), and the whole CSPDarknet53 against the composed oracle.

Outputs are pre-filled with a NaN sentinel and pad columns (pitch > width) hold it on input: a kernel that skips an element
or touches a pad column is caught by the bit pattern.  No label outside [0, N) other than -100 is ever fed: that contract
is read in the code (the label is only compared, never used in an address), not provoked."""
import numpy as np
import pytest
import torch

import classifier_cases as CC
import recipe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import check, int_array, lib
    return lib(), ops._ptr, ops._stream, check, int_array


def _up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                 # (a copy: the cached case arrays are read-only)


def _sent(shape, dev):
    return _up(CC.sentinel(shape), dev)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize('case', CC.POOL_CASES, ids=str)
def test_avgpool_fwd_bwd(dev, case):
    B, HW, C, ld = case
    L, ptr, stream, check, _ = _abi()
    c = CC.pool_case(case)
    x, dy = _up(c['x'], dev), _up(c['dy'], dev)
    y, dx = _sent((B, ld), dev), _sent((B, HW, ld), dev)
    check(L.y4_avgpool_global_fwd_f32(ptr(x), ld, ptr(y), ld, B, HW, C, stream()), 'avgpool_fwd')
    check(L.y4_avgpool_global_bwd_f32(ptr(dy), ld, ptr(dx), ld, B, HW, C, stream()), 'avgpool_bwd')
    y2 = _sent((B, ld), dev)
    check(L.y4_avgpool_global_fwd_f32(ptr(x), ld, ptr(y2), ld, B, HW, C, stream()), 'avgpool_fwd')
    torch.cuda.synchronize()
    yh, dxh = y.cpu().numpy(), dx.cpu().numpy()
    ok, frac = CC.pool_fwd_accept(yh[:, :C], c['y64'], c['absmean'], HW)
    okb, fracb = CC.pool_bwd_accept(dxh[..., :C], c['dx64'])
    print('avgpool %s (%s): fraction of the bound needed: fwd %.3f, bwd %.3f' % (case, CC.pool_path(C, ld, ld), frac, fracb))
    assert ok.all(), np.argwhere(~ok)[:5]
    assert okb.all(), np.argwhere(~okb)[:5]
    assert CC.is_sentinel(yh[:, C:]).all() and CC.is_sentinel(dxh[..., C:]).all()        # pad columns untouched
    assert np.array_equal(_bits(x), c['x'].view(np.uint32)) and np.array_equal(_bits(dy), c['dy'].view(np.uint32))
    assert _same_bits(y, y2)


# ------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize('case', CC.LINEAR_CASES, ids=str)
def test_linear_fwd_bwd(dev, case):
    M, K, N, ldx, ldy = case
    L, ptr, stream, check, _ = _abi()
    c = CC.linear_case(case)
    x, dy, w, bias = (_up(c[k], dev) for k in ('x', 'dy', 'w', 'bias'))

    def fwd(b):
        y = _sent((M, ldy), dev)
        check(L.y4_linear_fwd_f32(ptr(x), ldx, ptr(w), ptr(b), ptr(y), ldy, M, K, N, stream()), 'linear_fwd')
        return y

    def bwd(want_dx=True, want_dw=True, want_db=True):
        dx = _sent((M, ldx), dev) if want_dx else None
        dw = _sent((N, K), dev) if want_dw else None
        db = _sent((N,), dev) if want_db else None
        check(L.y4_linear_bwd_f32(ptr(x), ldx, ptr(w), ptr(dy), ldy, ptr(dx), ldx, ptr(dw), ptr(db), M, K, N, stream()),
              'linear_bwd')
        return dx, dw, db

    y, y_again, y_nobias = fwd(bias), fwd(bias), fwd(None)
    dx, dw, db = bwd()
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    res = {}
    for name, got, ref, ab, Lr in (('y', yh[:, :N], c['y64'], c['y_abs'], K),
                                   ('y_nobias', y_nobias.cpu().numpy()[:, :N], c['y64_nobias'], c['y_abs_nobias'], K),
                                   ('dx', dx.cpu().numpy()[:, :K], c['dx64'], c['dx_abs'], N),
                                   ('dw', dw.cpu().numpy(), c['dw64'], c['dw_abs'], M),
                                   ('dbias', db.cpu().numpy(), c['db64'], c['db_abs'], M)):
        ok, frac = CC.linear_accept(got, ref, ab, Lr)
        res[name] = (ok, frac)
    print('linear %s: fraction of the bound needed: %s' % (case, ', '.join('%s %.3f' % (k, v[1]) for k, v in res.items())))
    for name, (ok, _) in res.items():
        assert ok.all(), (name, np.argwhere(~ok)[:5])
    assert CC.is_sentinel(yh[:, N:]).all() and CC.is_sentinel(dx.cpu().numpy()[:, K:]).all()
    assert np.array_equal(_bits(x), c['x'].view(np.uint32)) and np.array_equal(_bits(dy), c['dy'].view(np.uint32))
    assert _same_bits(y, y_again)
    # each output NULL in turn: the others bit-equal to the full call; and a second full call bit-equal to the first
    for skip in range(3):
        part = bwd(*(i != skip for i in range(3)))
        torch.cuda.synchronize()
        assert part[skip] is None
        for i, (a, b) in enumerate(zip(part, (dx, dw, db))):
            if i != skip:
                assert _same_bits(a, b), (skip, i)
    for a, b in zip(bwd(), (dx, dw, db)):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------ cross-entropy
def _run_ce(dev, c, N, ldl):
    L, ptr, stream, check, _ = _abi()
    B = CC.CE_B
    zfull = CC.sentinel((B, ldl))
    zfull[:, :N] = c['z']
    z, t = _up(zfull, dev), _up(c['t'], dev)
    row = _sent((B,), dev)
    out = torch.full((2,), float('nan'), device=dev, dtype=torch.float64)
    gs = torch.full((1,), CC.CE_GSCALE, device=dev, dtype=torch.float32)
    d = _sent((B, ldl), dev)
    check(L.y4_ce_smooth_fwd_f32(ptr(z), ldl, ptr(t), B, N, CC.SMOOTHING, ptr(row), ptr(out), stream()), 'ce_fwd')
    check(L.y4_ce_smooth_bwd_f32(ptr(z), ldl, ptr(t), ptr(out), ptr(gs), ptr(d), ldl, B, N, CC.SMOOTHING, stream()), 'ce_bwd')
    torch.cuda.synchronize()
    assert np.array_equal(_bits(z), zfull.view(np.uint32))
    dh = d.cpu().numpy()
    assert CC.is_sentinel(dh[:, N:]).all()                                               # pad columns untouched
    return row.cpu().numpy(), out.cpu().numpy(), dh[:, :N]


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'ld+3'])
@pytest.mark.parametrize('N', CC.CE_NS)
def test_ce_smooth_fwd_bwd(dev, N, pad):
    c = CC.ce_case(N)
    row, out, grad = _run_ce(dev, c, N, N + pad)
    ok_r, f_r = CC.ce_row_accept(row, c)
    ok_m, f_m = CC.ce_mean_accept(out[0], c)
    ok_g, f_g = CC.ce_grad_accept(grad, c)
    print('ce N=%d ld=%d: fraction of the bound needed: rows %.3f, mean %.3f, gradient %.3f' % (N, N + pad, f_r, f_m, f_g))
    assert ok_r.all(), (row, c['row64'])
    assert ok_m, (out[0], c['mean64'])
    assert out[1] == c['counted'] == 5
    assert ok_g.all(), np.argwhere(~ok_g)[:5]
    assert row[3] == 0.0 and (grad[3] == 0.0).all()                                       # the ignored row: exactly 0


def test_ce_all_rows_ignored(dev):
    c = CC.ce_case(37, all_ignored=True)
    row, out, grad = _run_ce(dev, c, 37, 40)
    assert np.isnan(out[0]) and out[1] == 0.0
    assert (row == 0.0).all() and (grad == 0.0).all() and not np.signbit(grad).any()


# ------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize('ks', CC.TOPK_KS, ids=str)
@pytest.mark.parametrize('N', CC.TOPK_NS)
def test_topk_correct(dev, N, ks):
    L, ptr, stream, check, iarr = _abi()
    c = CC.topk_case(N)
    B = CC.TOPK_B
    z, t = _up(c['z'], dev), _up(c['t'], dev)
    correct = torch.full((len(ks),), -7, device=dev, dtype=torch.int32)
    rank = torch.full((B,), -7, device=dev, dtype=torch.int32)
    check(L.y4_topk_correct_f32(ptr(z), N, ptr(t), B, N, iarr(ks), len(ks), ptr(correct), ptr(rank), stream()), 'topk')
    correct2 = torch.full((len(ks),), -7, device=dev, dtype=torch.int32)
    check(L.y4_topk_correct_f32(ptr(z), N, ptr(t), B, N, iarr(ks), len(ks), ptr(correct2), None, stream()), 'topk')
    torch.cuda.synchronize()
    assert np.array_equal(rank.cpu().numpy(), c['rank'])
    assert np.array_equal(correct.cpu().numpy(), CC.correct_rule(c['rank'], ks))
    assert np.array_equal(correct2.cpu().numpy(), CC.correct_rule(c['rank'], ks))         # rank is optional


# ------------------------------------------------------------------------------------------ whole model
def _cpu_sd(model):
    return {k: v.detach().cpu().clone(memory_format=torch.contiguous_format) for k, v in model.state_dict().items()}


@pytest.fixture(scope='module')
def runs(dev):
    """Per step of CC.MODEL_STEPS, computed once: the HIP model's train step, its eval logits on calibrated BatchNorm
    statistics and one FusedAdam step, beside the composed oracle in fp32 and fp64."""
    from yolov4_amd.darknet.darknet import CSPDarknet53
    from yolov4_amd.darknet.loss import CrossEntropyLoss, accuracy
    from yolov4_amd.yolo.optim.optimizers.build import FusedAdam
    out = []
    for step in range(len(CC.MODEL_STEPS)):
        r = {}
        x, target = CC.model_input(step)
        model = CSPDarknet53(CC.MODEL_CLASSES)
        sd = model.state_dict()
        CC.fill_classifier_(sd, CC.MODEL_SEED)
        model.load_state_dict(sd)
        sd0 = _cpu_sd(model)
        model = model.to(dev).train()
        seen = {}
        hooks = [model.pool.register_forward_hook(lambda m, i, o: seen.__setitem__('pool', (i[0], o))),
                 model.classifier.register_forward_hook(lambda m, i, o: seen.__setitem__('classifier', (i[0], o)))]
        crit = CrossEntropyLoss(label_smoothing=CC.SMOOTHING)
        logits = model(x.to(dev))
        loss = crit(logits, target.to(dev))
        loss.backward()
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        r['seen'] = {k: tuple((tuple(t.shape), t.dtype, t.is_cuda) for t in v) for k, v in seen.items()}
        r['logits'], r['loss'] = logits.detach().cpu().numpy(), float(loss.detach())
        params = dict(model.named_parameters())
        r['grads'] = {k: params[k].grad.detach().cpu().numpy() for k in CC.GRAD_KEYS}
        r['acc'] = [float(a) for a in accuracy(logits.detach(), target.to(dev), topk=(1, 5))]
        r['acc_shapes'] = [tuple(a.shape) for a in accuracy(logits.detach(), target.to(dev), topk=(1,))]
        r['target'] = target.numpy()
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            net, lg, ls = CC.oracle_train_step(sd0, x, target, dt)
            r[f'o{bits}'] = dict(logits=lg.numpy().astype(np.float64), loss=float(ls),
                                 grads={k: net.p[k].grad.numpy().astype(np.float64) for k in CC.GRAD_KEYS})
        # eval on calibrated statistics; both sides use the HIP model's running statistics, as smoke() does
        model.load_state_dict(sd0)
        S = x.shape[-1]
        recipe.calibrate_bn_(model, recipe.randn((8, 3, S, S), 3).to(dev))
        model.eval()
        with torch.no_grad():
            r['eval'] = model(x.to(dev)).cpu().numpy()
        sd1 = _cpu_sd(model)
        r['eval32'] = CC.oracle_eval(sd1, x, torch.float32).numpy().astype(np.float64)
        r['eval64'] = CC.oracle_eval(sd1, x, torch.float64).numpy()
        # one FusedAdam step over the whole model against torch.optim.Adam on the CPU for the two classifier parameters
        model.train()
        cpu_p = [torch.nn.Parameter(params[k].detach().cpu().clone()) for k in ('classifier.weight', 'classifier.bias')]
        for p, k in zip(cpu_p, ('classifier.weight', 'classifier.bias')):
            p.grad = params[k].grad.detach().cpu().clone()
        stem_before = params['backbone.stem.conv.weight'].detach().cpu().clone()
        opt = FusedAdam(model.parameters(), lr=1e-3)
        opt.step()
        torch.optim.Adam(cpu_p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8).step()
        torch.cuda.synchronize()
        r['adam'] = [(params[k].detach().cpu().numpy(), p.detach().numpy())
                     for p, k in zip(cpu_p, ('classifier.weight', 'classifier.bias'))]
        r['adam_launches'] = opt.launches
        r['stem_moved'] = not torch.equal(params['backbone.stem.conv.weight'].detach().cpu(), stem_before)
        out.append(r)
        del model, opt
    return out


STEPS = range(len(CC.MODEL_STEPS))


@pytest.mark.parametrize('step', STEPS)
def test_model_train_step_against_the_composed_oracle(runs, step):
    """error versus fp64 at most max(floor, 1.5 x the fp32 oracle's own distance from fp64); smoke()'s floors: loss relative
    1e-4, gradients 1e-3 of the tensor's maximum, logits absolute 1e-4"""
    r = runs[step]
    o32, o64 = r['o32'], r['o64']
    e_lg, ref_lg = np.abs(r['logits'] - o64['logits']).max(), np.abs(o32['logits'] - o64['logits']).max()
    e_ls, ref_ls = abs(r['loss'] - o64['loss']) / abs(o64['loss']), abs(o32['loss'] - o64['loss']) / abs(o64['loss'])
    print('step %d: logits err %.2e (fp32 oracle %.2e), loss rel %.2e (fp32 oracle %.2e)' % (step, e_lg, ref_lg, e_ls, ref_ls))
    assert r['logits'].shape == (CC.MODEL_STEPS[step][0][0], CC.MODEL_CLASSES) and np.isfinite(r['logits']).all()
    assert e_lg <= max(1e-4, 1.5 * ref_lg)
    assert e_ls <= max(1e-4, 1.5 * ref_ls)
    for k in CC.GRAD_KEYS:
        g64 = o64['grads'][k]
        top = np.abs(g64).max()
        e, ref = np.abs(r['grads'][k] - g64).max() / top, np.abs(o32['grads'][k] - g64).max() / top
        print('step %d: grad %s err %.2e of max (fp32 oracle %.2e)' % (step, k, e, ref))
        assert r['grads'][k].shape == g64.shape and e <= max(1e-3, 1.5 * ref), k


@pytest.mark.parametrize('step', STEPS)
def test_model_eval_against_the_composed_oracle(runs, step):
    r = runs[step]
    e, ref = np.abs(r['eval'] - r['eval64']).max(), np.abs(r['eval32'] - r['eval64']).max()
    print('step %d: eval logits err %.2e (fp32 oracle %.2e)' % (step, e, ref))
    assert np.isfinite(r['eval']).all() and e <= max(1e-4, 1.5 * ref)


@pytest.mark.parametrize('step', STEPS)
def test_hooks_see_the_reference_shapes(runs, step):
    B = CC.MODEL_STEPS[step][0][0]
    S = CC.MODEL_STEPS[step][0][2] // 32
    seen = runs[step]['seen']
    f32 = torch.float32
    assert seen['pool'] == (((B, 1024, S, S), f32, True), ((B, 1024, 1, 1), f32, True))
    assert seen['classifier'] == (((B, 1024), f32, True), ((B, CC.MODEL_CLASSES), f32, True))


@pytest.mark.parametrize('step', STEPS)
def test_fused_adam_steps_the_classifier(runs, step):
    r = runs[step]
    assert r['adam_launches'] == 1 and r['stem_moved']
    for got, ref in r['adam']:
        np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-7)                        # tests/test_next_rows.py's tolerance


@pytest.mark.parametrize('step', STEPS)
def test_accuracy_follows_the_rank_rule(runs, step):
    r = runs[step]
    rank = CC.rank_rule(r['logits'], r['target'])
    B = len(r['target'])
    want = [float(np.float32(c) * np.float32(100.0 / B)) for c in CC.correct_rule(rank, (1, 5))]
    np.testing.assert_allclose(r['acc'], want, rtol=1e-6)
    assert r['acc_shapes'] == [(1,)]


def test_train_and_validate_loops(dev):
    """darknet/train.py on a two-batch loader: the schedule is applied before each step, the loss and the accuracies come
    back finite, validate() returns the average Prec@1 of the numpy rank rule on the eval-mode logits."""
    from yolov4_amd.darknet.darknet import CSPDarknet53
    from yolov4_amd.darknet.loss import CrossEntropyLoss
    from yolov4_amd.darknet.train import train, validate
    from yolov4_amd.yolo.optim.optimizers.build import FusedSGD
    model = CSPDarknet53(CC.MODEL_CLASSES)
    sd = model.state_dict()
    CC.fill_classifier_(sd, CC.MODEL_SEED)
    model.load_state_dict(sd)
    model = model.to(dev)
    loader = [(recipe.randn((2, 3, 64, 64), 21 + i).to(dev), torch.tensor([5 + i, 30 - i]).to(dev)) for i in range(2)]
    crit = CrossEntropyLoss(label_smoothing=CC.SMOOTHING)
    opt = FusedSGD(model.parameters(), lr=1.0, momentum=0.9, weight_decay=0.0)
    lines = []
    w0 = model.classifier.weight.detach().clone()
    avg = train(loader, model, crit, opt, 0, 1e-3, print_freq=1, log=lines.append)
    assert model.training and np.isfinite(avg) and len(lines) == 2 and opt.launches == 2
    assert opt.param_groups[0]['lr'] == 1e-3 * 3 / 10                                     # warm-up: (1 + step) / (5 * len)
    assert not torch.equal(model.classifier.weight.detach(), w0)
    top1 = validate(loader, model, crit, log=lines.append)
    assert not model.training and len(lines) == 3
    with torch.no_grad():
        ranks = [CC.rank_rule(model(x).cpu().numpy(), t.cpu().numpy()) for x, t in loader]
    want = np.mean([np.float32((r < 1).sum()) * np.float32(100.0 / 2) for r in ranks])
    assert abs(top1 - want) < 1e-4
