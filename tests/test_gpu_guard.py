# -*- coding: utf-8 -*-
"""On-device grad-norm clipping, non-finite step skip and ModelEMA on the MI355X, at the edges of the multi-tensor
dispatch: chunks of 65535 / 65536 / 65537 elements, 16-byte tails, a KRSC parameter, a gradient whose pointer is only
4-byte aligned (scalar path), and more chunks than the grid has blocks (2100 > 2048).

References are fp64 restatements written here: the sum of squares of fl32(g * scale) (math.fsum: exact),
torch.nn.utils.clip_grad_norm_ on double copies, and d * e + (1 - d) * s for the average.  The step arithmetic is
compared bit for bit with the unguarded optimizers run at grad_scale * fl32(coef), which isolates the new code from
Adam's own rounding: no tolerance there."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

import recipe
from yolov4_amd import _lib, ops
from yolov4_amd.yolo.optim.optimizers.build import FusedAdam, FusedSGD, build_optimizer
from yolov4_amd.yolo.util.ema import ModelEMA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
KEEP = torch.preserve_format

# 1, 3: below one 16-byte group; 65535 / 65536 / 65537: one chunk with a 3-element tail / exactly one chunk / a second
# chunk of one element; 'krsc': a (64, 32, 3, 3) channels_last parameter; 'odd': the gradient is a view starting one
# element into its storage (4-byte aligned pointer: scalar path of every kernel); last: two full chunks + a chunk of 7
# (one 16-byte group + a tail of 3), so the list's last element sits in the last chunk's tail.
SIZES = (1, 3, 65535, 65536, 65537, 'krsc', 'odd', 2 * 65536 + 7)
N_ODD = 4099
MANY = (5,) * 2100                       # nchunks = 2100 > 2048 blocks: grid-stride loop, > 2048 partials in the finalize


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1
    return torch.device('cuda:0')


def offset_view(values, dev):
    """values in a fresh buffer, starting one element into its storage."""
    base = torch.empty(values.numel() + 1, dtype=values.dtype, device=dev)
    view = base[1:]
    view.copy_(values.reshape(-1))
    return view


def build_list(dev, sizes, seed, grad_value=None):
    """Parameters with gradients attached, the same bits for the same seed."""
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    params = []
    for s in sizes:
        if s == 'krsc':
            p = torch.randn(64, 32, 3, 3, generator=g).to(dev).contiguous(memory_format=CL)
            gr = torch.randn(64, 32, 3, 3, generator=g).to(dev).contiguous(memory_format=CL)
        elif s == 'odd':
            p = torch.randn(N_ODD, generator=g).to(dev)
            gr = offset_view(torch.randn(N_ODD, generator=g), dev)
        else:
            p = torch.randn(s, generator=g).to(dev)
            gr = torch.randn(s, generator=g).to(dev)
        if grad_value is not None:
            gr.fill_(grad_value)
        p = nn.Parameter(p)
        p.grad = gr
        params.append(p)
    return params


def clone_grad(g):
    if g.storage_offset():
        return offset_view(g.detach(), g.device)
    return g.detach().clone(memory_format=KEEP)


def make_opt(kind, params, **kw):
    if kind == 'adam':
        return FusedAdam(params, lr=1e-3, weight_decay=0.01, **kw)
    return FusedSGD(params, lr=0.05, momentum=0.9, weight_decay=1e-4, **kw)


def state_tensors(opt, params):
    out = []
    for p in params:
        out.append(p)
        out.extend(v for _, v in sorted(opt.state[p].items()) if torch.is_tensor(v))
    return out


def twin(kind, params, opt):
    """An UNGUARDED optimizer of the same kind on clones of the parameters, gradients and state (step counts included)."""
    new = []
    for p in params:
        q = nn.Parameter(p.detach().clone(memory_format=KEEP))
        q.grad = clone_grad(p.grad)
        new.append(q)
    t = make_opt(kind, new)
    for p, q in zip(params, new):
        if p in opt.state:
            t.state[q] = {k: (v.detach().clone(memory_format=KEEP) if torch.is_tensor(v) else v)
                          for k, v in opt.state[p].items()}
    t.grad_scale = opt.grad_scale
    return new, t


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def assert_same_bits(xs, ys, what):
    assert len(xs) == len(ys)
    for i, (a, b) in enumerate(zip(xs, ys)):
        assert bits_equal(a, b), f'{what}: tensor {i} of shape {tuple(a.shape)} differs'


def scaled64(params, scale):
    """fl32(g * scale) as float64 arrays: the values the step kernels use."""
    return [(p.grad.detach().cpu().numpy().astype(np.float32).ravel() * np.float32(scale)).astype(np.float64)
            for p in params]


def ref_norm(params, scale):
    """sqrt of the exactly rounded fp64 sum of squares (a square of an fp32 value is exact in fp64)."""
    return math.sqrt(math.fsum(math.fsum(x * x) for x in scaled64(params, scale)))


def ref_clip(params, scale, max_norm):
    """(total_norm, coef) of torch.nn.utils.clip_grad_norm_ on double copies."""
    dbl = []
    for x in scaled64(params, scale):
        q = nn.Parameter(torch.zeros(x.size, dtype=torch.float64))
        q.grad = torch.from_numpy(x.copy())
        dbl.append(q)
    before = dbl[-1].grad.clone()
    total = float(torch.nn.utils.clip_grad_norm_(dbl, max_norm))
    coef = min(1.0, max_norm / (total + 1e-6))
    assert torch.allclose(dbl[-1].grad, before * coef, rtol=1e-14, atol=0)      # the formula is the one torch applied
    return total, coef


def n_elements(params):
    return sum(p.numel() for p in params)


def test_the_lists_hit_the_dispatch_edges(dev):
    params = build_list(dev, SIZES, 1)
    ptr = {s: p.grad.data_ptr() for s, p in zip(SIZES, params)}
    assert ptr['odd'] % 16 == 4 and all(v % 16 == 0 for s, v in ptr.items() if s != 'odd')
    assert params[SIZES.index('krsc')].is_contiguous(memory_format=CL)
    assert SIZES[-1] % 65536 == 7 and len(MANY) > 2048


# ------------------------------------------------------------------ 1. norm
@pytest.mark.parametrize('sizes', [SIZES, MANY], ids=['edges', 'many'])
@pytest.mark.parametrize('scale', [1.0, 0.25])
def test_total_norm_matches_fp64_and_is_reproducible(dev, sizes, scale):
    records = []
    for _ in range(2):
        params = build_list(dev, sizes, 2)
        opt = make_opt('adam', params, skip_nonfinite=True)
        opt.grad_scale = scale
        opt.step()
        records.append(opt.guard.clone())
    st = opt.guard_state()
    ref = ref_norm(params, scale)
    n = n_elements(params)
    rel = abs(st['total_norm'] - ref) / ref
    print(f'total_norm {st["total_norm"]!r} ref {ref!r} rel {rel:.3e} bound {n * 2.0 ** -52:.3e}')
    assert rel <= n * 2.0 ** -52                       # worst case of ANY fixed-order double summation of n terms
    assert st['applied'] is True and st['coef'] == 1.0 and st['skipped'] == 0
    assert torch.equal(records[0].view(torch.int64), records[1].view(torch.int64))
    t_total, _ = ref_clip(params, scale, 1.0)
    assert abs(t_total - ref) / ref < 1e-13            # the two references agree


# ------------------------------------------------------------------ 2. coefficient
@pytest.mark.parametrize('max_norm', [10.0, 1e4, None, float('inf')])
def test_clip_coefficient(dev, max_norm):
    params = build_list(dev, SIZES, 3)
    opt = make_opt('sgd', params, max_grad_norm=max_norm, skip_nonfinite=max_norm is None)
    opt.step()
    st = opt.guard_state()
    total = ref_norm(params, 1.0)
    assert 100.0 < total < 1e4                          # 10.0 lies below the norm, 1e4 above it
    if max_norm == 10.0:
        _, coef = ref_clip(params, 1.0, max_norm)
        print(f'coef {st["coef"]!r} ref {coef!r}')
        assert coef < 1.0 and abs(st['coef'] - coef) / coef <= 1e-12
    else:
        assert st['coef'] == 1.0
    assert st['applied'] is True and st['skipped'] == 0


# ------------------------------------------------------------------ 3. step arithmetic is exact
@pytest.mark.parametrize('sizes', [SIZES, MANY], ids=['edges', 'many'])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
@pytest.mark.parametrize('max_norm', [10.0, 1e30])
def test_guarded_step_equals_unguarded_step_at_the_clipped_scale(dev, kind, sizes, max_norm):
    params = build_list(dev, sizes, 4)
    opt = make_opt(kind, params, max_grad_norm=max_norm)
    opt.grad_scale = 0.25
    for it in range(2):                                # the second step starts from non-zero moments / momentum
        if it:
            for p in params:
                p.grad.mul_(-3.0)
        tparams, topt = twin(kind, params, opt)
        before = opt.launches
        opt.step()
        assert opt.launches == before + 3              # sumsq, guard, guarded step
        st = opt.guard_state()
        assert st['applied'] is True
        if max_norm == 1e30:
            assert st['coef'] == 1.0                   # ... and the twin runs at the plain grad_scale
        else:
            assert st['coef'] < 1.0
            topt.grad_scale = float(np.float32(opt.grad_scale) * np.float32(st['coef']))
        topt.step()
        assert topt.launches == 1 and topt.guard is None
        assert_same_bits(state_tensors(opt, params), state_tensors(topt, tparams), f'{kind} step {it}')


# ------------------------------------------------------------------ 4. skip
def poke(params, where):
    if where == 'last_tail':
        params[-1].grad[-1] = float('inf')
    elif where == 'first':
        params[0].grad[0] = float('nan')
    else:
        params[SIZES.index('odd')].grad[N_ODD // 2] = float('-inf')


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
@pytest.mark.parametrize('where', ['last_tail', 'first', 'odd_middle'])
def test_nonfinite_gradient_skips_the_step(dev, kind, where):
    params = build_list(dev, SIZES, 5)
    opt = make_opt(kind, params, max_grad_norm=10.0, skip_nonfinite=True)
    skipped = 0
    if kind == 'adam':                                 # Adam: skip from non-zero moments; SGD: the FIRST step is skipped
        opt.step()
        skipped = opt.guard_state()['skipped']
        assert skipped == 0
    clean = [clone_grad(p.grad) for p in params]
    keep = [t.detach().clone(memory_format=KEEP) for t in state_tensors(opt, params)] if kind == 'adam' else \
        [p.detach().clone(memory_format=KEEP) for p in params]
    poke(params, where)
    opt.step()
    st = opt.guard_state()
    assert st['applied'] is False and st['coef'] == 1.0 and not math.isfinite(st['total_norm'])
    assert st['skipped'] == skipped + 1
    if kind == 'adam':
        assert_same_bits(state_tensors(opt, params), keep, 'skipped step')
    else:
        assert_same_bits(params, keep, 'skipped step')
        for p in params:
            assert not opt.state[p]['momentum_buffer'].any()            # still the zeros it was created with
    # a following clean step is applied and equals the unguarded step from the same state
    for p, c in zip(params, clean):
        p.grad.copy_(c)
    tparams, topt = twin(kind, params, opt)
    opt.step()
    st = opt.guard_state()
    assert st['applied'] is True and st['skipped'] == skipped + 1 and st['coef'] < 1.0
    topt.grad_scale = float(np.float32(opt.grad_scale) * np.float32(st['coef']))
    topt.step()
    assert_same_bits(state_tensors(opt, params), state_tensors(topt, tparams), 'step after the skip')
    assert not bits_equal(params[2], keep[2 * 3 if kind == 'adam' else 2])          # ... and it moved the parameters


# ------------------------------------------------------------------ 5. huge gradients are clipped, not skipped
def test_huge_gradients_are_clipped_not_skipped(dev):
    params = build_list(dev, SIZES, 6, grad_value=1e30)                # fp32 squares overflow, the fp64 sum does not
    assert math.isinf(float(params[2].grad[0] * params[2].grad[0]))
    opt = make_opt('adam', params, max_grad_norm=10.0, skip_nonfinite=True)
    tparams, topt = twin('adam', params, opt)
    opt.step()
    st = opt.guard_state()
    ref, coef = ref_clip(params, 1.0, 10.0)
    n = n_elements(params)
    print(f'total_norm {st["total_norm"]!r} ref {ref!r}; coef {st["coef"]!r} ref {coef!r}')
    assert math.isfinite(st['total_norm']) and abs(st['total_norm'] - ref_norm(params, 1.0)) / ref <= n * 2.0 ** -52
    assert st['applied'] is True and st['skipped'] == 0
    assert abs(st['coef'] - coef) / coef <= 1e-12
    topt.grad_scale = float(np.float32(1.0) * np.float32(st['coef']))
    topt.step()
    assert_same_bits(state_tensors(opt, params), state_tensors(topt, tparams), 'clipped huge step')
    assert not any(bits_equal(p, q) for p, q in zip(params, build_list(dev, SIZES, 6)))      # the step moved everything


# ------------------------------------------------------------------ 6. defaults untouched
def test_defaults_issue_one_launch_and_keep_the_bits(dev):
    params = build_list(dev, SIZES, 7)
    opt = FusedAdam(params, lr=1e-3, weight_decay=0.01)
    single = [(p.detach().clone(memory_format=KEEP), clone_grad(p.grad), torch.zeros_like(p, memory_format=KEEP),
               torch.zeros_like(p, memory_format=KEEP)) for p in params]
    L = _lib.lib()
    for step in (1, 2):
        opt.step()
        assert opt.launches == step and opt.guard is None and not opt.guarded
        for p, g, m, v in single:                      # the per-tensor entry point: bit-identical by its contract
            _lib.check(L.y4_adam_step_f32(ops._ptr(p), ops._ptr(g), ops._ptr(m), ops._ptr(v), p.numel(), 1e-3, 0.9, 0.999,
                                          1e-8, 0.01, step, 1.0, ops._stream()), 'adam_step')
        got = state_tensors(opt, params)
        want = [t for p, g, m, v in single for t in (p, m, v)]
        assert_same_bits(got, want, f'default step {step}')
    with pytest.raises(ops.Y4Error):
        opt.guard_state()


# ------------------------------------------------------------------ 7. EMA
class Bag(nn.Module):
    """The size list as a module: parameters (the 'odd' one a view one element into its storage), a float buffer and
    an integer one."""

    def __init__(self, dev, seed):
        super().__init__()
        for i, p in enumerate(build_list(dev, SIZES, seed)):
            t = offset_view(p.detach(), dev) if SIZES[i] == 'odd' else p.detach()
            self.register_parameter(f'p{i}', nn.Parameter(t))
        self.register_buffer('running_var', torch.rand(33, device=dev) + 0.5)
        self.register_buffer('num_batches_tracked', torch.tensor(7, device=dev))


def perturb_(bag, seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    for v in bag.state_dict().values():
        if v.is_floating_point():
            v.add_(torch.randn(v.shape, generator=g).to(v.device))
        else:
            v.add_(5)


def test_ema_three_updates_against_fp64(dev):
    bag = Bag(dev, 8)
    assert bag.state_dict()[f'p{SIZES.index("odd")}'].data_ptr() % 16 == 4
    # tau = 1: d = 0.632, 0.865, 0.950, so 1 - d <= 0.5 and the per-update rounding stays inside the bound below
    ema = ModelEMA(bag, decay=0.9999, tau=1.0)
    assert ema.ema['p5'].is_contiguous(memory_format=CL) and ema.ema['p5'].data_ptr() != bag.p5.data_ptr()
    ref = {k: v.detach().cpu().double() for k, v in bag.state_dict().items()}
    peak = {k: v.abs() for k, v in ref.items()}
    for u in (1, 2, 3):
        perturb_(bag, 20 + u)
        ema.update(bag)
        assert ema.updates == u
        d = 0.9999 * (1.0 - math.exp(-u / 1.0))
        for k, s in bag.state_dict().items():
            s = s.detach().cpu()
            if not s.is_floating_point():
                assert torch.equal(ema.ema[k].cpu(), s) and int(s) == 7 + 5 * u          # integer entries are copied
                continue
            peak[k] = torch.maximum(peak[k], s.double().abs())
            ref[k] = d * ref[k] + (1.0 - d) * s.double()
            peak[k] = torch.maximum(peak[k], ref[k].abs())
            err = (ema.ema[k].cpu().double() - ref[k]).abs()
            # three fp32 roundings per element per update + the rounding of 1 - d: 4 * updates * 2^-24 * max(|e|, |s|),
            # the maximum taken over the updates so far (the error of an earlier update scales with ITS operands and is
            # carried on, times d, when the current ones happen to be small)
            bound = 4.0 * u * 2.0 ** -24 * peak[k]
            assert bool((err <= bound).all()), (k, u, float((err / bound.clamp_min(1e-300)).max()))
    assert not bits_equal(ema.ema['p2'], bag.p2)


def test_ema_guard_swap_and_integers(dev):
    bag = Bag(dev, 9)
    ema = ModelEMA(bag, decay=0.9, tau=1.0)
    perturb_(bag, 30)
    floats = [k for k, v in ema.ema.items() if v.is_floating_point()]
    before = {k: ema.ema[k].clone(memory_format=KEEP) for k in floats}
    skipped = torch.tensor([float('nan'), 1.0, 0.0, 1.0], dtype=torch.float64, device=dev)
    ema.update(bag, skipped)                                           # the step it follows was not applied
    for k in floats:
        assert bits_equal(ema.ema[k], before[k]), k
    assert int(ema.ema['num_batches_tracked']) == 12
    applied = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64, device=dev)
    ema.update(bag, applied)
    for k in floats:
        assert not bits_equal(ema.ema[k], before[k]), k
    # swap: the model carries the average, the average the live values; twice restores both bit for bit
    live = {k: v.detach().clone(memory_format=KEEP) for k, v in bag.state_dict().items()}
    avg = {k: v.clone(memory_format=KEEP) for k, v in ema.ema.items()}
    ema.swap(bag)
    for k, v in bag.state_dict().items():
        assert torch.equal(v, avg[k]) and torch.equal(ema.ema[k], live[k]), k
    ema.swap(bag)
    for k, v in bag.state_dict().items():
        if v.is_floating_point():
            assert bits_equal(v, live[k]) and bits_equal(ema.ema[k], avg[k]), k
        else:
            assert torch.equal(v, live[k]) and torch.equal(ema.ema[k], avg[k]), k
    with ema.applied_to(bag) as inside:
        assert inside is bag and torch.equal(bag.p2.detach(), avg['p2'])
    assert bits_equal(bag.p2, live['p2'])
    with pytest.raises(ops.Y4Error):
        ema.update(bag, torch.zeros(4, device=dev))                    # not a guard record (float32)


# ------------------------------------------------------------------ 8. end to end
def test_training_with_clipping_skip_and_ema_end_to_end(dev):
    """The 160x160, bs 4 recipe of test_training_loop_end_to_end_loss_falls with CLIP_GRAD_NORM / SKIP_NONFINITE and a
    ModelEMA; step 3 gets one inf gradient element and must leave parameters and average alone.  Steps 4-6 go through
    train_step, which hands the optimizer's guard record to the EMA itself."""
    from yolov4_amd.ddp import BucketedDDP
    from yolov4_amd.yolo.engine.build import train_step
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    cfg = dict(recipe.FULL_CFG)
    cfg['OPTIMIZER'] = {'TYPE': 'ADAM', 'LR': '3e-4', 'NO_BIAS': True, 'NO_NORM': True, 'CLIP_GRAD_NORM': 10.0,
                        'SKIP_NONFINITE': True}
    cfg['LR_SCHEDULER'] = {'TYPE': 'MultiStepLR', 'MILESTONES': [60, 90, 110], 'GAMMA': 0.1, 'IS_WARMUP': False,
                           'WARMUP_EPOCH': 0, 'MULTIPLIER': 1.0}
    cfg['TRAIN'] = {'IMGSIZE': 160, 'MAX_EPOCHS': 1, 'ACCUMULATION_STEPS': 1}
    torch.manual_seed(0)
    m = YOLOv4(recipe.MODEL_CFG, device=dev).to(dev).train()
    ddp = BucketedDDP(m)
    opt = build_optimizer(cfg, m)
    ema = ModelEMA(m)
    crit = YOLOLoss(recipe.MODEL_CFG, 0.7, device=dev)
    x = recipe.randn((4, 3, 160, 160), 80).to(dev)
    target = {'padded_labels': recipe.synth_labels(4, 160, 81)}
    losses = []
    for step in (1, 2, 3):
        ddp.zero_grad()
        loss = crit(ddp(x), target)
        loss.backward()
        ddp.finish_backward()
        if step == 3:
            p_before = [p.detach().clone(memory_format=KEEP) for p in m.parameters()]
            e_before = [e.clone(memory_format=KEEP) for e in ema.ema.values() if e.is_floating_point()]
            m.head.yolo2[1].conv.bias.grad[17] = float('inf')
        opt.step()
        ema.update(m, opt.guard)
        losses.append(float(loss.detach()))
        st = opt.guard_state()
        print(f'step {step}: loss {losses[-1]:.4f} guard {st}')
        assert st['applied'] is (step != 3) and st['skipped'] == (1 if step == 3 else 0)
        if step != 3:
            assert math.isfinite(st['total_norm']) and 0.0 < st['coef'] <= 1.0
    assert_same_bits(list(m.parameters()), p_before, 'parameters across the skipped step')
    assert_same_bits([e for e in ema.ema.values() if e.is_floating_point()], e_before, 'EMA across the skipped step')
    del p_before
    ddp.zero_grad()                    # train_step clears the gradients AFTER its step; the loop above did so before
    for i in range(3):
        loss = train_step(cfg, ddp, crit, opt, x, target, None, i, None, 0, ema)
        losses.append(float(loss.detach()))
    st = opt.guard_state()
    print(f'losses {losses} guard {st}')
    assert all(math.isfinite(v) for v in losses), losses
    assert st['skipped'] == 1 and st['applied'] is True and ema.updates == 6
    assert opt.launches == 18
    assert not all(bits_equal(a, b) for a, b in zip((e for e in ema.ema.values() if e.is_floating_point()), e_before))
    for p in m.parameters():
        assert bool(torch.isfinite(p).all())
    live_w = m.backbone.stem.conv.weight.detach().clone(memory_format=KEEP)
    avg_w = ema.ema['backbone.stem.conv.weight'].clone(memory_format=KEEP)
    m.eval()
    with ema.applied_to(m), torch.no_grad():
        assert bits_equal(m.backbone.stem.conv.weight, avg_w) and bits_equal(ema.ema['backbone.stem.conv.weight'], live_w)
        out = m(x)
    assert bool(torch.isfinite(out).all())
    assert bits_equal(m.backbone.stem.conv.weight, live_w)


# ------------------------------------------------------------------ 9. resources
def test_optimizer_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'optim.hip'), ('-ffp-contract=off',))
    names = [r['name'].split('(')[0] for r in rows]
    for k in ('grad_sumsq_kernel', 'grad_guard_kernel', 'ema_kernel', 'void multi_tensor_kernel<true, true>',
              'void multi_tensor_kernel<false, true>', 'void multi_tensor_kernel<true, false>',
              'void multi_tensor_kernel<false, false>'):
        assert k in names, (k, names)
    bad = [(n, r['scratch'], r['vgpr_spill']) for n, r in zip(names, rows) if r['scratch'] != 0 or r['vgpr_spill'] != 0]
    assert not bad, bad
