# -*- coding: utf-8 -*-
"""Cases, fp64 references and acceptance rules for the classifier kernels of csrc/classifier.hip (global average pool,
linear, label-smoothed cross-entropy, top-k), shared by tests/test_classifier_cases.py (CPU: every case reaches the branch
it is named for, torch's own fp32 results pass every rule) and tests/test_gpu_classifier.py (the kernels, through the
C ABI).  Nothing here imports the product package or needs a GPU.

Every bound comes from the arithmetic, not from what the kernels give:
  pool     a sum of HW fp32 terms in any order, then one division: |err| <= (HW + 1) u mean_p|x|, u = 2^-24;
           backward is one division: relative 2 u.
  linear   an fp32 sum of L products in any order, plus the bias add: |err| <= (L + 2) u (sum |a||b| + |bias|).
  CE       delta_b = (N + 16) u (max_j|z_j| + ln N + 1) per row (N rounded summands, the rounding of z - m scaled by its
           size, a few ulp of exp / log); the mean of the delta_b for the mean; for the gradient
           (delta_b p_j + 4 u (p_j + q_j)) |gscale| / counted + 2^-126, p the fp64 softmax, q the smoothed target.
  top-k    integers: exact.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SENT = 0x7fa5c3e1                        # a NaN bit pattern no kernel produces: pad columns and output pre-fill
IGNORE = -100
SMOOTHING = 0.1


def sentinel(shape):
    return np.full(shape, SENT, np.uint32).view(np.float32)


def is_sentinel(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == SENT


def rng_normal(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


# ------------------------------------------------------------------ host-side dispatch of the launchers, restated
THREADS, TILE, STEP = 256, 64, 32


def pool_path(C, ld_in, ld_out, aligned=True):
    """'vec4' when channels, both pitches and both base addresses allow 16-byte accesses, else 'scalar'
    (y4_avgpool_global_fwd_f32 and _bwd_f32 decide alike)."""
    return 'vec4' if (C % 4 == 0 and ld_in % 4 == 0 and ld_out % 4 == 0 and aligned) else 'scalar'


def pool_fwd_grid(B, C, path):
    """(channel blocks, images): 64 lanes of 4 or 1 channels per block, 4 pixel groups each"""
    per = 64 * (4 if path == 'vec4' else 1)
    return (-(-C // per), B)


def pool_bwd_blocks(B, HW, C, path):
    """grid-stride sweep: one thread per 4 or 1 channels, at most 8192 blocks"""
    total = B * HW * (C // 4 if path == 'vec4' else C)
    return min(-(-total // THREADS), 8192)


def gemm_grid(I, J, R):
    """(tiles along j, tiles along i, LDS stages) of one 64 x 64-tile product over a reduction of length R"""
    return (-(-J // TILE), -(-I // TILE), -(-R // STEP))


def linear_grids(M, K, N):
    """the three products of a linear layer: forward [M,N] over K, dx [M,K] over N, dw [N,K] over M"""
    return {'fwd': gemm_grid(M, N, K), 'dx': gemm_grid(M, K, N), 'dw': gemm_grid(N, K, M), 'dbias': -(-N // THREADS)}


def row_sweeps(N):
    """CE / top-k: one 256-thread block per row; the number of strided steps a thread takes over the row"""
    return -(-N // THREADS)


# ------------------------------------------------------------------ pool
#             (B, HW,  C,   ld)
POOL_CASES = [(1, 1, 1, 1), (2, 4, 1024, 1024), (3, 9, 1024, 1024), (2, 5, 37, 37), (2, 64, 40, 48), (1, 361, 32, 32)]
POOL_BRANCH = {(1, 1, 1, 1): 'scalar', (2, 4, 1024, 1024): 'vec4', (3, 9, 1024, 1024): 'vec4', (2, 5, 37, 37): 'scalar',
               (2, 64, 40, 48): 'vec4', (1, 361, 32, 32): 'vec4'}


@functools.lru_cache(maxsize=None)
def pool_case(case):
    """x [B,HW,ld] (pad columns hold the sentinel), dy [B,ld] likewise, and the fp64 results on the valid columns"""
    B, HW, C, ld = case
    x = sentinel((B, HW, ld))
    x[..., :C] = rng_normal((B, HW, C), 100 + HW + C) + 0.25
    dy = sentinel((B, ld))
    dy[:, :C] = rng_normal((B, C), 200 + HW + C)
    x64 = x[..., :C].astype(np.float64)
    out = dict(x=x, dy=dy, y64=x64.mean(1), absmean=np.abs(x64).mean(1),
               dx64=np.repeat(dy[:, None, :C].astype(np.float64) / HW, HW, 1))
    for a in out.values():
        a.setflags(write=False)
    return out


def pool_fwd_accept(got, y64, absmean, HW):
    err = np.abs(np.asarray(got, np.float64) - y64)
    bound = (HW + 1) * U * absmean
    return err <= bound, float((err / np.maximum(bound, 1e-300)).max())


def pool_bwd_accept(got, dx64):
    err = np.abs(np.asarray(got, np.float64) - dx64)
    bound = 2.0 ** -23 * np.abs(dx64)
    return err <= bound, float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------ linear
#               (M,  K,    N,   ldx,  ldy)
LINEAR_CASES = [(1, 1, 1, 1, 1), (3, 5, 7, 5, 7), (2, 1024, 37, 1024, 37), (5, 1024, 1000, 1024, 1000),
                (130, 96, 257, 96, 257), (6, 70, 33, 77, 40)]
# what each case is named for: the tiles of its three products (linear_grids)
LINEAR_BRANCH = {
    (1, 1, 1, 1, 1): {'fwd': (1, 1, 1), 'dx': (1, 1, 1), 'dw': (1, 1, 1), 'dbias': 1},
    (3, 5, 7, 5, 7): {'fwd': (1, 1, 1), 'dx': (1, 1, 1), 'dw': (1, 1, 1), 'dbias': 1},
    (2, 1024, 37, 1024, 37): {'fwd': (1, 1, 32), 'dx': (16, 1, 2), 'dw': (16, 1, 1), 'dbias': 1},
    (5, 1024, 1000, 1024, 1000): {'fwd': (16, 1, 32), 'dx': (16, 1, 32), 'dw': (16, 16, 1), 'dbias': 4},
    (130, 96, 257, 96, 257): {'fwd': (5, 3, 3), 'dx': (2, 3, 9), 'dw': (2, 5, 5), 'dbias': 2},
    (6, 70, 33, 77, 40): {'fwd': (1, 1, 3), 'dx': (2, 1, 2), 'dw': (2, 1, 1), 'dbias': 1},
}


@functools.lru_cache(maxsize=None)
def linear_case(case):
    """x [M,ldx] and dy [M,ldy] with sentinel pads, w [N,K], bias [N]; fp64 results and the |a||b| sums of each output"""
    M, K, N, ldx, ldy = case
    s = 300 + M + K + N
    x = sentinel((M, ldx))
    x[:, :K] = rng_normal((M, K), s)
    dy = sentinel((M, ldy))
    dy[:, :N] = rng_normal((M, N), s + 1)
    w = rng_normal((N, K), s + 2, 1.0 / math.sqrt(K))
    bias = rng_normal((N,), s + 3, 0.5)
    x64, d64, w64, b64 = x[:, :K].astype(np.float64), dy[:, :N].astype(np.float64), w.astype(np.float64), bias.astype(np.float64)
    out = dict(x=x, dy=dy, w=w, bias=bias,
               y64=x64 @ w64.T + b64, y_abs=np.abs(x64) @ np.abs(w64).T + np.abs(b64),
               y64_nobias=x64 @ w64.T, y_abs_nobias=np.abs(x64) @ np.abs(w64).T,
               dx64=d64 @ w64, dx_abs=np.abs(d64) @ np.abs(w64),
               dw64=d64.T @ x64, dw_abs=np.abs(d64).T @ np.abs(x64),
               db64=d64.sum(0), db_abs=np.abs(d64).sum(0))
    for a in out.values():
        a.setflags(write=False)
    return out


def linear_accept(got, ref64, absprod, L):
    err = np.abs(np.asarray(got, np.float64) - ref64)
    bound = (L + 2) * U * absprod
    return err <= bound, float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------ cross-entropy
CE_NS = [1, 2, 37, 1000, 1003]
CE_B = 6
CE_GSCALE = 0.75


@functools.lru_cache(maxsize=None)
def ce_case(N, all_ignored=False):
    """logits [6,N] ~ 4 N(0,1) with a +80 planted in row 0, a -90 in row 1, row 2 at 30 +- 1e-3 and row 3 ignored; labels;
    the fp64 row losses, mean, softmax p, smoothed target q and gradient for upstream CE_GSCALE."""
    r = np.random.RandomState(400 + N)
    z = (4.0 * r.standard_normal((CE_B, N))).astype(np.float32)
    z[0, r.randint(N)] = 80.0
    z[1, r.randint(N)] = -90.0
    z[2] = (30.0 + 1e-3 * r.uniform(-1, 1, N)).astype(np.float32)
    t = r.randint(0, N, CE_B).astype(np.int64)
    t[3] = IGNORE
    if all_ignored:
        t[:] = IGNORE
    return ce_reference(z, t)


def ce_reference(z, t, eps=SMOOTHING, gscale=CE_GSCALE):
    z = np.asarray(z, np.float32)
    B, N = z.shape
    z64 = z.astype(np.float64)
    m = z64.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z64 - m).sum(1))
    p = np.exp(z64 - lse[:, None])
    counted = t != IGNORE
    q = np.full((B, N), eps / N)
    for b in range(B):
        if counted[b]:
            q[b, t[b]] += 1.0 - eps
    zt = np.array([z64[b, t[b]] if counted[b] else 0.0 for b in range(B)])
    row = np.where(counted, lse - (1.0 - eps) * zt - eps * z64.mean(1), 0.0)
    n = int(counted.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.float64(row[counted].sum()) / np.float64(n)
    grad = np.where(counted[:, None], gscale / max(n, 1) * (p - q), 0.0)
    delta = (N + 16) * U * (np.abs(z64).max(1) + math.log(N) + 1.0)
    out = dict(z=z, t=t, row64=row, mean64=mean, counted=n, p=p, q=q, grad64=grad, delta=delta, mask=counted)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def ce_row_accept(got, ref):
    err = np.abs(np.asarray(got, np.float64) - ref['row64'])
    ok = np.where(ref['mask'], err <= ref['delta'], np.asarray(got) == 0.0)
    return ok, float((err / ref['delta'])[ref['mask']].max()) if ref['mask'].any() else 0.0


def ce_mean_accept(got, ref):
    if ref['counted'] == 0:
        return bool(np.isnan(got)), 0.0
    bound = float(ref['delta'][ref['mask']].mean())
    err = abs(float(got) - float(ref['mean64']))
    return err <= bound, err / bound


def ce_grad_accept(got, ref, gscale=CE_GSCALE):
    got = np.asarray(got, np.float64)
    if ref['counted'] == 0:
        return got == 0.0, 0.0
    k = abs(gscale) / ref['counted']
    bound = (ref['delta'][:, None] * ref['p'] + 2.0 ** -22 * (ref['p'] + ref['q'])) * k + 2.0 ** -126
    err = np.abs(got - ref['grad64'])
    ok = np.where(ref['mask'][:, None], err <= bound, got == 0.0)
    return ok, float((err / bound)[ref['mask']].max())


# ------------------------------------------------------------------ top-k
TOPK_NS = [1, 5, 37, 1000]
TOPK_B = 7
TOPK_KS = [(1, 5), (1,)]


def rank_rule(z, t):
    """rank_b = #{j: z_j > z_t} + #{j < t: z_j == z_t}; N for a row with a NaN or a label outside [0, N)"""
    z = np.asarray(z, np.float32)
    B, N = z.shape
    out = np.empty(B, np.int32)
    for b in range(B):
        tb = int(t[b])
        if not 0 <= tb < N or np.isnan(z[b]).any():
            out[b] = N
        else:
            out[b] = int((z[b] > z[b, tb]).sum()) + int((z[b, :tb] == z[b, tb]).sum())
    return out


def correct_rule(rank, ks):
    return np.array([int((rank < k).sum()) for k in ks], np.int32)


@functools.lru_cache(maxsize=None)
def topk_case(N):
    """logits [7,N], labels: row 0 ties its label's (top) value at a LOWER index (rank 1), row 1 at a HIGHER one (rank 0),
    row 2 holds a NaN, row 3 is labelled -100, the others are random; rows 4.. of the wide cases put the label 3rd and 7th."""
    r = np.random.RandomState(500 + N)
    z = r.standard_normal((TOPK_B, N)).astype(np.float32)
    t = r.randint(0, N, TOPK_B).astype(np.int64)
    if N >= 5:
        t[0], t[1] = 3, 1
        z[0, 3] = z[0, 1] = 9.0
        z[1, 1] = z[1, 3] = 9.0
    z[2, r.randint(N)] = np.nan
    t[3] = IGNORE
    if N >= 37:
        for b, place in ((4, 2), (5, 6)):
            order = np.argsort(-z[b], kind='stable')
            t[b] = order[place]
    rank = rank_rule(z, t)
    z.setflags(write=False)
    t.setflags(write=False)
    return dict(z=z, t=t, rank=rank)


# ------------------------------------------------------------------ whole model
MODEL_CLASSES = 37
#              (input shape,      labels)
MODEL_STEPS = [((2, 3, 64, 64), (3, 36)), ((3, 3, 96, 96), (0, 17, 36))]
MODEL_SEED = 7
GRAD_KEYS = ('classifier.weight', 'classifier.bias', 'backbone.stem.conv.weight')
STAT_KEYS = ('backbone.stem.norm.running_mean', 'backbone.stem.norm.running_var',
             'backbone.stage5.transition.norm.running_mean', 'backbone.stage5.transition.norm.running_var')


GOLDEN_THREADS = 8


def cpu_fingerprint():
    """sha256 over the fp32 bits of the primitives the composed oracle is made of -- 3x3, 1x1 and stride-2 convolutions
    with their backward, training-mode batch norm, Mish, pool, linear, cross-entropy -- on seeded inputs.  Two machines
    that give the same digest (at the same thread count) round fp32 sums alike; tests/golden/classifier.npz records the
    digest of the machine that wrote it, and only there is 'bit for bit' against the fixture a statement about the oracle
    rather than about the CPU's vector ISA (tests/test_oracle_golden.py has the history)."""
    import hashlib
    g = torch.Generator(device='cpu')
    g.manual_seed(99)
    h = hashlib.sha256()
    x = torch.randn((2, 32, 24, 24), generator=g).requires_grad_(True)
    ws = [torch.randn(shape, generator=g).mul_(0.1).requires_grad_(True) for shape in ((64, 32, 3, 3), (128, 64, 1, 1), (128, 128, 3, 3))]
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    wl = torch.randn((37, 128), generator=g).mul_(0.1).requires_grad_(True)
    y = F.conv2d(x, ws[0], padding=1)
    y = F.conv2d(y, ws[1])
    y = F.conv2d(y, ws[2], stride=2, padding=1)
    y = F.batch_norm(y, torch.zeros(128), torch.ones(128), gamma, beta, training=True, momentum=0.1, eps=1e-5)
    y = y * torch.tanh(F.softplus(y))
    z = F.linear(F.adaptive_avg_pool2d(y, (1, 1)).reshape(2, 128), wl)
    loss = F.cross_entropy(z, torch.tensor([3, 36]), label_smoothing=SMOOTHING)
    loss.backward()
    for t in [z, loss, x.grad, wl.grad] + [w.grad for w in ws]:
        h.update(t.detach().contiguous().numpy().tobytes())
    # the two ends of the backbone: the 3-channel stem on a large map, a 512 -> 1024 stride-2 conv on a 4 x 4 one
    for cin, cout, hw, st in ((3, 32, 64, 1), (512, 1024, 4, 2)):
        xe = torch.randn((2, cin, hw, hw), generator=g).requires_grad_(True)
        we = torch.randn((cout, cin, 3, 3), generator=g).mul_(0.05).requires_grad_(True)
        ye = F.conv2d(xe, we, stride=st, padding=1)
        (ye * ye).sum().backward()
        for t in (ye, xe.grad, we.grad):
            h.update(t.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def fill_classifier_(sd, seed):
    """recipe.fill_state_dict_ on the backbone.* keys; classifier.weight ~ N(0, 1/1024), classifier.bias ~ N(0, 0.1^2)"""
    import recipe
    recipe.fill_state_dict_({k: v for k, v in sd.items() if k.startswith('backbone.')}, seed)
    g = torch.Generator(device='cpu')
    g.manual_seed(seed + 1000)
    w, b = sd['classifier.weight'], sd['classifier.bias']
    w.copy_(torch.randn(w.shape, generator=g, dtype=torch.float32) / 32.0)
    b.copy_(torch.randn(b.shape, generator=g, dtype=torch.float32) * 0.1)


def model_input(step):
    import recipe
    shape, labels = MODEL_STEPS[step]
    return recipe.randn(shape, 11 + step), torch.tensor(labels, dtype=torch.int64)


def oracle_logits(net, x):
    """the composed oracle: RefNet.backbone(x)[2] -> adaptive_avg_pool2d -> linear"""
    f = F.adaptive_avg_pool2d(net.backbone(x)[2], (1, 1))
    return F.linear(f.reshape(f.shape[:2]), net.p['classifier.weight'], net.p['classifier.bias'])


def oracle_train_step(sd, x, target, dtype=torch.float32):
    """One train step of the composed oracle in `dtype` on a copy of sd: (net, logits, loss); gradients are left in
    net.p[k].grad, the updated running statistics in net.p."""
    from oracle import network as NW
    net = NW.RefNet({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()})
    net.training = True
    logits = oracle_logits(net, x.to(dtype))
    loss = F.cross_entropy(logits, target, label_smoothing=SMOOTHING)
    loss.backward()
    return net, logits.detach(), loss.detach()


def oracle_eval(sd, x, dtype=torch.float32):
    from oracle import network as NW
    net = NW.RefNet({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()})
    net.training = False
    with torch.no_grad():
        return oracle_logits(net, x.to(dtype))
