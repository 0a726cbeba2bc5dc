# -*- coding: utf-8 -*-
"""References, case lists and acceptance criteria for the direct tests of the glue kernels of csrc/pointwise.hip -- channel
copy, add, the stride-1 max pool, the two nearest upsamples, the flat activations -- and of the operand-maximum kernels of
csrc/conv_f16x2.hip (tests/test_glue_cases.py checks this module on the CPU, tests/test_gpu_glue_edges.py feeds it to the
kernels).  Numpy only; what tests/bn_cases.py already defines is imported from there.

Four parts:
  * a mirror of the HOST dispatch (grid_for, vec_ok, the amax kernel choice and its grid, the return code of every
    refused argument set): it lets a case STATE which branch it reaches; it is never the reference of a value;
  * references written from the definitions (fp64 where anything is summed or transcendental);
  * acceptance functions, all elementwise;
  * the case lists.

Acceptance, u = 2^-24 (unit roundoff of fp32), TINY = 2^-126:
  bit-exact (uint32 compare, NaN payloads included): copy; add against numpy's fp32 a + b (one IEEE addition has one
      correct result); max pool values and int8 codes; both upsample forwards; linear / relu / leaky forward (leaky is ONE
      fp32 multiply by float32(0.1)); dx = dy * act'(x) of linear / relu / leaky (one fp32 multiply by 1, 0 or float32(0.1));
      amax and merge words.
  fixed-order fp32 sums against the fp64 sum of the same addends, k addends (an accumulated old value counts as one):
      |got - ref| <= (k - 1) u sum|addends| + TINY;   k <= 1: no addition rounds, got == ref exactly
      (a source pixel without destinations / a pool input no output selected is exactly 0, or exactly the old value).
      k = 4 for upsample2x_bwd, the block size for upsample_nearest_bwd, <= ks^2 + 1 for maxpool_bwd.
  mish forward:   |got - mish(x)| <= (min(|x|, 20) + MISH_CONST) 2^-23 |mish(x)| + TINY
  mish backward:  |got - dy mish'(x)| <= (min(|x|, 20) + MISH_GRAD_CONST) 2^-23 A |dy| + u |dy mish'(x)| + TINY,
      A = |t| + |x (1 - t^2) sigmoid(x)| as bn_cases.mish_grad64(parts=True) returns it.
      MISH_CONST and MISH_GRAD_CONST are the allowances of the BatchNorm sweeps (bn_cases.py).  The cap at 20: the kernels
      clamp the exponent's argument there; the argument's rounding error no longer grows with |x| above it, and the true
      tanh(softplus x) is 1 to within 1e-15, the true derivative 1 to within 4e-16 x e^(-2 (x - 20)): for
      20 <= x <= FLT_MAX the bound demands mish(x) = x and mish'(x) = 1 to (20 + const) 2^-23.
  NaN / infinity: where the reference is NaN the result must be NaN, where it is +-inf the result must be that infinity.
      NaN in -> NaN out for everything that multiplies by x or dy; relu'(NaN) = 0 and leaky'(NaN) = 0.1 (NaN > 0 is false).
      The fp64 formulas are evaluated as numpy does: mish(-inf) = -inf * 0 = NaN and mish'(-inf) = NaN, as torch has them.
      At +inf the derivative's formula reads inf * 0 although its limit is 1; the reference takes the limit (the rule
      "mish'(x) = 1 for x >= 20" has no upper end), so mish'(+inf) = 1 and dy = 0 there gives dx = 0.

Nearest upsample, fp32 map against the exact rational floor(d in / out): a search over in, out <= 64 (fp32_map_differs) finds
15 pairs where they differ; the first is 14 -> 46, where d = 23 maps to fl32(23 * fl32(14 / 46)) = 6.99999.. -> 6 although
23 * 14 / 46 = 7 exactly.  ROUNDING_PAIR holds it (tests/test_glue_cases.py repeats the search) and NEAREST_SIZES has it.
"""
import numpy as np

from bn_cases import (ACT_LEAKY, ACT_LINEAR, ACT_MISH, ACT_NAMES, ACT_RELU, ACTS, ERR_NULL, ERR_SHAPE, F32, F64,  # noqa: F401
                      MISH_CONST, MISH_GRAD_CONST, SENT, TINY, U, act64, act_grad64, is_sentinel, judge, mish64, mish_grad64,
                      pad_rows, sentinel)

FLT_MAX = float(np.finfo(F32).max)
OK = 0

# ------------------------------------------------------------------------------------------ host dispatch mirror
PW_THREADS = 256
GRID_CAP = 4096                          # grid_for's default cap
AMAX_CAP = 1024                          # blocks of the amax kernels; each thread takes 4 items per lap at full width
AMAX_ITEMS_PER_BLOCK = 1024


def grid_for(total, cap=GRID_CAP):
    return int(max(min(-(-total // PW_THREADS), cap), 1))


def laps(total, cap=GRID_CAP):
    """trips of the busiest thread through the grid-stride loop"""
    return -(-total // (grid_for(total, cap) * PW_THREADS))


def vec_ok(addr, ld, C):
    """addr: byte address, 0 = NULL"""
    return bool(addr) and addr % 16 == 0 and ld % 4 == 0 and C % 4 == 0 and ld >= C and C > 0


def rc_rows(ptrs, M):
    """copy / add: ptrs = [(addr, ld, C), ...]"""
    return OK if all(vec_ok(*p) for p in ptrs) and M > 0 else ERR_SHAPE


def rc_image(ptrs, dims):
    """upsample2x: every pitch operand vec_ok, every dimension positive"""
    return OK if all(vec_ok(*p) for p in ptrs) and all(d > 0 for d in dims) else ERR_SHAPE


def rc_maxpool_fwd(ptrs, dims, ks):
    if rc_image(ptrs, dims):
        return ERR_SHAPE
    return OK if ks >= 1 and ks % 2 == 1 and ks <= 11 else ERR_SHAPE


def rc_maxpool_bwd(idx_addr, ptrs, dims, ks):
    if not idx_addr:
        return ERR_NULL
    return rc_maxpool_fwd(ptrs, dims, ks)


def rc_nearest(ptrs, B, H, W, Ho, Wo, integer_factor):
    if rc_image(ptrs, (B, H, W, Ho, Wo)):
        return ERR_SHAPE
    if integer_factor and (Ho % H or Wo % W):
        return ERR_SHAPE
    return OK


def rc_act(addrs, n, act):
    if not all(addrs):
        return ERR_NULL
    return OK if n > 0 and 0 <= act <= 3 else ERR_SHAPE


def rc_amax(x_addr, word_addr, ld, M, C):
    if not x_addr or not word_addr:
        return ERR_NULL
    return ERR_SHAPE if M < 0 or C <= 0 or ld < C else OK


def rc_merge(dst_addr, src_addr):
    return OK if dst_addr and src_addr else ERR_NULL


def amax_plan(addr, ld, M, C):
    """(kernel, blocks, laps): 'none' (M = 0: the word is only zeroed), 'vector' (16-B loads: rows start on 16-B boundaries
    and a row's last vector stays inside its pitch) or 'strided' (scalar loads)"""
    if M <= 0 or C <= 0:
        return 'none', 0, 0
    if ld % 4 == 0 and addr % 16 == 0 and (C + 3) // 4 * 4 <= ld:
        kind, total = 'vector', M * ((C + 3) // 4)
    else:
        kind, total = 'strided', M * C
    blocks = min(-(-total // AMAX_ITEMS_PER_BLOCK), AMAX_CAP)
    return kind, blocks, -(-total // (blocks * PW_THREADS))


def act_plan(n, aligned):
    """(grid, laps of the vector body, elements of the scalar loop): the flat activation kernels take 16-B vectors when
    every pointer is 16-B aligned and finish n % 4 elements one by one; otherwise the whole tensor goes one by one"""
    grid = grid_for((n + 3) // 4)
    threads = grid * PW_THREADS
    if aligned:
        return grid, -(-(n // 4) // threads), n % 4
    return grid, 0, n


# ------------------------------------------------------------------------------------------ small helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, ref):
    """elementwise: equal as 32-bit words"""
    return bits(got) == bits(ref)


def f32_from_bits(word, shape=()):
    return np.full(shape, word, dtype=np.uint32).view(F32)


NAN_A, NAN_B = 0x7fc00001, 0xffc00002          # two quiet NaNs told apart by sign and payload


def accept_close(got, ref, bound):
    """(ok, used) as bn_cases.judge, with the NaN / infinity rules: a NaN reference wants a NaN, an infinite one itself"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    nan_r, inf_r = np.isnan(ref), np.isinf(ref)
    with np.errstate(invalid='ignore'):
        ok, used = judge(got, np.where(nan_r | inf_r, 0.0, ref), np.where(nan_r | inf_r, 0.0, bound))
    ok = np.where(nan_r, np.isnan(got), np.where(inf_r, got == ref, ok))
    used = np.where(nan_r | inf_r, np.where(ok, 0.0, np.inf), used)
    return ok, used


def sum_bound(sum_abs, k):
    """(k - 1) u sum|addends|, + TINY from two addends on"""
    k = np.asarray(k, F64)
    return np.where(k <= 1, 0.0, np.maximum(k - 1.0, 0.0) * U * np.asarray(sum_abs, F64) + TINY)


def sum_accept(got, ref, sum_abs, k):
    """fixed-order fp32 sum of k addends against its fp64 value: (k - 1) u sum|addends| + TINY; k <= 1: exact"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    bound = np.broadcast_to(sum_bound(sum_abs, k), ref.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(got - ref)
        ok = (err <= bound) & ~np.isnan(got)
        used = np.where(err == 0, 0.0, err / bound)
    return ok, np.where(np.isnan(got), np.inf, used)


# ------------------------------------------------------------------------------------------ max pool
def maxpool_ref(x, ks):
    """nn.MaxPool2d(ks, 1, ks // 2) on x [B, H, W, C] by ATen's rule: the window is scanned row-major and
    (val > max) || isnan(val) replaces the running maximum, which starts at -inf with the code of the first valid tap:
    the first of equal maxima wins, the last NaN wins, a window of -inf keeps -inf and its first tap.
    Returns (y fp32 with x's bit patterns, code int8 = r * ks + q of the window offset)."""
    x = np.asarray(x, dtype=F32)
    B, H, W, C = x.shape
    p = ks // 2
    best = np.full(x.shape, -np.inf, dtype=F32)
    code = np.full(x.shape, -1, dtype=np.int8)
    for r in range(ks):
        for q in range(ks):
            dh, dw = r - p, q - p
            h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
            if h0 >= h1 or w0 >= w1:
                continue
            v = x[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
            b, c = best[:, h0:h1, w0:w1], code[:, h0:h1, w0:w1]
            c[c < 0] = r * ks + q
            with np.errstate(invalid='ignore'):
                take = (v > b) | np.isnan(v)
            b[take] = v[take]
            c[take] = r * ks + q
    return best, code


def code_to_flat(code, ks):
    """int8 window codes -> torch's flat input index h * W + w per output element"""
    B, H, W, C = code.shape
    p = ks // 2
    c = code.astype(np.int64)
    h = np.arange(H).reshape(1, H, 1, 1) + c // ks - p
    w = np.arange(W).reshape(1, 1, W, 1) + c % ks - p
    return h * W + w


def maxpool_bwd_ref(dy, code, ks, old=None):
    """dx[p] = sum of dy[o] over the outputs o whose code points at p (+ old[p]) in fp64 -> (dx, sum|addends|, k)"""
    dy = np.asarray(dy, F64)
    B, H, W, C = dy.shape
    p = ks // 2
    dx, sa, k = np.zeros(dy.shape), np.zeros(dy.shape), np.zeros(dy.shape)
    for r in range(ks):
        for q in range(ks):
            dh, dw = r - p, q - p
            h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
            if h0 >= h1 or w0 >= w1:
                continue
            sel = code[:, h0:h1, w0:w1] == r * ks + q
            g = np.where(sel, dy[:, h0:h1, w0:w1], 0.0)
            dx[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += g
            sa[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += np.abs(g)
            k[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += sel
    if old is not None:
        old = np.asarray(old, F64)
        dx, sa, k = dx + old, sa + np.abs(old), k + 1
    return dx, sa, k


POOL_LEVELS = np.array([-2.0, -0.5, 0.0, 0.25, 1.0], dtype=F32)


def make_pool_input(B, H, W, C, seed):
    """x [B, H, W, C]: five levels, so most windows hold ties; image 0 carries, in channels 1, 2, 3: a ks x ks corner of
    -inf (a whole window of -inf for every ks <= 11), two different NaNs one row and column apart, a +inf in the last
    pixel; channel 0 and the other images stay finite."""
    rng = np.random.RandomState(seed)
    x = POOL_LEVELS[rng.randint(0, len(POOL_LEVELS), (B, H, W, C))]
    x[0, :11, :11, 1] = -np.inf
    x[0, 0, 0, 2] = f32_from_bits(NAN_A)
    x[0, min(1, H - 1), min(1, W - 1), 2] = f32_from_bits(NAN_B)
    x[0, H - 1, W - 1, 3] = np.inf
    if H * W > 4:
        x[0, H // 2, W // 2, 3] = -np.inf
    return x


def make_pool_finite(B, H, W, C, seed):
    return POOL_LEVELS[np.random.RandomState(seed).randint(0, len(POOL_LEVELS), (B, H, W, C))]


# ------------------------------------------------------------------------------------------ upsample
def upsample2x_ref(x):
    return np.repeat(np.repeat(np.asarray(x, F32), 2, axis=1), 2, axis=2)


def upsample2x_bwd_ref(dy):
    """(dx, sum|addends|) in fp64: the 2 x 2 block sums; k = 4"""
    dy = np.asarray(dy, F64)
    B, H2, W2, C = dy.shape
    v = dy.reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    return v.sum(axis=(2, 4)), np.abs(v).sum(axis=(2, 4))


def nearest_index(n_in, n_out, integer_factor=False):
    """source index of every destination index.  integer_factor: d / f.  Otherwise ATen's
    nearest_neighbor_compute_source_index in fp32: min(floor(fl32(d * fl32(in / out))), in - 1)."""
    d = np.arange(n_out)
    if integer_factor:
        assert n_out % n_in == 0
        return d // (n_out // n_in)
    scale = F32(n_in) / F32(n_out)
    s = np.floor(d.astype(F32) * scale).astype(np.int64)
    return np.minimum(s, n_in - 1)


def nearest_index_exact(n_in, n_out):
    return np.minimum(np.arange(n_out) * n_in // n_out, n_in - 1)


def fp32_map_differs(limit=64):
    """all (in, out) <= limit where the fp32 map differs from floor(d in / out)"""
    return [(i, o) for i in range(1, limit + 1) for o in range(1, limit + 1)
            if not np.array_equal(nearest_index(i, o), nearest_index_exact(i, o))]


def nearest_ref(x, Ho, Wo, integer_factor=False):
    x = np.asarray(x, F32)
    hs, ws = nearest_index(x.shape[1], Ho, integer_factor), nearest_index(x.shape[2], Wo, integer_factor)
    return x[:, hs][:, :, ws]


def nearest_bwd_ref(dy, H, W, integer_factor=False):
    """adjoint of nearest_ref in fp64: (dx, sum|addends|, k = size of the source pixel's destination block)"""
    dy = np.asarray(dy, F64)
    B, Ho, Wo, C = dy.shape
    hs, ws = nearest_index(H, Ho, integer_factor), nearest_index(W, Wo, integer_factor)
    out = []
    for v in (dy, np.abs(dy)):
        t = np.zeros((B, Ho, W, C))
        np.add.at(t, (slice(None), slice(None), ws), v)
        dx = np.zeros((B, H, W, C))
        np.add.at(dx, (slice(None), hs), t)
        out.append(dx)
    k = np.bincount(hs, minlength=H).reshape(1, H, 1, 1) * np.bincount(ws, minlength=W).reshape(1, 1, W, 1)
    return out[0], out[1], np.broadcast_to(k, out[0].shape)


# ------------------------------------------------------------------------------------------ activations
def act_f32(x, act):
    """linear / relu / leaky forward as the one fp32 operation they are (bit patterns of x kept where x passes through)"""
    x = np.asarray(x, F32)
    with np.errstate(invalid='ignore'):
        if act == ACT_LEAKY:
            return np.where(x > 0, x, x * F32(0.1)).astype(F32)
        if act == ACT_RELU:
            return np.where(x < 0, F32(0.0), x).astype(F32)
    assert act == ACT_LINEAR
    return x.copy()


def act_grad_f32(x, dy, act):
    """dx = dy * act'(x) of linear / relu / leaky: one fp32 multiply"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    with np.errstate(invalid='ignore'):
        if act == ACT_LEAKY:
            d = np.where(x > 0, F32(1.0), F32(0.1))
        elif act == ACT_RELU:
            d = np.where(x > 0, F32(1.0), F32(0.0))
        else:
            d = np.ones_like(x)
        return (dy * d.astype(F32)).astype(F32)


def act_ref64(x, act):
    with np.errstate(invalid='ignore', over='ignore'):
        return act64(np.asarray(x, F64), act)


def mish_grad_ref64(x):
    """(mish'(x), A) in fp64; at +inf the limit 1 (module docstring)"""
    x = np.asarray(x, F64)
    with np.errstate(invalid='ignore', over='ignore'):
        d, A = mish_grad64(x, parts=True)
    top = np.isposinf(x)
    return np.where(top, 1.0, d), np.where(top, 1.0, A)


def act_grad_ref64(x, act):
    x = np.asarray(x, F64)
    if act == ACT_MISH:
        return mish_grad_ref64(x)[0]
    with np.errstate(invalid='ignore'):
        return act_grad64(x, act)


def mish_fwd_ref(x):
    """(mish(x), bound) in fp64"""
    x = np.asarray(x, F64)
    ref = act_ref64(x, ACT_MISH)
    with np.errstate(invalid='ignore'):
        return ref, (np.minimum(np.abs(x), 20.0) + MISH_CONST) * 2.0 ** -23 * np.abs(ref)


def mish_bwd_ref(x, dy):
    """(dy mish'(x), bound) in fp64"""
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    d, A = mish_grad_ref64(x)
    with np.errstate(invalid='ignore'):
        ref = dy * d
        return ref, (np.minimum(np.abs(x), 20.0) + MISH_GRAD_CONST) * 2.0 ** -23 * A * np.abs(dy) + U * np.abs(ref)


def mish_fwd_accept(got, x):
    return accept_close(got, *mish_fwd_ref(x))


def mish_bwd_accept(got, x, dy):
    return accept_close(got, *mish_bwd_ref(x, dy))


def act_fwd_accept(got, x, act):
    """(ok, used): mish by its bound, the others bit for bit (used = 0 or inf)"""
    if act == ACT_MISH:
        return mish_fwd_accept(got, x)
    ok = same_bits(got, act_f32(x, act))
    return ok, np.where(ok, 0.0, np.inf)


def act_bwd_accept(got, x, dy, act):
    if act == ACT_MISH:
        return mish_bwd_accept(got, x, dy)
    ok = same_bits(got, act_grad_f32(x, dy, act))
    return ok, np.where(ok, 0.0, np.inf)


_D = 2.0 ** -149
ACT_GRID = np.array([0.0, -0.0, _D, -_D, 2.0 ** -127, -2.0 ** -127, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, 19.9, -19.9, 20.0, -20.0,
                     20.1, -20.1, 50.0, -50.0, 88.0, -88.0, 104.0, -104.0, 1e10, 1e17, 1e22, FLT_MAX, -FLT_MAX,
                     np.inf, -np.inf, np.nan], dtype=F32)
ACT_LARGE_X = np.array([20.0, 20.1, 50.0, 88.0, 104.0, 1e10, 1e17, 1e22, FLT_MAX, np.inf], dtype=F32)


def make_act_input(n, seed):
    """(x, dy) of n elements: the grid (each point with dy = 1.5, the large-x points again with dy = 0), then a seeded
    N(0, 3) bulk with N(0, 1) gradients; a short tensor takes the head of that sequence rotated by its seed, so the small
    sizes together still see the whole grid"""
    rng = np.random.RandomState(seed)
    gx = np.concatenate([ACT_GRID, ACT_LARGE_X])
    gd = np.concatenate([np.full(ACT_GRID.size, 1.5, F32), np.zeros(ACT_LARGE_X.size, F32)])
    m = max(n, gx.size) - gx.size
    x = np.concatenate([gx, (rng.standard_normal(m) * 3.0).astype(F32)])
    dy = np.concatenate([gd, rng.standard_normal(m).astype(F32)])
    if n < gx.size:
        x, dy = np.roll(x, -seed * 5), np.roll(dy, -seed * 5)
    return x[:n].copy(), dy[:n].copy()


# ------------------------------------------------------------------------------------------ amax
def amax_ref(x, C):
    """x [M, ld] fp32: the integer maximum of the `& 0x7fffffff` bit patterns below 0x7f800000 over the first C channels"""
    b = bits(x)[:, :C] & 0x7fffffff
    b = b[b < 0x7f800000]
    return int(b.max()) if b.size else 0


def merge_ref(dst, src):
    return max(int(dst), int(src))


# ------------------------------------------------------------------------------------------ case lists
# C: (C / 4, what it is here for)
CHANNEL_TABLE = {4: (1, 'one vector per row'), 8: (2, 'power of two'), 12: (3, 'no power of two'), 20: (5, 'no power of two'),
                 36: (9, 'no power of two'), 64: (16, 'power of two')}
CHANNELS = tuple(CHANNEL_TABLE)
ROWS = (1, 2, 255, 257)


def pitches(C):
    """(pitch, column offset of the slice): dense rows; a channel slice in the middle of a buffer 8 wider, neighbours on
    both sides; a slice at the start of a buffer 4 wider"""
    return ((C, 0), (C + 8, 4), (C + 4, 0))


# one grid-stride case per kernel: total just above 4096 * 256 and no multiple of 256
BIG_ROWS = (12, 349527)                                  # (C, M) of copy / add: total = 3 M = 1048581
BIG_IMAGE = (1, 1027, 1023, 4)                           # (B, H, W, C) of the pool (ks = 3) and of upsample2x_bwd's dx
BIG_HALF = (1, 515, 511, 4)                              # upsample2x_fwd's x: 4 H W = 1052660 outputs
BIG_NEAREST_FWD = ((1, 515, 511, 4), (1031, 1021))       # x, (Ho, Wo): 1052651 outputs
BIG_NEAREST_BWD = ((1, 1027, 1023, 4), (1029, 1025))     # dx, (Ho, Wo) of dy
BIG_ACT = 4 * 4096 * 256 + 7
BIG_AMAX = ((1024 * 1024 + 5, 4, 4), (349527, 3, 3))     # (M, C, ld): vector kernel, strided kernel, both over 1024 blocks

POOL_KS = (1, 3, 5, 9, 11)
POOL_IMAGES = ((1, 1), (2, 3), (4, 1), (12, 13))          # the first three smaller than the half window of ks = 9 and 11
POOL_BATCH = (1, 3)
UP2_IMAGES = ((1, 1), (1, 5), (3, 2), (19, 19))
UP2_BATCH = (1, 2)
ROUNDING_PAIR = (14, 46)                                 # fp32 map != floor(d in / out) at d = 23
NEAREST_SIZES = (((9, 9), (9, 9)), ((19, 19), (38, 38)), ((38, 38), (75, 75)), ((5, 7), (13, 9)), ((10, 10), (7, 5)),
                 ((1, 1), (17, 17)), ((17, 17), (1, 1)), ((3, 1), (4099, 2)), ((ROUNDING_PAIR[0], 3), (ROUNDING_PAIR[1], 5)))
NEAREST_FACTORS = (((5, 7), (1, 1)), ((5, 7), (2, 3)), ((3, 4), (4, 1)))      # (H, W), (fh, fw)
ACT_SIZES = (1, 3, 4, 5, 7, 1023, 1024, 1025)
ACT_OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))    # floats by which x, dy, out start off a 16-B boundary
AMAX_CHANNELS = (1, 3, 4, 5, 255, 256)
PAD_HUGE = F32(3e38)


def amax_cases():
    """(name, x [M, ld] fp32 host array with its pad columns poisoned, C, float offset of the base pointer, expected
    kernel).  Pad columns alternate 3e38 and the sentinel: neither may count."""
    out = []
    rng = np.random.RandomState(11)

    def rows(M, C, ld):
        x = sentinel((M, ld))
        x[:, C::2] = PAD_HUGE
        x[:, :C] = rng.standard_normal((M, C)).astype(F32)
        return x

    for C in AMAX_CHANNELS:
        ld = (C + 3) // 4 * 4 + 4
        M = 37
        for where, (m, c) in (('first', (0, 0)), ('last', (M - 1, C - 1)), ('middle', (M // 2, C // 2))):
            x = rows(M, C, ld)
            x[m, c] = F32(-77.25) if where == 'middle' else F32(55.5)       # once as a negative number
            out.append(('vector C%d %s' % (C, where), x, C, 0, 'vector'))
        x = rows(M, C, ld + 1)
        x[M - 1, C - 1] = F32(-9.75)
        out.append(('strided C%d ld%%4' % C, x, C, 0, 'strided'))
        x = rows(M, C, ld)
        x[0, 0] = F32(12.5)
        out.append(('strided C%d base+1' % C, x, C, 1, 'strided'))
    x = rows(9, 6, 6)
    x[8, 5] = F32(31.0)
    out.append(('strided C6 ld6', x, 6, 0, 'strided'))
    for name, fill in (('zeros', 0.0), ('-0.0', -0.0), ('denormals', -3 * _D), ('inf', np.inf), ('nan', np.nan)):
        for ld, kind in ((8, 'vector'), (7, 'strided')):
            x = rows(5, 5, ld)
            x[:, :5] = F32(fill)
            if name == 'denormals':
                x[2, 3] = F32(5 * _D)
            if name == 'inf':
                x[::2, :5] = -np.inf
                x[1, 1] = np.nan
            out.append(('%s %s' % (kind, name), x, 5, 0, kind))
    return out


MERGE_CASES = ((0x3f800000, 0x40000000), (0x40000000, 0x3f800000), (0x40000000, 0), (0, 0), (5, 0x7f7fffff))


# Refused argument sets: name -> overrides of a valid base call (tests/test_gpu_glue_edges.py builds the call, tests/
# test_glue_cases.py derives the code again through the mirror).  `off` entries shift a pointer by floats, None is NULL.
def _rows_rejects(names):
    """every pitch operand in turn: C % 4, ld % 4, ld < C, base + 4 bytes, NULL"""
    out = [('C%4', dict(C=6), ERR_SHAPE), ('C=0', dict(C=0), ERR_SHAPE)]
    for n in names:
        out += [('%s ld%%4' % n, {'ld_' + n: 10}, ERR_SHAPE), ('%s ld<C' % n, {'ld_' + n: 4}, ERR_SHAPE),
                ('%s base+4B' % n, {'off_' + n: 1}, ERR_SHAPE), ('%s NULL' % n, {'null_' + n: True}, ERR_SHAPE)]
    return out


REJECT_BASE = dict(C=8, M=3, B=1, H=2, W=3, ks=3, Ho=4, Wo=6, integer_factor=0, n=16, act=ACT_MISH, accumulate=0)
REJECTS = {
    'copy': _rows_rejects(('src', 'dst')) + [('M=0', dict(M=0), ERR_SHAPE), ('M<0', dict(M=-1), ERR_SHAPE)],
    'add': _rows_rejects(('a', 'b', 'out')) + [('M=0', dict(M=0), ERR_SHAPE), ('M<0', dict(M=-5), ERR_SHAPE)],
    'maxpool_fwd': _rows_rejects(('x', 'y')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in 'BHW' for v in (0, -1)] +
                   [('ks=%d' % k, dict(ks=k), ERR_SHAPE) for k in (0, 2, 4, 13, -3)],
    'maxpool_bwd': _rows_rejects(('dy', 'dx')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in 'BHW' for v in (0, -1)] +
                   [('ks=%d' % k, dict(ks=k), ERR_SHAPE) for k in (0, 2, 4, 13, -3)] +
                   [('idx NULL', dict(null_idx=True), ERR_NULL), ('idx NULL, accumulate', dict(null_idx=True, accumulate=1), ERR_NULL)],
    'upsample2x_fwd': _rows_rejects(('x', 'y')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in 'BHW' for v in (0, -1)],
    'upsample2x_bwd': _rows_rejects(('dy', 'dx')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in 'BHW' for v in (0, -1)],
    'nearest_fwd': _rows_rejects(('x', 'y')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in ('B', 'H', 'W', 'Ho', 'Wo') for v in (0, -1)] +
                   [('factor, Ho %% H', dict(integer_factor=1, Ho=5), ERR_SHAPE), ('factor, Wo %% W', dict(integer_factor=1, Wo=7), ERR_SHAPE),
                    ('factor, Ho < H', dict(integer_factor=1, Ho=1), ERR_SHAPE)],
    'nearest_bwd': _rows_rejects(('dy', 'dx')) + [(k + '=%d' % v, {k: v}, ERR_SHAPE) for k in ('B', 'H', 'W', 'Ho', 'Wo') for v in (0, -1)] +
                   [('factor, Ho %% H', dict(integer_factor=1, Ho=5), ERR_SHAPE), ('factor, Wo %% W', dict(integer_factor=1, Wo=7), ERR_SHAPE),
                    ('factor, Ho < H', dict(integer_factor=1, Ho=1), ERR_SHAPE)],
    'act_fwd': [('act=-1', dict(act=-1), ERR_SHAPE), ('act=4', dict(act=4), ERR_SHAPE), ('n=0', dict(n=0), ERR_SHAPE),
                ('n<0', dict(n=-4), ERR_SHAPE), ('x NULL', dict(null_x=True), ERR_NULL), ('y NULL', dict(null_y=True), ERR_NULL)],
    'act_bwd': [('act=-1', dict(act=-1), ERR_SHAPE), ('act=4', dict(act=4), ERR_SHAPE), ('n=0', dict(n=0), ERR_SHAPE),
                ('n<0', dict(n=-4), ERR_SHAPE), ('x NULL', dict(null_x=True), ERR_NULL), ('dy NULL', dict(null_dy=True), ERR_NULL),
                ('dx NULL', dict(null_dx=True), ERR_NULL)],
    'amax': [('ld<C', dict(ld_x=4), ERR_SHAPE), ('C=0', dict(C=0), ERR_SHAPE), ('C<0', dict(C=-4), ERR_SHAPE), ('M<0', dict(M=-1), ERR_SHAPE),
             ('x NULL', dict(null_x=True), ERR_NULL), ('word NULL', dict(null_word=True), ERR_NULL)],
    'merge': [('dst NULL', dict(null_dst=True), ERR_NULL), ('src NULL', dict(null_src=True), ERR_NULL)],
}
REJECT_OPERANDS = {'copy': ('src', 'dst'), 'add': ('a', 'b', 'out'), 'maxpool_fwd': ('x', 'y'), 'maxpool_bwd': ('dy', 'dx'),
                   'upsample2x_fwd': ('x', 'y'), 'upsample2x_bwd': ('dy', 'dx'), 'nearest_fwd': ('x', 'y'),
                   'nearest_bwd': ('dy', 'dx'), 'amax': ('x',)}


def reject_args(entry, over):
    """the argument set of a refused call: the base with the overrides applied"""
    a = dict(REJECT_BASE)
    for n in REJECT_OPERANDS.get(entry, ()):
        a['ld_' + n] = 8
    a.update(over)
    return a


def mirror_rc(entry, a, base_addr=4096):
    """the code the host code returns for reject_args(entry, .), derived through the mirror"""
    def addr(n):
        return 0 if a.get('null_' + n) else base_addr + 4 * a.get('off_' + n, 0)

    ptrs = [(addr(n), a['ld_' + n], a['C']) for n in REJECT_OPERANDS.get(entry, ())]
    if entry in ('copy', 'add'):
        return rc_rows(ptrs, a['M'])
    if entry == 'maxpool_fwd':
        return rc_maxpool_fwd(ptrs, (a['B'], a['H'], a['W']), a['ks'])
    if entry == 'maxpool_bwd':
        return rc_maxpool_bwd(addr('idx'), ptrs, (a['B'], a['H'], a['W']), a['ks'])
    if entry.startswith('upsample2x'):
        return rc_image(ptrs, (a['B'], a['H'], a['W']))
    if entry.startswith('nearest'):
        return rc_nearest(ptrs, a['B'], a['H'], a['W'], a['Ho'], a['Wo'], a['integer_factor'])
    if entry == 'act_fwd':
        return rc_act((addr('x'), addr('y')), a['n'], a['act'])
    if entry == 'act_bwd':
        return rc_act((addr('x'), addr('dy'), addr('dx')), a['n'], a['act'])
    if entry == 'amax':
        return rc_amax(addr('x'), addr('word'), a['ld_x'], a['M'], a['C'])
    assert entry == 'merge'
    return rc_merge(addr('dst'), addr('src'))
