# -*- coding: utf-8 -*-
"""The IoU-family box losses of csrc/yolo_loss.hip (y4_yolo_box_loss_fwd/bwd_f32) against the float64 restatement of
tests/boxloss_cases.py: through the C ABI on planted boxes (equal, disjoint, nested both ways, 1:40 and 40:1, touching,
1e-3 cells wide) for every kind, layer, class count and label count on both sides of the 64-label wave kernel, and
through YOLOLayer + YOLOLoss down to the gradient of the logits.

Tolerance: boxloss_cases.bounds -- BOX_FACTOR x the error that a plain fp32 evaluation of the same formulas makes on
the same inputs; every figure is printed before it is asserted.  Everything a box loss must leave alone (objectness
and class parts, obj_mask, dense targets, the gradient outside the four box channels of the positive cells) is compared
bit for bit with a run without it.  tests/test_boxloss_cases.py shows without a GPU that the inputs hold the geometric
classes they are named for."""
import numpy as np
import pytest
import torch

import boxloss_cases as BC
import head_cases as HC
from oracle import head as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import check, float_array, int_array, lib
    return lib(), ops._ptr, ops._stream, check, float_array, int_array


def _up(a, dev, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(dev)        # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


class _Layer:
    """One layer's loss forward + dense backward through the existing entry points (the 'mse' run), after which the box
    entry points can be run any number of times on copies of its loss parts and gradient."""

    def __init__(self, dev, output, pred, labels, l, C):
        L, ptr, stream, check, farr, iarr = _abi()
        cfg = HC.cfg_with_classes(C)
        B, A, F, _, n_ch = output.shape
        K = labels.shape[1]
        self.dims = (B, F, A, K, C)
        self.dev = dev
        self.od, self.pd = _up(output, dev), _up(pred, dev)
        lab = _up(labels, dev)
        self.nbytes = L.y4_yolo_loss_workspace(B, F, A, K, C)
        self.ws = torch.full((self.nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        self.obj = torch.full((B, A, F, F), float('nan'), device=dev)
        self.parts = torch.full((4,), float('nan'), dtype=torch.float64, device=dev)
        anchors = H.all_anchors(cfg, l)
        check(L.y4_yolo_loss_fwd_f32(ptr(self.od), ptr(self.pd), ptr(lab), K, B, F, A, C, float(H.STRIDES[l]),
                                     float(np.float32(0.7)), farr(anchors.ravel()), len(anchors),
                                     iarr(cfg['ANCHOR_MASK'][l]), ptr(self.obj), ptr(self.parts), ptr(self.ws), self.nbytes,
                                     stream()), 'loss_fwd')
        self.one = torch.ones(1, device=dev)
        self.g = torch.full_like(self.od, float('nan'))
        check(L.y4_yolo_loss_bwd_f32(ptr(self.od), 0, ptr(self.obj), ptr(self.one), ptr(self.g), B, F, A, K, C, ptr(self.ws),
                                     self.nbytes, stream()), 'loss_bwd')

    def dense_targets(self):
        L, ptr, stream, check, _, _ = _abi()
        B, F, A, K, C = self.dims
        t = [torch.full((B, A, F, F, n), float('nan'), device=self.dev) for n in (5 + C, 4 + C, 2)]
        check(L.y4_yolo_loss_dense_targets_f32(ptr(t[0]), ptr(t[1]), ptr(t[2]), B, F, A, K, C, ptr(self.ws), self.nbytes,
                                               stream()), 'dense_targets')
        return [x.cpu().numpy() for x in t]

    def box(self, kind, gain):
        """(parts [4], grad) after the box forward / backward on copies of the mse run's parts and gradient"""
        L, ptr, stream, check, _, _ = _abi()
        B, F, A, K, C = self.dims
        parts, g = self.parts.clone(), self.g.clone()
        check(L.y4_yolo_box_loss_fwd_f32(ptr(self.pd), BC.KIND_IDS[kind], gain, B, F, A, K, C, ptr(parts), ptr(self.ws),
                                         self.nbytes, stream()), 'box_loss_fwd')
        check(L.y4_yolo_box_loss_bwd_f32(ptr(self.pd), BC.KIND_IDS[kind], gain, ptr(self.one), ptr(g), B, F, A, K, C,
                                         ptr(self.ws), self.nbytes, stream()), 'box_loss_bwd')
        torch.cuda.synchronize()
        return parts.cpu().numpy(), g.cpu().numpy()


def _positive_mask(shape, cells):
    m = np.zeros(shape[:4], bool)
    if len(cells):
        m[tuple(cells.T)] = True
    return m


def _check_untouched(tag, parts, g, parts_mse, g_mse, cells):
    """what a box loss leaves alone, bit for bit"""
    assert parts[1] == 0.0 and not np.signbit(parts[1]), tag
    assert np.array_equal(_bits(parts[2:]), _bits(parts_mse[2:])), tag
    assert np.array_equal(_bits(g[..., 4:]), _bits(g_mse[..., 4:])), tag
    pos = _positive_mask(g.shape, cells)
    assert np.array_equal(_bits(g[~pos]), _bits(g_mse[~pos])), tag


def _judge(tag, kind, gain, parts, g, r64, r32, plants):
    """loss and per-record gradient against float64 under boxloss_cases.bounds; returns (loss error, worst row error)"""
    b_loss, b_grad = BC.bounds(kind, gain)
    e_loss = abs(parts[0] - r64['loss'])
    cells = r64['cells']
    got = np.stack([g[b, a, j, i, :4] for b, a, j, i in cells]) if len(cells) else np.zeros((0, 4), np.float32)
    assert np.isfinite(got).all(), tag
    rows = BC.judged_rows(r64, plants)
    e_rows = BC.row_rel_err(got[rows], r64['grad'][rows]) if rows.any() else np.zeros(1)
    e32 = abs(r32['loss'] - r64['loss'])
    print('%s: loss %.9g ref %.9g err %.3g (fp32 restatement %.3g, bound %.3g); gradient row-relative err %.3g (bound %.3g) '
          'over %d judged of %d records' % (tag, parts[0], r64['loss'], e_loss, e32, b_loss, float(e_rows.max()), b_grad,
                                          int(rows.sum()), len(cells)))
    assert np.isfinite(parts[0]) and e_loss <= b_loss, (tag, parts[0], r64['loss'], e_loss, b_loss)
    if rows.any():
        q = int(e_rows.argmax())
        assert e_rows.max() <= b_grad, (tag, float(e_rows.max()), b_grad, got[rows][q], r64['grad'][rows][q])
    return e_loss, float(e_rows.max())


@pytest.mark.parametrize('K', BC.BOX_K)
@pytest.mark.parametrize('C', BC.BOX_C)
@pytest.mark.parametrize('kind', BC.KINDS)
def test_box_loss_through_the_c_abi(dev, kind, C, K):
    """loss_parts[0] and the four gradient channels of every positive cell against float64, at gain 1 and 0.05, on the
    three layers; parts[1] == 0; parts 2 and 3, obj_mask, the dense targets, the gradient of channels 4 and up and the
    gradient of every non-positive cell bit-equal to the run without a box loss.  Records with an exact tie (the equal
    box, the touching boxes) are judged on the loss; their gradient must be finite."""
    case = BC.make_case(C, K)
    worst = [0.0, 0.0]
    for l, lay in enumerate(case['layers']):
        run = _Layer(dev, lay['output'], lay['pred'], case['labels'], l, C)
        torch.cuda.synchronize()
        parts_mse, g_mse, obj_mse = run.parts.cpu().numpy(), run.g.cpu().numpy(), run.obj.cpu().numpy()
        dense_mse = run.dense_targets()
        for gain in BC.GAINS:
            r64, r32 = BC.references(C, K, kind, gain)[l]
            tag = '%s C%d K%d layer %d gain %g' % (kind, C, K, l, gain)
            parts, g = run.box(kind, gain)
            _check_untouched(tag, parts, g, parts_mse, g_mse, r64['cells'])
            e_loss, e_row = _judge(tag, kind, gain, parts, g, r64, r32, lay['plants'])
            f_loss, f_grad = BC.fp32_errors(kind, gain)
            worst = [max(worst[0], e_loss / f_loss), max(worst[1], e_row / f_grad)]
        assert np.array_equal(_bits(run.obj.cpu().numpy()), _bits(obj_mse))
        for a, b in zip(run.dense_targets(), dense_mse):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(run.parts.cpu().numpy()), _bits(parts_mse))       # the box calls ran on copies
    print('%s C%d K%d: kernel error / fp32-restatement error of the case set: loss %.3f, gradient %.3f (allowed %.1f)'
          % (kind, C, K, worst[0], worst[1], BC.BOX_FACTOR))


@pytest.mark.parametrize('kind', BC.KINDS)
def test_k64_and_k65_agree_exactly(dev, kind):
    """The same labels under the wave assign kernel (K = 64) and, with a 65th empty row, under the one-thread-per-image
    kernel: both store the same last-writer truth boxes, so loss and gradient are identical."""
    case = BC.make_case(33, 64)
    more = np.concatenate([case['labels'], np.zeros((3, 1, 5))], 1)
    for l, lay in enumerate(case['layers']):
        a = _Layer(dev, lay['output'], lay['pred'], case['labels'], l, 33).box(kind, 1.0)
        b = _Layer(dev, lay['output'], lay['pred'], more, l, 33).box(kind, 1.0)
        assert a[0][0] > 0
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), (kind, l)


def test_two_runs_agree_bit_for_bit(dev):
    case = BC.make_case(33, 65)
    for l, lay in enumerate(case['layers']):
        for kind in BC.KINDS:
            a = _Layer(dev, lay['output'], lay['pred'], case['labels'], l, 33).box(kind, 0.05)
            b = _Layer(dev, lay['output'], lay['pred'], case['labels'], l, 33).box(kind, 0.05)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), (kind, l)


@pytest.mark.parametrize('kind', BC.KINDS)
def test_nan_in_a_positive_pred_reaches_the_loss(dev, kind):
    """fmaxf / fminf drop a NaN operand: with a NaN centre the IoU of the record would come out finite.  Each of the
    four components in turn, on one positive cell."""
    case = BC.make_case(1, 64)
    lay = case['layers'][0]
    r64 = BC.references(1, 64, kind, 1.0)[0][0]
    b, a, j, i = r64['cells'][len(r64['cells']) // 2]
    for comp in range(4):
        pred = lay['pred'].copy()
        pred[b, a, j, i, comp] = np.nan
        parts, g = _Layer(dev, lay['output'], pred, case['labels'], 0, 1).box(kind, 1.0)
        assert np.isnan(parts[0]), (kind, comp, parts)
        assert parts[1] == 0.0 and np.isfinite(parts[2:]).all()
        assert np.isnan(g[b, a, j, i, :4]).all()
        other = np.ones(g.shape[:4], bool)
        other[b, a, j, i] = False
        assert np.isfinite(g[other]).all()


# ------------------------------------------------------------------------------------------ YOLOLayer + YOLOLoss
E2E_C, E2E_K = 33, 64


def _run_module(dev, logits, labels, **kw):
    """YOLOLayer (train) on the three layers -> YOLOLoss(**kw) -> backward: loss, parts, logits' gradients, and the
    layers' output / pred as they were before the loss touched them."""
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    cfg = HC.cfg_with_classes(E2E_C)
    crit = YOLOLoss(cfg, 0.7, device=dev, **kw)
    lgs = [torch.from_numpy(np.array(lg)).to(dev).requires_grad_(True) for lg in logits]
    ods = [YOLOLayer(cfg, l, device=dev).train()(lg) for l, lg in enumerate(lgs)]
    outs = [od['output'].detach().clone().cpu().numpy() for od in ods]
    preds = [od['pred'].detach().clone().cpu().numpy() for od in ods]
    loss = crit(ods, {'padded_labels': torch.from_numpy(np.array(labels))})
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach().cpu().numpy(), parts=[crit.last[l]['parts'].cpu().numpy() for l in range(3)],
                grads=[lg.grad.cpu().numpy() for lg in lgs], outs=outs, preds=preds,
                final_outs=[od['output'].detach().cpu().numpy() for od in ods])


@pytest.fixture(scope='module')
def e2e_mse(dev):
    case = BC.make_case(E2E_C, E2E_K)
    logits = [lay['logits'] for lay in case['layers']]
    return {m: _run_module(dev, logits, case['labels'], mutate_outputs=m) for m in (True, False)}


def test_default_constructor_is_the_mse_loss(dev, e2e_mse):
    case = BC.make_case(E2E_C, E2E_K)
    logits = [lay['logits'] for lay in case['layers']]
    r = _run_module(dev, logits, case['labels'], box_loss='mse')
    d = e2e_mse[True]
    assert np.array_equal(_bits(r['loss'].reshape(1)), _bits(d['loss'].reshape(1)))
    for l in range(3):
        assert np.array_equal(_bits(r['parts'][l]), _bits(d['parts'][l])) and d['parts'][l][1] > 0
        assert np.array_equal(_bits(r['grads'][l]), _bits(d['grads'][l]))


@pytest.mark.parametrize('mutate', (True, False), ids=('mutate', 'keep'))
@pytest.mark.parametrize('kind', BC.KINDS)
def test_box_loss_through_yololoss_and_yololayer(dev, e2e_mse, kind, mutate):
    """YOLOLayer -> YOLOLoss(box_loss=kind, box_gain=0.05) -> backward on the three layers, with the in-place masking of
    outputs[*]['output'] on and off (the box backward reads pred, so both give the same gradient).

    The restatement is evaluated on the pred the layer produced.  Loss part 0 per layer: BOX_FACTOR x the plain-fp32
    evaluation's error on the same pred (largest of the three layers).  Gradient of the logits: everything but the four
    box channels of the positive cells is bit-equal to the run without a box loss; those channels against the float64
    composition g_logit = g_box * (1 - o) * o (x, y) or g_box (w, h), within
        BWD_CONST * 2^-23 * S  +  fac * BOX_FACTOR * e32 * max|g_box of the record|
    -- the decode backward's own bar (head_cases.decode_bwd_ref64: S = |g| (1 + o) o or |g|) plus the box gradient's
    bar (e32: the fp32 evaluation's largest row-relative error on this pred) carried through fac = (1 - o) o or 1."""
    gain = 0.05
    case = BC.make_case(E2E_C, E2E_K)
    logits = [lay['logits'] for lay in case['layers']]
    r = _run_module(dev, logits, case['labels'], mutate_outputs=mutate, box_loss=kind, box_gain=gain)
    base = e2e_mse[mutate]
    refs = []
    for l in range(3):
        assert np.array_equal(_bits(r['preds'][l]), _bits(base['preds'][l]))
        a = (r['outs'][l], r['preds'][l], case['labels'], case['cfg'], kind, gain, l)
        refs.append((BC.layer_box_loss(*a), BC.layer_box_loss(*a, dtype=np.float32)))
    e32_loss = max(abs(r32['loss'] - r64['loss']) for r64, r32 in refs)
    e32_grad = max(float(BC.row_rel_err(r32['grad'][~r64['ties']], r64['grad'][~r64['ties']]).max()) for r64, r32 in refs)
    assert e32_loss > 0 and e32_grad > 0
    total = 0.0
    for l, (r64, r32) in enumerate(refs):
        parts = r['parts'][l]
        total += parts.sum()
        err = abs(parts[0] - r64['loss'])
        print('%s layer %d: box loss %.9g ref %.9g err %.3g (bound %.3g)' % (kind, l, parts[0], r64['loss'], err,
                                                                              BC.BOX_FACTOR * e32_loss))
        assert err <= BC.BOX_FACTOR * e32_loss and parts[1] == 0.0
        assert np.array_equal(_bits(parts[2:]), _bits(base['parts'][l][2:]))
        assert np.array_equal(_bits(r['final_outs'][l]), _bits(base['final_outs'][l]))   # the masking side effect, or none
        B, _, F, _ = logits[l].shape
        n_ch = 5 + E2E_C
        g = r['grads'][l].reshape(B, 3, n_ch, F, F).transpose(0, 1, 3, 4, 2)
        g0 = base['grads'][l].reshape(B, 3, n_ch, F, F).transpose(0, 1, 3, 4, 2)
        pos = _positive_mask(g.shape, r64['cells'])
        assert np.array_equal(_bits(g[..., 4:]), _bits(g0[..., 4:])) and np.array_equal(_bits(g[~pos]), _bits(g0[~pos]))
        v = logits[l].reshape(B, 3, n_ch, F, F).transpose(0, 1, 3, 4, 2)
        worst = 0.0
        for q, (b, a, j, i) in enumerate(r64['cells']):
            if r64['ties'][q]:
                assert np.isfinite(g[b, a, j, i, :4]).all()
                continue
            gb = r64['grad'][q]
            o = 1.0 / (1.0 + np.exp(-v[b, a, j, i, :2].astype(np.float64)))
            fac = np.array([(1 - o[0]) * o[0], (1 - o[1]) * o[1], 1.0, 1.0])
            S = np.abs(gb) * np.array([(1 + o[0]) * o[0], (1 + o[1]) * o[1], 1.0, 1.0])
            tol = HC.BWD_CONST * 2.0 ** -23 * S + fac * BC.BOX_FACTOR * e32_grad * np.abs(gb).max() + HC.TINY
            e = np.abs(g[b, a, j, i, :4].astype(np.float64) - gb * fac)
            worst = max(worst, float((e / tol).max()))
            assert (e <= tol).all(), (kind, l, q, g[b, a, j, i, :4], gb * fac, tol)
        print('%s layer %d: logit gradient, largest error / tolerance %.3f' % (kind, l, worst))
    # the module adds the three layers' fp32(sum of parts) in fp32: three roundings to fp32 and two fp32 additions
    assert abs(float(r['loss']) - total) <= 2.0 ** -22 * abs(total)
