# -*- coding: utf-8 -*-
"""The YOLOv4 head options of csrc/yolo_decode.hip and csrc/yolo_loss.hip -- scale_x_y in the three decodes, several
positive anchors per label (iou_thresh), class label smoothing, and scale_x_y in the box-loss gradient -- through the C ABI (the *_ex entries)
against the float64 restatement of tests/headopt_cases.py, then through YOLOLayer + YOLOLoss and through YOLOv4.

With the options off the new entries must give the bits of the entries they generalise.  tests/test_headopt_cases.py
shows without a GPU that the inputs used here hold what they are named for: more records than labels on layers 0 and 1,
same-cell collisions, labels positive on all three anchors, an IoU exactly on the threshold."""
import functools

import numpy as np
import pytest
import torch

import boxloss_cases as BC
import head_cases as HC
import headopt_cases as HO
import recipe
from oracle import head as H

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = 0x7fa5c3e1                        # a NaN bit pattern no kernel produces


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
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _case_id(c):
    return 'C%d-A%d-F%d-B%d-ld%d' % c


# ------------------------------------------------------------------------------------------ decode
@functools.lru_cache(maxsize=None)
def _decode_inputs(C, A, F, B):
    nt = A * (5 + C)
    lg, _ = HC.make_logits(B, F, A, C, nt, 5)
    anc = HC.decode_anchors(A, 1)
    v = HC.logit_view(lg, nt, B, F, A, C)
    lg.setflags(write=False)
    return lg, anc, v


def _logits_at_pitch(C, A, F, B, ldl, dev):
    lg, anc, _ = _decode_inputs(C, A, F, B)
    full, _ = HC.make_logits(B, F, A, C, ldl, 5)
    assert np.array_equal(full[:, :A * (5 + C)], lg)
    return _up(full, dev), anc


def _decode_train(dev, lgd, ldl, B, F, A, C, anc, s=None):
    """(output, pred) of the existing entry (s None) or of the _ex entry"""
    L, ptr, stream, check, farr, _ = _abi()
    out = torch.full((B, A, F, F, 5 + C), float('nan'), device=dev)
    pred = torch.full((B, A, F, F, 4), float('nan'), device=dev)
    if s is None:
        check(L.y4_yolo_decode_train_f32(ptr(lgd), ldl, ptr(out), ptr(pred), B, F, A, C, farr(anc.ravel()), stream()), 'train')
    else:
        check(L.y4_yolo_decode_train_ex_f32(ptr(lgd), ldl, ptr(out), ptr(pred), B, F, A, C, farr(anc.ravel()), s, stream()),
              'train_ex')
    torch.cuda.synchronize()
    return out.cpu().numpy(), pred.cpu().numpy()


def _decode_eval(dev, lgd, ldl, B, F, A, C, anc, stride, box_off, s=None):
    """the whole sentinel-filled int32 buffer [4 + B * n_total * n_ch + 4] after an eval decode at box_off"""
    L, ptr, stream, check, farr, _ = _abi()
    n_ch, nb = 5 + C, A * F * F
    n_total = nb + box_off + 2
    buf = torch.full((4 + B * n_total * n_ch + 4,), SENT, dtype=torch.int32, device=dev)
    if s is None:
        check(L.y4_yolo_decode_eval_f32(ptr(lgd), ldl, ptr(buf[4:]), n_total, box_off, B, F, A, C, farr(anc.ravel()), stride,
                                        stream()), 'eval')
    else:
        check(L.y4_yolo_decode_eval_ex_f32(ptr(lgd), ldl, ptr(buf[4:]), n_total, box_off, B, F, A, C, farr(anc.ravel()),
                                           stride, s, stream()), 'eval_ex')
    torch.cuda.synchronize()
    return buf.cpu().numpy(), n_total


def _decode_bwd(dev, lgd, ldl, B, F, A, C, anc, god, gpd, s=None):
    L, ptr, stream, check, farr, _ = _abi()
    gl = torch.full((B * F * F, ldl), float('nan'), device=dev)
    if s is None:
        check(L.y4_yolo_decode_bwd_f32(ptr(lgd), ldl, ptr(god), ptr(gpd), ptr(gl), B, F, A, C, farr(anc.ravel()), stream()), 'bwd')
    else:
        check(L.y4_yolo_decode_bwd_ex_f32(ptr(lgd), ldl, ptr(god), ptr(gpd), ptr(gl), B, F, A, C, farr(anc.ravel()), s,
                                          stream()), 'bwd_ex')
    torch.cuda.synchronize()
    return gl.cpu().numpy()


def _bwd_grads(B, F, A, C, dev):
    rng = np.random.RandomState(77)
    go = rng.standard_normal((B, A, F, F, 5 + C)).astype(np.float32)
    gp = rng.standard_normal((B, A, F, F, 4)).astype(np.float32)
    return go, gp, _up(go, dev), _up(gp, dev)


def _eval_offsets(B, F):
    return (0, 3) if B * F * F >= 100000 else (0, 1, 2, 3)


@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_defaults_give_the_existing_bits(dev, case):
    """scale_xy = 1 through the three _ex entries: np.array_equal (on the bit patterns) to the existing entries, for the
    tiled and the per-channel kernel, train, eval at every box offset, and backward with either and both gradients."""
    C, A, F, B, ldl = case
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    o0, p0 = _decode_train(dev, lgd, ldl, B, F, A, C, anc)
    o1, p1 = _decode_train(dev, lgd, ldl, B, F, A, C, anc, 1.0)
    assert _same(o0, o1) and _same(p0, p1)
    for box_off in _eval_offsets(B, F):
        a, _ = _decode_eval(dev, lgd, ldl, B, F, A, C, anc, 8.0, box_off)
        b, _ = _decode_eval(dev, lgd, ldl, B, F, A, C, anc, 8.0, box_off, 1.0)
        assert np.array_equal(a, b), box_off
    go, gp, god, gpd = _bwd_grads(B, F, A, C, dev)
    for ad, bd in ((god, None), (None, gpd), (god, gpd)):
        assert _same(_decode_bwd(dev, lgd, ldl, B, F, A, C, anc, ad, bd), _decode_bwd(dev, lgd, ldl, B, F, A, C, anc, ad, bd, 1.0))


@pytest.mark.parametrize('s', (1.2, 2.0))
@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_train_with_scale(dev, case, s):
    """`output` and pred[..., 2:4] bit-equal to the existing entry's; the centres per element against float64 under
    |got - ref| <= (|v| + DEC_CONST + 2) * 2^-23 * (sigma * s + h + i)."""
    C, A, F, B, ldl = case
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    lg, _, v = _decode_inputs(C, A, F, B)
    o0, p0 = _decode_train(dev, lgd, ldl, B, F, A, C, anc)
    o, p = _decode_train(dev, lgd, ldl, B, F, A, C, anc, s)
    assert _same(o, o0) and _same(p[..., 2:], p0[..., 2:])
    _, ref, S = HO.decode_ref64(lg, A * (5 + C), B, F, A, C, anc, 1.0, True, s)
    print('decode_train_ex %s s %g: constant needed %.2f (allowed %.1f)'
          % (_case_id(case), s, HO.decode_xy_needed(p[..., :2], ref[..., :2], v[..., :2], S), HO.DEC_CONST))
    ok = HO.decode_xy_accept(p[..., :2], ref[..., :2], v[..., :2], S)
    assert ok.all(), [(tuple(i), p[..., :2][tuple(i)], ref[..., :2][tuple(i)]) for i in np.argwhere(~ok)[:5]]


@pytest.mark.parametrize('s', (1.2, 2.0))
@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_eval_with_scale_into_shared_buffer(dev, case, s):
    """Into rows [box_off, box_off + A*F*F) of a sentinel-filled buffer at every 16-byte phase: everything but the two
    centre columns of those rows -- the other rows and the guard words included -- bit-equal to the existing entry's
    buffer; the centres against float64 with S = (sigma * s + h + i) * stride."""
    C, A, F, B, ldl = case
    n_ch, nb = 5 + C, A * F * F
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    lg, _, v = _decode_inputs(C, A, F, B)
    vv = v.reshape(B, nb, n_ch)[..., :2]
    ref, S = HO.decode_ref64(lg, A * n_ch, B, F, A, C, anc, 8.0, False, s)
    for box_off in _eval_offsets(B, F):
        h0, n_total = _decode_eval(dev, lgd, ldl, B, F, A, C, anc, 8.0, box_off)
        h1, _ = _decode_eval(dev, lgd, ldl, B, F, A, C, anc, 8.0, box_off, s)
        assert np.array_equal(h0[:4], h1[:4]) and np.array_equal(h0[-4:], h1[-4:])
        b0, b1 = h0[4:-4].reshape(B, n_total, n_ch), h1[4:-4].reshape(B, n_total, n_ch)
        assert np.array_equal(b0[..., 2:], b1[..., 2:]), box_off
        assert np.array_equal(b0[:, :box_off], b1[:, :box_off]) and np.array_equal(b0[:, box_off + nb:], b1[:, box_off + nb:])
        got = np.ascontiguousarray(b1[:, box_off:box_off + nb, :2]).view(np.float32)
        print('decode_eval_ex %s s %g box_off %d: constant needed %.2f (allowed %.1f)'
              % (_case_id(case), s, box_off, HO.decode_xy_needed(got, ref[..., :2], vv, S), HO.DEC_CONST))
        ok = HO.decode_xy_accept(got, ref[..., :2], vv, S)
        assert ok.all(), (box_off, [(tuple(i), got[tuple(i)], ref[..., :2][tuple(i)]) for i in np.argwhere(~ok)[:5]])


@pytest.mark.parametrize('s', (1.2, 2.0))
@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_backward_with_scale(dev, case, s):
    """g_pred alone and with g_output: head_cases.decode_bwd_accept with S from the generalised restatement (the addend
    is |s * g_pred|) and the constant BWD_CONST + 1; pad columns exactly 0."""
    C, A, F, B, ldl = case
    nt = A * (5 + C)
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    lg = _decode_inputs(C, A, F, B)[0]
    go, gp, god, gpd = _bwd_grads(B, F, A, C, dev)
    for a, ad in ((None, None), (go, god)):
        got = _decode_bwd(dev, lgd, ldl, B, F, A, C, anc, ad, gpd, s)
        ref, S = HO.decode_bwd_ref64(lg, nt, B, F, A, C, anc, a, gp, s)
        assert np.array_equal(got[:, nt:].view(np.int32), np.zeros((B * F * F, ldl - nt), np.int32))
        got = got[:, :nt]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            err = np.abs(got - HC.to_f32_range(ref))
            need = err / (2.0 ** -23 * S)
        print('decode_bwd_ex %s s %g: constant needed %.2f (allowed %.1f)'
              % (_case_id(case), s, float(need[np.isfinite(need) & (err > HC.TINY)].max()), HO.BWD_CONST))
        ok = HC.decode_bwd_accept(got, ref, S, HO.BWD_CONST)
        assert ok.all(), [(tuple(i), got[tuple(i)], ref[tuple(i)]) for i in np.argwhere(~ok)[:5]]


# ------------------------------------------------------------------------------------------ loss through the C ABI
def _run_loss(dev, output, pred, labels, l, C, iou=1.0, eps=0.0, ex=True, box=None):
    """The loss entries on one layer -- the _ex forms, or the existing ones with ex=False -- and with box = (kind, gain,
    scale_xy) the box-loss entries on copies of the parts and the gradient.  Everything comes back as numpy."""
    L, ptr, stream, check, farr, iarr = _abi()
    cfg = HC.cfg_with_classes(C)
    B, A, F, _, n_ch = output.shape
    K = labels.shape[1]
    od, pd, lab = _up(output, dev), _up(pred, dev), _up(labels, dev)
    nbytes = L.y4_yolo_loss_workspace_ex(B, F, A, K, C, iou) if ex else L.y4_yolo_loss_workspace(B, F, A, K, C)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)     # the kernels initialise what they read
    obj = torch.full((B, A, F, F), float('nan'), device=dev)
    parts = torch.full((4,), float('nan'), dtype=torch.float64, device=dev)
    anchors = H.all_anchors(cfg, l)
    head = (ptr(od), ptr(pd), ptr(lab), K, B, F, A, C, float(H.STRIDES[l]), float(np.float32(0.7)), farr(anchors.ravel()),
            len(anchors), iarr(cfg['ANCHOR_MASK'][l]))
    tail = (ptr(obj), ptr(parts), ptr(ws), nbytes, stream())
    target = torch.full((B, A, F, F, n_ch), float('nan'), device=dev)
    tgt_mask = torch.full((B, A, F, F, 4 + C), float('nan'), device=dev)
    tgt_scale = torch.full((B, A, F, F, 2), float('nan'), device=dev)
    one = torch.ones(1, device=dev)
    g, g2, mo = torch.full_like(od, float('nan')), torch.full_like(od, float('nan')), od.clone()
    dims = (B, F, A, K, C)
    if ex:
        check(L.y4_yolo_loss_fwd_ex_f32(*head, iou, eps, *tail), 'loss_fwd_ex')
        check(L.y4_yolo_loss_dense_targets_ex_f32(ptr(target), ptr(tgt_mask), ptr(tgt_scale), *dims, iou, eps, ptr(ws), nbytes,
                                                  stream()), 'dense_targets_ex')
        check(L.y4_yolo_loss_bwd_ex_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), *dims, iou, eps, ptr(ws), nbytes, stream()),
              'loss_bwd_ex')
        check(L.y4_yolo_loss_mask_output_ex_f32(ptr(mo), ptr(obj), *dims, iou, ptr(ws), nbytes, stream()), 'mask_output_ex')
        check(L.y4_yolo_loss_bwd_ex_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), *dims, iou, eps, ptr(ws), nbytes, stream()),
              'loss_bwd_ex')
    else:
        check(L.y4_yolo_loss_fwd_f32(*head, *tail), 'loss_fwd')
        check(L.y4_yolo_loss_dense_targets_f32(ptr(target), ptr(tgt_mask), ptr(tgt_scale), *dims, ptr(ws), nbytes, stream()),
              'dense_targets')
        check(L.y4_yolo_loss_bwd_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), *dims, ptr(ws), nbytes, stream()), 'loss_bwd')
        check(L.y4_yolo_loss_mask_output_f32(ptr(mo), ptr(obj), *dims, ptr(ws), nbytes, stream()), 'mask_output')
        check(L.y4_yolo_loss_bwd_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), *dims, ptr(ws), nbytes, stream()), 'loss_bwd')
    r = dict(obj_mask=obj, parts=parts, target=target, tgt_mask=tgt_mask, tgt_scale=tgt_scale, grad=g, mutated=mo, grad_masked=g2)
    if box is not None:
        kind, gain, sxy = box
        bp, bg = parts.clone(), g.clone()
        if ex:
            check(L.y4_yolo_box_loss_fwd_ex_f32(ptr(pd), BC.KIND_IDS[kind], gain, *dims, iou, ptr(bp), ptr(ws), nbytes, stream()),
                  'box_fwd_ex')
            check(L.y4_yolo_box_loss_bwd_ex_f32(ptr(pd), BC.KIND_IDS[kind], gain, ptr(one), ptr(bg), *dims, iou, sxy, ptr(ws),
                                                nbytes, stream()), 'box_bwd_ex')
        else:
            check(L.y4_yolo_box_loss_fwd_f32(ptr(pd), BC.KIND_IDS[kind], gain, *dims, ptr(bp), ptr(ws), nbytes, stream()), 'box_fwd')
            check(L.y4_yolo_box_loss_bwd_f32(ptr(pd), BC.KIND_IDS[kind], gain, ptr(one), ptr(bg), *dims, ptr(ws), nbytes,
                                             stream()), 'box_bwd')
        r.update(box_parts=bp, box_grad=bg)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in r.items()}


def _check_loss(got, ref, tag):
    """the bars of test_gpu_head_edges._check_loss, restated"""
    assert np.array_equal(got['obj_mask'], ref['obj_mask']), tag
    assert np.array_equal(got['tgt_mask'], ref['tgt_mask']), tag
    assert np.array_equal(got['target'] != 0, ref['target'] != 0), tag
    HC.close(got['target'], ref['target'], 1e-6, 1e-6, scale=False)
    HC.close(got['tgt_scale'], ref['tgt_scale'], 1e-6, 1e-6, scale=False)
    loss = float(got['parts'].sum())
    assert np.isfinite(got['parts']).all() and abs(loss - ref['loss']) <= 1e-4 * abs(ref['loss']), (tag, loss, ref['loss'])
    for q, name in enumerate(('xy', 'wh', 'obj', 'cls')):
        assert abs(got['parts'][q] - ref[name]) <= 1e-4 * abs(ref[name]), (tag, name, got['parts'][q], ref[name])
    for key in ('grad', 'grad_masked'):
        assert np.isfinite(got[key]).all(), (tag, key)
        HC.close(got[key], ref['grad_output'], 1e-5, 1e-4)
    HC.close(got['mutated'], ref['mutated_output'], 1e-6, 1e-6, scale=False)


LOSS_KEYS = ('obj_mask', 'parts', 'target', 'tgt_mask', 'tgt_scale', 'grad', 'mutated', 'grad_masked', 'box_parts', 'box_grad')


@pytest.mark.parametrize('K', (64, 65))
def test_loss_defaults_give_the_existing_bits(dev, K):
    """iou_thresh = 1, label_smooth = 0, scale_xy = 1 through every _ex loss entry against the existing entries, on one
    (C, K) per assign form: every output bit for bit, the CIoU box loss and its gradient included."""
    d = HO.loss_inputs(33, K)
    for l, (lg, out, pred) in enumerate(d['layers']):
        a = _run_loss(dev, out, pred, d['labels'], l, 33, ex=False, box=('ciou', 0.05, 1.0))
        b = _run_loss(dev, out, pred, d['labels'], l, 33, 1.0, 0.0, box=('ciou', 0.05, 1.0))
        for k in LOSS_KEYS:
            assert _same(a[k], b[k]), (k, l)
        assert a['box_parts'][0] > 0


@pytest.mark.parametrize('opts', ((0.213, 0.0), (1.0, 0.1), (0.213, 0.1)), ids=('anchors', 'smooth', 'both'))
@pytest.mark.parametrize('K', HO.HEAD_K)
@pytest.mark.parametrize('C', HO.HEAD_C)
def test_loss_with_options(dev, C, K, opts):
    """Every loss output on the three layers against the float64 restatement, with several anchors, with label smoothing
    and with both; pred decoded by the oracle from the same logits."""
    iou, eps = opts
    d = HO.loss_inputs(C, K)
    n_extra = 0
    for l, (lg, out, pred) in enumerate(d['layers']):
        got = _run_loss(dev, out, pred, d['labels'], l, C, iou, eps)
        ref = HO.loss_ref(out, pred, l, d['labels'], d['cfg'], 0.7, iou, eps)
        _check_loss(got, ref, (C, K, l, opts))
        n_extra += sum(sum(inf['first_extra']) for inf in ref['info'])
        if eps:
            pos = ref['tgt_mask'][..., 0] > 0
            if pos.any():
                lo, hi = HO.smooth_targets(eps)
                assert set(np.unique(got['target'][..., 5:][pos])) <= {F32(lo), F32(hi)}
    if iou < 1 and K >= 64:
        assert n_extra > 0


def test_threshold_is_strict(dev):
    """iou_thresh set to the fp32 shape IoU of a (label, non-arg-max anchor) pair: the pair is not positive; one ulp
    below it is.  The masks are exact either way."""
    d = HO.loss_inputs(33, 64)
    l = 1
    lg, out, pred = d['layers'][l]
    thr, b, t, a = HO.planted_tie(d['labels'], d['cfg'], l)
    below = float(np.nextafter(F32(thr), F32(0)))
    refs = [HO.loss_ref(out, pred, l, d['labels'], d['cfg'], 0.7, x, 0.0) for x in (thr, below)]
    assert refs[0]['tgt_mask'].sum() < refs[1]['tgt_mask'].sum()
    for x, ref in zip((thr, below), refs):
        _check_loss(_run_loss(dev, out, pred, d['labels'], l, 33, x, 0.0), ref, x)


def test_saturated_logits_with_label_smoothing(dev):
    """+-30 logits on positive and background cells, label_smooth = 0.1 (so no class target is 0 or 1), several anchors:
    finite results, the gradient under HC.close(1e-5, 1e-4)."""
    d = HO.loss_inputs(33, 64, True)
    for l, (lg, out, pred) in enumerate(d['layers']):
        got = _run_loss(dev, out, pred, d['labels'], l, 33, 0.213, 0.1)
        ref = HO.loss_ref(out, pred, l, d['labels'], d['cfg'], 0.7, 0.213, 0.1)
        for k in ('parts', 'grad', 'grad_masked', 'mutated', 'target'):
            assert np.isfinite(got[k]).all(), (k, l)
        _check_loss(got, ref, ('saturated', l))


# ------------------------------------------------------------------------------------------ box loss on the grown records
def _record_rows(g, cells):
    return np.stack([g[b, a, j, i, :4] for b, a, j, i in cells]) if len(cells) else np.zeros((0, 4), np.float32)


@pytest.mark.parametrize('CK', HO.BOX_SETS, ids=lambda ck: 'C%d-K%d' % ck)
@pytest.mark.parametrize('kind', BC.KINDS)
def test_box_loss_with_several_anchors_and_scale(dev, kind, CK):
    """Loss and per-record gradient (channels 0 and 1 times s) on planted boxes at every record, extra-anchor records
    included, scales (1.2, 1.1, 1.05), gains 1 and 0.05, by boxloss_cases' rule: BOX_FACTOR x the plain-fp32 evaluation's
    error.  Tie plants are judged on the loss only.  Everything outside the four box channels of the record cells is
    bit-equal to the run without a box loss."""
    C, K = CK
    case = HO.box_case(C, K)
    worst = [0.0, 0.0]
    for l, lay in enumerate(case['layers']):
        s = HO.scale_of(case['scale'], l)
        for gain in BC.GAINS:
            r64, r32 = HO.box_references(C, K, kind, gain)[l]
            tag = '%s C%d K%d layer %d gain %g' % (kind, C, K, l, gain)
            got = _run_loss(dev, lay['output'], lay['pred'], case['labels'], l, C, 0.213, 0.1, box=(kind, gain, s))
            parts, g = got['box_parts'], got['box_grad']
            assert parts[1] == 0.0 and _same(parts[2:], got['parts'][2:]), tag
            pos = np.zeros(g.shape[:4], bool)
            pos[tuple(r64['cells'].T)] = True
            assert _same(g[..., 4:], got['grad'][..., 4:]) and _same(g[~pos], got['grad'][~pos]), tag
            b_loss, b_grad = HO.box_bounds(kind, gain)
            f_loss, f_grad = HO.box_fp32_errors(kind, gain)
            e_loss = abs(parts[0] - r64['loss'])
            rows = BC.judged_rows(r64, lay['plants'])
            rec = _record_rows(g, r64['cells'])
            assert np.isfinite(rec).all(), tag
            e_rows = BC.row_rel_err(rec[rows], r64['grad'][rows])
            print('%s: loss %.9g ref %.9g err %.3g (bound %.3g); gradient row-relative err %.3g (bound %.3g) over %d judged of '
                  '%d records, %d of them extra-anchor' % (tag, parts[0], r64['loss'], e_loss, b_loss, float(e_rows.max()),
                                                          b_grad, int(rows.sum()), len(rows), int(r64['extra'].sum())))
            assert np.isfinite(parts[0]) and e_loss <= b_loss, (tag, parts[0], r64['loss'])
            assert e_rows.max() <= b_grad, (tag, float(e_rows.max()), b_grad)
            worst = [max(worst[0], e_loss / f_loss), max(worst[1], float(e_rows.max()) / f_grad)]
    print('%s C%d K%d: kernel error / fp32-restatement error: loss %.3f, gradient %.3f (allowed %.1f)'
          % (kind, C, K, worst[0], worst[1], BC.BOX_FACTOR))


def test_k64_and_k65_agree_exactly_with_all_options_on(dev):
    """The wave assign form (K = 64) and, with one zero row more, the one-thread form: the same records in the same
    order, so every output -- the box-loss sum included -- has the same bits."""
    case = HO.box_case(33, 64)
    more = np.concatenate([case['labels'], np.zeros((3, 1, 5))], 1)
    for l, lay in enumerate(case['layers']):
        s = HO.scale_of(case['scale'], l)
        for kind in BC.KINDS:
            a = _run_loss(dev, lay['output'], lay['pred'], case['labels'], l, 33, 0.213, 0.1, box=(kind, 1.0, s))
            b = _run_loss(dev, lay['output'], lay['pred'], more, l, 33, 0.213, 0.1, box=(kind, 1.0, s))
            assert a['box_parts'][0] > 0
            for k in LOSS_KEYS:
                assert _same(a[k], b[k]), (k, l, kind)


def test_two_runs_agree_bit_for_bit(dev):
    for C, K in ((33, 65), (33, 64)):
        case = HO.box_case(C, K)
        for l, lay in enumerate(case['layers']):
            s = HO.scale_of(case['scale'], l)
            a = _run_loss(dev, lay['output'], lay['pred'], case['labels'], l, C, 0.213, 0.1, box=('ciou', 0.05, s))
            b = _run_loss(dev, lay['output'], lay['pred'], case['labels'], l, C, 0.213, 0.1, box=('ciou', 0.05, s))
            for k in LOSS_KEYS:
                assert _same(a[k], b[k]), (k, l, K)


@pytest.mark.parametrize('kind', BC.KINDS)
def test_nan_in_an_extra_anchor_record_reaches_the_box_loss(dev, kind):
    """A NaN in the pred of a record that exists only through iou_thresh: the box loss and that record's gradient are
    NaN, every other gradient stays finite."""
    case = HO.box_case(33, 64)
    lay = case['layers'][1]
    r64 = HO.box_references(33, 64, kind, 1.0)[1][0]
    q = int(np.nonzero(r64['extra'])[0][3])
    b, a, j, i = r64['cells'][q]
    for comp in (0, 3):
        pred = lay['pred'].copy()
        pred[b, a, j, i, comp] = np.nan
        got = _run_loss(dev, lay['output'], pred, case['labels'], 1, 33, 0.213, 0.1, box=(kind, 1.0, 1.1))
        assert np.isnan(got['box_parts'][0]) and got['box_parts'][1] == 0.0 and np.isfinite(got['box_parts'][2:]).all()
        assert np.isnan(got['box_grad'][b, a, j, i, :4]).all()
        other = np.ones(got['box_grad'].shape[:4], bool)
        other[b, a, j, i] = False
        assert np.isfinite(got['box_grad'][other]).all()


# ------------------------------------------------------------------------------------------ YOLOLayer + YOLOLoss
E2E_C, E2E_K = 33, 64
E2E_SCALE = [1.2, 1.1, 1.05]


@pytest.mark.parametrize('mutate', (True, False), ids=('mutate', 'keep'))
def test_options_through_yololayer_and_yololoss(dev, mutate):
    """YOLOLayer (cfg with SCALE_X_Y) -> YOLOLoss(box_loss='ciou', iou_thresh=0.213, label_smooth=0.1) -> backward down
    to the logits, against the composed float64 restatement evaluated on the output / pred the layers produced:
      pred centres: the decode bound against float64; loss parts: box part BOX_FACTOR x the fp32 evaluation's error,
      objectness and class parts 1e-4 relative; gradient of the logits: HC.close(1e-5, 1e-4) everywhere but the four box
      channels of the record cells, which carry the box gradient through the decode backward --
      BWD_CONST' * 2^-23 * S + fac * BOX_FACTOR * e32 * max|g_box of the record| as in test_gpu_boxloss."""
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    gain = 0.05
    d = HO.loss_inputs(E2E_C, E2E_K)
    cfg = dict(d['cfg'], SCALE_X_Y=E2E_SCALE)
    crit = YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=mutate, box_loss='ciou', box_gain=gain, iou_thresh=0.213,
                    label_smooth=0.1)
    lgs = [torch.from_numpy(np.array(lay[0])).to(dev).requires_grad_(True) for lay in d['layers']]
    ods = [YOLOLayer(cfg, l, device=dev).train()(lg) for l, lg in enumerate(lgs)]
    outs = [od['output'].detach().clone().cpu().numpy() for od in ods]
    preds = [od['pred'].detach().clone().cpu().numpy() for od in ods]
    labels = torch.from_numpy(np.array(d['labels']))
    loss = crit(ods, {'padded_labels': labels})
    loss.backward()
    torch.cuda.synchronize()
    total = 0.0
    n_ch = 5 + E2E_C
    for l in range(3):
        s = E2E_SCALE[l]
        lg = d['layers'][l][0]
        B, _, F, _ = lg.shape
        nhwc = np.ascontiguousarray(lg.transpose(0, 2, 3, 1)).reshape(-1, 3 * n_ch)
        v = HC.logit_view(nhwc, 3 * n_ch, B, F, 3, E2E_C)
        _, p64, S = HO.decode_ref64(nhwc, 3 * n_ch, B, F, 3, E2E_C, H.masked_anchors(cfg, l), 1.0, True, s)
        assert HO.decode_xy_accept(preds[l][..., :2], p64[..., :2], v[..., :2], S).all()
        ref = HO.loss_ref(outs[l], preds[l], l, d['labels'], cfg, 0.7, 0.213, 0.1)
        r64 = HO.box_ref(preds[l], ref['info'], 'ciou', gain, s)
        r32 = HO.box_ref(preds[l], ref['info'], 'ciou', gain, s, F32)
        assert r64['extra'].any()
        parts = crit.last[l]['parts'].cpu().numpy()
        total += parts.sum()
        e32 = abs(r32['loss'] - r64['loss'])
        assert abs(parts[0] - r64['loss']) <= BC.BOX_FACTOR * e32 and parts[1] == 0.0, (l, parts[0], r64['loss'], e32)
        assert abs(parts[2] - ref['obj']) <= 1e-4 * ref['obj'] and abs(parts[3] - ref['cls']) <= 1e-4 * ref['cls']
        assert crit.last[l]['rec_cap'] == 3 * E2E_K
        # the in-place masking side effect, or none
        final = ods[l]['output'].detach().cpu().numpy()
        if mutate:
            HC.close(final, ref['mutated_output'], 1e-6, 1e-6, scale=False)
        else:
            assert _same(final, outs[l])
        # gradient of the logits: g_output (the box channels of the record cells replaced) through the decode backward
        go = ref['grad_output'].copy()
        pos = np.zeros(go.shape[:4], bool)
        for q, (b, a, j, i) in enumerate(r64['cells']):
            go[b, a, j, i, :4] = r64['grad'][q]
            pos[b, a, j, i] = True
        gref, _ = HC.decode_bwd_ref64(nhwc, 3 * n_ch, B, F, 3, E2E_C, H.masked_anchors(cfg, l), go, None)
        gref = gref.reshape(B, F, F, 3, n_ch).transpose(0, 3, 1, 2, 4)
        g = lgs[l].grad.cpu().numpy().reshape(B, 3, n_ch, F, F).transpose(0, 1, 3, 4, 2)
        assert np.isfinite(g).all()
        box = np.zeros(g.shape, bool)
        box[..., :4] = pos[..., None]
        HC.close(np.where(box, 0.0, g), np.where(box, 0.0, gref), 1e-5, 1e-4)
        rows = ~r64['ties']
        e32g = float(BC.row_rel_err(r32['grad'][rows], r64['grad'][rows]).max())
        for q, (b, a, j, i) in enumerate(r64['cells']):
            if r64['ties'][q]:
                continue
            gb = r64['grad'][q]
            o = 1.0 / (1.0 + np.exp(-v[b, a, j, i, :2].astype(np.float64)))
            fac = np.array([(1 - o[0]) * o[0], (1 - o[1]) * o[1], 1.0, 1.0])
            Sb = np.abs(gb) * np.array([(1 + o[0]) * o[0], (1 + o[1]) * o[1], 1.0, 1.0])
            tol = HO.BWD_CONST * 2.0 ** -23 * Sb + fac * BC.BOX_FACTOR * e32g * np.abs(gb).max() + HC.TINY
            e = np.abs(g[b, a, j, i, :4].astype(np.float64) - gb * fac)
            assert (e <= tol).all(), (l, q, g[b, a, j, i, :4], gb * fac, tol)
        # build_target: the smoothed, several-anchor dense targets
        tgt, om, tm, ts = crit.build_target(torch.from_numpy(outs[l]).to(dev), torch.from_numpy(preds[l]).to(dev), l, labels)
        assert np.array_equal(om.cpu().numpy(), ref['obj_mask']) and np.array_equal(tm.cpu().numpy(), ref['tgt_mask'])
        t = tgt.cpu().numpy()
        assert np.array_equal(t != 0, ref['target'] != 0)
        HC.close(t, ref['target'], 1e-6, 1e-6, scale=False)
        HC.close(ts.cpu().numpy(), ref['tgt_scale'], 1e-6, 1e-6, scale=False)
        lo, hi = HO.smooth_targets(0.1)
        assert set(np.unique(t[..., 5:][ref['tgt_mask'][..., 0] > 0])) == {F32(lo), F32(hi)}
    assert abs(float(loss.detach()) - total) <= 2.0 ** -22 * abs(total)


# ------------------------------------------------------------------------------------------ through the model
def test_scale_through_the_model_eval_path(dev):
    """Two YOLOv4 from the same weights at 64 x 64, B = 1, eval: cfg and cfg + SCALE_X_Y.  Every column but the first two
    is bit-equal.  The centres: with x1 the unscaled result, sigma = x1 / stride - i and v = logit(sigma), the scaled
    result must be ((sigma * s) - h + i) * stride within the decode bound of the scaled entry plus s times the bound
    of the unscaled one (x1 is itself a decode result, (|v| + DEC_CONST) * 2^-23 * |x1| from the exact value)."""
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    scale = [1.2, 1.1, 1.05]
    S_, B = 64, 1
    m1 = YOLOv4(recipe.MODEL_CFG, device=dev)
    sd = m1.state_dict()
    recipe.fill_state_dict_(sd, 7)
    m1.load_state_dict(sd)
    m1 = m1.to(dev).train()
    recipe.calibrate_bn_(m1, recipe.randn((8, 3, S_, S_), 3).to(dev))
    m2 = YOLOv4(dict(recipe.MODEL_CFG, SCALE_X_Y=scale), device=dev)
    m2.load_state_dict({k: t.cpu() for k, t in m1.state_dict().items()})
    m2 = m2.to(dev)
    x = recipe.randn((B, 3, S_, S_), 1).to(dev)
    m1.eval(), m2.eval()
    with torch.no_grad():
        o1, o2 = m1(x).cpu().numpy(), m2(x).cpu().numpy()
    assert o1.shape == o2.shape and np.isfinite(o1).all()
    assert _same(o1[..., 2:], o2[..., 2:])
    off = 0
    for l, st in enumerate((8, 16, 32)):
        F = S_ // st
        n = 3 * F * F
        s, h = HO.s_h(scale[l])
        cell = np.stack([np.tile(np.arange(F), F), np.repeat(np.arange(F), F)], -1).astype(np.float64)        # (i, j) of a row
        cell = np.tile(cell, (3, 1)).reshape(1, n, 2)
        x1 = o1[:, off:off + n, :2].astype(np.float64)
        x2 = o2[:, off:off + n, :2].astype(np.float64)
        sig = x1 / st - cell
        assert (sig > -1e-5).all() and (sig < 1 + 1e-5).all()
        sc = np.clip(sig, 2.0 ** -60, 1 - 2.0 ** -53)
        v = np.abs(np.log(sc / (1 - sc)))
        ref = (sig * s - h + cell) * st
        Ssum = (np.abs(sig) * s + h + cell) * st
        tol = (v + HO.DEC_CONST) * 2.0 ** -23 * Ssum + s * (v + HC.DEC_CONST) * 2.0 ** -23 * np.abs(x1)
        assert (np.abs(x2 - ref) <= tol).all(), (l, float((np.abs(x2 - ref) / tol).max()))
        assert not np.array_equal(x1, x2)
        off += n
    assert off == o1.shape[1]
