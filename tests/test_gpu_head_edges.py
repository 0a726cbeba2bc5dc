# -*- coding: utf-8 -*-
"""The head, loss, IoU and NMS kernels of csrc/yolo_decode.hip, yolo_loss.hip and postprocess.hip, each driven through the
C ABI at the sizes where the host picks another kernel or a kernel takes another branch: pitch and alignment of the decode, label counts on both
sides of the 64-label wave kernel, class counts on both sides of a 32-bit mask word, NMS chunk seams, segments above the
LDS sort limit, tiles of the candidate count that span several images, and logits that saturate the fp32 sigmoid.

The references are tests/head_cases.py (fp64 decode) and oracle.head; tests/test_head_cases.py shows, without a GPU,
that every input used here reaches the path it is named for."""
import functools

import numpy as np
import pytest
import torch

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
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _worst(ok, got, ref, v):
    """text for a failed acceptance: the worst elements with their logits"""
    bad = np.argwhere(~ok)[:5]
    return [(tuple(i), float(np.asarray(got)[tuple(i)]), float(np.asarray(ref)[tuple(i)]), float(np.asarray(v)[tuple(i)]))
            for i in bad]


def _needed_const(got, ref64, v):
    """the constant c that (|v| + c) * 2^-23 * |ref| would need over the elements the relative criterion judges"""
    got = np.asarray(got, np.float64)
    ref = HC.to_f32_range(ref64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got - ref)
        rel = err / (2.0 ** -23 * np.abs(ref)) - np.abs(v)
    rel = rel[np.isfinite(rel) & (err > HC.TINY)]
    return float(rel.max()) if rel.size else 0.0


# ------------------------------------------------------------------------------------------ decode
def _case_id(c):
    return 'C%d-A%d-F%d-B%d-ld%d' % c


@functools.lru_cache(maxsize=None)
def _decode_ref(C, A, F, B):
    """logit content and fp64 references of a shape: the same for every pitch it runs at"""
    nt = A * (5 + C)
    lg, _ = HC.make_logits(B, F, A, C, nt, 5)
    anc = HC.decode_anchors(A, 1)
    out, pred = HC.decode_ref64(lg, nt, B, F, A, C, anc, 1.0, True)
    v = HC.logit_view(lg, nt, B, F, A, C)
    for a in (lg, out, pred):
        a.setflags(write=False)
    return lg, anc, out, pred, v


def _logits_at_pitch(C, A, F, B, ldl, dev):
    lg, anc, out, pred, v = _decode_ref(C, A, F, B)
    full, props = HC.make_logits(B, F, A, C, ldl, 5)
    assert np.array_equal(full[:, :A * (5 + C)], lg)
    return _up(full, dev), anc


@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_train(dev, case):
    """y4_yolo_decode_train_f32 against the fp64 decode, element by element under head_cases.decode_accept; the raw
    w / h logits of `output` bit-equal to the input.  A shape listed at two pitches runs the tiled and the per-channel
    kernel on the same logits against the same reference."""
    C, A, F, B, ldl = case
    L, ptr, stream, check, farr, _ = _abi()
    n_ch = 5 + C
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    _, _, ref_out, ref_pred, v = _decode_ref(C, A, F, B)
    out = torch.full((B, A, F, F, n_ch), float('nan'), device=dev)
    pred = torch.full((B, A, F, F, 4), float('nan'), device=dev)
    check(L.y4_yolo_decode_train_f32(ptr(lgd), ldl, ptr(out), ptr(pred), B, F, A, C, farr(anc.ravel()), stream()),
          'decode_train')
    torch.cuda.synchronize()
    o, p = out.cpu().numpy(), pred.cpu().numpy()
    print('decode_train %s: constant needed: output %.2f, pred %.2f (allowed %.1f)'
          % (_case_id(case), _needed_const(o, ref_out, v), _needed_const(p, ref_pred, v[..., :4]), HC.DEC_CONST))
    assert not np.isnan(o).any() and not np.isnan(p).any()
    assert np.array_equal(o[..., 2:4].view(np.int32), np.ascontiguousarray(v[..., 2:4]).view(np.int32))
    ok = HC.decode_accept(o, ref_out, v)
    assert ok.all(), _worst(ok, o, ref_out, v)
    ok = HC.decode_accept(p, ref_pred, v[..., :4])
    assert ok.all(), _worst(ok, p, ref_pred, v[..., :4])


SENT = 0x7fa5c3e1                        # a NaN bit pattern no kernel produces


@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_eval_into_shared_buffer(dev, case):
    """y4_yolo_decode_eval_f32 into rows [box_off, box_off + A*F*F) of a sentinel-filled [B, n_total, 5+C] buffer, at
    box offsets that put a run's first float on each 16-byte phase (0..3 with an odd row length): the rows against
    the fp64 decode, every float outside them -- other rows and 16 bytes before and after the buffer -- untouched."""
    C, A, F, B, ldl = case
    L, ptr, stream, check, farr, _ = _abi()
    n_ch = 5 + C
    nb = A * F * F
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    lg = _decode_ref(C, A, F, B)[0]
    v = HC.logit_view(lg, A * n_ch, B, F, A, C).reshape(B, nb, n_ch)
    stride = 8.0
    ref = HC.decode_ref64(lg, A * n_ch, B, F, A, C, anc, stride, False)
    for box_off in ((0, 3) if B * F * F >= 100000 else (0, 1, 2, 3)):
        n_total = nb + box_off + 2
        buf = torch.full((4 + B * n_total * n_ch + 4,), SENT, dtype=torch.int32, device=dev)
        check(L.y4_yolo_decode_eval_f32(ptr(lgd), ldl, ptr(buf[4:]), n_total, box_off, B, F, A, C, farr(anc.ravel()),
                                        stride, stream()), 'decode_eval')
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:4] == SENT).all() and (h[-4:] == SENT).all(), box_off
        body = h[4:-4].reshape(B, n_total, n_ch)
        assert (body[:, :box_off] == SENT).all() and (body[:, box_off + nb:] == SENT).all(), box_off
        got = np.ascontiguousarray(body[:, box_off:box_off + nb]).view(np.float32)
        print('decode_eval %s box_off %d: constant needed %.2f' % (_case_id(case), box_off, _needed_const(got, ref, v)))
        ok = HC.decode_accept(got, ref, v)
        assert ok.all(), (box_off, _worst(ok, got, ref, v))


@pytest.mark.parametrize('case', HC.DECODE_CASES, ids=_case_id)
def test_decode_backward(dev, case):
    """y4_yolo_decode_bwd_f32 with g_output only, g_pred only and both: |got - ref| <= 16 * 2^-23 * S against the fp64
    backward (S: head_cases.decode_bwd_ref64), pad columns exactly 0 on every pixel, and exactly 0 wherever the fp32
    sigmoid is exactly 0 or 1."""
    C, A, F, B, ldl = case
    L, ptr, stream, check, farr, _ = _abi()
    n_ch = 5 + C
    nt = A * n_ch
    lgd, anc = _logits_at_pitch(C, A, F, B, ldl, dev)
    lg = _decode_ref(C, A, F, B)[0]
    rng = np.random.RandomState(77)
    go = rng.standard_normal((B, A, F, F, n_ch)).astype(np.float32)
    gp = rng.standard_normal((B, A, F, F, 4)).astype(np.float32)
    god, gpd = _up(go, dev), _up(gp, dev)
    v = HC.logit_view(lg, nt, B, F, A, C)
    sat = np.zeros(v.shape, bool)
    sig = np.r_[0:2, 4:n_ch]
    with np.errstate(over='ignore'):
        o32 = H._sigmoid(np.ascontiguousarray(v[..., sig]))
    sat[..., sig] = (o32 == 0) | (o32 == 1)
    sat = sat.transpose(0, 2, 3, 1, 4).reshape(B * F * F, nt)
    assert sat.any()
    for a, b, ad, bd in ((go, None, god, None), (None, gp, None, gpd), (go, gp, god, gpd)):
        gl = torch.full((B * F * F, ldl), float('nan'), device=dev)
        check(L.y4_yolo_decode_bwd_f32(ptr(lgd), ldl, ptr(ad), ptr(bd), ptr(gl), B, F, A, C, farr(anc.ravel()), stream()),
              'decode_bwd')
        torch.cuda.synchronize()
        got = gl.cpu().numpy()
        ref, S = HC.decode_bwd_ref64(lg, nt, B, F, A, C, anc, a, b)
        assert np.array_equal(got[:, nt:].view(np.int32), np.zeros((B * F * F, ldl - nt), np.int32))
        got = got[:, :nt]
        assert not np.isnan(got).any()
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            err = np.abs(got - HC.to_f32_range(ref))
            need = err / (2.0 ** -23 * S)
        print('decode_bwd %s: constant needed %.2f (allowed %.1f)'
              % (_case_id(case), float(need[np.isfinite(need) & (err > HC.TINY)].max()), HC.BWD_CONST))
        ok = HC.decode_bwd_accept(got, ref, S)
        assert ok.all(), _worst(ok, got, ref, S)
        assert (got[sat] == 0).all()


# ------------------------------------------------------------------------------------------ loss
def _run_loss(dev, output, pred, labels, l, C, masked_bwd=False):
    """The four y4_yolo_loss_* entry points on one layer; everything comes back as numpy."""
    L, ptr, stream, check, farr, iarr = _abi()
    cfg = HC.cfg_with_classes(C)
    B, A, F, _, n_ch = output.shape
    K = labels.shape[1]
    od, pd = _up(output, dev), _up(pred, dev)
    lab = _up(labels, dev)                                              # labels.to(float32), yololoss.py:129
    nbytes = L.y4_yolo_loss_workspace(B, F, A, K, C)
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)     # the kernels initialise what they read
    obj = torch.full((B, A, F, F), float('nan'), device=dev)
    parts = torch.full((4,), float('nan'), dtype=torch.float64, device=dev)
    anchors = H.all_anchors(cfg, l)
    check(L.y4_yolo_loss_fwd_f32(ptr(od), ptr(pd), ptr(lab), K, B, F, A, C, float(H.STRIDES[l]), float(np.float32(0.7)),
                                 farr(anchors.ravel()), len(anchors), iarr(cfg['ANCHOR_MASK'][l]), ptr(obj), ptr(parts),
                                 ptr(ws), nbytes, stream()), 'loss_fwd')
    target = torch.full((B, A, F, F, n_ch), float('nan'), device=dev)
    tgt_mask = torch.full((B, A, F, F, 4 + C), float('nan'), device=dev)
    tgt_scale = torch.full((B, A, F, F, 2), float('nan'), device=dev)
    check(L.y4_yolo_loss_dense_targets_f32(ptr(target), ptr(tgt_mask), ptr(tgt_scale), B, F, A, K, C, ptr(ws), nbytes,
                                           stream()), 'dense_targets')
    one = torch.ones(1, device=dev)
    g = torch.full_like(od, float('nan'))
    check(L.y4_yolo_loss_bwd_f32(ptr(od), 0, ptr(obj), ptr(one), ptr(g), B, F, A, K, C, ptr(ws), nbytes, stream()), 'loss_bwd')
    r = dict(obj_mask=obj, parts=parts, target=target, tgt_mask=tgt_mask, tgt_scale=tgt_scale, grad=g)
    if masked_bwd:
        mo = od.clone()
        check(L.y4_yolo_loss_mask_output_f32(ptr(mo), ptr(obj), B, F, A, K, C, ptr(ws), nbytes, stream()), 'mask_output')
        g2 = torch.full_like(od, float('nan'))
        check(L.y4_yolo_loss_bwd_f32(ptr(mo), 1, ptr(obj), ptr(one), ptr(g2), B, F, A, K, C, ptr(ws), nbytes, stream()),
              'loss_bwd')
        r.update(mutated=mo, grad_masked=g2)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in r.items()}


def _check_loss(got, ref, tag):
    """the bars of test_yololoss_golden / test_loss_edge_cases_vs_oracle"""
    assert np.array_equal(got['obj_mask'], ref['obj_mask']), tag
    assert np.array_equal(got['tgt_mask'], ref['tgt_mask']), tag
    assert np.array_equal(got['target'] != 0, ref['target'] != 0), tag
    HC.close(got['target'], ref['target'], 1e-6, 1e-6, scale=False)
    HC.close(got['tgt_scale'], ref['tgt_scale'], 1e-6, 1e-6, scale=False)
    loss = float(got['parts'].sum())
    assert np.isfinite(got['parts']).all() and abs(loss - ref['loss']) <= 1e-4 * abs(ref['loss']), (tag, loss, ref['loss'])
    # every part is a sum of non-negative terms, each a few fp32 roundings from the oracle's: the same bar holds per part
    for q, name in enumerate(('xy', 'wh', 'obj', 'cls')):
        assert abs(got['parts'][q] - ref[name]) <= 1e-4 * abs(ref[name]), (tag, name, got['parts'][q], ref[name])
    for key in ('grad', 'grad_masked'):
        if key in got:
            assert np.isfinite(got[key]).all(), (tag, key)
            HC.close(got[key], ref['grad_output'], 1e-5, 1e-4)
    if 'mutated' in got:
        HC.close(got['mutated'], ref['mutated_output'], 1e-6, 1e-6, scale=False)


@functools.lru_cache(maxsize=None)
def _loss_inputs(C, seed=900, saturate_K=0):
    """oracle decode of the three layers' logits: what the loss kernels and the oracle's loss are both given"""
    cfg = HC.cfg_with_classes(C)
    labels = HC.make_labels(saturate_K, C, 100 + saturate_K)[0] if saturate_K else None
    lgs, props = HC.make_loss_logits(C, seed, labels, saturate=bool(saturate_K))
    return [(lg,) + H.yolo_decode(lg, l, cfg, True) for l, lg in enumerate(lgs)], props


@pytest.mark.parametrize('K', HC.LOSS_K)
@pytest.mark.parametrize('C', HC.LOSS_CLASSES)
def test_loss_class_words_and_label_counts(dev, C, K):
    """Loss forward, dense targets, mask-output and both backward forms against oracle.head, for class counts on both
    sides of a 32-bit mask word and label counts on both sides of the 64-label wave kernel; label sets with n == K, a zero
    row between valid rows, two classes on one cell and anchor, and a class in the last mask word."""
    cfg = HC.cfg_with_classes(C)
    labels, props = HC.make_labels(K, C, 100 + K)
    assert props['n_eq_K'] and props['class_in_last_word']
    decoded, _ = _loss_inputs(C)
    for l, (lg, out, pred) in enumerate(decoded):
        ref = H.yolo_loss_layer(out, pred, l, labels, cfg, 0.7)
        got = _run_loss(dev, out, pred, labels, l, C, masked_bwd=True)
        _check_loss(got, ref, (C, K, l))


@pytest.mark.parametrize('C', (33, 65))
def test_loss_k64_and_k65_agree_exactly(dev, C):
    """The same labels under the wave kernel (K = 64) and, with one more zero row, under the one-thread-per-image kernel
    (K = 65): masks, targets, loss parts and gradient are identical."""
    labels, props = HC.make_labels(64, C, 164)
    more = np.concatenate([labels, np.zeros((3, 1, 5))], 1)
    decoded, _ = _loss_inputs(C)
    for l, (lg, out, pred) in enumerate(decoded):
        a = _run_loss(dev, out, pred, labels, l, C)
        b = _run_loss(dev, out, pred, more, l, C)
        assert a['target'].any()
        for k in a:
            assert np.array_equal(a[k], b[k]), (C, l, k)


@pytest.mark.parametrize('C,K', [(33, 64), (65, 100)])
def test_loss_saturated_logits(dev, C, K):
    """+-30 on objectness, class and xy logits of positive and of background cells: the fp32 sigmoid is exactly 0 or 1
    there, BCE runs into its -100 log clamp and its gradient into the 1e-12 floor.  GPU decode -> loss -> loss backward
    -> decode backward, each stage against the oracle on the oracle's own inputs to that stage; no NaN or inf anywhere.
    The loss gradient holds elements of 1e12 next to elements of 1e-2, so beside the project's range-scaled bar each
    element is held to rel 1e-4 + abs 1e-5 of its own reference: both sides evaluate the same short fp32 expression
    on the same fp32 `output`."""
    L, ptr, stream, check, farr, _ = _abi()
    cfg = HC.cfg_with_classes(C)
    labels = HC.make_labels(K, C, 100 + K)[0]
    decoded, props = _loss_inputs(C, 900, K)
    assert props['planted_positive'] >= 6 and props['planted_background'] >= 6
    n_ch = 5 + C
    for l, (lg, out, pred) in enumerate(decoded):
        B, _, F, _ = lg.shape
        assert (out == 1.0).any()
        ref = H.yolo_loss_layer(out, pred, l, labels, cfg, 0.7)
        got = _run_loss(dev, out, pred, labels, l, C, masked_bwd=True)
        _check_loss(got, ref, (C, K, l))
        for key in ('grad', 'grad_masked'):
            err = np.abs(got[key].astype(np.float64) - ref['grad_output'])
            assert (err <= 1e-4 * np.abs(ref['grad_output']) + 1e-5).all(), (l, key, float(err.max()))
        assert np.abs(ref['grad_output']).max() >= 1e11
        # the decode backward takes that gradient to the logits: (1 - o) * o is exactly 0 where the 1e12 sit
        rows = np.ascontiguousarray(lg.transpose(0, 2, 3, 1)).reshape(B * F * F, 3 * n_ch)
        anc = H.masked_anchors(cfg, l)
        gl = torch.full((B * F * F, 3 * n_ch), float('nan'), device=dev)
        rows_d, go_d = _up(rows, dev), _up(ref['grad_output'], dev)
        check(L.y4_yolo_decode_bwd_f32(ptr(rows_d), 3 * n_ch, ptr(go_d), None, ptr(gl), B, F, 3, C, farr(anc.ravel()),
                                       stream()), 'decode_bwd')
        torch.cuda.synchronize()
        g = gl.cpu().numpy()
        g_ref = H.yolo_decode_backward(lg, ref['grad_output'], None, l, cfg).transpose(0, 2, 3, 1).reshape(B * F * F, 3 * n_ch)
        assert np.isfinite(g).all()
        HC.close(g, g_ref, 1e-5, 1e-4)


# ------------------------------------------------------------------------------------------ IoU
@pytest.mark.parametrize('shape', HC.IOU_SHAPES, ids=lambda s: '%dx%d' % s)
def test_bboxes_iou_bit_exact(dev, shape):
    """y4_bboxes_iou_f32, corner and centre / size forms: bit-exact against oracle.head.bboxes_iou on touching, nested,
    identical, zero-area and NaN boxes, NaN positions included; Na * Nb = 1, 255, 257 (around one block) and 5 * 4097."""
    L, ptr, stream, check, _, _ = _abi()
    Na, Nb = shape
    a, b, props = HC.make_iou_boxes(Na, Nb, 7)
    ad, bd = _up(a, dev), _up(b, dev)
    for xyxy in (True, False):
        out = torch.full((Na * Nb + 1,), float('inf'), device=dev)
        check(L.y4_bboxes_iou_f32(ptr(ad), Na, ptr(bd), Nb, 1 if xyxy else 0, ptr(out), stream()), 'bboxes_iou')
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert h[-1] == np.inf                                          # nothing written past Na * Nb
        got = h[:-1].reshape(Na, Nb)
        ref = H.bboxes_iou(a, b, xyxy)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), xyxy
        m = ~np.isnan(ref)
        assert np.array_equal(got[m].view(np.int32), ref[m].view(np.int32)), xyxy


# ------------------------------------------------------------------------------------------ NMS
def _run_nms(dev, box, score, thresh, limit=0):
    L, ptr, stream, check, _, _ = _abi()
    R = len(box)
    bd = _up(box, dev)
    sd = _up(score, dev) if score is not None else None
    keep = torch.full((R + 1,), -7, dtype=torch.int32, device=dev)
    nkeep = torch.full((1,), -1, dtype=torch.int32, device=dev)
    nbytes = L.y4_nms_workspace(R)
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    check(L.y4_nms_f32(ptr(bd), ptr(sd), R, float(thresh), int(limit), ptr(keep), ptr(nkeep), ptr(ws), nbytes, stream()), 'nms')
    torch.cuda.synchronize()
    n = int(nkeep.item())
    k = keep.cpu().numpy()
    assert 0 <= n <= R and (k[n:] == -7).all()
    return k[:n]


@pytest.mark.parametrize('R', HC.NMS_SIZES)
def test_nms_chunk_sizes(dev, R):
    """R on both sides of the 256-candidate chunk, scores on a 0.01 lattice (ties -> lower index first): survivors and
    order equal to the oracle's, with scores, without (index order), and with a limit."""
    box, score, thr = HC.make_nms_clusters(R, 20 + R)
    assert np.array_equal(_run_nms(dev, box, score, thr), H.nms(box, thr, score=score))
    assert np.array_equal(_run_nms(dev, box, None, thr), H.nms(box, thr))
    lim = max(1, len(H.nms(box, thr, score=score)) // 2)
    assert np.array_equal(_run_nms(dev, box, score, thr, lim), H.nms(box, thr, score=score, limit=lim))


def test_nms_many_survivors_limit_and_chains_across_chunks(dev):
    """More than 512 survivors (three staging trips of kept boxes), boxes suppressed only by a kept box of the first
    chunk / of the second staging trip, IoU == threshold, zero-area boxes, tie groups, a limit that expires inside the
    second chunk, and the same boxes without scores."""
    box, score, thr = HC.make_nms_grid()
    ref = H.nms(box, thr, score=score)
    assert len(ref) > 512
    assert np.array_equal(_run_nms(dev, box, score, thr), ref)
    assert np.array_equal(_run_nms(dev, box, score, thr, HC.NMS_LIMIT), H.nms(box, thr, score=score, limit=HC.NMS_LIMIT))
    assert np.array_equal(_run_nms(dev, box, score, thr, HC.NMS_LIMIT), ref[:HC.NMS_LIMIT])
    assert np.array_equal(_run_nms(dev, box, None, thr), H.nms(box, thr))
    assert np.array_equal(_run_nms(dev, box, None, thr, 257), H.nms(box, thr, limit=257))


@functools.lru_cache(maxsize=None)
def _post_case(kind):
    return HC.make_post_case(kind)


@pytest.mark.parametrize('kind', HC.POST_KINDS)
def test_postprocess_segment_and_tile_edges(dev, kind):
    """postprocess (count, scan, fill, sort + NMS, compaction): survivors and order exactly the oracle's, the in-place
    corner conversion exact.  'big': a segment above the 2048-key LDS sort with more than 512 survivors; 'four': a 64-row
    tile over four images; N = 63 / 64 / 65; one class; an image whose candidates all sit in its last class, and an image
    without candidates between two that have some."""
    from yolov4_amd.yolo.util.utils import postprocess
    p, C, conf, thre, props = _post_case(kind)
    if kind == 'big':
        assert props['cand'][0, 0] > 2048 and props['surv'][0, 0] > 512
    pd = _up(p, dev)
    got = postprocess(pd, C, conf, thre)
    assert np.array_equal(pd[:, :, :4].cpu().numpy().view(np.int32), props['xyxy'].view(np.int32))
    assert np.array_equal(pd[:, :, 4:].cpu().numpy(), p[:, :, 4:])
    for b, ref in enumerate(props['ref']):
        assert (ref is None) == (got[b] is None), (kind, b)
        if ref is not None:
            g = got[b].cpu().numpy()
            assert g.shape == ref.shape and np.array_equal(g, ref), (kind, b)
