# -*- coding: utf-8 -*-
"""Letterboxed / rectangular-batch inference on the GPU: the batch preprocess kernel against letterbox_cases.letterbox_ref
(bit for bit), the rectangular eval decode against the fp64 decode, the models on rectangular inputs, and the entry points
(detect_images, COCOBatchLoader, validate) against the manual chain.  tests/test_letterbox_cases.py pins the references."""
import ctypes
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

import head_cases as HC
import jpeg_cases as J
import letterbox_cases as LC
import recipe
from oracle import network as NW

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_NULL = 1, 2
SENT = 0x7fa5c3e1                        # a NaN bit pattern no kernel produces
PAD = 8                                  # canary floats before and after every destination


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _abi():
    from yolov4_amd import ops
    from yolov4_amd._lib import LetterboxSrc, check, float_array, lib
    return lib(), ops._ptr, ops._stream, check, float_array, LetterboxSrc


# ------------------------------------------------------------------------------------------ preprocess kernel
def _table(records, dev):
    """records: (device uint8 tensor [h, w, 3], nh, nw, top, left, swap) -> (host ctypes array, device copy of its bytes)"""
    LetterboxSrc = _abi()[5]
    host = (LetterboxSrc * len(records))()
    for r, (t, nh, nw, top, left, swap) in zip(host, records):
        r.src, r.h, r.w, r.pitch, r.swap_rb = t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), int(swap)
        r.nh, r.nw, r.top, r.left, r.reserved = nh, nw, top, left, 0
    raw = np.frombuffer(bytes(host), dtype=np.uint8).copy()
    return host, torch.from_numpy(raw).to(dev)


def _call(host, table_dev, B, dst, strides, Hc, Wc, fill=114, dst_ptr=None):
    L, ptr, stream = _abi()[:3]
    return L.y4_letterbox_batch_u8_f32(table_dev.data_ptr() if table_dev is not None else None,
                                       ctypes.addressof(host) if host is not None else None, B,
                                       dst.data_ptr() if dst_ptr is None else dst_ptr, *strides, Hc, Wc, fill, stream())


@functools.lru_cache(maxsize=None)
def _batch_ref():
    Hc, Wc = LC.CANVAS
    imgs = [LC.image(h, w, 40 + k) for k, (h, w, *_) in enumerate(LC.BATCH)]
    ref = np.stack([LC.letterbox_ref(im, nh, nw, top, left, Hc, Wc, 114, bool(swap))
                    for im, (_, _, nh, nw, top, left, swap) in zip(imgs, LC.BATCH)])
    ref.setflags(write=False)
    return imgs, ref


@pytest.mark.parametrize('layout', ['planar', 'nhwc', 'planar_misaligned'])
def test_letterbox_batch_kernel_is_the_restatement(dev, layout):
    """One launch over LC.BATCH (every source size, placements flush to each edge, a 1-pixel-high image, the 2x area path,
    both swap_rb values) on a 64 x 96 canvas: np.array_equal with letterbox_ref, into a planar batch (16-byte stores), an
    NHWC-strided one and a planar one whose base is 4 bytes past a 16-byte boundary (scalar stores); the canary around the
    destination untouched."""
    Hc, Wc = LC.CANVAS
    imgs, ref = _batch_ref()
    B = len(imgs)
    srcs = [torch.from_numpy(im).to(dev) for im in imgs]
    host, tdev = _table([(t,) + rec[2:] for t, rec in zip(srcs, LC.BATCH)], dev)
    n = B * 3 * Hc * Wc
    shift = 1 if layout == 'planar_misaligned' else 0
    buf = torch.full((PAD + shift + n + PAD,), SENT, dtype=torch.int32, device=dev)
    body = buf[PAD + shift:PAD + shift + n]
    assert body.data_ptr() % 16 == (4 if shift else 0)
    if layout == 'nhwc':
        strides = (Hc * Wc * 3, 1, Wc * 3, 3)
    else:
        strides = (3 * Hc * Wc, Hc * Wc, Wc, 1)
    assert _call(host, tdev, B, body, strides, Hc, Wc) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:PAD + shift] == SENT).all() and (h[-PAD:] == SENT).all()
    got = h[PAD + shift:PAD + shift + n].view(np.float32)
    got = got.reshape(B, Hc, Wc, 3).transpose(0, 3, 1, 2) if layout == 'nhwc' else got.reshape(B, 3, Hc, Wc)
    for b in range(B):
        assert np.array_equal(got[b], ref[b]), (layout, b, LC.BATCH[b], np.argwhere(got[b] != ref[b])[:4])


def test_letterbox_batch_python_entry(dev):
    """letterbox_batch: geometry, canvas and offsets of a mixed batch in 'rect' and 'square' mode, equal to the restatement;
    numpy and device sources give the same bytes; `out=` is written in place."""
    from yolov4_amd.yolo.data.transform import letterbox_batch
    imgs = [LC.image(37, 29, 1), LC.image(24, 60, 2), LC.image(96, 128, 3)]
    for mode, canvas in (('rect', (64, 64)), ('square', (64, 64))):
        x, infos = letterbox_batch(imgs, 64, mode, 32)
        assert tuple(x.shape) == (3, 3) + canvas and x.dtype == torch.float32 and x.is_cuda
        assert infos == [[37, 29, 64, 50, 0, 7], [24, 60, 26, 64, 19, 0], [96, 128, 48, 64, 8, 0]]
        for b, (im, inf) in enumerate(zip(imgs, infos)):
            assert np.array_equal(x[b].cpu().numpy(), LC.letterbox_ref(im, *inf[2:], *canvas))
    x, infos = letterbox_batch([imgs[1]], 64, 'rect', 32)
    assert tuple(x.shape) == (1, 3, 32, 64) and infos == [[24, 60, 26, 64, 3, 0]]
    assert np.array_equal(x[0].cpu().numpy(), LC.letterbox_ref(imgs[1], 26, 64, 3, 0, 32, 64))
    out = torch.zeros((1, 3, 32, 64), device=dev)
    y, _ = letterbox_batch([torch.from_numpy(imgs[1]).to(dev)], 64, 'rect', 32, out=out)
    assert y is out and torch.equal(out, x)
    z, _ = letterbox_batch([imgs[1]], 64, 'rect', 32, fill=0)
    assert float(z[0, :, :3].abs().max()) == 0.0 and torch.equal(z[0, :, 3:29], x[0, :, 3:29])


@pytest.mark.parametrize('S,sizes', [(64, [(37, 29), (300, 9), (1, 1), (128, 128), (64, 64)]), (48, [(96, 96), (13, 21)])])
def test_stretch_geometry_is_the_per_image_kernel(dev, S, sizes):
    """nh = nw = Hc = Wc = S, top = left = 0: bit-equal to y4_preprocess_u8_f32 (image_resize_into), the 2x area path
    (128 x 128 at 64, 96 x 96 at 48) included."""
    from yolov4_amd.yolo.data.transform import val_batch
    imgs = [LC.image(h, w, 70 + k) for k, (h, w) in enumerate(sizes)]
    srcs = [torch.from_numpy(im).to(dev) for im in imgs]
    want, _ = val_batch(srcs, S)
    host, tdev = _table([(t, S, S, 0, 0, 1) for t in srcs], dev)
    got = torch.full_like(want, float('nan'))
    assert _call(host, tdev, len(srcs), got, got.stride(), S, S) == 0
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_letterbox_batch_errors_come_before_any_launch(dev):
    Hc, Wc = 32, 48
    src = torch.from_numpy(LC.image(20, 30, 9)).to(dev)
    dst = torch.full((2, 3, Hc, Wc), float('nan'), device=dev)
    st = dst.stride()
    good = (src, 20, 30, 3, 4, 1)

    def code(rec=good, B=2, Hc_=Hc, Wc_=Wc, fill=114, null=None, patch=None):
        host, tdev = _table([good, rec], dev)
        if patch:
            patch(host[1])
        return _call(None if null == 'host' else host, None if null == 'dev' else tdev, B, dst, st, Hc_, Wc_, fill,
                     dst_ptr=0 if null == 'dst' else None)

    assert code() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all())
    dst.fill_(float('nan'))
    for null in ('host', 'dev', 'dst'):
        assert code(null=null) == ERR_NULL, null
    assert code(patch=lambda r: setattr(r, 'src', None)) == ERR_NULL
    shape_cases = {
        'B0': dict(B=0), 'Hc0': dict(Hc_=0), 'Wc0': dict(Wc_=0), 'Hc65536': dict(Hc_=65536), 'Wc65536': dict(Wc_=65536),
        'h0': dict(patch=lambda r: setattr(r, 'h', 0)), 'w0': dict(patch=lambda r: setattr(r, 'w', 0)),
        'h65536': dict(patch=lambda r: setattr(r, 'h', 65536)), 'w65536': dict(patch=lambda r: setattr(r, 'w', 65536)),
        'pitch': dict(patch=lambda r: setattr(r, 'pitch', 3 * 30 - 1)),
        'nh0': dict(rec=(src, 0, 30, 3, 4, 1)), 'nw0': dict(rec=(src, 20, 0, 3, 4, 1)),
        'top<0': dict(rec=(src, 20, 30, -1, 4, 1)), 'left<0': dict(rec=(src, 20, 30, 3, -1, 1)),
        'bottom': dict(rec=(src, 20, 30, 13, 4, 1)), 'right': dict(rec=(src, 20, 30, 3, 19, 1)),
        'nh>Hc': dict(rec=(src, 33, 30, 0, 0, 1)), 'nw>Wc': dict(rec=(src, 20, 49, 0, 0, 1)),
        'fill-1': dict(fill=-1), 'fill256': dict(fill=256),
    }
    for name, kw in shape_cases.items():
        assert code(**kw) == ERR_SHAPE, name
    assert code(rec=(src, 20, 30, 12, 18, 1)) == 0                   # flush bottom and right is legal
    torch.cuda.synchronize()
    dst.fill_(float('nan'))
    for name, kw in shape_cases.items():
        code(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()), 'a refused call wrote to dst'


# ------------------------------------------------------------------------------------------ rect decode
def _case_id(c):
    return 'C%d-A%d-Fh%d-Fw%d-B%d-ld%d' % c


@functools.lru_cache(maxsize=None)
def _rect_logits(case):
    C, A, Fh, Fw, B, ldl = case
    lg = LC.make_logits_rect(B, Fh, Fw, A, C, ldl, 5)
    anc = HC.decode_anchors(A, 1)
    v = LC.logit_view_rect(lg, ldl, B, Fh, Fw, A, C).reshape(B, A * Fh * Fw, 5 + C)
    lg.setflags(write=False)
    return lg, anc, v


def _needed_const(got, ref64, v):
    got = np.asarray(got, np.float64)
    ref = HC.to_f32_range(ref64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got - ref)
        rel = err / (2.0 ** -23 * np.abs(ref)) - np.abs(v)
    rel = rel[np.isfinite(rel) & (err > HC.TINY)]
    return float(rel.max()) if rel.size else 0.0


def _run_rect(case, scale, dev, box_off, extra):
    C, A, Fh, Fw, B, ldl = case
    L, ptr, stream, check, farr, _ = _abi()
    n_ch, nb = 5 + C, A * Fh * Fw
    lg, anc, v = _rect_logits(case)
    lgd = torch.from_numpy(np.array(lg)).to(dev)
    n_total = nb + box_off + extra
    buf = torch.full((4 + B * n_total * n_ch + 4,), SENT, dtype=torch.int32, device=dev)
    check(L.y4_yolo_decode_eval_rect_f32(ptr(lgd), ldl, ptr(buf[4:]), n_total, box_off, B, Fh, Fw, A, C, farr(anc.ravel()),
                                         8.0, scale, stream()), 'decode_eval_rect')
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:4] == SENT).all() and (h[-4:] == SENT).all()
    body = h[4:-4].reshape(B, n_total, n_ch)
    assert (body[:, :box_off] == SENT).all() and (body[:, box_off + nb:] == SENT).all()
    return np.ascontiguousarray(body[:, box_off:box_off + nb]).view(np.float32)


@pytest.mark.parametrize('scale', LC.SCALES)
@pytest.mark.parametrize('case', LC.RECT_DECODE_CASES, ids=_case_id)
def test_rect_decode_against_fp64(dev, case, scale):
    """y4_yolo_decode_eval_rect_f32 into rows [box_off, box_off + A*Fh*Fw) of a sentinel-filled shared buffer against the
    fp64 rect decode under head_cases.decode_accept (DEC_CONST = 8), at scale_xy 1.0 and 1.2; every other row and 16 bytes
    on either side of the buffer untouched.

    At scale 1.2 the centres of the first column / row cancel (sigma * 1.2 - 0.1 near 0) and the bound, relative to |ref|, goes to
    zero with them: the kernels evaluate those two channels in fp64 and round once (csrc/yolo_decode.hip, eval_centre64)."""
    C, A, Fh, Fw, B, ldl = case
    lg, anc, v = _rect_logits(case)
    ref = LC.decode_ref64_rect(lg, ldl, B, Fh, Fw, A, C, anc, 8.0, scale)
    got = _run_rect(case, scale, dev, box_off=3, extra=2)
    print('decode_eval_rect %s scale %.1f: constant needed: centres %.2f, rest %.2f (allowed %.1f)'
          % (_case_id(case), scale, _needed_const(got[..., :2], ref[..., :2], v[..., :2]),
             _needed_const(got[..., 2:], ref[..., 2:], v[..., 2:]), HC.DEC_CONST))
    ok = HC.decode_accept(got, ref, v)
    bad = np.argwhere(~ok)
    print('   elements outside decode_accept: %d of %d, channels %s' % (len(bad), ok.size, sorted(set(int(i[2]) for i in bad))))
    assert ok.all(), [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)]), float(v[tuple(i)])) for i in bad[:5]]


@pytest.mark.parametrize('case', LC.RECT_DECODE_CASES, ids=_case_id)
def test_rect_decode_centres_at_scale_1_2_within_their_addends(dev, case):
    """scale_xy = 1.2, the centres also against the sum S of their absolute addends (headopt_cases.decode_xy_accept, the
    criterion tests/test_gpu_headopt.py holds the square entry to, same DEC_CONST); every other channel under decode_accept."""
    import headopt_cases as HO
    C, A, Fh, Fw, B, ldl = case
    lg, anc, v = _rect_logits(case)
    ref = LC.decode_ref64_rect(lg, ldl, B, Fh, Fw, A, C, anc, 8.0, 1.2)
    s, h = HO.s_h(1.2)
    sig = HC._sig64(v[..., :2].astype(np.float64)).reshape(B, A, Fh, Fw, 2)
    cell = np.stack(np.broadcast_arrays(np.arange(Fw, dtype=np.float64).reshape(1, 1, 1, Fw),
                                        np.arange(Fh, dtype=np.float64).reshape(1, 1, Fh, 1)), -1)
    Sabs = ((sig * s + h + cell) * 8.0).reshape(B, A * Fh * Fw, 2)
    got = _run_rect(case, 1.2, dev, box_off=2, extra=1)
    print('decode_eval_rect %s scale 1.2: centres need constant %.2f against S (allowed %.1f)'
          % (_case_id(case), HO.decode_xy_needed(got[..., :2], ref[..., :2], v[..., :2], Sabs), HC.DEC_CONST))
    assert HO.decode_xy_accept(got[..., :2], ref[..., :2], v[..., :2], Sabs).all()
    assert HC.decode_accept(got[..., 2:], ref[..., 2:], v[..., 2:]).all()


@pytest.mark.parametrize('scale', LC.SCALES)
@pytest.mark.parametrize('case', [(80, 3, 19, 19, 2, 256), (20, 3, 3, 3, 2, 75), (1, 3, 320, 320, 1, 20)], ids=_case_id)
def test_rect_decode_on_a_square_map_is_the_square_entry(dev, case, scale):
    """Fh == Fw: bit-equal to y4_yolo_decode_eval_ex_f32, on the tiled kernel (16- and 32-pixel tiles) and the per-channel one"""
    C, A, Fh, Fw, B, ldl = case
    L, ptr, stream, check, farr, _ = _abi()
    n_ch, nb = 5 + C, A * Fh * Fw
    lg, anc, _ = _rect_logits(case)
    lgd = torch.from_numpy(np.array(lg)).to(dev)
    want = torch.full((B, nb + 1, n_ch), float('nan'), device=dev)
    check(L.y4_yolo_decode_eval_ex_f32(ptr(lgd), ldl, ptr(want), nb + 1, 1, B, Fh, A, C, farr(anc.ravel()), 8.0, scale, stream()),
          'decode_eval_ex')
    got = _run_rect(case, scale, dev, box_off=1, extra=0)
    assert np.array_equal(got.view(np.int32), want[:, 1:].cpu().numpy().view(np.int32))


def test_rect_decode_refuses_rows_beyond_the_buffer(dev):
    L, ptr, stream, check, farr, _ = _abi()
    C, A, Fh, Fw, B, ldl = 1, 3, 3, 5, 2, 20
    lg = torch.zeros((B * Fh * Fw, ldl), device=dev)
    anc = HC.decode_anchors(A, 1)
    out = torch.full((B, 50, 6), float('nan'), device=dev)
    args = lambda n_total, off, fh=Fh, fw=Fw, s=1.0: (ptr(lg), ldl, ptr(out), n_total, off, B, fh, fw, A, C, farr(anc.ravel()), 8.0, s, stream())
    assert L.y4_yolo_decode_eval_rect_f32(*args(45 + 4, 5)) == ERR_SHAPE          # 5 + 45 > 49
    assert L.y4_yolo_decode_eval_rect_f32(*args(50, -1)) == ERR_SHAPE
    assert L.y4_yolo_decode_eval_rect_f32(*args(50, 0, fh=0)) == ERR_SHAPE
    assert L.y4_yolo_decode_eval_rect_f32(*args(50, 0, fw=0)) == ERR_SHAPE
    assert L.y4_yolo_decode_eval_rect_f32(*args(50, 0, s=2.5)) == ERR_SHAPE
    assert L.y4_yolo_decode_eval_rect_f32(None, *args(50, 0)[1:]) == ERR_NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert L.y4_yolo_decode_eval_rect_f32(*args(50, 5)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:, 5:]).all()) and bool(torch.isnan(out[:, :5]).all())


def test_yololayer_eval_on_a_rectangular_map(dev):
    """YOLOLayer.forward (eval) and decode_into on [B, 255, 9, 13]: the oracle's decode arithmetic with x from the column
    and y from the row; the training branch still refuses the shape."""
    from yolov4_amd import Y4Error
    from yolov4_amd.yolo.model.yololayer import YOLOLayer
    cfg = dict(recipe.MODEL_CFG, SCALE_X_Y=[1.2, 1.1, 1.05])
    B, Fh, Fw = 2, 9, 13
    x = recipe.synth_head_logits(B, 16, 4)[:, :, :Fh, :Fw].contiguous()
    for layer_no in (0, 2):
        lay = YOLOLayer(cfg, layer_no).eval()
        got = lay(x.to(dev)).cpu().numpy()
        nhwc = np.ascontiguousarray(x.numpy().transpose(0, 2, 3, 1)).reshape(B * Fh * Fw, 255)
        anc = np.array(lay._anchors_f32(), np.float32)
        ref = LC.decode_ref64_rect(nhwc, 255, B, Fh, Fw, 3, 80, anc, lay.stride, lay.scale_xy)
        assert got.shape == (B, 3 * Fh * Fw, 85)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * lay.stride)
        out = torch.full((B, 3 * Fh * Fw + 7, 85), float('nan'), device=dev)
        lay.decode_into(x.to(dev), out, 3 * Fh * Fw + 7, 7)
        assert np.array_equal(out[:, 7:].cpu().numpy(), got) and bool(torch.isnan(out[:, :7]).all())
        with pytest.raises(Y4Error):
            lay.train()(x.to(dev))


# ------------------------------------------------------------------------------------------ models
def _close(a, b, atol, rtol):
    a = a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = max(1.0, float(np.abs(b).max()))
    np.testing.assert_allclose(a, b, atol=atol * s, rtol=rtol)


@pytest.fixture(scope='module')
def hip_model(dev, golden):
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    m = YOLOv4(recipe.MODEL_CFG, device=dev)
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, int(golden('model')['seed']))
    m.load_state_dict(sd)
    return m.to(dev)


def _reset(m, golden):
    cpu = {k: v.cpu() for k, v in m.state_dict().items()}
    recipe.fill_state_dict_(cpu, int(golden('model')['seed']))
    m.load_state_dict(cpu)


def test_model_logits_match_oracle_at_288x416(dev, golden, hip_model):
    """(1, 3, 288, 416), train-mode statistics: the three logit maps against oracle.network.RefNet run on the host here and
    now, under test_model_matches_oracle_at_608's close(a, b, 2e-4, 1e-3)."""
    m = hip_model
    _reset(m, golden)
    x = recipe.randn((1, 3, 288, 416), 123)
    sd = NW.empty_state_dict()
    recipe.fill_state_dict_(sd, int(golden('model')['seed']))
    net = NW.RefNet(sd, recipe.MODEL_CFG)
    with torch.no_grad():
        ref = net.forward_train(x)
    m.train()
    with torch.no_grad():
        lg = m.head.logits(*m.neck(*m.backbone(x.to(dev))))
    assert [tuple(t.shape[2:]) for t in lg] == [(36, 52), (18, 26), (9, 13)]
    for a, b in zip(lg, ref):
        d = np.abs(a.cpu().numpy().astype(np.float64) - b.numpy())
        print('logits %s: max |hip - oracle| %.3e, oracle range %.3e' % (tuple(a.shape), d.max(), float(b.abs().max())))
    for a, b in zip(lg, ref):
        _close(a, b, 2e-4, 1e-3)


def test_model_eval_on_rectangular_inputs(dev, golden, hip_model):
    """eval mode on calibrated BatchNorm statistics: the output's shape, every centre inside its input, and 288x416 ->
    416x288 -> 288x416 gives the first and third results bit-equal (no per-shape state survives a shape change)."""
    m = hip_model
    _reset(m, golden)
    recipe.calibrate_bn_(m, recipe.rand((4, 3, 96, 96), 77).to(dev))      # the law of the inputs below (training stays square)
    m.eval()
    B = 2
    xa = recipe.rand((B, 3, 288, 416), 5).to(dev)
    xb = recipe.rand((B, 3, 416, 288), 6).to(dev)
    with torch.no_grad():
        o1 = m(xa).clone()
        o2 = m(xb).clone()
        o3 = m(xa).clone()
    n = 3 * (36 * 52 + 18 * 26 + 9 * 13)
    assert tuple(o1.shape) == (B, n, 85) and tuple(o2.shape) == (B, n, 85)
    for o, (H, W) in ((o1, (288, 416)), (o2, (416, 288))):
        # (a random-weight net may overflow exp() in a width or height; centres and confidences are sigmoids)
        assert bool(torch.isfinite(o[..., :2]).all()) and bool(torch.isfinite(o[..., 4:]).all())
        assert 0.0 <= float(o[..., 4:].min()) and float(o[..., 4:].max()) <= 1.0
        assert 0.0 <= float(o[..., 0].min()) and float(o[..., 0].max()) <= W
        assert 0.0 <= float(o[..., 1].min()) and float(o[..., 1].max()) <= H
        assert float(o[..., 0].max()) > W - 32 and float(o[..., 1].max()) > H - 32          # the last column / row of cells is there
    assert torch.equal(o1, o3)
    # the rows are the three layers' maps, row-major: the x-centre of the stride-32 layer's first anchor walks 13 columns
    xs = o1[0, 3 * (36 * 52 + 18 * 26):3 * (36 * 52 + 18 * 26) + 9 * 13, 0].reshape(9, 13).cpu().numpy()
    cell = xs / 32 - np.arange(13)[None, :]
    assert (cell >= 0).all() and (cell <= 1).all()


def test_tiny_model_eval_on_a_rectangular_input(dev):
    from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
    m = YOLOv4Tiny(default_cfg())
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, 7)
    m.load_state_dict(sd)
    m = m.to(dev)
    recipe.calibrate_bn_(m, recipe.randn((4, 3, 64, 64), 3).to(dev))
    m.eval()
    with torch.no_grad():
        o = m(recipe.rand((2, 3, 96, 160), 4).to(dev))
    assert tuple(o.shape) == (2, 3 * (6 * 10 + 3 * 5), 85) and bool(torch.isfinite(o).all())
    assert float(o[..., 0].max()) <= 160 and float(o[..., 1].max()) <= 96 and float(o[..., 0].max()) > 96


# ------------------------------------------------------------------------------------------ end to end
S = 64
CFG = {'MODEL': recipe.MODEL_CFG, 'TEST': {'IMGSIZE': S, 'CONFTHRE': 0.3, 'NMSTHRE': 0.45}}
SOURCES = ['s29x37_420', 's48x40_444', 's16x2_444']           # three aspects: 37 x 29, 40 x 48, 2 x 16 (h x w)


def test_detect_images_rect_is_the_manual_chain(dev, golden, hip_model):
    """detect_images(letterbox='rect') on three golden JPEGs of different aspect, in chunks of two: row for row the chain
    decode_jpeg_batch -> letterbox_batch -> model -> postprocess -> letterbox2yxyx; every box inside its image;
    letterbox=None is the call without the keyword."""
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.data.jpeg import decode_jpeg_batch
    from yolov4_amd.yolo.data.transform import letterbox_batch
    from yolov4_amd.yolo.util.utils import letterbox2yxyx, postprocess
    m = hip_model
    _reset(m, golden)
    recipe.calibrate_bn_(m, recipe.randn((8, 3, S, S), 3).to(dev))
    files = [J.read(n) for n in SOURCES]
    conf = 0.02
    out = detect_images(m, CFG, files, conf_thre=conf, letterbox='rect', draw=False, encode=False, batch=2)
    assert len(out) == 3 and not m.training
    total = 0
    canvases = []
    for start in (0, 2):
        imgs = decode_jpeg_batch(files[start:start + 2])
        x, infos = letterbox_batch(imgs, S, 'rect', 32)
        canvases.append(tuple(x.shape[2:]))
        with torch.no_grad():
            dets = postprocess(m(x), 80, conf_thre=conf, nms_thre=0.45)
        for k, (d, info) in enumerate(zip(dets, infos)):
            got = out[start + k]['detections']
            h, w = info[:2]
            assert tuple(out[start + k]['image'].shape) == (h, w, 3) and out[start + k]['jpeg'] is None
            if d is None:
                assert got.shape == (0, 7)
                continue
            r = d.cpu().numpy().astype(np.float64)
            y1, x1, y2, x2 = letterbox2yxyx([r[:, 1], r[:, 0], r[:, 3], r[:, 2]], info)
            want = np.concatenate([np.stack([y1, x1, y2, x2], 1), r[:, 4:7]], 1)
            assert got.dtype == np.float64 and np.array_equal(got, want)
            assert (got[:, [0, 2]] >= 0).all() and (got[:, [0, 2]] <= h).all()
            assert (got[:, [1, 3]] >= 0).all() and (got[:, [1, 3]] <= w).all()
            total += len(got)
    assert canvases == [(64, 64), (32, 64)], canvases               # the second chunk holds the flat image alone
    assert total > 0, 'no detection at all: the comparison above compared nothing'
    sq = detect_images(m, CFG, files, conf_thre=conf, letterbox='square', draw=False, encode=False, batch=2)
    assert len(sq) == 3 and all(r['detections'].shape[1] == 7 for r in sq)
    a = detect_images(m, CFG, files, conf_thre=conf, draw=False, encode=False, batch=2)
    b = detect_images(m, CFG, files, conf_thre=conf, letterbox=None, draw=False, encode=False, batch=2)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra['detections'], rb['detections']) and torch.equal(ra['image'], rb['image'])
    with pytest.raises(ValueError):
        detect_images(m, CFG, files, letterbox='tight')


def test_detect_images_rect_with_tiny_scale_xy_and_nms_options(dev):
    """YOLOv4-tiny, SCALE_X_Y and the NMS options sit behind the same decode and postprocess: they run with 'rect'."""
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
    from yolov4_amd.yolo.util.utils import NMSOptions
    mc = dict(default_cfg(), SCALE_X_Y=[1.05, 1.05])
    m = YOLOv4Tiny(mc)
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, 7)
    m.load_state_dict(sd)
    m = m.to(dev)
    recipe.calibrate_bn_(m, recipe.randn((4, 3, S, S), 3).to(dev))
    cfg = {'MODEL': mc, 'TEST': {'IMGSIZE': S, 'CONFTHRE': 0.02, 'NMSTHRE': 0.45}}
    files = [J.read(n) for n in SOURCES]
    out = detect_images(m, cfg, files, letterbox='rect', draw=False, encode=False,
                        nms_options=NMSOptions(metric='diou', agnostic=True, max_det=5))
    for r, n in zip(out, SOURCES):
        d = r['detections']
        w, h = J.FIXTURES[n]['width'], J.FIXTURES[n]['height']
        assert d.shape[1] == 7 and len(d) <= 5 and np.isfinite(d).all()
        assert (d[:, [0, 2]] >= 0).all() and (d[:, [0, 2]] <= h).all() and (d[:, [1, 3]] >= 0).all() and (d[:, [1, 3]] <= w).all()


def test_validate_maps_boxes_back_through_the_pad(dev):
    """validate() over a two-batch stand-in loader that emits target['pad']: every record's bbox is letterbox2xywh of the raw
    detection; without the key the records are the stretch arithmetic's."""
    from yolov4_amd.yolo.engine.build import validate
    from yolov4_amd.yolo.util.utils import letterbox2xywh, postprocess, yolobox2xywh
    p, C, conf, thre, props = HC.make_post_case('n65')               # 3 images: batches of 2 and 1
    pred = torch.from_numpy(p)

    class Stub(torch.nn.Module):
        at = 0

        def forward(self, x):
            out = pred[self.at:self.at + x.shape[0]].clone().to(x.device)
            self.at += x.shape[0]
            return out

    # [h, w, nh, nw, id, index] and (top, left) on a 400 x 400 canvas, the extent of the case's boxes
    info = torch.tensor([[480., 640., 300., 400., 17., 0.], [500., 333., 400., 266., 42., 1.], [400., 400., 400., 400., 7., 2.]])
    pads = [[50, 0], [0, 67], [0, 0]]
    loader = [(torch.zeros(2, 3, 8, 8), {'img_info': info[:2], 'pad': pads[:2]}),
              (torch.zeros(1, 3, 8, 8), {'img_info': info[2:], 'pad': torch.tensor(pads[2:])})]
    assert validate(loader, Stub(), conf, thre, device=dev, num_classes=C) == (0, 0)
    recs = validate.records
    raw = postprocess(pred.clone().to(dev), C, conf, thre)
    want, stretch = [], []
    for d, i, pad in zip(raw, info.tolist(), pads):
        for r in (d.cpu().numpy().astype(np.float64) if d is not None else []):
            box = (float(r[1]), float(r[0]), float(r[3]), float(r[2]))
            want.append(letterbox2xywh(box, i[:4] + [float(pad[0]), float(pad[1])]))
            stretch.append(yolobox2xywh(box, i[:4]))
    assert len(recs) == len(want) > 0 and [r['bbox'] for r in recs] == want
    assert [r['image_id'] for r in recs] == [int(i[4]) for d, i in zip(raw, info.tolist()) for _ in range(0 if d is None else len(d))]
    for r in recs:
        i = next(row for row in info.tolist() if int(row[4]) == r['image_id'])
        x, y, w, h = r['bbox']
        assert 0 <= x <= i[1] and 0 <= y <= i[0] and 0 <= w and x + w <= i[1] + 1e-9 and 0 <= h and y + h <= i[0] + 1e-9
    loader = [(torch.zeros(2, 3, 8, 8), {'img_info': info[:2]}), (torch.zeros(1, 3, 8, 8), {'img_info': info[2:]})]
    validate(loader, Stub(), conf, thre, device=dev, num_classes=C)
    assert [r['bbox'] for r in validate.records] == stretch and stretch != want


# ------------------------------------------------------------------------------------------ loader
IMAGES = [(42, 's48x40_420'), (7, 's17x33_444'), (1000, 's29x37_422'), (9, 's16x2_420')]       # (image id, fixture), JSON order
LOADER_CFG = {'DATA': {'MAX_NUM_LABELS': 6}, 'MODEL': recipe.MODEL_CFG}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('coco_lb'))
    doc = {'images': [{'id': i, 'file_name': '%012d.jpg' % i, 'width': J.FIXTURES[n]['width'], 'height': J.FIXTURES[n]['height']}
                      for i, n in IMAGES],
           'categories': [{'id': 3, 'name': 'c'}, {'id': 1, 'name': 'a'}],
           'annotations': [
               {'id': 1, 'image_id': 42, 'category_id': 3, 'bbox': [4.0, 5.0, 10.0, 12.0], 'area': 120.0, 'iscrowd': 0},
               {'id': 2, 'image_id': 1000, 'category_id': 1, 'bbox': [1.0, 2.0, 20.0, 30.0], 'area': 600.0, 'iscrowd': 0},
               {'id': 3, 'image_id': 7, 'category_id': 1, 'bbox': [3.0, 3.0, 9.0, 20.0], 'area': 180.0, 'iscrowd': 0}]}
    os.makedirs(os.path.join(root, 'annotations'))
    with open(os.path.join(root, 'annotations', 'instances_val2017.json'), 'w') as f:
        json.dump(doc, f)
    os.makedirs(os.path.join(root, 'images', 'val2017'))
    for i, n in IMAGES:
        shutil.copy(os.path.join(J.JPEG_DIR, n + '.jpg'), os.path.join(root, 'images', 'val2017', '%012d.jpg' % i))
    return root


def test_batch_loader_letterbox(dev, golden, tree):
    """COCOBatchLoader(letterbox=...) in validation: inputs equal to letterbox_ref of the decoded files, labels mapped onto
    the canvas, img_info rows [h, w, nh, nw, id, index], target['pad'] rows (top, left); 'rect' orders by h / w; None is
    the loader without the keyword."""
    from yolov4_amd.yolo.data.cocodataset import COCOBatchLoader, COCODataset
    npz = golden('jpeg')
    bgr = {n: np.ascontiguousarray(npz[n][..., ::-1]) for _, n in IMAGES}
    ds = COCODataset(tree, name='val2017', img_size=64, is_train=False)
    hw = [bgr[n].shape[:2] for _, n in IMAGES]
    assert [ds.img_hw(k) for k in range(4)] == hw
    order = sorted(range(4), key=lambda k: hw[k][0] / hw[k][1])
    assert order != [0, 1, 2, 3]
    for mode, want_order in (('rect', order), ('square', [0, 1, 2, 3])):
        batches = list(COCOBatchLoader(ds, 2, LOADER_CFG, letterbox=mode))
        assert len(batches) == 2
        seen = []
        for x, target in batches:
            Hc, Wc = x.shape[2:]
            assert (Hc, Wc) == (64, 64) if mode == 'square' else (Hc % 32 == 0 and Wc % 32 == 0 and max(Hc, Wc) == 64)
            assert sorted(target) == ['img_info', 'pad', 'padded_labels'] and tuple(target['padded_labels'].shape) == (2, 6, 5)
            for b, (info, pad) in enumerate(zip(target['img_info'], target['pad'])):
                h, w, nh, nw, img_id, index = info
                n = IMAGES[index][1]
                assert (h, w) == hw[index] and img_id == IMAGES[index][0]
                assert list(pad) == [(Hc - nh) // 2, (Wc - nw) // 2]
                assert np.array_equal(x[b].cpu().numpy(), LC.letterbox_ref(bgr[n], nh, nw, pad[0], pad[1], Hc, Wc))
                lab = target['padded_labels'][b].numpy()
                rows = ds.get_labels(index)
                assert (lab[len(rows):] == 0).all()
                for r, g_ in zip(rows, lab):
                    x1, y1, x2, y2 = LC.forward_box([r[0], r[1], r[0] + r[2], r[1] + r[3]], [h, w, nh, nw, pad[0], pad[1]])
                    assert list(g_) == [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, r[4]]
                seen.append(index)
        assert seen == want_order
    plain = list(COCOBatchLoader(ds, 2, LOADER_CFG))
    same = list(COCOBatchLoader(ds, 2, LOADER_CFG, letterbox=None))
    for (x1, t1), (x2, t2) in zip(plain, same):
        assert torch.equal(x1, x2) and t1['img_info'] == t2['img_info'] and 'pad' not in t1 and 'pad' not in t2
        assert torch.equal(t1['padded_labels'], t2['padded_labels'])
