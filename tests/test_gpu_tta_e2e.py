# -*- coding: utf-8 -*-
"""Test-time augmentation end to end on a randomly initialised YOLOv4-tiny at a 64 x 96 input (conf 0.001 gives candidates
without training): tta_predict against the model itself, detect_images(tta=...) and validate(tta=...) against the manual
composition views -> model -> merge -> post-process, both merges, letterboxed ('rect') and stretched input; tta=None is the
call without the keyword.  The kernels themselves are pinned in tests/test_gpu_tta.py."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

CONF, NMS = 0.001, 0.45
C = 80


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tiny(dev):
    from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
    mc = default_cfg()
    m = YOLOv4Tiny(mc)
    sd = m.state_dict()
    recipe.fill_state_dict_(sd, 7)
    m.load_state_dict(sd)
    m = m.to(dev)
    recipe.calibrate_bn_(m, recipe.randn((4, 3, 64, 64), 3).to(dev))
    m.eval()
    return m, mc


def _opts(merge='nms', **kw):
    from yolov4_amd.yolo.util.tta import TTAOptions
    return TTAOptions(merge=merge, **kw)


def _manual(m, x, opts, nms_options=None):
    """views -> model -> merge -> post-process, step by step"""
    from yolov4_amd.yolo.util.tta import merge_views, tta_views
    from yolov4_amd.yolo.util.utils import postprocess, postprocess_nms, postprocess_wbf
    views = tta_views(x, opts, 32)
    with torch.no_grad():
        preds = [m(v) for v, _ in views]
    merged = merge_views(preds, [meta for _, meta in views])
    assert merged.shape[1] == sum(p.shape[1] for p in preds)
    if opts.merge == 'wbf':
        kw = {k: v for k, v in (nms_options or {}).items() if k in ('agnostic', 'max_det')}
        return postprocess_wbf(merged, C, CONF, opts.wbf_thre, views=len(views), **kw)
    if nms_options is None:
        return postprocess(merged, C, CONF, NMS)
    return postprocess_nms(merged, C, CONF, NMS, **nms_options)


def _same(a, b):
    assert len(a) == len(b)
    n = 0
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            n += len(x)
    return n


def test_identity_view_alone_is_the_model(dev, tiny):
    from yolov4_amd.yolo.util.tta import tta_predict
    m, _ = tiny
    x = recipe.rand((2, 3, 64, 96), 4).to(dev)
    with torch.no_grad():
        want = m(x)
        got = tta_predict(m, x, _opts(scales=(1.0,), flips=(False,)))
        both = tta_predict(m, x, _opts(scales=(1.0, 1.0), flips=(False, True)))
    N = want.shape[1]
    assert N == 3 * (4 * 6 + 2 * 3) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert tuple(both.shape) == (2, 2 * N, 85) and torch.equal(both[:, :N].view(torch.int32), want.view(torch.int32))
    # the mirrored view's rows: the model on the column-reversed input, centres mirrored back (W - cx, one subtraction)
    with torch.no_grad():
        flipped = m(torch.flip(x, dims=[3]).contiguous())
    back = flipped.clone()
    back[:, :, 0] = 96.0 - flipped[:, :, 0]
    assert torch.equal(both[:, N:].view(torch.int32), back.view(torch.int32))
    assert bool(torch.isfinite(both).all())


def test_default_views_row_counts_and_boxes_in_the_base_canvas(dev, tiny):
    from yolov4_amd.yolo.util.tta import tta_predict
    m, _ = tiny
    x = recipe.rand((2, 3, 64, 96), 4).to(dev)
    with torch.no_grad():
        merged = tta_predict(m, x, _opts())
    # 1.0: 64 x 96; 0.83 mirrored: 53 x 79 -> 64 x 96; 0.67: 42 x 64 -> 64 x 64
    assert merged.shape[1] == 3 * (4 * 6 + 2 * 3) * 2 + 3 * (4 * 4 + 2 * 2)
    cx, cy = merged[:, :, 0], merged[:, :, 1]
    assert float(cx.min()) >= 0 and float(cy.min()) >= 0
    assert float(cx.max()) <= 96 * 96.0 / 79 + 1e-3 and float(cy.max()) <= 64 * 64.0 / 42 + 1e-3


SIZES = [(40, 60), (30, 50), (48, 40)]


def _sources(dev):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev) for h, w in SIZES]


@pytest.mark.parametrize('nms_options', (None, dict(agnostic=True, max_det=30)), ids=('plain', 'agnostic-maxdet'))
@pytest.mark.parametrize('merge', ('nms', 'wbf'))
@pytest.mark.parametrize('letterbox', (None, 'rect'), ids=('stretch', 'rect'))
def test_detect_images_tta_is_the_manual_chain(dev, tiny, letterbox, merge, nms_options):
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.data.transform import letterbox_batch, val_batch
    from yolov4_amd.yolo.util.utils import letterbox2yxyx, yolobox2yxyx
    m, mc = tiny
    S = 96 if letterbox else 64
    cfg = {'MODEL': mc, 'TEST': {'IMGSIZE': S, 'CONFTHRE': CONF, 'NMSTHRE': NMS}}
    opts = _opts(merge)
    src = _sources(dev)
    out = detect_images(m, cfg, src, letterbox=letterbox, tta=opts, nms_options=nms_options, draw=False, encode=False, batch=2)
    total = 0
    for start in (0, 2):
        imgs = [s.clone() for s in src[start:start + 2]]
        x, infos = letterbox_batch(imgs, S, 'rect', 32) if letterbox else val_batch(imgs, S)
        if letterbox and start == 0:
            assert tuple(x.shape) == (2, 3, 64, 96)
        dets = _manual(m, x, opts, nms_options)
        for k, (d, info) in enumerate(zip(dets, infos)):
            got = out[start + k]['detections']
            if d is None:
                assert got.shape == (0, 7)
                continue
            r = d.cpu().numpy().astype(np.float64)
            box = [r[:, 1], r[:, 0], r[:, 3], r[:, 2]]
            y1, x1, y2, x2 = letterbox2yxyx(box, info) if letterbox else yolobox2yxyx(box, info[:4])
            want = np.concatenate([np.stack([y1, x1, y2, x2], 1), r[:, 4:7]], 1)
            assert np.array_equal(got, want)
            if nms_options:
                assert len(got) <= 30
            if merge == 'wbf':
                assert (got[:, 4] == 1.0).all()
            total += len(got)
    assert total > 0, 'no detection at all: the comparison above compared nothing'


def test_detect_images_without_tta_is_unchanged(dev, tiny):
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.data.transform import val_batch
    from yolov4_amd.yolo.util.utils import postprocess, postprocess_nms, yolobox2yxyx
    m, mc = tiny
    cfg = {'MODEL': mc, 'TEST': {'IMGSIZE': 64, 'CONFTHRE': CONF, 'NMSTHRE': NMS}}
    src = _sources(dev)[:2]
    for nms_options in (None, dict(metric='diou', max_det=20)):
        a = detect_images(m, cfg, src, draw=False, encode=False, nms_options=nms_options)
        b = detect_images(m, cfg, src, draw=False, encode=False, nms_options=nms_options, tta=None)
        x, infos = val_batch([s.clone() for s in src], 64)
        with torch.no_grad():
            p = m(x)
        dets = postprocess(p, C, CONF, NMS) if nms_options is None else postprocess_nms(p, C, CONF, NMS, **nms_options)
        assert sum(len(r['detections']) for r in a) > 0
        for ra, rb, d, info in zip(a, b, dets, infos):
            r = d.cpu().numpy().astype(np.float64)
            y1, x1, y2, x2 = yolobox2yxyx([r[:, 1], r[:, 0], r[:, 3], r[:, 2]], info[:4])
            want = np.concatenate([np.stack([y1, x1, y2, x2], 1), r[:, 4:7]], 1)
            assert np.array_equal(ra['detections'], want) and np.array_equal(rb['detections'], want)
    with pytest.raises(ValueError):
        detect_images(m, cfg, src, tta=_opts('wbf'), nms_options=dict(soft='linear'))


@pytest.mark.parametrize('merge', ('nms', 'wbf'))
@pytest.mark.parametrize('padded', (False, True), ids=('stretch', 'letterbox'))
def test_validate_tta_is_the_manual_chain(dev, tiny, padded, merge):
    from yolov4_amd.yolo.engine.build import validate
    from yolov4_amd.yolo.util.utils import detections_to_coco, postprocess
    m, _ = tiny
    xs = [recipe.rand((2, 3, 64, 96), 4), recipe.rand((1, 3, 64, 96), 5)]
    # [h, w, nh, nw, id, index]; letterboxed: (top, left) of the nh x nw image on the 64 x 96 canvas
    info = torch.tensor([[400., 600., 64., 96., 17., 0.], [300., 500., 58., 96., 42., 1.], [480., 400., 64., 54., 7., 2.]])
    pads = [[0, 0], [3, 0], [0, 21]]

    def loader():
        for x, sl in zip(xs, (slice(0, 2), slice(2, 3))):
            t = {'img_info': info[sl]}
            if padded:
                t['pad'] = pads[sl]
            yield x, t

    def records(dets):
        out = []
        for d, i, pad in zip(dets, info.tolist(), pads):
            kw = {'pad': [float(v) for v in pad]} if padded else {}
            out.extend(detections_to_coco(d, i[:4], int(i[4]), **kw))
        return out
    opts = _opts(merge)
    assert validate(loader(), m, CONF, NMS, device=dev, num_classes=C, tta=opts) == (0, 0)
    got = validate.records
    want = records([d for x in xs for d in _manual(m, x.to(dev), opts)])
    assert got == want and len(got) > 0
    # tta=None: the parent's calls
    validate(loader(), m, CONF, NMS, device=dev, num_classes=C, tta=None)
    plain = validate.records
    validate(loader(), m, CONF, NMS, device=dev, num_classes=C)
    with torch.no_grad():
        direct = records([d for x in xs for d in postprocess(m(x.to(dev)), C, CONF, NMS)])
    assert plain == validate.records == direct and len(direct) > 0 and direct != want
