# -*- coding: utf-8 -*-
"""CPU checks of letterboxed / rectangular-batch inference: the geometry, the NumPy restatement of the batch kernel
(letterbox_cases.letterbox_ref) pinned against oracle.preprocess and float bilinear sampling, the box mapping, the rect
decode restatement, and the command line.  No GPU."""
import os

import numpy as np
import pytest
import torch

import head_cases as HC
import letterbox_cases as LC
from oracle import preprocess as OP
from yolov4_amd import detect as DET
from yolov4_amd.yolo.data import transform as T
from yolov4_amd.yolo.util.utils import (COCO_CLASS_IDS, detections_to_coco, letterbox2xywh, letterbox2yxyx, yolobox2xywh)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize('hws,size,canvas,off', LC.GEOMETRY, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_geometry_table(hws, size, canvas, off):
    h, w, S = hws
    assert T.letterbox_geometry(h, w, S) == size
    Hc, Wc = T.letterbox_canvas([size], S, 'rect', 32)
    assert (Hc, Wc) == canvas
    assert T.letterbox_offsets(size[0], size[1], Hc, Wc) == off
    assert T.letterbox_canvas([size], S, 'square', 32) == (S, S)
    assert Hc % 32 == 0 and Wc % 32 == 0 and Hc <= S and Wc <= S and max(size) == S


def test_geometry_mixed_batch_and_errors():
    a, b = T.letterbox_geometry(480, 640, 608), T.letterbox_geometry(640, 480, 608)
    assert T.letterbox_canvas([a, b], 608, 'rect', 32) == (608, 608)
    assert T.letterbox_offsets(a[0], a[1], 608, 608) == (76, 0) and T.letterbox_offsets(b[0], b[1], 608, 608) == (0, 76)
    for mode in ('square', 'rect'):
        with pytest.raises(ValueError):
            T.letterbox_canvas([(600, 450)], 600, mode, 32)
    with pytest.raises(ValueError):
        T.letterbox_canvas([a], 608, 'stretch', 32)
    assert T.letterbox_mode(None) is None and T.letterbox_mode('off') is None and T.letterbox_mode('rect') == 'rect'
    with pytest.raises(ValueError):
        T.letterbox_mode('tight')
    # the stride comes from the model's configuration: 32 for both networks
    from yolov4_amd.yolo.model.yololayer import layer_strides
    from yolov4_amd.yolo.model.yolov4_tiny import default_cfg as tiny_cfg
    import recipe
    assert max(layer_strides(recipe.MODEL_CFG, [8, 16, 32])) == 32 and max(layer_strides(tiny_cfg(), [8, 16, 32])) == 32


def test_every_batch_record_fits_its_canvas():
    Hc, Wc = LC.CANVAS
    tops, lefts, bottoms, rights = set(), set(), set(), set()
    for h, w, nh, nw, top, left, swap in LC.BATCH:
        assert 0 <= top and top + nh <= Hc and 0 <= left and left + nw <= Wc and nh >= 1 and nw >= 1
        tops.add(top == 0); lefts.add(left == 0); bottoms.add(top + nh == Hc); rights.add(left + nw == Wc)
    assert all(True in s for s in (tops, lefts, bottoms, rights)), 'a placement flush to each edge'
    assert any(nh == 1 for _, _, nh, _, _, _, _ in LC.BATCH) and any(w == 2 * nw and h == 2 * nh for h, w, nh, nw, _, _, _ in LC.BATCH)
    assert {s for *_, s in LC.BATCH} == {0, 1}
    assert any(left % 4 for *_, left, _ in LC.BATCH)
    assert sorted({(h, w) for h, w, *_ in LC.BATCH}) == sorted([(37, 29), (29, 37), (1, 300), (300, 9), (96, 128), (1, 1), (13, 21)])


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('h,w,S', [(37, 29, 64), (29, 37, 64), (1, 300, 64), (300, 9, 64), (96, 96, 48), (1, 1, 64), (480, 640, 96),
                                   (128, 128, 64)])
def test_letterbox_ref_in_stretch_geometry_is_the_oracle(h, w, S):
    img = LC.image(h, w, 5 + h + w)
    want, _ = OP.val_input(img, S)
    got = LC.letterbox_ref(img, S, S, 0, 0, S, S, 114, swap_rb=True)
    assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize('h,w,nh,nw', [(37, 29, 64, 50), (480, 640, 72, 96), (13, 21, 40, 64), (300, 9, 64, 2), (96, 128, 48, 64)])
def test_letterbox_ref_interior_is_within_one_lsb_of_float_bilinear(h, w, nh, nw):
    img = LC.image(h, w, 11)
    top, left = 3, 5
    got = LC.letterbox_ref(img, nh, nw, top, left, nh + 7, nw + 9, 114, swap_rb=False)
    inner = got[:, top:top + nh, left:left + nw].transpose(1, 2, 0).astype(np.float64) * 255.0
    assert np.abs(inner - LC.bilinear_float(img, nh, nw)).max() <= 1.0 + 1e-9
    outside = np.ones(got.shape[1:], bool)
    outside[top:top + nh, left:left + nw] = False
    assert (got[:, outside] == np.float32(114) / np.float32(255)).all()


def test_letterbox_ref_swaps_channels_and_takes_the_area_path_on_both_axes_only():
    img = LC.image(96, 128, 3)
    a = LC.letterbox_ref(img, 48, 64, 0, 0, 48, 64, 0, swap_rb=True)
    b = LC.letterbox_ref(img, 48, 64, 0, 0, 48, 64, 0, swap_rb=False)
    assert np.array_equal(a, b[::-1])
    box = ((img[0::2, 0::2].astype(int) + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2)
    assert np.array_equal(b, box.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    # 2x in y only: the linear path
    c = LC.resize_linear_u8(img, 48, 60)
    assert c.shape == (48, 60, 3) and not np.array_equal(c[:, :8], box[:, :8].astype(np.uint8))


# ------------------------------------------------------------------------------------------ box mapping
def test_box_round_trip():
    rng = np.random.RandomState(2)
    for (h, w, S), (nh, nw), (Hc, Wc), (top, left) in LC.GEOMETRY:
        info = [h, w, nh, nw, top, left]
        for _ in range(20):
            x = np.sort(rng.uniform(0, w, 2)); y = np.sort(rng.uniform(0, h, 2))
            fx1, fy1, fx2, fy2 = LC.forward_box([x[0], y[0], x[1], y[1]], info)
            y1, x1, y2, x2 = letterbox2yxyx([fy1, fx1, fy2, fx2], info)
            assert max(abs(x1 - x[0]), abs(x2 - x[1]), abs(y1 - y[0]), abs(y2 - y[1])) <= 1e-9
            bx = letterbox2xywh([fy1, fx1, fy2, fx2], info)
            assert bx == [x1, y1, x2 - x1, y2 - y1]
    # arrays go through in float64, as yolobox2yxyx takes them
    arr = letterbox2yxyx([np.array([12.0, 500.0]), np.array([0.0, 700.0]), np.array([240.0, 480.0]), np.array([304.0, 608.0])],
                         [480, 640, 456, 608, 12, 0])
    assert arr[0].dtype == np.float64 and np.array_equal(arr[0], [0.0, 480.0]) and np.array_equal(arr[3], [320.0, 640.0])


def test_box_in_the_pad_band_is_clipped_onto_the_edge():
    info = [480, 640, 456, 608, 12, 0]                      # 12 rows of padding above and below
    assert letterbox2yxyx([2.0, 100.0, 10.0, 200.0], info) == [0.0, 100.0 * 640 / 608, 0.0, 200.0 * 640 / 608]
    assert letterbox2yxyx([470.0, -5.0, 479.0, 700.0], info) == [480.0, 0.0, 480.0, 640.0]
    assert letterbox2xywh([2.0, 100.0, 10.0, 200.0], info)[2:] == [100.0 * 640 / 608, 0.0]
    # multiply, then divide, in double
    assert letterbox2yxyx([100.3, 7.1, 150.9, 33.7], info) == [(100.3 - 12) * 480 / 456, 7.1 * 640 / 608, (150.9 - 12) * 480 / 456,
                                                              33.7 * 640 / 608]


def test_detections_to_coco_without_pad_is_unchanged():
    g = np.load(os.path.join(GOLDEN, 'coco.npz'))
    for ci in range(3):
        det = torch.from_numpy(g['c%d.det' % ci])
        info = list(g['c%d.info' % ci])
        recs = detections_to_coco(det, info, image_id=ci, pad=None)
        assert recs == detections_to_coco(det, info, image_id=ci) and len(recs) == det.shape[0]
        for r, bb, sc in zip(recs, g['c%d.bbox' % ci], g['c%d.score' % ci]):
            assert r['bbox'] == list(bb) and r['score'] == sc
        # with a pad the boxes are letterbox2xywh's, clipped; everything else stays
        h, w = int(info[0]), int(info[1])
        nh, nw = T.letterbox_geometry(h, w, int(info[2]))
        top, left = T.letterbox_offsets(nh, nw, int(info[2]), int(info[3]))
        padded = detections_to_coco(det, [h, w, nh, nw], image_id=ci, pad=(top, left))
        for r, p, d in zip(recs, padded, g['c%d.det' % ci].astype(np.float64)):
            assert p['bbox'] == letterbox2xywh((d[1], d[0], d[3], d[2]), [h, w, nh, nw, top, left])
            assert 0 <= p['bbox'][0] <= w and 0 <= p['bbox'][1] <= h and p['bbox'][0] + p['bbox'][2] <= w + 1e-9
            assert {k: v for k, v in p.items() if k != 'bbox'} == {k: v for k, v in r.items() if k != 'bbox'}
    assert detections_to_coco(None, [1, 1, 1, 1], 0, pad=(0, 0)) == []
    assert yolobox2xywh((1.0, 2.0, 3.0, 4.0), (10, 20, 5, 5)) == [2.0 / 5 * 20, 1.0 / 5 * 10, 2.0 / 5 * 20, 2.0 / 5 * 10]


def test_letterbox_labels_are_the_forward_mapping():
    info = [480, 640, 456, 608, 12, 0]
    rows = np.array([[10.0, 20.0, 100.0, 50.0, 3.0], [0.0, 0.0, 640.0, 480.0, 7.0]])
    got = T.letterbox_labels(rows, info)
    for r, g_ in zip(rows, got):
        assert list(g_[:4]) == LC.forward_box([r[0], r[1], r[0] + r[2], r[1] + r[3]], info) and g_[4] == r[4]
    assert list(got[1][:4]) == [0.0, 12.0, 608.0, 468.0]


# ------------------------------------------------------------------------------------------ rect decode restatement
@pytest.mark.parametrize('case', [c for c in HC.DECODE_CASES if c[2] <= 19], ids=lambda c: 'C%d-A%d-F%d-B%d-ld%d' % c)
def test_rect_decode_ref_is_the_square_one_on_square_maps(case):
    C, A, F, B, ldl = case
    lg, _ = HC.make_logits(B, F, A, C, ldl, 5)
    assert np.array_equal(LC.make_logits_rect(B, F, F, A, C, ldl, 5), lg, equal_nan=True)
    anc = HC.decode_anchors(A, 1)
    want = HC.decode_ref64(lg, ldl, B, F, A, C, anc, 16.0, False)
    got = LC.decode_ref64_rect(lg, ldl, B, F, F, A, C, anc, 16.0)
    assert np.array_equal(got, want)
    import headopt_cases as HO
    want12, _ = HO.decode_ref64(lg, ldl, B, F, A, C, anc, 16.0, False, 1.2)
    assert np.array_equal(LC.decode_ref64_rect(lg, ldl, B, F, F, A, C, anc, 16.0, 1.2), want12)


def test_rect_decode_ref_takes_x_from_columns_and_y_from_rows():
    C, A, Fh, Fw, B, ldl = 1, 3, 3, 5, 2, 20
    lg = np.zeros((B * Fh * Fw, ldl), np.float32)           # sigmoid(0) = 0.5, exp(0) = 1
    anc = HC.decode_anchors(A, 1)
    r = LC.decode_ref64_rect(lg, ldl, B, Fh, Fw, A, C, anc, 8.0).reshape(B, A, Fh, Fw, 6)
    assert np.array_equal(r[0, 0, :, :, 0], np.tile((np.arange(Fw) + 0.5) * 8.0, (Fh, 1)))
    assert np.array_equal(r[1, 2, :, :, 1], np.tile(((np.arange(Fh) + 0.5) * 8.0)[:, None], (1, Fw)))
    assert np.array_equal(r[0, 1, :, :, 2], np.full((Fh, Fw), np.float64(anc[1, 0]) * 8.0))
    # the case table: tiles and dispatch as the comments say
    sizes = {(c[2] * c[3]) % LC.rect_tile(c[4], c[2], c[3]) for c in LC.RECT_DECODE_CASES}
    assert 13 in sizes and LC.rect_tile(1, 250, 400) == 32 and LC.rect_tile(2, 15, 19) == 16
    assert not HC.decode_takes_tiled(20, 3, 75) and HC.decode_takes_tiled(59, 4, 256) and HC.decode_takes_tiled(80, 3, 256)


# ------------------------------------------------------------------------------------------ command line
def test_cli_letterbox_flag_and_cfg_default():
    ap = DET.build_parser()
    base = ['--cfg', 'c.json', '--source', 'x.jpg']
    assert ap.parse_args(base).letterbox is None
    for v in ('off', 'square', 'rect'):
        assert ap.parse_args(base + ['--letterbox', v]).letterbox == v
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--letterbox', 'tight'])
    none = ap.parse_args(base)
    assert DET.letterbox_from_args(none, {'TEST': {}}) is None and DET.letterbox_from_args(none, {}) is None
    assert DET.letterbox_from_args(none, {'TEST': {'LETTERBOX': 'rect'}}) == 'rect'
    assert DET.letterbox_from_args(none, {'TEST': {'LETTERBOX': 'off'}}) is None
    assert DET.letterbox_from_args(ap.parse_args(base + ['--letterbox', 'off']), {'TEST': {'LETTERBOX': 'rect'}}) is None
    assert DET.letterbox_from_args(ap.parse_args(base + ['--letterbox', 'square']), {'TEST': {'LETTERBOX': 'rect'}}) == 'square'
    with pytest.raises(ValueError):
        DET.letterbox_from_args(none, {'TEST': {'LETTERBOX': 'tight'}})


def test_loader_orders_rect_batches_by_aspect_without_reading_images(tmp_path):
    import json
    from yolov4_amd.yolo.data.cocodataset import COCOBatchLoader, COCODataset
    root = tmp_path / 'coco'
    (root / 'annotations').mkdir(parents=True)
    sizes = [(480, 640), (640, 480), (500, 500), (427, 640), (640, 427)]
    doc = {'images': [{'id': 10 + k, 'height': h, 'width': w} for k, (h, w) in enumerate(sizes)],
           'categories': [{'id': 1}], 'annotations': []}
    (root / 'annotations' / 'instances_val2017.json').write_text(json.dumps(doc))
    ds = COCODataset(str(root), 'val2017', img_size=608, is_train=False)
    assert [ds.img_hw(k) for k in range(5)] == sizes
    cfg = {'DATA': {'MAX_NUM_LABELS': 4}, 'MODEL': {}}
    assert COCOBatchLoader(ds, 2, cfg, letterbox='rect')._order() == [3, 0, 2, 1, 4]          # h / w ascending, no image file exists
    assert COCOBatchLoader(ds, 2, cfg, letterbox='square')._order() == [0, 1, 2, 3, 4]
    assert COCOBatchLoader(ds, 2, cfg)._order() == [0, 1, 2, 3, 4]
    ds.is_train = True
    with pytest.raises(ValueError):
        COCOBatchLoader(ds, 2, cfg, letterbox='rect')
