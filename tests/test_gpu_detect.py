# -*- coding: utf-8 -*-
"""`detect_images` (yolov4_amd/detect.py) end to end on the GPU.  A stub model plants a fixed prediction, so every stage after
the network has a known answer: the boxes in source pixels (yolobox2yxyx in fp64), the annotated image (tests/draw_cases.py
on the decoded source), the file (the encoder restatement in tests/jpegenc_cases.py).  Then one run of the real YOLOv4 at
IMGSIZE 64 for shapes and dtypes.  Sources are JPEG fixtures of 29 x 37 and 48 x 40 pixels."""
import numpy as np
import pytest
import torch

import draw_cases as D
import jpeg_cases as J
import jpegenc_cases as E
import recipe
from yolov4_amd import detect as DET
from yolov4_amd.detect import detect_images
from yolov4_amd.yolo.data.jpeg_enc import encode_jpeg_batch
from yolov4_amd.yolo.util import glyphs as G
from yolov4_amd.yolo.util.utils import yolobox2yxyx
from yolov4_amd.yolo.util.vis import class_colors

pytestmark = pytest.mark.gpu

S = 64
CFG = {'MODEL': recipe.MODEL_CFG, 'TEST': {'IMGSIZE': S, 'CONFTHRE': 0.3, 'NMSTHRE': 0.45}}
SOURCES = ['s29x37_420', 's48x40_444']
# planted predictions in network-input pixels: (xc, yc, w, h, obj, class, class probability); every number is exact in fp32
PLANTED = [(40.0, 36.0, 24.0, 40.0, 0.75, 17, 0.5),
           (16.0, 20.0, 16.0, 24.0, 0.75, 3, 0.5),
           (48.0, 12.0, 8.0, 8.0, 0.25, 5, 0.5)]          # score 0.125: below the cfg's threshold


class Planted(torch.nn.Module):
    """returns the same [B, 8, 85] prediction for every image"""

    def forward(self, x):
        assert x.shape[1:] == (3, S, S) and x.dtype == torch.float32 and x.is_cuda and not self.training
        p = torch.zeros((x.shape[0], 8, 85), dtype=torch.float32)
        for k, (xc, yc, w, h, obj, cls, prob) in enumerate(PLANTED):
            p[:, 2 * k, :5] = torch.tensor([xc, yc, w, h, obj])
            p[:, 2 * k, 5 + cls] = prob
        return p.to(x.device)


def expected_rows(src_h, src_w, conf):
    """[n, 7] (y1, x1, y2, x2, obj, cls_conf, cls) in source pixels, class ascending (one box per class here)"""
    rows = []
    for xc, yc, w, h, obj, cls, prob in sorted(PLANTED, key=lambda p: p[5]):
        if obj * prob >= conf:
            box = yolobox2yxyx([yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2], (src_h, src_w, S, S))
            rows.append(box + [obj, prob, float(cls)])
    return np.array(rows, dtype=np.float64).reshape(-1, 7)


def expected_image(bgr, rows, names=None):
    boxes = [(int(r[1]), int(r[0]), int(r[3]), int(r[2])) for r in rows]
    labels = ['%s %.2f' % (names[int(r[6])] if names else str(int(r[6])), r[5]) for r in rows]
    colors = [class_colors(80)[int(r[6])] for r in rows]
    return D.draw(bgr, boxes, labels, colors, 3, G.GLYPHS, G.CHARS)


@pytest.fixture(scope='module')
def decoded(golden):
    return {n: np.ascontiguousarray(golden('jpeg')[n][..., ::-1]) for n in SOURCES}          # BGR


def test_yolobox2yxyx_is_the_formula_in_fp64():
    box = [10.3, 7.1, 50.9, 33.7]
    got = yolobox2yxyx(box, (37, 29, 64, 48))
    assert got == [10.3 * 37 / 64, 7.1 * 29 / 48, 50.9 * 37 / 64, 33.7 * 29 / 48]
    arr = yolobox2yxyx([np.array([1.5, 2.5]), np.array([3.0, 4.0]), np.array([5.0, 6.0]), np.array([7.0, 8.0])], (480, 640, 608, 608))
    assert arr[0].dtype == np.float64 and np.array_equal(arr[1], np.array([3.0, 4.0]) * 640 / 608)
    assert [int(v) for v in yolobox2yxyx([63.9, 63.9, 64.0, 64.0], (37, 29, 64, 64))] == [36, 28, 37, 29]


def test_planted_predictions_through_the_whole_path(decoded, tmp_path):
    a, b = (J.read(n) for n in SOURCES)
    path = tmp_path / 'b.jpg'
    path.write_bytes(b)
    tensor = torch.from_numpy(decoded[SOURCES[0]]).cuda()
    keep = tensor.clone()
    model = Planted().train()
    out = detect_images(model, CFG, [a, str(path), tensor], batch=2)                # two batches: 2 + 1 images
    assert not model.training and len(out) == 3
    assert torch.equal(tensor, keep), 'a tensor source was drawn on'
    for r, name in zip(out, [SOURCES[0], SOURCES[1], SOURCES[0]]):
        src = decoded[name]
        h, w = src.shape[:2]
        want = expected_rows(h, w, 0.3)
        assert len(want) == 2
        det = r['detections']
        assert det.dtype == np.float64 and det.shape == (2, 7) and np.array_equal(det, want)
        assert list(det[:, 6]) == [3.0, 17.0]
        img = r['image']
        assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (h, w, 3)
        drawn = expected_image(src, want)
        assert np.array_equal(img.cpu().numpy(), drawn) and not np.array_equal(drawn, src)
        assert r['jpeg'] == encode_jpeg_batch([img])[0]
        # ... and that file is what libjpeg-turbo's arithmetic gives for the annotated pixels at quality 95, 4:2:0
        coef, qt, p = J.entropy(r['jpeg'])
        want_coef, real, want_qt = E.coefficients(np.ascontiguousarray(drawn[..., ::-1]), '420', 95)
        assert (p['width'], p['height']) == (w, h) and np.array_equal(qt, want_qt)
        assert np.array_equal(coef[real], want_coef[real])
    assert out[0]['jpeg'] == out[2]['jpeg']


def test_thresholds_names_and_switches(decoded, tmp_path):
    a = J.read(SOURCES[0])
    src = decoded[SOURCES[0]]
    names_file = tmp_path / 'names.txt'
    names = ['c%d' % i for i in range(80)]
    names_file.write_text('\n'.join(names) + '\n')
    model = Planted()
    low = detect_images(model, CFG, [a], conf_thre=0.1, names=names)[0]
    want = expected_rows(src.shape[0], src.shape[1], 0.1)
    assert len(want) == 3 and np.array_equal(low['detections'], want)
    assert np.array_equal(low['image'].cpu().numpy(), expected_image(src, want, names))
    from_file = detect_images(model, CFG, [a], conf_thre=0.1, names=str(names_file))[0]
    assert from_file['jpeg'] == low['jpeg']
    assert len(detect_images(model, CFG, [a], conf_thre=-0.1, nms_thre=-1.0)[0]['detections']) == 2      # negative: the cfg's
    plain = detect_images(model, CFG, [a], draw=False, encode=False)[0]
    assert plain['jpeg'] is None and np.array_equal(plain['image'].cpu().numpy(), src) and len(plain['detections']) == 2
    none = detect_images(model, CFG, [a], conf_thre=0.9)[0]
    assert none['detections'].shape == (0, 7) and np.array_equal(none['image'].cpu().numpy(), src)
    with pytest.raises(ValueError):
        detect_images(model, CFG, [a], names=['only', 'two'])
    assert DET.increment_path(str(tmp_path / 'exp')) == str(tmp_path / 'exp')
    (tmp_path / 'exp').mkdir()
    assert DET.increment_path(str(tmp_path / 'exp')) == str(tmp_path / 'exp2')
    (tmp_path / 'cfg.json').write_text('{"TEST": {"IMGSIZE": 64}}')
    assert DET.load_cfg(str(tmp_path / 'cfg.json')) == {'TEST': {'IMGSIZE': 64}}


def test_host_waits_do_not_grow_with_the_batch(decoded, monkeypatch):
    """every host wait counted (Tensor.cpu / .item, synchronize of device, stream and event): as many for four images as for two"""
    counts = {'n': 0}

    def counted(owner, name):
        original = getattr(owner, name)

        def wrapper(*a, **kw):
            counts['n'] += 1
            return original(*a, **kw)
        monkeypatch.setattr(owner, name, wrapper)

    for owner, name in [(torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')]:
        counted(owner, name)
    model = Planted()
    files = [J.read(n) for n in SOURCES]
    seen = []
    for k in (2, 4):
        counts['n'] = 0
        out = detect_images(model, CFG, (files * 2)[:k], batch=8)
        assert len(out) == k and all(len(r['detections']) == 2 for r in out)
        seen.append(counts['n'])
    assert seen[0] == seen[1] and 1 <= seen[0] <= 4, seen


def test_full_model_once():
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    dev = torch.device('cuda:0')
    model = YOLOv4(recipe.MODEL_CFG, device=dev)
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 7)
    model.load_state_dict(sd)
    model = model.to(dev)
    recipe.calibrate_bn_(model, recipe.randn((8, 3, S, S), 3).to(dev))
    files = [J.read(n) for n in SOURCES]
    out = detect_images(model, CFG, files, conf_thre=0.6)
    assert len(out) == 2 and not model.training
    for r, n in zip(out, SOURCES):
        w, h = J.FIXTURES[n]['width'], J.FIXTURES[n]['height']
        d = r['detections']
        assert d.dtype == np.float64 and d.ndim == 2 and d.shape[1] == 7
        assert ((d[:, 6] >= 0) & (d[:, 6] < 80) & (d[:, 6] == np.floor(d[:, 6]))).all()
        assert (d[:, 4] * d[:, 5] >= 0.6 - 1e-6).all()
        assert r['image'].is_cuda and r['image'].dtype == torch.uint8 and tuple(r['image'].shape) == (h, w, 3)
        p = J.parse(r['jpeg'])
        assert (p['width'], p['height'], p['ncomp']) == (w, h, 3) and r['jpeg'][-2:] == b'\xff\xd9'
