# -*- coding: utf-8 -*-
"""`draw_detections` (one launch of y4_draw_boxes_u8 per batch) against the numpy painter's-algorithm oracle in
tests/draw_cases.py, exactly: images of one and of several workgroups, box lists from empty to overlapping, boxes across and
outside the image edges, degenerate boxes, both plate positions, both glyph scales, an unknown character, pitched views and a
mixed batch.  The images are at most 300 x 40, so the file runs in a second or two."""
import ctypes

import numpy as np
import pytest
import torch

import draw_cases as D
import yolov4_amd
from yolov4_amd import Y4Error
from yolov4_amd._lib import DrawBox, DrawJob
from yolov4_amd.yolo.util import glyphs as G
from yolov4_amd.yolo.util.vis import class_colors, draw_detections

pytestmark = pytest.mark.gpu

OK, ERR_SHAPE, ERR_NULL = 0, 1, 2
FILL = 0xA5
SIZES = [(37, 29), (300, 40)]          # (w, h): one workgroup column; five of them


def background(w, h, seed):
    return np.random.RandomState(seed).randint(0, 100, (h, w, 3)).astype(np.uint8)


# name -> (boxes, labels, colours); coordinates fit the 37 x 29 image and are reused on the wide one
CASES = {
    'no_boxes': ([], [], []),
    'one_box': ([(5, 12, 30, 25)], ['cat 0.87'], [(200, 130, 160)]),
    'overlap_ab': ([(3, 10, 25, 25), (12, 4, 34, 20)], ['a', 'b'], [(250, 140, 130), (130, 250, 140)]),
    'overlap_ba': ([(12, 4, 34, 20), (3, 10, 25, 25)], ['b', 'a'], [(130, 250, 140), (250, 140, 130)]),
    'partly_outside': ([(-6, -4, 12, 9), (28, 20, 50, 44)], ['x1', 'yz'], [(200, 200, 128), (128, 200, 200)]),
    'wholly_outside': ([(-60, -40, -20, -9), (400, 100, 500, 144), (10, 60, 20, 70)], ['q', 'r', 's'],
                       [(200, 200, 128), (128, 200, 200), (222, 222, 222)]),
    'inverted': ([(20, 8, 10, 22)], [None], [(240, 240, 130)]),                        # x2 < x1
    'thin': ([(10, 8, 11, 22), (20, 8, 30, 9)], [None, None], [(240, 130, 130), (130, 240, 130)]),    # narrower than the line
    'plate_above': ([(4, 20, 30, 27)], ['dog-7'], [(180, 180, 250)]),                  # y1 - plate height >= 3
    'plate_inside': ([(4, 5, 30, 27)], ['94%'], [(180, 250, 180)]),
    'unknown_char': ([(2, 19, 35, 27)], ['aB_9'], [(250, 180, 180)]),
    'float_boxes': ([(5.9, 12.2, 30.99, 25.5), (-0.7, 3.3, 8.2, 9.9)], ['f', None], [(200, 130, 160), (150, 150, 250)]),
    'every_glyph': ([(0, 18, 36, 28)], [G.CHARS], [(140, 140, 140)]),
}


def run(img_np, boxes, labels, colors, line_width, pitched=False):
    """-> (drawn pixels, whole backing buffer, pitch)"""
    h, w = img_np.shape[:2]
    pitch = -(-(3 * w + 5) // 64) * 64 if pitched else 3 * w
    buf = torch.full((h * pitch,), FILL, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(buf, (h, w, 3), (pitch, 3, 1))
    view.copy_(torch.from_numpy(img_np).cuda())
    out = draw_detections([view], [boxes], [labels], [colors], line_width=line_width)
    assert out[0] is view
    return view.cpu().numpy(), buf.cpu().numpy().reshape(h, pitch), pitch


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('line_width', [2, 3], ids=['scale1', 'scale2'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_equals_the_painters_oracle(name, line_width, size):
    w, h = size
    boxes, labels, colors = CASES[name]
    if w > 100:                                                      # the same boxes, the last one moved across workgroups
        boxes = [tuple(b) if k + 1 < len(boxes) else (b[0] + 50, b[1] + 9, b[2] + 215, b[3] + 9) for k, b in enumerate(boxes)]
    img = background(w, h, 3)
    got, _, _ = run(img, boxes, labels, colors, line_width)
    want = D.draw(img, boxes, labels, colors, line_width, G.GLYPHS, G.CHARS)
    assert np.array_equal(got, want)
    if name in ('no_boxes', 'wholly_outside'):
        assert np.array_equal(got, img)
    elif name not in ('inverted',):
        assert not np.array_equal(got, img)


def test_order_matters():
    img = background(37, 29, 4)
    ab = run(img, *CASES['overlap_ab'], 3)[0]
    ba = run(img, *CASES['overlap_ba'], 3)[0]
    assert not np.array_equal(ab, ba)


def test_plate_positions_and_scales():
    img = background(37, 29, 5)
    above = run(img, *CASES['plate_above'], 2)[0]
    assert (above[12:20, 4:4 + 30] != img[12:20, 4:4 + 30]).any(axis=2).all(), 'an 8-row plate over the box at scale 1'
    inside = run(img, *CASES['plate_inside'], 2)[0]
    assert np.array_equal(inside[:4], img[:4]) and (inside[5:13, 4:22] != img[5:13, 4:22]).any(axis=2).all()
    assert (above == 255).all(axis=2).any() and (inside == 255).all(axis=2).any(), 'white text'


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_pitched_view_keeps_the_row_padding(size):
    w, h = size
    img = background(w, h, 6)
    boxes, labels, colors = CASES['partly_outside']
    got, whole, pitch = run(img, boxes, labels, colors, 3, pitched=True)
    assert pitch > 3 * w and pitch % 64 == 0
    assert np.array_equal(got, D.draw(img, boxes, labels, colors, 3, G.GLYPHS, G.CHARS))
    assert (whole[:, 3 * w:] == FILL).all(), 'bytes beyond 3 w were touched'


def test_batch_of_three_with_different_box_counts():
    names = ['overlap_ab', 'no_boxes', 'wholly_outside']
    sizes = [(37, 29), (300, 40), (41, 33)]
    imgs = [background(w, h, 10 + k) for k, (w, h) in enumerate(sizes)]
    dev = [torch.from_numpy(a).cuda() for a in imgs]
    draw_detections(dev, [CASES[n][0] for n in names], [CASES[n][1] for n in names], [CASES[n][2] for n in names])
    for a, t, n in zip(imgs, dev, names):
        assert np.array_equal(t.cpu().numpy(), D.draw(a, *CASES[n], 3, G.GLYPHS, G.CHARS)), n
    # defaults: no labels, white frames
    t = torch.from_numpy(imgs[0]).cuda()
    draw_detections([t], [CASES['one_box'][0]])
    assert np.array_equal(t.cpu().numpy(), D.draw(imgs[0], CASES['one_box'][0], [None], [(255, 255, 255)], 3, G.GLYPHS, G.CHARS))


def test_palette_and_glyph_table():
    c = class_colors(80)
    assert c.shape == (80, 3) and c.dtype == np.uint8 and c.min() >= 128
    assert np.array_equal(c, class_colors(80)) and np.array_equal(c, np.random.RandomState(0).randint(128, 255, (80, 3)))
    assert not np.array_equal(c, class_colors(80, seed=1))
    assert G.GLYPHS.shape == (len(G.CHARS), 8) and G.GLYPHS.dtype == np.uint8 and (G.GLYPHS < 32).all()
    assert set('abcdefghijklmnopqrstuvwxyz0123456789 .-%') <= set(G.CHARS)
    rows = [tuple(g) for g in G.GLYPHS]
    assert len(set(rows)) == len(rows), 'two characters share a glyph'
    assert G.indices('a?') == [0, G.UNKNOWN]


def test_errors_before_the_launch():
    L = yolov4_amd.lib()
    img = torch.full((29, 37, 3), 7, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        draw_detections([], [])
    with pytest.raises(ValueError):
        draw_detections([img], [[(1, 2, 3, 4)]], [['a', 'b']])
    with pytest.raises(Y4Error):
        draw_detections([img.cpu()], [[]])
    with pytest.raises(Y4Error):
        draw_detections([img.permute(1, 0, 2)], [[]])

    host = torch.zeros(ctypes.sizeof(DrawJob) + ctypes.sizeof(DrawBox) + 16, dtype=torch.uint8)
    job = DrawJob.from_buffer(host.numpy())
    box = DrawBox.from_buffer(host.numpy(), ctypes.sizeof(DrawJob))
    dev = torch.zeros_like(host, device='cuda')
    box.x1, box.y1, box.x2, box.y2, box.half, box.scale, box.px2, box.py2 = 3, 3, 20, 20, 1, 1, -1, -1
    box.text_off, box.text_len = 0, 4
    box.color[:] = (9, 9, 9, 0)
    job.image, job.pitch, job.width, job.height = img.data_ptr(), 3 * 37, 37, 29
    job.boxes = dev.data_ptr() + ctypes.sizeof(DrawJob)
    job.boxes_host = host.data_ptr() + ctypes.sizeof(DrawJob)
    job.text = dev.data_ptr() + ctypes.sizeof(DrawJob) + ctypes.sizeof(DrawBox)
    job.n_boxes, job.text_bytes, job.n_glyphs = 1, 4, 0
    good = bytes(host.numpy())
    call = lambda n=1: L.y4_draw_boxes_u8(dev.data_ptr(), host.data_ptr(), n, None)

    def broken(target, field, value):
        setattr(target, field, value)
        rc = call()
        host.numpy()[:] = np.frombuffer(good, dtype=np.uint8)
        return rc

    assert L.y4_draw_boxes_u8(None, host.data_ptr(), 1, None) == ERR_NULL
    assert L.y4_draw_boxes_u8(dev.data_ptr(), None, 1, None) == ERR_NULL
    assert call(0) == ERR_SHAPE
    assert broken(job, 'image', None) == ERR_NULL
    assert broken(job, 'boxes', None) == ERR_NULL
    assert broken(job, 'boxes_host', None) == ERR_NULL
    assert broken(job, 'text', None) == ERR_NULL
    assert broken(job, 'pitch', 3 * 37 - 1) == ERR_SHAPE
    assert broken(job, 'width', 0) == ERR_SHAPE
    assert broken(job, 'n_boxes', -1) == ERR_SHAPE
    assert broken(box, 'text_len', 5) == ERR_SHAPE                  # past text_bytes
    assert broken(box, 'text_off', -1) == ERR_SHAPE
    assert broken(box, 'scale', 0) == ERR_SHAPE
    assert broken(box, 'half', -1) == ERR_SHAPE
    assert broken(box, 'x2', 1 << 30) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((img == 7).all()), 'a refused call launched'
    dev.copy_(host)
    assert call() == OK
    torch.cuda.synchronize()
    assert not bool((img == 7).all())
