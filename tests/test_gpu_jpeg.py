# -*- coding: utf-8 -*-
"""The JPEG device stage and the COCO dataset / batch loader on the GPU.  Pixels are compared bit for bit with the recorded
libjpeg-turbo decode (tests/golden/jpeg.npz, RGB; the library's default is BGR).  Every fixture is a few dozen pixels wide,
so the whole file runs in a few seconds; together they reach every path of the two kernels: the three samplings and gray,
fancy and plain upsampling, partial 4-pixel groups, the aligned three-dword store and the byte store, images of more than one
workgroup in either kernel, the eight orientations."""
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

import jpeg_cases as J
from yolov4_amd import Y4Error
from yolov4_amd.yolo.data.cocodataset import COCOBatchLoader, COCODataset
from yolov4_amd.yolo.data.jpeg import decode_jpeg_batch, imread
from yolov4_amd.yolo.data.transform import Transform, sample_train_params, train_batch, val_batch

pytestmark = pytest.mark.gpu

CFG = {'AUGMENTATION': {'JITTER': 0.3, 'RANDOM_HORIZONTAL_FLIP': True, 'COLOR_DITHERING': True, 'HUE': 0.1,
                        'SATURATION': 1.5, 'EXPOSURE': 1.5, 'IS_MOSAIC': True, 'MIN_OFFSET': 0.2},
       'DATA': {'MAX_NUM_LABELS': 60}}
FILL = 0xA5


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpeg')


@pytest.fixture(scope='module')
def files():
    return {n: J.read(n) for n in J.SUPPORTED + J.UNSUPPORTED}


def bgr(a):
    return np.ascontiguousarray(a[..., ::-1])


def test_mixed_batch_equals_libjpeg_turbo_in_bgr(npz, files):
    names = J.SUPPORTED
    out = decode_jpeg_batch([files[n] for n in names])
    assert len(out) == len(names)
    for n, t in zip(names, out):
        assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == npz[n].shape
        assert t.stride(1) == 3 and t.stride(2) == 1
        assert np.array_equal(t.cpu().numpy(), bgr(npz[n])), n
    assert len({t.untyped_storage().data_ptr() for t in out}) == 1, 'views into one batch buffer'


@pytest.mark.parametrize('row_align', [4, 1])
def test_swap_rb_gives_rgb(npz, files, row_align):
    names = J.SUPPORTED
    out = decode_jpeg_batch([files[n] for n in names], swap_rb=True, row_align=row_align, workers=2)
    for n, t in zip(names, out):
        assert np.array_equal(t.cpu().numpy(), npz[n]), n


def test_padding_between_rows_and_images_is_never_written(npz, files):
    names = J.SUPPORTED
    buf = torch.full((1 << 20,), FILL, dtype=torch.uint8, device='cuda')
    out = decode_jpeg_batch([files[n] for n in names], out=buf, row_align=64)
    want = np.full(buf.numel(), FILL, dtype=np.uint8)
    for n, t in zip(names, out):
        h, w = npz[n].shape[:2]
        assert t.stride(0) % 64 == 0 and t.stride(0) >= 3 * w
        for y in range(h):
            at = t.storage_offset() + y * t.stride(0)
            want[at:at + 3 * w] = bgr(npz[n])[y].reshape(-1)
    assert np.array_equal(buf.cpu().numpy(), want)


def test_orientation(npz, files):
    turned = decode_jpeg_batch([files[n] for n in J.ORIENT])
    stored = decode_jpeg_batch([files[n] for n in J.ORIENT], apply_orientation=False)
    for n, a, b in zip(J.ORIENT, turned, stored):
        assert tuple(a.shape) == npz[n].shape and np.array_equal(a.cpu().numpy(), bgr(npz[n])), n
        assert tuple(b.shape) == (21, 13, 3) and np.array_equal(b.cpu().numpy(), bgr(npz[n + '__raw'])), n
    assert tuple(turned[5].shape) == (13, 21, 3)


def test_train_batch_takes_the_decoded_tensors(npz, files):
    groups = [['s48x40_420', 's29x37_422', 's17x33_444', 'gray_29x37'], ['q95_29x37_420']]
    rng = random.Random(5)
    boxes = [[np.array([[2.0, 3.0, 9.0, 11.0, 1.0], [5.0, 1.0, 6.0, 7.0, 4.0]]) for _ in g] for g in groups]
    params = [sample_train_params(CFG, [npz[n].shape[:2] for n in g], 64, rng, [2] * len(g)) for g in groups]
    flat = decode_jpeg_batch([files[n] for g in groups for n in g])
    decoded = [(flat[:4], boxes[0]), (flat[4:], boxes[1])]
    uploaded = [([bgr(npz[n]) for n in g], bb) for g, bb in zip(groups, boxes)]
    x1, l1 = train_batch(decoded, 64, CFG, params=params)
    x2, l2 = train_batch(uploaded, 64, CFG, params=params)
    assert torch.equal(x1, x2) and torch.equal(l1, l2)
    assert float(x1.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ dataset

IMAGES = [(42, 's48x40_420'), (7, 'gray_29x37'), (1000, 's29x37_422'), (9, 's17x33_444')]       # (image id, fixture), JSON order


def make_tree(root):
    doc = {'images': [{'id': i, 'file_name': '%012d.jpg' % i, 'width': J.FIXTURES[n]['width'], 'height': J.FIXTURES[n]['height']}
                      for i, n in IMAGES],
           'categories': [{'id': 3, 'name': 'c'}, {'id': 1, 'name': 'a'}, {'id': 17, 'name': 'q'}],
           'annotations': [
               {'id': 1, 'image_id': 42, 'category_id': 3, 'bbox': [4.0, 5.0, 10.0, 12.0], 'area': 120.0, 'iscrowd': 0},
               {'id': 2, 'image_id': 1000, 'category_id': 1, 'bbox': [1.0, 2.0, 20.0, 30.0], 'area': 600.0, 'iscrowd': 0},
               {'id': 3, 'image_id': 42, 'category_id': 1, 'bbox': [8.0, 8.0, 0.5, 5.0], 'area': 2.5, 'iscrowd': 0},    # too narrow
               {'id': 4, 'image_id': 42, 'category_id': 17, 'bbox': [20.0, 10.0, 15.5, 8.0], 'area': 124.0, 'iscrowd': 1},
               {'id': 5, 'image_id': 9, 'category_id': 17, 'bbox': [3.0, 3.0, 9.0, 20.0], 'area': 180.0, 'iscrowd': 0},
               {'id': 6, 'image_id': 42, 'category_id': 1, 'bbox': [30.0, 20.0, 10.0, 10.0], 'area': 100.0, 'iscrowd': 0}]}
    os.makedirs(os.path.join(root, 'annotations'))
    for split in ('train2017', 'val2017'):
        with open(os.path.join(root, 'annotations', 'instances_%s.json' % split), 'w') as f:
            json.dump(doc, f)
        os.makedirs(os.path.join(root, 'images', split))
        for i, n in IMAGES:
            shutil.copy(os.path.join(J.JPEG_DIR, n + '.jpg'), os.path.join(root, 'images', split, '%012d.jpg' % i))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('coco'))
    make_tree(root)
    return root


def test_dataset_lists_and_labels(npz, tree):
    ds = COCODataset(tree, name='train2017', img_size=64, is_train=True)
    assert len(ds) == 4 and ds.ids == [42, 7, 1000, 9] and ds.class_ids == [1, 3, 17]
    assert ds.get_img_size() == 64
    ds.set_img_size(96)
    assert ds.get_img_size() == 96
    data, boxes, img_id = ds.get_img_and_labels(0)
    assert img_id == 42 and data == J.read('s48x40_420')
    # reversed annotation order, the narrow box dropped, class = position in the sorted category ids
    assert np.array_equal(boxes, np.array([[30.0, 20.0, 10.0, 10.0, 0.0], [20.0, 10.0, 15.5, 8.0, 2.0], [4.0, 5.0, 10.0, 12.0, 1.0]]))
    assert len(ds.get_img_and_labels(1)[1]) == 0
    img, _, _ = ds.get_img_and_labels(2, decode=True)
    assert img.is_cuda and np.array_equal(img.cpu().numpy(), bgr(npz['s29x37_422']))
    assert np.array_equal(imread(ds.img_file(3)).cpu().numpy(), bgr(npz['s17x33_444']))
    two = COCODataset(tree, name='train2017', num_classes=2)
    assert np.array_equal(two.get_img_and_labels(0)[1], np.array([[30.0, 20.0, 10.0, 10.0, 0.0], [4.0, 5.0, 10.0, 12.0, 1.0]]))
    big = COCODataset(tree, name='val2017', min_size=10)
    assert len(big.get_img_and_labels(0)[1]) == 0
    with pytest.raises(ValueError):
        COCODataset(tree, name='test2017')


def test_getitem_keeps_the_reference_contract(npz, tree):
    random.seed(3)
    np.random.seed(3)
    ds = COCODataset(tree, name='train2017', img_size=64, is_train=True, transform=Transform(CFG, is_train=True))
    img, target = ds[2]
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (3, 64, 64)
    assert sorted(target) == ['img_info', 'padded_labels']
    assert tuple(target['padded_labels'].shape) == (60, 5) and target['padded_labels'].dtype == torch.float64
    assert target['img_info'] == [1000, 2]
    val = COCODataset(tree, name='val2017', img_size=64, is_train=False, transform=Transform(CFG, is_train=False))
    img, target = val[0]
    assert tuple(img.shape) == (3, 64, 64) and target['img_info'] == [40, 48, 64, 64, 42, 0]
    want, _ = val_batch([bgr(npz['s48x40_420'])], 64)
    assert torch.equal(img, want[0])
    lab = target['padded_labels'].numpy()
    assert np.allclose(lab[0], [(30 + 5) * 64 / 48, (20 + 5) * 64 / 40, 10 * 64 / 48, 10 * 64 / 40, 0], rtol=0, atol=1e-12)
    assert np.all(lab[3:] == 0)


def test_batch_loader(npz, tree):
    ds = COCODataset(tree, name='train2017', img_size=64, is_train=True)
    loader = COCOBatchLoader(ds, 2, CFG, shuffle=True, seed=11, workers=4)
    assert len(loader) == 2
    first = list(loader)
    assert len(first) == 2
    for x, target in first:
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (2, 3, 64, 64)
        assert tuple(target['padded_labels'].shape) == (2, 60, 5)
        assert len(target['img_info']) == 2 and all(ds.ids[i] == img_id for img_id, i in target['img_info'])
        assert bool(torch.isfinite(x).all()) and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    assert sorted(i for _, t in first for _, i in t['img_info']) == [0, 1, 2, 3]
    again = list(COCOBatchLoader(ds, 2, CFG, shuffle=True, seed=11, workers=1))
    for (x1, t1), (x2, t2) in zip(first, again):
        assert torch.equal(x1, x2) and torch.equal(t1['padded_labels'], t2['padded_labels']) and t1['img_info'] == t2['img_info']
    other = list(COCOBatchLoader(ds, 2, CFG, shuffle=True, seed=12))
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(first, other))
    shard = COCOBatchLoader(ds, 2, CFG, shuffle=True, seed=11, rank=1, world_size=2)
    assert len(shard) == 1
    order = [i for _, t in first for _, i in t['img_info']]
    assert [i for _, t in shard for _, i in t['img_info']] == order[1::2]

    val = COCODataset(tree, name='val2017', img_size=64, is_train=False)
    batches = list(COCOBatchLoader(val, 3, CFG))
    assert [tuple(x.shape) for x, _ in batches] == [(3, 3, 64, 64), (1, 3, 64, 64)]
    x, target = batches[0]
    assert target['img_info'] == [[40, 48, 64, 64, 42, 0], [37, 29, 64, 64, 7, 1], [37, 29, 64, 64, 1000, 2]]
    want, _ = val_batch([bgr(npz[n]) for _, n in IMAGES[:3]], 64)
    assert torch.equal(x, want)
    assert np.all(target['padded_labels'][1].numpy() == 0) and tuple(target['padded_labels'].shape) == (3, 60, 5)


def test_errors_name_the_file_and_launch_nothing(npz, files):
    good = files['s9x5_420']
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device='cuda')
    with pytest.raises(Y4Error, match=r'JPEG 1 of the batch.*code 6'):
        decode_jpeg_batch([good, good[:len(good) // 2], good], out=buf)
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()), 'something was launched'
    with pytest.raises(Y4Error, match=r'JPEG 2 of the batch.*code 7'):
        decode_jpeg_batch([good, good, files['progressive_17x33']], out=buf)
    with pytest.raises(Y4Error, match=r'JPEG 0 of the batch.*code 7'):
        decode_jpeg_batch([files['cmyk_9x5']])
    assert bool((buf == FILL).all())
    calls = []

    def fallback(data):
        calls.append(data)
        return bgr(npz['progressive_17x33'])
    out = decode_jpeg_batch([good, files['progressive_17x33']], fallback=fallback)
    assert calls == [files['progressive_17x33']], 'the fallback sees unsupported files only'
    assert np.array_equal(out[0].cpu().numpy(), bgr(npz['s9x5_420']))
    assert np.array_equal(out[1].cpu().numpy(), bgr(npz['progressive_17x33']))
    with pytest.raises(Y4Error, match=r'JPEG 1 of the batch.*code 6'):          # a corrupt file never goes to the fallback
        decode_jpeg_batch([good, good[:40]], fallback=fallback)
    with pytest.raises(Y4Error):
        decode_jpeg_batch([good], device='cpu')
