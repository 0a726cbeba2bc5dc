# -*- coding: utf-8 -*-
"""The JPEG encoder on the GPU: device coefficients against the numpy restatement (tests/jpegenc_cases.py) on every real block,
whole files against the bytes Pillow (libjpeg-turbo) wrote for the same pixels (tests/golden/jpegenc.npz), and the decoder on
the encoder's output.  All goldens go through as ONE mixed batch (sizes 1x1 .. 300x9, three samplings and gray, five
qualities); the images are a few dozen pixels wide, so the file runs in seconds, and they reach every path of the kernel: the
aligned six-dword load and the byte load, clamped right / bottom edges, h2v1 and h2v2 downsampling, dummy blocks on both edges,
images of more than one workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_cases as J
import jpegenc_cases as E
import yolov4_amd
from yolov4_amd import Y4Error
from yolov4_amd._lib import JpegEncJob, JpegInfo
from yolov4_amd.yolo.data.jpeg import decode_jpeg_batch
from yolov4_amd.yolo.data.jpeg_enc import coefficients_batch, encode_jpeg_batch, huffman_batch, imwrite

pytestmark = pytest.mark.gpu

OK, ERR_SHAPE, ERR_NULL = 0, 1, 2
FILL = 0xA5


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpegenc')


def device_image(px, swap_rb=False, row_align=None):
    """RGB / gray numpy pixels -> device tensor in the library's memory order (BGR unless swap_rb), optionally a pitched view"""
    a = px if (px.ndim == 2 or swap_rb) else np.ascontiguousarray(px[..., ::-1])
    if row_align is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    h, w = a.shape[:2]
    row = w * (1 if a.ndim == 2 else 3)
    pitch = -(-(row + 1) // row_align) * row_align
    buf = torch.full((h * pitch,), FILL, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(buf, tuple(a.shape), (pitch, 1) if a.ndim == 2 else (pitch, 3, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return view


def batch_args(npz, names):
    return ([E.CASES[n]['quality'] for n in names], [E.CASES[n]['sampling'] or '444' for n in names])


@pytest.fixture(scope='module')
def mixed(npz):
    """every golden in one batch: (EncBatch, list of files)"""
    q, s = batch_args(npz, E.NAMES)
    eb = coefficients_batch([device_image(npz[n + '__px']) for n in E.NAMES], q, s)
    return eb, huffman_batch(eb, workers=4)


def coef_of(eb, i):
    n = int(eb.infos[i].coef_count)
    return eb.host.numpy()[eb.offsets[i]:eb.offsets[i] + 2 * n].view(np.int16)


@pytest.mark.parametrize('name', E.NAMES)
def test_device_coefficients_equal_the_restatement(npz, mixed, name):
    i = E.NAMES.index(name)
    c = E.CASES[name]
    want, real, qt = E.coefficients(npz[name + '__px'], c['sampling'], c['quality'])
    got = coef_of(mixed[0], i)
    assert got.shape == want.shape
    assert np.array_equal(np.asarray(mixed[0].qts[i]), qt)
    assert np.array_equal(got[real], want[real])


@pytest.mark.parametrize('name', E.NAMES)
def test_bytes_equal_pillow(npz, mixed, name):
    assert mixed[1][E.NAMES.index(name)] == npz[name + '__jpg'].tobytes()


def test_dummy_blocks_are_never_written():
    """the coefficient buffer pre-filled through the C ABI: positions of dummy blocks keep the fill"""
    L = yolov4_amd.lib()
    rng = np.random.RandomState(5)
    for (w, h), (hs, vs) in [((17, 33), (2, 2)), ((48, 40), (2, 2)), ((17, 9), (2, 1))]:
        px = torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        table = torch.zeros(ctypes.sizeof(JpegEncJob), dtype=torch.uint8)
        job = JpegEncJob.from_buffer(table.numpy())
        assert L.y4_jpeg_encode_setup(w, h, 3, hs, vs, 75, ctypes.byref(job.info), job.qt) == OK
        coef = torch.full((int(job.info.coef_count),), 0x5A5A, dtype=torch.int16, device='cuda')
        job.pixels, job.coef, job.pitch = px.data_ptr(), coef.data_ptr(), 3 * w
        dev = table.cuda()
        assert L.y4_jpeg_encode_u8(dev.data_ptr(), table.data_ptr(), 1, None) == OK
        torch.cuda.synchronize()
        sampling = {(2, 2): '420', (2, 1): '422'}[(hs, vs)]
        want, real, _ = E.coefficients(px.cpu().numpy()[..., ::-1], sampling, 75)
        got = coef.cpu().numpy()
        assert (~real).any() and (got[~real] == 0x5A5A).all()
        assert np.array_equal(got[real], want[real])


def test_pitched_views_and_swap_rb(npz):
    names = ['e29x37_420', 'e17x33_422', 'e50x9_444', 'egray_29x37']
    q, s = batch_args(npz, names)
    want = [npz[n + '__jpg'].tobytes() for n in names]
    pitched = [device_image(npz[n + '__px'], row_align=64) for n in names]
    assert all(t.stride(0) % 64 == 0 and not t.is_contiguous() for t in pitched)
    assert encode_jpeg_batch(pitched, q, s) == want
    odd = [device_image(npz[n + '__px'], row_align=1) for n in names]          # rows that are not dword-aligned
    assert encode_jpeg_batch(odd, q, s) == want
    rgb = [device_image(npz[n + '__px'], swap_rb=True) for n in names]
    assert encode_jpeg_batch(rgb, q, s, swap_rb=True) == want
    assert encode_jpeg_batch(rgb[:1], q[:1], s[:1], swap_rb=False) != want[:1]


def test_decoder_reads_back_what_libjpeg_turbo_would(npz, mixed):
    for n, t in zip(E.NAMES, decode_jpeg_batch(mixed[1], swap_rb=True)):
        assert np.array_equal(t.cpu().numpy(), J.decode(npz[n + '__jpg'].tobytes())), n


def test_defaults_and_imwrite(npz, tmp_path):
    img = device_image(npz['e29x37_420__px'])
    data = encode_jpeg_batch([img])[0]
    p = J.parse(data)
    assert (p['comps'][0][1], p['comps'][0][2]) == (2, 2)
    assert np.array_equal(np.asarray(p['qt'][0], dtype=np.uint16), E.quality_tables(95)[0])
    imwrite(str(tmp_path / 'a.jpg'), img, quality=30, subsampling='444')
    assert (tmp_path / 'a.jpg').read_bytes() == encode_jpeg_batch([img], 30, '444')[0]


def test_errors_before_any_launch(npz):
    L = yolov4_amd.lib()
    img = device_image(npz['e17x33_420__px'])
    with pytest.raises(ValueError):
        encode_jpeg_batch([])
    for q in (0, 101):
        with pytest.raises(ValueError):
            encode_jpeg_batch([img], quality=q)
    with pytest.raises(ValueError):
        encode_jpeg_batch([img], subsampling='411')
    with pytest.raises(Y4Error):
        encode_jpeg_batch([img.cpu()])
    with pytest.raises(Y4Error):
        encode_jpeg_batch([img.permute(1, 0, 2)])
    with pytest.raises(Y4Error):
        encode_jpeg_batch([img.float()])

    table = torch.zeros(2 * ctypes.sizeof(JpegEncJob), dtype=torch.uint8)
    jobs = (JpegEncJob * 2).from_buffer(table.numpy())
    coef = []
    for j in jobs:
        assert L.y4_jpeg_encode_setup(17, 33, 3, 2, 2, 75, ctypes.byref(j.info), j.qt) == OK
        coef.append(torch.full((int(j.info.coef_count),), 0x5A5A, dtype=torch.int16, device='cuda'))
        j.pixels, j.coef, j.pitch = img.data_ptr(), coef[-1].data_ptr(), 3 * 17
    dev = table.cuda()
    call = lambda n=2: L.y4_jpeg_encode_u8(dev.data_ptr(), table.data_ptr(), n, None)
    assert L.y4_jpeg_encode_u8(None, table.data_ptr(), 2, None) == ERR_NULL
    assert L.y4_jpeg_encode_u8(dev.data_ptr(), None, 2, None) == ERR_NULL
    assert call(0) == ERR_SHAPE and call(65536) == ERR_SHAPE
    good = bytes(table.numpy())

    def broken(change):
        table.numpy()[:] = np.frombuffer(good, dtype=np.uint8)
        change(jobs[1])
        rc = call()
        table.numpy()[:] = np.frombuffer(good, dtype=np.uint8)
        return rc

    assert broken(lambda j: setattr(j, 'pixels', None)) == ERR_NULL
    assert broken(lambda j: setattr(j, 'coef', None)) == ERR_NULL
    assert broken(lambda j: setattr(j, 'pitch', 3 * 17 - 1)) == ERR_SHAPE
    assert broken(lambda j: setattr(j, 'coef', j.coef + 2)) == ERR_SHAPE

    def sampling_12(j):
        j.info.hs[0], j.info.vs[0] = 1, 2

    assert broken(sampling_12) == ERR_SHAPE
    assert broken(lambda j: setattr(j.info, 'width', 18 + 16)) == ERR_SHAPE          # another MCU grid than the record's

    def zero_divisor(j):
        j.qt[1][3] = 0

    assert broken(zero_divisor) == ERR_SHAPE
    torch.cuda.synchronize()
    assert all(bool((c == 0x5A5A).all()) for c in coef), 'a refused call launched'
    assert call() == OK
    torch.cuda.synchronize()
