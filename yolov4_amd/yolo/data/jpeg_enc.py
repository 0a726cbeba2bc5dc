# -*- coding: utf-8 -*-
"""JPEG encoding for the detect path: what `cv2.imwrite` does for the reference (detect.py writes the annotated image).

The decoder's mirror image, in two stages (include/yolov4_amd.h, csrc/jpeg_enc.hip, csrc/jpeg_enc_host.h):

  device   `coefficients_batch`: one job table copied to the device, y4_jpeg_encode_u8 (colour conversion, downsampling, FDCT
           and quantisation of the whole batch in ONE launch), then ONE device -> host copy of every image's quantised
           coefficients into pinned memory;
  host     `huffman_batch`: markers and Huffman coding, one file per task on a thread pool (ctypes releases the GIL).

`encode_jpeg_batch` is the two in a row.  The arithmetic and the file layout are libjpeg-turbo's defaults, so the bytes are the
ones Pillow's `save` gives for the same pixels, quality and subsampling.  There is no CPU path for the device stage.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..._lib import JpegEncJob, JpegInfo, Y4Error, lib

MAX_WORKERS = 16
SAMPLING = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}
_JOB = ctypes.sizeof(JpegEncJob)


def _round16(v):
    return (int(v) + 15) & ~15


class EncBatch(object):
    """What the device stage leaves: the pinned coefficient buffer, every image's offset (bytes) in it, the records and tables."""

    def __init__(self, host, offsets, infos, qts):
        self.host, self.offsets, self.infos, self.qts = host, offsets, infos, qts


def coefficients_batch(images, quality=95, subsampling='420', swap_rb=False):
    """The device stage of a batch: list of [h, w, 3] (BGR; RGB with swap_rb) or [h, w] (gray) uint8 device tensors ->
    EncBatch.  quality and subsampling: one for the batch, or a list with one per image.  Rows may be pitched: stride(1) == 3
    and stride(2) == 1 (gray: stride(1) == 1).  One launch, one copy back, one wait."""
    L = lib()
    images = list(images)
    if len(images) < 1:
        raise ValueError('an empty batch')
    samplings = list(subsampling) if isinstance(subsampling, (list, tuple)) else [subsampling] * len(images)
    qualities = [int(q) for q in quality] if isinstance(quality, (list, tuple)) else [int(quality)] * len(images)
    if len(samplings) != len(images) or len(qualities) != len(images):
        raise ValueError('one quality and one subsampling per image, or one for all')
    for s in samplings:
        if s not in SAMPLING:
            raise ValueError("subsampling is '444', '422' or '420', not %r" % (s,))
    for q in qualities:
        if not 1 <= q <= 100:
            raise ValueError('quality is 1..100, not %d' % q)
    device = images[0].device
    if device.type != 'cuda':
        raise Y4Error('the JPEG device stage runs on the GPU only: there is no CPU path')
    n = len(images)
    infos, qts, pitches = [], [], []
    for i, t in enumerate(images):
        gray = t.dim() == 2
        ok = t.dtype == torch.uint8 and t.device == device and t.numel() > 0 and (
            (gray and (t.stride(1) == 1 or t.shape[1] == 1)) or
            (t.dim() == 3 and t.shape[2] == 3 and t.stride(2) == 1 and (t.stride(1) == 3 or t.shape[1] == 1)))
        if not ok or (t.shape[0] > 1 and t.stride(0) < (1 if gray else 3) * t.shape[1]):
            raise Y4Error('image %d of the batch: expected a uint8 [h, w, 3] or [h, w] tensor on %s with dense pixels '
                          '(stride(1) == 3, stride(2) == 1), got %s strides %s' % (i, device, tuple(t.shape), t.stride()))
        hs, vs = (1, 1) if gray else SAMPLING[samplings[i]]
        info, qt = JpegInfo(), ((ctypes.c_uint16 * 64) * 3)()
        rc = L.y4_jpeg_encode_setup(int(t.shape[1]), int(t.shape[0]), 1 if gray else 3, hs, vs, qualities[i], ctypes.byref(info),
                                    qt)
        if rc != 0:
            raise Y4Error('image %d of the batch: y4_jpeg_encode_setup: %s (code %d)' % (i, L.y4_strerror(rc).decode(), rc))
        infos.append(info)
        qts.append(qt)
        pitches.append(int(t.stride(0)) if t.shape[0] > 1 else (1 if gray else 3) * int(t.shape[1]))
    offsets, at = [], 0
    for f in infos:
        offsets.append(at)
        at += _round16(2 * f.coef_count)
    with torch.cuda.device(device):
        table = torch.empty(n * _JOB, dtype=torch.uint8, pin_memory=True)
        jobs = (JpegEncJob * n).from_buffer(table.numpy(), 0)
        dev_table = torch.empty(n * _JOB, dtype=torch.uint8, device=device)
        dev_coef = torch.empty(at, dtype=torch.uint8, device=device)
        for i, t in enumerate(images):
            job = jobs[i]
            job.pixels = t.data_ptr()
            job.coef = dev_coef.data_ptr() + offsets[i]
            job.pitch = pitches[i]
            job.info = infos[i]
            job.swap_rb = int(bool(swap_rb))
            job.qt = qts[i]
        dev_table.copy_(table, non_blocking=True)
        rc = L.y4_jpeg_encode_u8(dev_table.data_ptr(), table.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            torch.cuda.current_stream().synchronize()          # the pinned table must outlive its copy
            raise Y4Error('y4_jpeg_encode_u8: %s (code %d)' % (L.y4_strerror(rc).decode(), rc))
        host = torch.empty(at, dtype=torch.uint8, pin_memory=True)
        host.copy_(dev_coef, non_blocking=True)
        torch.cuda.current_stream().synchronize()              # the one wait: the host stage reads `host` next
    return EncBatch(host, offsets, infos, qts)


def huffman_batch(eb, workers=8, pool=None):
    """The host stage: EncBatch (its copy complete) -> list of bytes, one JPEG file per image."""
    L = lib()
    n = len(eb.infos)
    workers = max(1, min(int(workers), MAX_WORKERS))
    base = eb.host.data_ptr()

    def one(i):
        cap = int(L.y4_jpeg_encode_bound(ctypes.byref(eb.infos[i])))
        out = np.empty(cap, dtype=np.uint8)
        size = ctypes.c_size_t(0)
        rc = L.y4_jpeg_encode_host(base + eb.offsets[i], ctypes.byref(eb.infos[i]), eb.qts[i], out.ctypes.data, cap,
                                   ctypes.byref(size))
        return rc, out[:size.value].tobytes()

    own = None
    if pool is None and workers > 1 and n > 1:
        pool = own = ThreadPoolExecutor(max_workers=min(workers, n))
    try:
        results = list(pool.map(one, range(n))) if pool is not None else [one(i) for i in range(n)]
    finally:
        if own is not None:
            own.shutdown()
    for i, (rc, _) in enumerate(results):
        if rc != 0:
            raise Y4Error('image %d of the batch: y4_jpeg_encode_host: %s (code %d)' % (i, L.y4_strerror(rc).decode(), rc))
    return [data for _, data in results]


def encode_jpeg_batch(images, quality=95, subsampling='420', swap_rb=False, workers=8):
    """List of [h, w, 3] uint8 device tensors, BGR in memory like `decode_jpeg_batch` returns (RGB with swap_rb), or [h, w]
    gray ones -> list of bytes, baseline JFIF files.  quality 1..100 and subsampling '444' / '422' / '420' as libjpeg
    understands them; the defaults are cv2.imwrite's.  Sizes may differ within the batch.  workers: threads of the host
    stage, at most 16."""
    return huffman_batch(coefficients_batch(images, quality, subsampling, swap_rb), workers)


def imwrite(path, image, **kw):
    """One [h, w, 3] uint8 BGR (or [h, w] gray) device tensor -> a JPEG file."""
    data = encode_jpeg_batch([image], workers=1, **kw)[0]
    with open(path, 'wb') as f:
        f.write(data)
