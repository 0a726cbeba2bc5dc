# -*- coding: utf-8 -*-
"""JPEG decoding for the input pipeline: what `cv2.imread` does for the reference (yolo/data/cocodataset.py:97).

Two stages (include/yolov4_amd.h, csrc/jpeg_host.h, csrc/jpeg.hip):

  host     `entropy_batch`: markers and Huffman decoding, one file per task on a thread pool (ctypes releases the GIL), written
           straight into ONE pinned buffer per batch: the job table followed by every image's quantised coefficients;
  device   `decode_entropy_batch`: one asynchronous copy of that buffer on the current stream, then y4_jpeg_decode_u8: IDCT,
           chroma upsampling, colour conversion, EXIF orientation and the HWC store in two launches for the whole batch.

`decode_jpeg_batch` is the two in a row.  The arithmetic is libjpeg-turbo's default path bit for bit, so the pixels are the
ones `cv2.imread` hands the reference.  There is no CPU path for the device stage.  Supported: Huffman sequential JPEG, 8-bit,
one interleaved scan, gray or YCbCr at 4:4:4 / 4:2:2 / 4:2:0; everything else raises `Y4Error` (a progressive file may go to
a caller-supplied `fallback` instead).
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..._lib import ERR_UNSUPPORTED, JpegInfo, JpegJob, Y4Error, lib

MAX_WORKERS = 16
MAX_COEFS = 1 << 28          # per image (16384 x 16384 samples): a forged frame header must not allocate the machine away
_JOB = ctypes.sizeof(JpegJob)
_QT_OFFSET = JpegJob.qt.offset


def _round16(v):
    return (int(v) + 15) & ~15


def _raise(index, code, stage):
    raise Y4Error('JPEG %d of the batch: %s: %s (code %d)' % (index, stage, lib().y4_strerror(code).decode(), code))


class HostBatch(object):
    """What the host stage leaves: the pinned buffer (job table, then coefficients), the byte offset of every image's
    coefficients in it, the parse records, and the images a fallback decoded instead (index -> HWC uint8 BGR array)."""

    def __init__(self, n, host, jobs, jobs_of, coef_offsets, infos, fallbacks, apply_orientation):
        self.n, self.host, self.jobs, self.coef_offsets, self.infos = n, host, jobs, coef_offsets, infos
        self.jobs_of = jobs_of          # job j decodes image jobs_of[j] (the others went to the fallback)
        self.fallbacks, self.apply_orientation = fallbacks, apply_orientation
        self.copied = None              # event behind the last asynchronous copy of `host`, once there has been one

    def shape(self, i):
        """(h, w) of output i"""
        if i in self.fallbacks:
            return tuple(self.fallbacks[i].shape[:2])
        f = self.infos[i]
        turned = self.apply_orientation and f.orientation >= 5
        return (f.width, f.height) if turned else (f.height, f.width)


def entropy_batch(list_of_bytes, workers=8, apply_orientation=True, fallback=None, pin=True, pool=None):
    """The host stage of a batch; touches no GPU apart from allocating pinned memory (pin=False: pageable memory, for hosts
    without one).  Raises Y4Error naming the first failing file."""
    L = lib()
    n = len(list_of_bytes)
    if n < 1:
        raise ValueError('an empty batch')
    workers = max(1, min(int(workers), MAX_WORKERS))
    own = None
    if pool is None and workers > 1 and n > 1:
        pool = own = ThreadPoolExecutor(max_workers=min(workers, n))

    def run(fn, count):
        return list(pool.map(fn, range(count))) if pool is not None else [fn(k) for k in range(count)]

    try:
        infos = [JpegInfo() for _ in range(n)]
        # the header walk takes about 3 us per file: 256 of them cost 0.7 ms on this thread and 6-8 ms as pool tasks
        codes = [L.y4_jpeg_parse_host(d, len(d), ctypes.byref(f)) for d, f in zip(list_of_bytes, infos)]
        fallbacks, jobs_of = {}, []
        for i, rc in enumerate(codes):
            if rc == ERR_UNSUPPORTED and fallback is not None:
                arr = np.ascontiguousarray(fallback(list_of_bytes[i]))
                if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
                    raise Y4Error('JPEG %d of the batch: the fallback has to return an HWC uint8 array of 3 channels' % i)
                fallbacks[i] = arr
            elif rc != 0:
                _raise(i, rc, 'y4_jpeg_parse_host')
            elif infos[i].coef_count > MAX_COEFS:
                raise Y4Error('JPEG %d of the batch: %d x %d is beyond the size this loader accepts'
                              % (i, infos[i].width, infos[i].height))
            else:
                jobs_of.append(i)
        nj = len(jobs_of)
        coef_offsets, at = [], _round16(nj * _JOB)
        for i in jobs_of:
            coef_offsets.append(at)
            at += _round16(2 * infos[i].coef_count)
        host = torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=bool(pin))
        base = host.data_ptr()
        jobs = (JpegJob * nj).from_buffer(host.numpy(), 0) if nj else None

        def one(j):
            i = jobs_of[j]
            data = list_of_bytes[i]
            jobs[j].info = infos[i]
            return L.y4_jpeg_entropy_host(data, len(data), ctypes.byref(infos[i]), base + coef_offsets[j],
                                          infos[i].coef_count, base + j * _JOB + _QT_OFFSET)

        for j, rc in enumerate(run(one, nj)):
            if rc != 0:
                _raise(jobs_of[j], rc, 'y4_jpeg_entropy_host')
    finally:
        if own is not None:
            own.shutdown()
    return HostBatch(n, host, jobs, jobs_of, coef_offsets, infos, fallbacks, bool(apply_orientation))


def decode_entropy_batch(hb, device=None, swap_rb=False, out=None, row_align=4):
    """The device stage: HostBatch -> list of [h, w, 3] uint8 tensors, views into one batch buffer with
    stride(1) == 3 and stride(2) == 1 and rows padded to row_align bytes.  out: an optional 1-D uint8 device buffer to use as
    that batch buffer (bytes between 3 w and the row pitch are never written).  One copy and two launches on the current
    stream; nothing synchronises, unless the same HostBatch is decoded again while its previous copy is in flight."""
    jobs_of = hb.jobs_of
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if device.type != 'cuda':
        raise Y4Error('the JPEG device stage runs on the GPU only: there is no CPU path')
    L = lib()
    shapes = [hb.shape(i) for i in range(hb.n)]
    pitches = [-(-3 * w // row_align) * row_align for _, w in shapes]
    out_offsets, at = [], 0
    for (h, _), p in zip(shapes, pitches):
        out_offsets.append(at)
        at += _round16(h * p)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(at, dtype=torch.uint8, device=device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.numel() >= at and out.is_contiguous()
        views = [torch.as_strided(out, (h, w, 3), (p, 3, 1), o) for (h, w), p, o in zip(shapes, pitches, out_offsets)]
        nj = len(jobs_of)
        if nj:
            if hb.copied is not None:
                # a second decode of the same HostBatch: the device pointers below are written into the pinned table the
                # earlier copy may still be reading (its kernels would then follow a half-new table).  Decoding a batch
                # once, as the loader does, never waits here.
                hb.copied.synchronize()
            dev = torch.empty(hb.host.numel(), dtype=torch.uint8, device=device)
            info_arr = (JpegInfo * nj)(*[hb.infos[i] for i in jobs_of])
            ws_bytes = int(L.y4_jpeg_workspace(info_arr, nj))
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
            ws_at = 0
            for j, i in enumerate(jobs_of):
                job = hb.jobs[j]
                job.coef = dev.data_ptr() + hb.coef_offsets[j]
                job.out = views[i].data_ptr()
                job.out_pitch = pitches[i]
                job.ws_offset = ws_at
                job.apply_orientation = int(hb.apply_orientation)
                job.swap_rb = int(bool(swap_rb))
                ws_at += _round16(hb.infos[i].coef_count)
            dev.copy_(hb.host, non_blocking=True)
            hb.copied = torch.cuda.Event()
            hb.copied.record()
            rc = L.y4_jpeg_decode_u8(dev.data_ptr(), hb.host.data_ptr(), nj, ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                raise Y4Error('y4_jpeg_decode_u8: %s (code %d)' % (L.y4_strerror(rc).decode(), rc))
        for i, arr in hb.fallbacks.items():
            t = torch.from_numpy(arr[..., ::-1].copy() if swap_rb else arr)
            views[i].copy_(t, non_blocking=False)
    return views


def decode_jpeg_batch(list_of_bytes, device=None, workers=8, apply_orientation=True, swap_rb=False, fallback=None, out=None,
                      row_align=4):
    """JPEG files (bytes) -> list of [h, w, 3] uint8 device tensors, BGR like cv2.imread (RGB with swap_rb), the EXIF
    orientation applied like cv2.imread (apply_orientation=False: as stored).  The tensors are views into one batch buffer
    and go to `train_batch` / `val_batch` without a copy.

    workers: threads of the host stage, at most 16.  A file that fails raises Y4Error naming its index and the code before
    anything is launched.  fallback: optional callable bytes -> HWC uint8 BGR ndarray, used ONLY for files the library reports
    as unsupported (progressive, CMYK, ...); without it they raise too."""
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if device.type != 'cuda':
        raise Y4Error('the JPEG device stage runs on the GPU only: there is no CPU path')
    prepared = entropy_batch(list_of_bytes, workers, apply_orientation, fallback)
    return decode_entropy_batch(prepared, device, swap_rb, out, row_align)


def imread(path, device=None, **kw):
    """One file -> [h, w, 3] uint8 BGR device tensor (cv2.imread's pixels)."""
    with open(path, 'rb') as f:
        data = f.read()
    return decode_jpeg_batch([data], device=device, workers=1, **kw)[0]
