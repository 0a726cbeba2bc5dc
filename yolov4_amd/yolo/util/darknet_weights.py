# -*- coding: utf-8 -*-
"""Darknet `.weights` files (the format YOLOv4-tiny's pre-trained weights are published in), read and written with numpy only.

    header   int32 major, minor, revision; then `seen`: uint64 if major * 10 + minor >= 2, else uint32
    per conv with BatchNorm, float32:  beta[n], gamma[n], running_mean[n], running_var[n], filter[n, c, k, k]
    per conv without BatchNorm:        bias[n], filter[n, c, k, k]

in the order of the cfg's layers.  A model takes part through `darknet_convs()`: its ConvBNAct modules in that order (and
`darknet_layers()`, their cfg layer indices, for `cutoff`).  Such a file is plain numbers: it is never unpickled."""
import numpy as np
import torch

from ..._lib import Y4Error

HEADER_OUT = (0, 2, 5)          # what save writes (Darknet's current major, minor, revision), seen = 0


def _convs(model):
    if not hasattr(model, 'darknet_convs'):
        raise Y4Error(f'{type(model).__name__} has no darknet_convs(): its Darknet layer order is not known')
    return list(model.darknet_convs())


def _fields(m):
    """[(tensor, numel)] of ConvBNAct m in file order"""
    if m.has_bn:
        ts = [m.norm.bias, m.norm.weight, m.norm.running_mean, m.norm.running_var, m.conv.weight]
    else:
        if m.conv.bias is None:
            raise Y4Error('a conv without BatchNorm and without bias has no Darknet form')
        ts = [m.conv.bias, m.conv.weight]
    return [(t, t.numel()) for t in ts]


def load_darknet_weights(model, path):
    """Fills the model's convs, in Darknet order, from the file and returns how many were filled.  The file may end at any
    conv boundary (yolov4-tiny.conv.29 holds the first 17 convs): the remaining convs keep their values.  Y4Error -- and
    nothing is written -- for a file that ends inside a conv, has bytes left after the last conv, or is no such file."""
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size < 16:
        raise Y4Error(f'{path}: too short for a Darknet weights header')
    major, minor, _ = (int(v) for v in raw[:12].view('<i4'))
    if not (0 <= major < 1000 and 0 <= minor < 1000):
        raise Y4Error(f'{path}: not a Darknet weights file (version {major}.{minor})')
    off = 12 + (8 if major * 10 + minor >= 2 else 4)
    if raw.size < off or (raw.size - off) % 4:
        raise Y4Error(f'{path}: the file ends inside a value')
    data = raw[off:].view('<f4')
    plan, at, n_loaded = [], 0, 0
    for m in _convs(model):
        if at == data.size:
            break                                        # the file ends here, at a conv boundary
        need = sum(n for _, n in _fields(m))
        if data.size - at < need:
            raise Y4Error(f'{path}: the file ends inside conv {n_loaded} ({data.size - at} of {need} values)')
        for t, n in _fields(m):
            plan.append((t, data[at:at + n]))
            at += n
        n_loaded += 1
    if at != data.size:
        raise Y4Error(f'{path}: {(data.size - at) * 4} bytes left after the last conv')
    with torch.no_grad():
        for t, vals in plan:
            # the filter is [n, c, k, k] in the file; copy_ takes care of the parameter's KRSC memory
            t.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).view(tuple(t.shape)))
    return n_loaded


def save_darknet_weights(model, path, cutoff=None):
    """Writes the model's convs in Darknet order.  cutoff: a Darknet layer number -- only the convs of layers below it are
    written (29 for YOLOv4-tiny: the 17 backbone convs of yolov4-tiny.conv.29).  Returns the number of convs written."""
    convs = _convs(model)
    if cutoff is not None:
        if not hasattr(model, 'darknet_layers'):
            raise Y4Error(f'{type(model).__name__} has no darknet_layers(): cutoff needs the cfg layer indices')
        convs = [m for m, layer in zip(convs, model.darknet_layers()) if layer < int(cutoff)]
    with open(path, 'wb') as f:
        f.write(np.asarray(HEADER_OUT, dtype='<i4').tobytes())
        f.write(np.asarray([0], dtype='<u8').tobytes())
        for m in convs:
            for t, _ in _fields(m):
                f.write(t.detach().to('cpu', torch.float32).contiguous().numpy().astype('<f4', copy=False).tobytes())
    return len(convs)
