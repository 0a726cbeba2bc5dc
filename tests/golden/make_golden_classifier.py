# -*- coding: utf-8 -*-
"""Golden vectors of the ImageNet classifier.  Like make_golden.py this runs ONLY in the build container, where the
reference (zjykzj/YOLOv4) is mounted read-only at /root/reference: it imports the reference's
darknet.darknet.CSPDarknet53, fills it by the seeded recipe (tests/classifier_cases.fill_classifier_) and runs the two
train steps of classifier_cases.MODEL_STEPS on the PyTorch CPU path, once in fp32 and once in fp64, each from the freshly
filled weights.  classifier.npz holds data only: logits, loss, three gradients, four running statistics, the
state_dict's key / shape list and the digest of classifier_cases.cpu_fingerprint() on the machine that wrote it.

    python tests/golden/make_golden_classifier.py

Stored per step s and precision p in {32, 64}: logits{p}_{s}, loss{p}_{s}, grad{p}_{s}_<key>, stat{p}_{s}_<key>.  The fp64
arrays are float64 except the classifier.weight gradient, which is stored rounded to float32 to keep the file small (it
is only ever used as the centre of a distance that is 100x coarser than that rounding).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, '/root/reference')

import numpy as np
import torch

import classifier_cases as CC

from darknet.darknet import CSPDarknet53                                          # noqa: E402

torch.set_num_threads(CC.GOLDEN_THREADS)


def run(step, dtype):
    torch.manual_seed(0)
    model = CSPDarknet53(CC.MODEL_CLASSES)
    sd = model.state_dict()
    CC.fill_classifier_(sd, CC.MODEL_SEED)
    model.load_state_dict(sd)
    model = model.to(dtype).train()
    x, target = CC.model_input(step)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=CC.SMOOTHING)
    logits = model(x.to(dtype))
    loss = criterion(logits, target)
    loss.backward()
    params = dict(model.named_parameters())
    out = {'logits': logits.detach().numpy(), 'loss': loss.detach().numpy()}
    for k in CC.GRAD_KEYS:
        g = params[k].grad.numpy()
        out['grad_' + k] = g.astype(np.float32) if k == 'classifier.weight' else g
    now = model.state_dict()
    for k in CC.STAT_KEYS:
        out['stat_' + k] = now[k].numpy()
    return out, model


def main():
    arrs = {}
    for step in range(len(CC.MODEL_STEPS)):
        for bits, dtype in ((32, torch.float32), (64, torch.float64)):
            out, model = run(step, dtype)
            for k, v in out.items():
                name, _, key = k.partition('_')
                arrs[f'{name}{bits}_{step}' + ('_' + key if key else '')] = v
    sd = model.state_dict()
    arrs['fingerprint'] = np.array(CC.cpu_fingerprint())    # how this machine rounds fp32 (see classifier_cases.cpu_fingerprint)
    arrs['keys'] = np.array(list(sd.keys()))
    arrs['shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(HERE, 'classifier.npz')
    np.savez_compressed(path, **arrs)
    print(f'classifier.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays, {len(sd)} keys')


if __name__ == '__main__':
    main()
