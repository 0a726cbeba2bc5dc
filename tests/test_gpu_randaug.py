# -*- coding: utf-8 -*-
"""The kernels of csrc/randaug.hip -- y4_rcrop_randaug_u8_f32 -- driven through the C ABI on every case of
tests/randaug_cases.py (tests/test_randaug_cases.py shows without a GPU that the restatement there is Pillow's arithmetic and
that every case reaches its branch), then through the public interface: `imagenet_batch` with `aug`,
`ImageNetBatchLoader(randaugment=...)` and `python -m yolov4_amd.darknet.main --randaugment`.

Everything is compared bit for bit, with the restatement AND with the committed Pillow pixels.  Sources, the two tables, both
workspaces and the destination each lie between two guards of a NaN bit pattern no kernel produces; pitch padding, the
destination's gaps and every guard must hold that pattern afterwards.  Pillow is not needed here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import randaug_cases as RA
import resample_cases as R
from test_gpu_resample import Bytes, Launch, _stream, _tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
OK, ERR_SHAPE = 0, 1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def npz(golden):
    return golden('randaug')


@pytest.fixture(scope='module')
def sources(npz):
    return {name: npz['src_' + name] for name in RA.SOURCES}


@pytest.fixture(scope='module')
def expected(npz, sources):
    """case -> [B, 3, S, S] float32 from the restatement, computed once; its uint8 images are checked here against the
    committed Pillow pixels so that the GPU results below are compared with Pillow's, not only with the restatement's"""
    out = {}
    for name, c in RA.CASES.items():
        aug, pasted = RA.batch(sources, c['samples'], c['S'])
        for b in range(len(c['samples'])):
            assert np.array_equal(aug[b], npz['pil_%s_%d' % (name, b)]), (name, b)
        out[name] = pasted
    return out


def fill_ops(table, samples, S, n_ops):
    for b, s in enumerate(samples):
        for r, (name, m) in enumerate(RA.sample_ops(s, S)):
            o = table[b * n_ops + r]
            o.op, a, o.factor, o.bits, o.threshold = RA.record(name, m, S)
            o.a[:] = a


class AugLaunch(Launch):
    """test_gpu_resample.Launch plus the operation table and the second workspace, guarded alike"""

    def __init__(self, dev, c, sources):
        from yolov4_amd._lib import RandaugOp
        Launch.__init__(self, dev, c, sources)
        self.n_ops = c['n_ops']
        self.ops = (RandaugOp * max(self.B * self.n_ops, 1))()
        fill_ops(self.ops, c['samples'], self.S, self.n_ops)
        self.op_table = Bytes(dev, ctypes.sizeof(self.ops), np.frombuffer(self.ops, dtype=np.uint8))
        self.ws2_bytes = int(self.L.y4_randaug_workspace(self.B, self.S, self.n_ops))
        assert (self.ws2_bytes > 0) == (self.n_ops > 0)
        self.ws2 = Bytes(dev, max(self.ws2_bytes, 16))

    def run(self, ops=None, n_ops=None):
        sb, sc, sh, sw = self.strides
        m, s = (ctypes.c_float * 3)(*R.MEAN.tolist()), (ctypes.c_float * 3)(*R.STD.tolist())
        host = ctypes.addressof(self.ops if ops is None else ops)
        return self.L.y4_rcrop_randaug_u8_f32(self.table.ptr(), ctypes.addressof(self.jobs), self.B, self.S, m, s,
                                              self.dst.ptr(4 * self.off), sb, sc, sh, sw, self.ws.ptr(), self.ws_bytes,
                                              self.op_table.ptr(), host, self.n_ops if n_ops is None else n_ops,
                                              self.ws2.ptr(), self.ws2_bytes, _stream())

    def check(self, pasted):
        self.check_tables()
        self.check_pixels(pasted)                              # the sources and the job table are unchanged, too
        assert self.op_table.unchanged(), 'the operation table was written'
        self.ws2.get()                                         # the guards around the second workspace
        if self.n_ops == 0:
            assert self.ws2.unchanged(), 'n_ops = 0 leaves the second workspace alone'


@gpu
@pytest.mark.parametrize('name', sorted(RA.CASES))
def test_pixels_equal_pillow(dev, sources, expected, name):
    run = AugLaunch(dev, RA.CASES[name], sources)
    assert run.run() == OK
    torch.cuda.synchronize()
    run.check(expected[name])


@gpu
def test_no_operations_is_the_plain_entry(dev, sources, expected):
    c = RA.CASES['zero_s37']
    a, b = AugLaunch(dev, c, sources), Launch(dev, c, sources)
    assert a.run() == OK and b.gather() == OK
    torch.cuda.synchronize()
    assert np.array_equal(a.dst.get(), b.dst.get()) and np.array_equal(a.ws.get(), b.ws.get())
    a.check(expected['zero_s37'])
    # ... and so is a table of operations with n_ops = 0
    c2 = RA.CASES['cutmix_s37']
    a = AugLaunch(dev, c2, sources)
    assert a.run(n_ops=0) == OK
    torch.cuda.synchronize()
    a.check_pixels(R.batch(sources, c2['samples'], c2['S'])[1])
    assert a.ws2.unchanged()


@gpu
def test_the_same_call_twice_gives_the_same_bits(dev, sources, expected):
    """the statistics are integer sums: their order cannot show; the second call finds both workspaces used"""
    for name in ('cutmix_s37', 'two_s96'):
        run = AugLaunch(dev, RA.CASES[name], sources)
        assert run.run() == OK
        torch.cuda.synchronize()
        first = run.dst.get()
        assert run.run() == OK
        torch.cuda.synchronize()
        assert np.array_equal(run.dst.get(), first)
        run.check(expected[name])


@gpu
def test_refused_calls_write_nothing(dev, sources):
    from yolov4_amd._lib import RandaugOp
    run = AugLaunch(dev, RA.CASES['cutmix_s37'], sources)
    bad = (RandaugOp * len(run.ops))()
    ctypes.memmove(bad, run.ops, ctypes.sizeof(bad))
    bad[5].op = 14
    assert run.run(ops=bad) == ERR_SHAPE and run.run(n_ops=9) == ERR_SHAPE
    torch.cuda.synchronize()
    assert run.dst.unchanged() and run.ws.unchanged() and run.ws2.unchanged()


# ------------------------------------------------------------------------------------------------ the public interface

@gpu
def test_imagenet_batch_with_operations(dev, sources, expected):
    from yolov4_amd.darknet import data as D
    c = RA.CASES['cutmix_s37']
    S = c['S']
    imgs = [torch.from_numpy(sources[s['src']]).to(dev) for s in c['samples']]
    params = [D.CropParams(*s['crop'], *s['res'], *s['win'], s['flip'], s['paste_from'], s['paste'], tuple(RA.sample_ops(s, S)))
              for s in c['samples']]
    for flag in (0, 1):                                       # swap_rb is one flag per call here
        x = D.imagenet_batch(imgs, params, S, memory_format=torch.channels_last, swap_rb=bool(flag))
        want = RA.batch(sources, [dict(s, swap_rb=flag) for s in c['samples']], S)[1]
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # lists of unequal length are padded with Identity; no list at all is the plain entry
    short = [params[0]._replace(aug=params[0].aug[:1]), params[1]._replace(aug=()), params[2]]
    x = D.imagenet_batch(imgs, short, S, swap_rb=False)
    samples = [dict(s, swap_rb=0, ops=s['ops'][:k]) for s, k in zip(c['samples'], (1, 0, 2))]
    assert np.array_equal(x.cpu().numpy().view(np.uint32), RA.batch(sources, samples, S)[1].view(np.uint32))
    x = D.imagenet_batch(imgs, [p._replace(aug=()) for p in params], S, swap_rb=False)
    want = RA.batch(sources, [dict(s, swap_rb=0, ops=[]) for s in c['samples']], S)[1]
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))


@gpu
def test_train_loader_with_randaugment_equals_the_restatement(dev, golden, tmp_path):
    """the loader's batches from the same draws, recomputed by the restatement from the decoded golden pixels"""
    from yolov4_amd.darknet import data as D
    jz = golden('jpeg')
    ds = D.ImageFolder(_tree(tmp_path))
    S, seed = 16, 11
    ra = D.RandAugment()
    loader = D.ImageNetBatchLoader(ds, 3, train=True, crop_size=S, seed=seed, workers=2, cutmix_prob=1.0, randaugment=ra)
    got = [x.cpu().numpy() for x, _ in loader]
    assert len(got) == 2
    seen = set()
    for k, x in enumerate(got):
        rgbs = [jz[os.path.basename(p)[:-4]] for p, _ in ds.samples[3 * k:3 * k + 3]]
        rng = np.random.default_rng([seed, 0, k])
        params = [D.train_params(im.shape[0], im.shape[1], S, rng) for im in rgbs]
        params = [p._replace(aug=ra.sample(S, rng)) for p in params]
        params = D.with_cutmix(params, D.sample_cutmix(3, S, rng, 1.0))
        aug = []
        for im, p in zip(rgbs, params):
            win = R.resample(im[p.crop_y:p.crop_y + p.crop_h, p.crop_x:p.crop_x + p.crop_w], S, S)
            aug.append(RA.apply_ops(np.ascontiguousarray(win[:, ::-1] if p.flip else win), p.aug))
            seen.update(name for name, _ in p.aug)
        for b, p in enumerate(params):
            x0, y0, x1, y1 = p.paste
            mixed = aug[b].copy()
            mixed[y0:y1, x0:x1] = aug[p.paste_from][y0:y1, x0:x1]
            want = R.normalise(np.ascontiguousarray(mixed.transpose(2, 0, 1)))
            assert np.array_equal(x[b].view(np.uint32), want.view(np.uint32)), (k, b, p.aug)
    assert len(seen) >= 4


@gpu
def test_train_loader_without_randaugment_is_unchanged(dev, tmp_path):
    """randaugment=None, and a RandAugment of no operations, give the plain entry's batches from the same draws"""
    from yolov4_amd.darknet import data as D
    ds = D.ImageFolder(_tree(tmp_path))

    def run(**kw):
        loader = D.ImageNetBatchLoader(ds, 3, train=True, crop_size=16, shuffle=True, seed=5, workers=2, cutmix_prob=1.0, **kw)
        return [x.cpu().numpy() for x, _ in loader]

    plain = run()
    for x, y in zip(plain, run(randaugment=None)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # a RandAugment of no operations draws nothing
    for x, y in zip(plain, run(randaugment=D.RandAugment(num_ops=0))):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert any(not np.array_equal(x, y) for x, y in zip(plain, run(randaugment=D.RandAugment(2, 30))))


@gpu
def test_main_with_randaugment_runs_one_epoch(dev, tmp_path):
    data = tmp_path / 'data'
    _tree(data, 'train')
    _tree(data, 'val')
    work = tmp_path / 'work'
    work.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'yolov4_amd.darknet.main', str(data), '--epochs', '1', '-b', '3', '--crop-size',
                        '64', '--val-size', '72', '--num-classes', '2', '--cutmix-prob', '1', '--print-freq', '1', '-j', '2',
                        '--randaugment', '--ra-num-ops', '3', '--ra-magnitude', '15'],
                       cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'Epoch: [0][2/2]' in r.stdout and ' * Prec@1' in r.stdout, r.stdout[-2000:]
    assert 'randaugment=True' in r.stdout and 'ra_num_ops=3' in r.stdout
    ckpt = torch.load(str(work / 'checkpoint.pth.tar'), map_location='cpu', weights_only=True)
    assert ckpt['epoch'] == 1
    assert all(bool(torch.isfinite(v).all()) for v in ckpt['state_dict'].values() if v.is_floating_point())
