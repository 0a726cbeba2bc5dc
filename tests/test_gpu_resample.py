# -*- coding: utf-8 -*-
"""The kernels of csrc/resample.hip -- y4_rcrop_coeffs_i32 and y4_rcrop_u8_f32 -- driven through the C ABI on every case of
tests/resample_cases.py (tests/test_resample_cases.py shows without a GPU that the restatement there is Pillow's arithmetic
and that every case reaches its branch), then through the public interface: `imagenet_batch`, `ImageNetBatchLoader` and
`python -m yolov4_amd.darknet.main`.

Everything is compared bit for bit: the tables with the restatement's bounds and taps, the pixels with the restatement AND
with the committed Pillow pixels.  Sources (at their pitches and byte offsets), the job table, the workspace and the
destination each lie between two guards of a NaN bit pattern no kernel produces; pitch padding, the workspace's alignment
padding, the destination's gaps and every guard must hold that pattern afterwards.  Pillow is not needed here."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_cases as J
import resample_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
G = 128                                  # guard bytes in front of and behind every device buffer
SENT_BYTES = np.array([R.SENT], np.uint32).view(np.uint8)
OK, ERR_SHAPE = 0, 1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def npz(golden):
    return golden('resample')


@pytest.fixture(scope='module')
def sources(npz):
    return {name: npz['src_' + name] for name in R.SOURCES}


@pytest.fixture(scope='module')
def expected(npz, sources):
    """case -> (plain, pasted) [B, 3, S, S] float32 from the restatement, computed once; checked here against the committed
    Pillow pixels so that the GPU results below are compared with Pillow's, not only with the restatement's"""
    out = {}
    for name, c in R.CASES.items():
        S = c['S']
        plain, pasted = R.batch(sources, c['samples'], S)
        for b, s in enumerate(c['samples']):
            win = npz['pil_%s_%d' % (name, b)][s['win'][1]:s['win'][1] + S, s['win'][0]:s['win'][0] + S]
            win = win[:, :, ::-1] if s['swap_rb'] else win
            win = win[:, ::-1] if s['flip'] else win
            assert np.array_equal(plain[b], R.normalise(np.ascontiguousarray(win.transpose(2, 0, 1))))
        out[name] = (plain, pasted)
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bytes(object):
    """n bytes on the device between two guards; body = the sentinel pattern unless `init` (uint8) is given"""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        h = np.resize(SENT_BYTES, self.n + 2 * G)
        if init is not None:
            h[G:G + self.n] = np.ascontiguousarray(init, dtype=np.uint8).ravel()
        self.before = h.copy()
        self.t = torch.from_numpy(h).to(dev)

    def ptr(self, off=0):
        return self.t.data_ptr() + G + off

    def get(self):
        h = self.t.cpu().numpy()
        assert np.array_equal(h[:G], self.before[:G]) and np.array_equal(h[G + self.n:], self.before[G + self.n:]), \
            'write outside the buffer'
        return h[G:G + self.n].copy()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before)


class Launch(object):
    """device copies of one case: sources at their pitches and offsets, the job table, the workspace, the destination"""

    def __init__(self, dev, c, sources):
        from yolov4_amd._lib import RcropJob, lib
        self.L = lib()
        self.c, self.S, self.B = c, c['S'], len(c['samples'])
        self.imgs = []
        self.jobs = (RcropJob * self.B)()
        at = 0
        self.ws_at = []
        for b, s in enumerate(c['samples']):
            img = sources[s['src']]
            h, w = img.shape[:2]
            pitch = 3 * w + s['pitch_extra']
            rows = np.resize(SENT_BYTES, (h, pitch)).copy()            # pitch padding holds the pattern too
            rows[:, :3 * w] = img.reshape(h, 3 * w)
            body = np.concatenate([np.resize(SENT_BYTES, s['offset']), rows.ravel()])
            buf = Bytes(dev, body.size, body)
            self.imgs.append(buf)
            j = self.jobs[b]
            j.src, j.src_pitch, j.src_h, j.src_w, j.swap_rb = buf.ptr(s['offset']), pitch, h, w, s['swap_rb']
            j.crop_x, j.crop_y, j.crop_w, j.crop_h = s['crop']
            j.res_w, j.res_h = s['res']
            j.win_x, j.win_y = s['win']
            j.flip, j.paste_from = s['flip'], s['paste_from']
            j.paste_x0, j.paste_y0, j.paste_x1, j.paste_y1 = s['paste']
            j.ws_offset = at
            self.ws_at.append(at)
            at += R.job_bytes(s, self.S)
        self.ws_bytes = at
        assert self.L.y4_rcrop_workspace(self.jobs, self.B, self.S) == at
        self.ws = Bytes(dev, at)
        self.table = Bytes(dev, ctypes.sizeof(self.jobs), np.frombuffer(self.jobs, dtype=np.uint8))
        self.total, self.off, self.strides = R.dst_layout(c['layout'], self.B, self.S)
        self.dst = Bytes(dev, 4 * self.total)

    def coeffs(self):
        return self.L.y4_rcrop_coeffs_i32(self.table.ptr(), ctypes.addressof(self.jobs), self.B, self.S, self.ws.ptr(),
                                          self.ws_bytes, _stream())

    def gather(self, mean=R.MEAN, std=R.STD, jobs=None):
        sb, sc, sh, sw = self.strides
        m, s = (ctypes.c_float * 3)(*mean.tolist()), (ctypes.c_float * 3)(*std.tolist())
        host = ctypes.addressof(self.jobs if jobs is None else jobs)
        return self.L.y4_rcrop_u8_f32(self.table.ptr(), host, self.B, self.S, m, s, self.dst.ptr(4 * self.off), sb, sc, sh, sw,
                                      self.ws.ptr(), self.ws_bytes, _stream())

    def check_tables(self):
        got = self.ws.get().view(np.int32)
        want = np.resize(SENT_BYTES, self.ws_bytes).view(np.int32).copy()      # alignment padding stays untouched
        for s, at in zip(self.c['samples'], self.ws_at):
            words = R.job_tables(s, self.S)
            want[at // 4:at // 4 + words.size] = words
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, 'first differing table word %d: %d, expected %d' % (bad[0], got[bad[0]], want[bad[0]])

    def check_pixels(self, pasted):
        got = self.dst.get().view(np.uint32)
        want = np.resize(SENT_BYTES, 4 * self.total).view(np.uint32).copy()    # gaps and margins stay untouched
        want[R.dst_index(self.c['layout'], self.B, self.S).ravel()] = pasted.ravel().view(np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, '%d differing words, the first at %d: %08x, expected %08x' % (bad.size, bad[0], got[bad[0]],
                                                                                            want[bad[0]])
        for buf in self.imgs:
            assert buf.unchanged(), 'a source was written'
        assert self.table.unchanged(), 'the job table was written'


@gpu
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_tables_equal_the_restatement(dev, sources, name):
    run = Launch(dev, R.CASES[name], sources)
    assert run.coeffs() == OK
    torch.cuda.synchronize()
    run.check_tables()
    assert run.dst.unchanged(), 'y4_rcrop_coeffs_i32 fills the tables only'


@gpu
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_pixels_equal_pillow(dev, sources, expected, name):
    run = Launch(dev, R.CASES[name], sources)
    assert run.gather() == OK
    torch.cuda.synchronize()
    run.check_tables()
    run.check_pixels(expected[name][1])


@gpu
def test_pasted_pixels_are_the_partners_plain_pixels(dev, sources, expected):
    """the same batch without its pastes gives `plain`; with them every rectangle holds plain[paste_from] and the rest plain[b]"""
    c = R.CASES['cutmix']
    bare = dict(c, samples=[dict(s, paste_from=-1) for s in c['samples']])
    run = Launch(dev, bare, sources)
    assert run.gather() == OK
    torch.cuda.synchronize()
    plain, pasted = expected['cutmix']
    run.check_pixels(plain)
    assert not np.array_equal(plain.view(np.uint32), pasted.view(np.uint32))


@gpu
def test_other_normalisation_constants(dev, sources):
    """a mean and std that are not the defaults, different per channel: the division is the correctly rounded one"""
    c = R.CASES['down_crop_flip']
    mean, std = np.array([3.25, 100.7, 254.9], np.float32), np.array([0.3, 7.0, 59.123], np.float32)
    run = Launch(dev, c, sources)
    assert run.gather(mean, std) == OK
    torch.cuda.synchronize()
    run.check_pixels(R.batch(sources, c['samples'], c['S'], mean, std)[1])


@gpu
def test_refused_calls_write_nothing(dev, sources):
    from yolov4_amd._lib import RcropJob
    run = Launch(dev, R.CASES['cutmix'], sources)
    bad = (RcropJob * run.B)()
    ctypes.memmove(bad, run.jobs, ctypes.sizeof(bad))
    bad[3].win_x = bad[3].res_w - run.S + 1
    assert run.gather(jobs=bad) == ERR_SHAPE
    assert run.gather(std=np.array([1, 0, 1], np.float32)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert run.dst.unchanged() and run.ws.unchanged()


# ------------------------------------------------------------------------------------------------ the public interface

FILES = [('ant', ['s29x37_420', 's17x33_444', 'orient6_13x21']), ('bee', ['s48x40_422', 'q95_29x37_420', 'gray_48x40'])]


def _tree(root, split=None):
    base = os.path.join(str(root), split) if split else str(root)
    for cls, names in FILES:
        os.makedirs(os.path.join(base, cls))
        for n in names:
            shutil.copyfile(os.path.join(J.JPEG_DIR, n + '.jpg'), os.path.join(base, cls, n + '.jpg'))
    return base


@gpu
def test_imagenet_batch_on_tensors(dev, sources):
    """the Python entry: the cutmix case from packed BGR-or-not tensors, channels-last result"""
    from yolov4_amd.darknet import data as D
    c = R.CASES['cutmix_nhwc']
    imgs = [torch.from_numpy(sources[s['src']]).to(dev) for s in c['samples']]
    params = [D.CropParams(*s['crop'], *s['res'], *s['win'], s['flip'], s['paste_from'], s['paste']) for s in c['samples']]
    # swap_rb is one flag per call here: compare per sample with the flag the case gives it
    for flag in (0, 1):
        x = D.imagenet_batch(imgs, params, c['S'], memory_format=torch.channels_last, swap_rb=bool(flag))
        assert x.is_contiguous(memory_format=torch.channels_last)
        want = R.batch(sources, [dict(s, swap_rb=flag) for s in c['samples']], c['S'])[1]
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    out = torch.full((3, 3, 16, 16), float('nan'), device=dev)
    assert D.imagenet_batch(imgs, params, 16, out=out) is out and not bool(torch.isnan(out).any())


@gpu
def test_val_loader_equals_the_restatement(dev, golden, tmp_path):
    from yolov4_amd.darknet import data as D
    jz = golden('jpeg')
    ds = D.ImageFolder(_tree(tmp_path))
    assert ds.classes == ['ant', 'bee'] and len(ds) == 6
    loader = D.ImageNetBatchLoader(ds, 4, train=False, crop_size=16, val_size=18, workers=2)
    assert len(loader) == 2
    got = list(loader)
    assert [tuple(x.shape) for x, _ in got] == [(4, 3, 16, 16), (2, 3, 16, 16)]
    assert all(t.dtype == torch.int64 and t.is_cuda for _, t in got)
    assert torch.cat([t for _, t in got]).tolist() == [0, 0, 0, 1, 1, 1]
    x = torch.cat([x for x, _ in got]).cpu().numpy()
    for k, (path, _) in enumerate(ds.samples):
        rgb = jz[os.path.basename(path)[:-4]]                       # the decoded pixels, RGB, orientation applied
        h, w = rgb.shape[:2]
        res_h, res_w, wy, wx = D.val_geometry(h, w, 18, 16)
        want = R.normalise(np.ascontiguousarray(R.resample(rgb, res_w, res_h, wx, wy, 16, 16).transpose(2, 0, 1)))
        assert np.array_equal(x[k].view(np.uint32), want.view(np.uint32)), path


@gpu
def test_train_loader_is_reproducible(dev, tmp_path):
    from yolov4_amd.darknet import data as D
    from yolov4_amd.darknet.loss import MixedTarget
    ds = D.ImageFolder(_tree(tmp_path))

    def run(seed, epoch=0, prob=1.0):
        loader = D.ImageNetBatchLoader(ds, 3, train=True, crop_size=16, shuffle=True, seed=seed, workers=2, cutmix_prob=prob)
        loader.set_epoch(epoch)
        return [(x.cpu().numpy(), t) for x, t in loader]

    a, b, c = run(5), run(5), run(6)
    assert len(a) == 2
    for (xa, ta), (xb, tb) in zip(a, b):
        assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
        assert isinstance(ta, MixedTarget) and torch.equal(ta.a, tb.a) and torch.equal(ta.b, tb.b) and ta.lam == tb.lam
        assert ta.a.dtype == torch.int64 and ta.a.is_cuda and 0.0 <= ta.lam <= 1.0 and np.isfinite(xa).all()
    assert sorted(torch.cat([t.a for _, t in a]).tolist()) == [0, 0, 0, 1, 1, 1]
    assert any(not np.array_equal(xa, xc) for (xa, _), (xc, _) in zip(a, c))
    assert any(not np.array_equal(xa, xe) for (xa, _), (xe, _) in zip(a, run(5, epoch=1)))
    assert all(torch.is_tensor(t) for _, t in run(5, prob=0.0))


@gpu
def test_main_trains_one_epoch_and_leaves_a_backbone_checkpoint(dev, tmp_path):
    import recipe
    from yolov4_amd.yolo.model.yolov4 import YOLOv4
    data = tmp_path / 'data'
    _tree(data, 'train')
    _tree(data, 'val')
    work = tmp_path / 'work'
    work.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'yolov4_amd.darknet.main', str(data), '--epochs', '1', '-b', '3', '--crop-size',
                        '64', '--val-size', '72', '--num-classes', '2', '--cutmix-prob', '1', '--print-freq', '1', '-j', '2'],
                       cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'Epoch: [0][2/2]' in r.stdout and ' * Prec@1' in r.stdout, r.stdout[-2000:]
    path = str(work / 'checkpoint.pth.tar')
    assert os.path.isfile(path)
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    assert ckpt['epoch'] == 1 and all(k.startswith('module.') for k in ckpt['state_dict'])
    assert ckpt['state_dict']['module.classifier.weight'].shape == (2, 1024)
    det = YOLOv4(dict(recipe.MODEL_CFG, BACKBONE_PRETRAINED=path))           # strict load of the backbone's 432 entries
    for k, v in det.backbone.state_dict().items():
        assert torch.equal(v, ckpt['state_dict']['module.backbone.' + k]), k
    assert all(bool(torch.isfinite(v).all()) for v in ckpt['state_dict'].values() if v.is_floating_point())
