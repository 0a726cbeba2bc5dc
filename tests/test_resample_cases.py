# -*- coding: utf-8 -*-
"""The ImageNet input pipeline without a GPU: the numpy restatement of tests/resample_cases.py against the committed Pillow
pixels (tests/golden/resample.npz) and, where Pillow is installed, against Pillow itself; that every case of the list reaches
the branch it exists for; the host-side samplers of yolov4_amd/darknet/data.py; every host-side error of the three entry
points through the loaded library; mixed_loss on a plain target."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_cases as R
import yolov4_amd
from yolov4_amd._lib import RcropJob
from yolov4_amd.darknet import data as D
from yolov4_amd.darknet.loss import MixedTarget, mixed_loss

OK, ERR_SHAPE, ERR_NULL, ERR_WORKSPACE = 0, 1, 2, 4
ALL = sorted(R.CASES)


@pytest.fixture(scope='module')
def npz(golden):
    return golden('resample')


def _crop(src, s):
    cx, cy, cw, ch = s['crop']
    return src[cy:cy + ch, cx:cx + cw]


# ------------------------------------------------------------------------------------------------ fixture and restatement

def test_fixture_holds_the_case_list(npz):
    assert ctypes.sizeof(RcropJob) == 96
    for name, spec in R.SOURCES.items():
        assert np.array_equal(npz['src_' + name], R.make_source(*spec)), name
    for name, c in R.CASES.items():
        assert np.array_equal(npz['par_' + name], R.case_params(c)), name
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resample.npz')) < 300 * 1024


@pytest.mark.parametrize('name', ALL)
def test_restatement_equals_the_fixture(npz, name):
    c = R.CASES[name]
    for b, s in enumerate(c['samples']):
        want = npz['pil_%s_%d' % (name, b)]
        crop = _crop(npz['src_' + s['src']], s)
        assert np.array_equal(R.resample(crop, s['res'][0], s['res'][1]), want)
        # the window alone, from tables of S rows and columns, is that window of the whole image
        S, (wx, wy) = c['S'], s['win']
        assert np.array_equal(R.resample(crop, s['res'][0], s['res'][1], wx, wy, S, S), want[wy:wy + S, wx:wx + S])


@pytest.mark.parametrize('name', ALL)
def test_restatement_equals_live_pillow(name):
    Image = pytest.importorskip('PIL.Image')
    sources = R.make_sources()
    c = R.CASES[name]
    for s in c['samples']:
        cx, cy, cw, ch = s['crop']
        im = Image.fromarray(sources[s['src']], 'RGB').crop((cx, cy, cx + cw, cy + ch)).resize(tuple(s['res']), Image.BILINEAR)
        assert np.array_equal(R.resample(_crop(sources[s['src']], s), s['res'][0], s['res'][1]), np.asarray(im))


def test_live_pillow_on_more_geometries():
    """sizes the case list does not hold: a 37-fold downscale, equal sizes, 1 x 1 results, near-ties of the scale"""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(5)
    for (h, w), (rw, rh) in [((37, 74), (2, 1)), ((12, 12), (12, 12)), ((1, 1), (5, 3)), ((100, 3), (3, 100)), ((31, 17), (16, 16)),
                             ((64, 48), (63, 47)), ((48, 64), (49, 65)), ((375, 50), (30, 225)), ((2, 3), (1, 1))]:
        src = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        want = np.asarray(Image.fromarray(src, 'RGB').resize((rw, rh), Image.BILINEAR))
        assert np.array_equal(R.resample(src, rw, rh), want), ((h, w), (rw, rh))


def test_val_geometry_is_resize_then_centre_crop_in_pillow():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(6)
    for (h, w), val_size, crop_size in [((33, 40), 39, 32), ((40, 33), 39, 32), ((29, 29), 18, 16), ((20, 61), 18, 16)]:
        src = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        res_h, res_w, wy, wx = D.val_geometry(h, w, val_size, crop_size)
        im = Image.fromarray(src, 'RGB').resize((res_w, res_h), Image.BILINEAR)
        want = np.asarray(im.crop((wx, wy, wx + crop_size, wy + crop_size)))
        assert np.array_equal(R.resample(src, res_w, res_h, wx, wy, crop_size, crop_size), want)


# ------------------------------------------------------------------------------------------------ every case reaches its branch

def _tables(s, S):
    bx, kx = R.coeffs(s['crop'][2], s['res'][0], s['win'][0], S)
    by, ky = R.coeffs(s['crop'][3], s['res'][1], s['win'][1], S)
    return bx, kx, by, ky


def test_case_properties(npz):
    C = R.CASES
    s = C['down_whole']['samples'][0]
    assert s['crop'] == (0, 0, 37, 53) and R.ksize(37, 16) == 7 and R.ksize(53, 16) == 9
    for n in ('down_crop', 'down_crop_flip', 'down_crop_pitch'):
        assert C[n]['samples'][0]['crop'] == (5, 3, 30, 24)
    assert C['down_crop']['samples'][0]['flip'] == 0 and C['down_crop_flip']['samples'][0]['flip'] == 1
    # upscale: fs = 1, 3 taps, clamped edge taps
    s = C['up']['samples'][0]
    bx, kx, by, ky = _tables(s, 16)
    assert s['crop'][2:] == (9, 7) and kx.shape[1] == 3 and ky.shape[1] == 3
    assert bx[:, 1].min() < 3 and by[:, 1].min() < 3 and bx[0, 0] == 0 and bx[-1, 0] + bx[-1, 1] == 9
    # long tap loops on either axis: more taps than a wave has lanes, more source rows than a tile has output rows
    s = C['long_taps']['samples'][0]
    assert s['crop'] == (4, 2, 290, 13) and npz['src_' + s['src']].shape == (17, 300, 3) and R.ksize(290, 8) >= 73
    assert _tables(s, 8)[0][:, 1].max() > 64
    s = C['long_taps_y']['samples'][0]
    assert R.ksize(290, 8) >= 73 and _tables(s, 8)[2][:, 1].max() > 64 and s['crop'][3] == 290
    assert C['one_pixel']['samples'][0]['crop'][2:] == (1, 1) and C['one_pixel']['S'] == 8
    # the identity pass: taps {2^22, 0}
    s = C['identity_x']['samples'][0]
    bx, kx, by, ky = _tables(s, 16)
    assert s['crop'][2] == s['res'][0] and s['crop'][3] != s['res'][1]
    assert all(kx[i, :bx[i, 1]].tolist() in ([1 << 22, 0], [1 << 22]) for i in range(16)) and ky.shape[1] > 3
    s = C['identity_both']['samples'][0]
    assert s['crop'][2:] == s['res'] == (16, 16)
    crop = _crop(npz['src_' + s['src']], s)
    assert np.array_equal(R.resample(crop, 16, 16), crop)
    assert C['odd_size']['S'] == 33 and all(33 % t for t in (2, 4, 6, 8, 16, 64))      # no tile height, no wave
    # the validation geometry: a window strictly inside the resampled image, at different origins on x and y
    for n in ('val_window', 'val_window_binary'):
        s, S = C[n]['samples'][0], C[n]['S']
        assert s['crop'][2:] == (40, 33) and s['res'] == (48, 39) and S == 32
        assert s['win'] == (int(round((48 - 32) / 2.0)), int(round((39 - 32) / 2.0))) and s['win'][0] != s['win'][1]
        assert 0 < s['win'][0] < 48 - S and 0 < s['win'][1] < 39 - S
    flat = [s for c in C.values() for s in c['samples']]
    assert any(s['pitch_extra'] > 0 for s in flat) and any(s['offset'] % 2 == 1 for s in flat)
    assert {s['swap_rb'] for s in flat} == {0, 1} and {s['flip'] for s in flat} == {0, 1}
    assert {R.SOURCES[s['src']][0] for s in flat} == {'random', 'binary', 'checker'}
    for name, (kind, _, _, _) in R.SOURCES.items():
        if kind != 'random':
            assert set(np.unique(npz['src_' + name])) == {0, 255}
    assert {c['layout'] for c in C.values()} == {'nchw', 'nhwc', 'gaps'}
    # the taps of a row sum to 2^22 up to their rounding: no accumulator leaves int32
    for s in flat:
        for k in _tables(s, 8)[1::2]:
            assert np.abs(k.sum(axis=1) - (1 << 22)).max() <= k.shape[1]


def test_cutmix_case_properties():
    c = R.CASES['cutmix']
    S, sm = c['S'], c['samples']
    perm = [s['paste_from'] for s in sm]
    assert len(sm) == 5 and sorted(perm) == list(range(5)) and any(p == b for b, p in enumerate(perm))
    assert len({(s['crop'][2:], s['res']) for s in sm}) == 5                       # mixed sizes
    boxes = [s['paste'] for s in sm]
    assert any(sum([x0 == 0, y0 == 0, x1 == S, y1 == S]) == 2 and x1 > x0 and y1 > y0 for x0, y0, x1, y1 in boxes)
    assert any(x0 == x1 or y0 == y1 for x0, y0, x1, y1 in boxes)
    assert any(sm[s['paste_from']]['flip'] == 1 and s['flip'] == 0 and s['paste'][2] > s['paste'][0] for s in sm)
    # rectangles whose edges fall inside a tile of rows, whatever its height, and one that holds whole tiles of rows
    assert any(y0 % 2 and y1 % 2 for _, y0, _, y1 in boxes) and any(y1 - y0 >= 24 for _, y0, _, y1 in boxes)
    sources = R.make_sources()
    plain, out = R.batch(sources, sm, S)
    for b, s in enumerate(sm):
        x0, y0, x1, y1 = s['paste']
        inside = np.zeros((S, S), bool)
        inside[y0:y1, x0:x1] = True
        assert np.array_equal(out[b][:, inside], plain[s['paste_from']][:, inside])
        assert np.array_equal(out[b][:, ~inside], plain[b][:, ~inside])
        if s['paste_from'] != b and inside.any():
            assert not np.array_equal(out[b], plain[b])
    c = R.CASES['cutmix_nhwc']
    assert c['samples'][0]['paste'] == (0, 0, 16, 16) and c['samples'][1]['paste_from'] == -1    # a whole-image paste


def test_normalisation_is_the_references():
    assert R.MEAN.dtype == np.float32 and np.array_equal(R.MEAN, torch.tensor([0.485 * 255, 0.456 * 255, 0.406 * 255]).numpy())
    assert np.array_equal(R.STD, torch.tensor([0.229 * 255, 0.224 * 255, 0.225 * 255]).numpy())
    assert np.array_equal(np.array(D.MEAN, np.float32), R.MEAN) and np.array_equal(np.array(D.STD, np.float32), R.STD)
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16).repeat(3, axis=0)
    want = torch.from_numpy(u8).float().sub_(torch.from_numpy(R.MEAN).view(3, 1, 1)).div_(torch.from_numpy(R.STD).view(3, 1, 1))
    assert np.array_equal(R.normalise(u8), want.numpy())


# ------------------------------------------------------------------------------------------------ host-side samplers

def test_sample_crop_invariants():
    lo, hi = 3. / 4., 4. / 3.
    accepted = flips = 0
    for seed in range(400):
        rng = np.random.default_rng(seed)
        h, w = [(375, 500), (500, 375), (64, 64), (17, 300), (1, 1)][seed % 5]
        top, left, ch, cw, flip = D.sample_crop(h, w, rng)
        assert 0 < ch <= h and 0 < cw <= w and 0 <= top <= h - ch and 0 <= left <= w - cw
        flips += flip
        if (h, w) in ((375, 500), (500, 375), (64, 64)):
            # sqrt(t a) and sqrt(t / a) each move by at most 0.5 under the rounding
            assert (cw - 0.5) / (ch + 0.5) <= hi and (cw + 0.5) / (ch - 0.5) >= lo
            assert 0.08 * h * w * 0.9 - (ch + cw) <= ch * cw <= h * w
            accepted += 1
    assert accepted == 240 and 120 < flips < 280
    # same generator state, same draw
    assert D.sample_crop(375, 500, np.random.default_rng(3)) == D.sample_crop(375, 500, np.random.default_rng(3))


def test_sample_crop_falls_back_to_the_central_crop():
    for seed in range(20):
        top, left, ch, cw, _ = D.sample_crop(1000, 10, np.random.default_rng(seed))
        assert (cw, ch) == (10, int(round(10 / (3. / 4.)))) == (10, 13) and (top, left) == ((1000 - 13) // 2, 0)
        top, left, ch, cw, _ = D.sample_crop(10, 1000, np.random.default_rng(seed))
        assert (cw, ch) == (int(round(10 * (4. / 3.))), 10) == (13, 10) and (top, left) == (0, (1000 - 13) // 2)
    # inside the ratio range but never accepted: scale above 1 asks for more than the image
    assert D.sample_crop(30, 40, np.random.default_rng(0), scale=(4.0, 5.0))[:4] == (0, 0, 30, 40)


def test_val_geometry():
    assert D.val_geometry(375, 500, 288, 256) == (288, 384, 16, 64)
    assert D.val_geometry(500, 375, 288, 256) == (384, 288, 64, 16)
    assert D.val_geometry(288, 288, 288, 256) == (288, 288, 16, 16)
    assert D.val_geometry(300, 1000, 288, 256) == (288, 960, 16, 352)
    assert D.val_geometry(33, 40, 39, 32) == (39, 47, 4, 8)           # int(), not round(): 39 * 40 / 33 = 47.27; 3.5 -> 4, 7.5 -> 8
    with pytest.raises(ValueError):
        D.val_geometry(375, 500, 200, 256)
    p = D.val_params(375, 500, 288, 256)
    assert (p.crop_x, p.crop_y, p.crop_w, p.crop_h, p.res_w, p.res_h, p.win_x, p.win_y, p.flip, p.paste_from) == \
        (0, 0, 500, 375, 384, 288, 64, 16, 0, -1)


def test_sample_cutmix():
    fired = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        S, B = [16, 33, 256][seed % 3], 1 + seed % 7
        mix = D.sample_cutmix(B, S, rng, 0.5)
        if mix is None:
            continue
        fired += 1
        perm, (x0, y0, x1, y1), lam = mix
        assert sorted(perm) == list(range(B))
        assert 0 <= x0 <= x1 <= S and 0 <= y0 <= y1 <= S
        inside = np.zeros((S, S), bool)
        inside[y0:y1, x0:x1] = True
        assert lam == 1.0 - float(inside.sum()) / float(S * S) and 0.0 <= lam <= 1.0
    assert 60 < fired < 140
    assert D.sample_cutmix(4, 16, np.random.default_rng(0), 0.0) is None
    assert all(D.sample_cutmix(4, 16, np.random.default_rng(s), 1.0) is not None for s in range(20))
    params = [D.CropParams(0, 0, 8, 8, 16, 16)] * 3
    assert D.with_cutmix(params, None) == params
    mixed = D.with_cutmix(params, ([2, 0, 1], (1, 2, 3, 4), 0.9))
    assert [p.paste_from for p in mixed] == [2, 0, 1] and all(p.paste == (1, 2, 3, 4) for p in mixed)


def test_image_folder_order(tmp_path):
    def put(*parts):
        path = tmp_path.joinpath(*parts)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(('/'.join(parts)).encode())
    put('zebra', 'b.jpg')
    put('zebra', 'a.JPEG')
    put('zebra', 'notes.txt')                   # a foreign file
    put('ant', 'z.jpg')
    put('ant', 'deep', 'y.JPG')                 # a nested directory, an upper-case extension
    put('ant', 'deep', 'deeper', 'x.jpeg')
    put('ant', 'c.png')
    (tmp_path / 'stray.jpg').write_bytes(b'x')  # a file beside the class directories is no class
    ds = D.ImageFolder(str(tmp_path))
    assert ds.classes == ['ant', 'zebra'] and ds.class_to_idx == {'ant': 0, 'zebra': 1}
    rel = [(os.path.relpath(p, str(tmp_path)).replace(os.sep, '/'), t) for p, t in ds.samples]
    assert rel == [('ant/z.jpg', 0), ('ant/deep/y.JPG', 0), ('ant/deep/deeper/x.jpeg', 0), ('zebra/a.JPEG', 1), ('zebra/b.jpg', 1)]
    assert len(ds) == 5 and ds[1] == (b'ant/deep/y.JPG', 0) and ds.targets == [0, 0, 0, 1, 1]
    assert [p for p, _ in D.ImageFolder(str(tmp_path), extensions=('.jpg',)).samples] == \
        [str(tmp_path / 'ant' / 'z.jpg'), str(tmp_path / 'ant' / 'deep' / 'y.JPG'), str(tmp_path / 'zebra' / 'b.jpg')]
    (tmp_path / 'empty').mkdir()
    with pytest.raises(FileNotFoundError, match='empty'):
        D.ImageFolder(str(tmp_path))
    bare = tmp_path / 'ant' / 'deep' / 'deeper'
    with pytest.raises(FileNotFoundError):
        D.ImageFolder(str(bare))                # no class directory at all


# ------------------------------------------------------------------------------------------------ the C ABI's host side

FAKE = 0x10000          # never dereferenced: every call below is refused before a launch


def _job(**over):
    j = RcropJob()
    j.src, j.src_pitch, j.src_h, j.src_w, j.swap_rb = FAKE, 3 * 40, 33, 40, 0
    j.crop_x, j.crop_y, j.crop_w, j.crop_h, j.res_w, j.res_h = 2, 1, 30, 24, 20, 18
    j.win_x, j.win_y, j.flip, j.paste_from = 3, 1, 0, -1
    j.ws_offset = 0
    for k, v in over.items():
        setattr(j, k, v)
    return j


def _calls(jobs, S=16, ws_bytes=None, mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0), dev=FAKE, host=True, ws=FAKE, dst=FAKE,
           mean_ptr=True, std_ptr=True, gather_only=False):
    """(code of y4_rcrop_coeffs_i32, code of y4_rcrop_u8_f32) for one table.  gather_only: the refusal concerns an argument
    y4_rcrop_coeffs_i32 does not have, so that entry point, which would find nothing wrong and launch, is not called."""
    L = yolov4_amd.lib()
    arr = (RcropJob * len(jobs))(*jobs)
    n = len(jobs)
    need = int(L.y4_rcrop_workspace(arr, n, S))
    ws_bytes = need if ws_bytes is None else ws_bytes
    hp = ctypes.addressof(arr) if host else None
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    a = None if gather_only else L.y4_rcrop_coeffs_i32(dev, hp, n, S, ws, ws_bytes, None)
    b = L.y4_rcrop_u8_f32(dev, hp, n, S, m if mean_ptr else None, s if std_ptr else None, dst, 3 * S * S, S * S, S, 1, ws,
                          ws_bytes, None)
    return a, b


def test_workspace_query():
    L = yolov4_amd.lib()
    S = 16
    jobs = [_job(), _job(crop_w=1, crop_h=1, crop_x=0, crop_y=0), _job(crop_x=0, crop_w=40, res_w=3, win_x=0, res_h=16, win_y=0)]
    arr = (RcropJob * 3)(*jobs)
    sizes = []
    for j in jobs:
        s = dict(crop=(j.crop_x, j.crop_y, j.crop_w, j.crop_h), res=(j.res_w, j.res_h))
        sizes.append(R.job_bytes(s, S))
        p = D.CropParams(j.crop_x, j.crop_y, j.crop_w, j.crop_h, j.res_w, j.res_h)
        assert D.job_bytes(p, S) == sizes[-1]
    assert sizes[0] == 4 * (16 * (2 + 5) + 16 * (2 + 5)) and sizes[2] == (4 * (16 * (2 + 29) + 16 * (2 + 5)) + 15) // 16 * 16
    assert L.y4_rcrop_workspace(arr, 3, S) == sum(sizes) and L.y4_rcrop_workspace(arr, 1, S) == sizes[0]
    assert all(v % 16 == 0 for v in sizes)
    assert L.y4_rcrop_workspace(None, 3, S) == 0 and L.y4_rcrop_workspace(arr, 0, S) == 0
    assert L.y4_rcrop_workspace(arr, 3, 0) == 0 and L.y4_rcrop_workspace(arr, 3, 65536) == 0
    bad = (RcropJob * 1)(_job(res_w=0))
    assert L.y4_rcrop_workspace(bad, 1, S) == 0


def test_every_host_side_error_is_reported_before_a_launch():
    S = 16
    # the job itself is acceptable up to the launch: every refusal below is due to the one field changed
    shape = [dict(src_h=0), dict(src_w=0), dict(src_h=65536, crop_y=0), dict(src_w=65536, src_pitch=3 * 65536),
             dict(src_pitch=3 * 40 - 1),
             dict(crop_w=0), dict(crop_h=0), dict(crop_w=-3), dict(crop_x=-1), dict(crop_y=-1), dict(crop_x=11), dict(crop_y=10),
             dict(crop_w=39), dict(crop_h=33),
             dict(res_w=0), dict(res_h=0), dict(res_w=-5), dict(res_h=65536), dict(res_w=65536),
             dict(win_x=-1), dict(win_y=-1), dict(win_x=5), dict(win_y=3), dict(res_w=15, win_x=0), dict(res_h=15, win_y=0),
             dict(paste_from=-2), dict(paste_from=7),
             dict(paste_from=0, paste_x0=-1, paste_x1=3), dict(paste_from=0, paste_x1=17), dict(paste_from=0, paste_y1=17),
             dict(paste_from=0, paste_x0=5, paste_x1=4), dict(paste_from=0, paste_y0=9, paste_y1=8), dict(paste_from=0, paste_y0=-1),
             dict(ws_offset=-16), dict(ws_offset=8)]
    for over in shape:
        assert _calls([_job(**over)], S, ws_bytes=1 << 30) == (ERR_SHAPE, ERR_SHAPE), over
        assert _calls([_job(), _job(**over)], S, ws_bytes=1 << 30) == (ERR_SHAPE, ERR_SHAPE), over    # ... in any record
    assert _calls([_job(paste_from=1)], S, ws_bytes=1 << 30) == (ERR_SHAPE, ERR_SHAPE)      # n itself is outside [-1, n)
    # the limits themselves are accepted as far as the table goes (the next refusal is the workspace's)
    for over in [dict(crop_x=10), dict(crop_y=9), dict(win_x=4), dict(win_y=2), dict(paste_from=0, paste_x1=16, paste_y1=16),
                 dict(paste_from=0, paste_x0=16, paste_x1=16), dict(paste_from=-1, paste_x0=-9, paste_x1=99)]:
        assert _calls([_job(**over)], S, ws_bytes=0) == (ERR_WORKSPACE, ERR_WORKSPACE), over
    for S_bad in (0, -1, 65536):
        L = yolov4_amd.lib()
        arr = (RcropJob * 1)(_job())
        assert L.y4_rcrop_coeffs_i32(FAKE, arr, 1, S_bad, FAKE, 1 << 30, None) == ERR_SHAPE
        assert L.y4_rcrop_u8_f32(FAKE, arr, 1, S_bad, (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(1, 1, 1), FAKE, 1, 1,
                                 1, 1, FAKE, 1 << 30, None) == ERR_SHAPE
        assert L.y4_rcrop_coeffs_i32(FAKE, arr, 0, 16, FAKE, 1 << 30, None) == ERR_SHAPE
        assert L.y4_rcrop_coeffs_i32(FAKE, arr, 65536, 16, FAKE, 1 << 30, None) == ERR_SHAPE
    # NULL pointers
    assert _calls([_job()], S, dev=None) == (ERR_NULL, ERR_NULL)
    assert _calls([_job()], S, host=False) == (ERR_NULL, ERR_NULL)
    assert _calls([_job()], S, ws=None) == (ERR_NULL, ERR_NULL)
    assert _calls([_job(src=None)], S) == (ERR_NULL, ERR_NULL)
    assert _calls([_job()], S, dst=None, gather_only=True)[1] == ERR_NULL
    assert _calls([_job()], S, mean_ptr=False, gather_only=True)[1] == ERR_NULL
    assert _calls([_job()], S, std_ptr=False, gather_only=True)[1] == ERR_NULL
    # std: zero (either sign) or not finite; mean: not finite
    for std in [(0.0, 1.0, 1.0), (1.0, -0.0, 1.0), (1.0, 1.0, float('nan')), (float('inf'), 1.0, 1.0)]:
        assert _calls([_job()], S, std=std, gather_only=True)[1] == ERR_SHAPE, std
    assert _calls([_job()], S, mean=(0.0, float('nan'), 0.0), gather_only=True)[1] == ERR_SHAPE
    # the workspace: one byte short, and a job whose offset pushes it past the end
    L = yolov4_amd.lib()
    need = int(L.y4_rcrop_workspace((RcropJob * 1)(_job()), 1, S))
    assert need == R.job_bytes(dict(crop=(2, 1, 30, 24), res=(20, 18)), S)
    assert _calls([_job()], S, ws_bytes=need - 1) == (ERR_WORKSPACE, ERR_WORKSPACE)
    assert _calls([_job(), _job(ws_offset=need)], S, ws_bytes=2 * need - 1) == (ERR_WORKSPACE, ERR_WORKSPACE)
    assert _calls([_job(ws_offset=16)], S, ws_bytes=need) == (ERR_WORKSPACE, ERR_WORKSPACE)


# ------------------------------------------------------------------------------------------------ the loss

def test_mixed_loss_on_a_plain_target_is_the_criterion():
    calls = []

    def criterion(output, target):
        calls.append(target)
        return (output * target.float().unsqueeze(1)).sum()

    out = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    t = torch.tensor([1, 2])
    got = mixed_loss(criterion, out, t)
    assert len(calls) == 1 and calls[0] is t and torch.equal(got, criterion(out, t))
    a, b = torch.tensor([1, 2]), torch.tensor([2, 0])
    got = mixed_loss(criterion, out, MixedTarget(a, b, 0.25))
    assert torch.equal(got, criterion(out, a) * 0.25 + criterion(out, b) * 0.75)
    got = mixed_loss(torch.nn.CrossEntropyLoss(label_smoothing=0.1), out, MixedTarget(a, a, 0.3))
    assert abs(float(got) - float(torch.nn.CrossEntropyLoss(label_smoothing=0.1)(out, a))) < 1e-6
    assert not isinstance((a, b, 0.5), MixedTarget)


def test_train_step_takes_a_mixed_target():
    """train_step on the CPU with a torch model and criterion: a tensor target gives what it gave before, bit for bit"""
    from yolov4_amd.darknet.train import train_step
    torch.manual_seed(0)
    x = torch.randn(4, 5)
    a, b = torch.tensor([0, 1, 2, 1]), torch.tensor([2, 2, 0, 1])

    def run(target):
        torch.manual_seed(1)
        model = torch.nn.Linear(5, 3)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        crit = torch.nn.CrossEntropyLoss()
        out, loss = train_step(model, crit, opt, x, target)
        return out.detach(), loss.detach(), model.weight.detach().clone()

    o1, l1, w1 = run(a)
    torch.manual_seed(1)
    model = torch.nn.Linear(5, 3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    out = model(x)
    loss = torch.nn.CrossEntropyLoss()(out, a)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert torch.equal(o1, out.detach()) and torch.equal(l1, loss.detach()) and torch.equal(w1, model.weight.detach())
    o2, l2, w2 = run(MixedTarget(a, b, 0.4))
    assert torch.equal(o2, o1) and not torch.equal(w2, w1)
    want = 0.4 * torch.nn.CrossEntropyLoss()(o1, a) + 0.6 * torch.nn.CrossEntropyLoss()(o1, b)
    assert abs(float(l2) - float(want)) < 1e-6


def test_resample_kernels_use_no_scratch():
    """compile-only: the compiler's resource remarks for csrc/resample.hip"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(root, 'yolov4_amd', 'csrc', 'resample.hip'), ('-ffp-contract=off',))
    assert sorted(r['name'].split('(')[0] for r in rows) == ['rcrop_coeffs_kernel', 'rcrop_gather_kernel']
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0 for r in rows), rows
