# -*- coding: utf-8 -*-
"""postprocess_nms (DIoU- / Soft- / class-agnostic NMS, per-image cap) against tests/nms_cases.py's restatement: bit for
bit for hard NMS and the linear decay, rows and order exact and the decayed confidence inside the derived bound for the
Gaussian decay.  Segment sizes around the 256-candidate chunk, one segment above the 2048-candidate LDS bound, tile
heights 63 / 64 / 65.  tests/test_nms_cases.py shows without a GPU what each input contains.

The option checks at the end need no GPU: they run wherever the library loads."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import head_cases as HC
import nms_cases as NC

gpu = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def _post_case(kind):
    return HC.make_post_case(kind)


def _freeze(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _ref(case, kw, f64=False):
    """the restatement's result for a case (computed once): (rows per image, info, xyxy)"""
    p, C, conf, thre = _case(case)
    q = p.copy()
    out, info = NC.postprocess_nms_ref(q, C, conf, thre, f64=f64, **dict(kw))
    return out, info, q[:, :, :4].copy()


def _case(case):
    kind, arg = case
    if kind == 'post':
        return _post_case(arg)[:4]
    if kind == 'seg':
        return NC.make_seg_case(*arg)
    if kind == 'gauss':
        return NC.make_gauss_case(arg[0], **dict(arg[1]))[:4]
    if kind == 'wide':
        return NC.make_wide_case(arg)
    if kind == 'gtile':
        return NC.make_gauss_tile_case(arg[0], **dict(arg[1]))[:4]
    return dict(diou=NC.make_diou_case, soft=NC.make_soft_case, agnostic=NC.make_agnostic_case,
                maxdet=NC.make_maxdet_case)[kind]()


def _run(dev, case, kw):
    from yolov4_amd.yolo.util.utils import postprocess_nms
    p, C, conf, thre = _case(case)
    pd = _up(p, dev)
    got = postprocess_nms(pd, C, conf, thre, **dict(kw))
    return [None if g is None else g.cpu().numpy() for g in got], pd.cpu().numpy(), p


def _assert_exact(dev, case, kw):
    got, after, p = _run(dev, case, kw)
    ref, _, xyxy = _ref(case, kw)
    assert np.array_equal(after[:, :, :4].view(np.int32), xyxy.view(np.int32))
    assert np.array_equal(after[:, :, 4:], p[:, :, 4:])
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (case, kw, b)
        if r is not None:
            assert g.dtype == np.float32 and g.shape == r.shape, (case, kw, b, g.shape, r.shape)
            assert np.array_equal(g.view(np.int32), r.view(np.int32)), (case, kw, b)


def _assert_gaussian(dev, case, kw):
    got, after, _ = _run(dev, case, kw)
    ref, info, xyxy = _ref(case, kw, True)
    assert np.array_equal(after[:, :, :4].view(np.int32), xyxy.view(np.int32))
    agn = dict(kw).get('agnostic', False)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (case, kw, b)
        if r is None:
            continue
        assert g.shape == r.shape, (case, kw, b, g.shape, r.shape)
        cols = [0, 1, 2, 3, 4, 6]
        assert np.array_equal(g[:, cols], r[:, cols].astype(F32)), (case, kw, b)
        tol = np.array([NC.gauss_tol(info['segments'][(b, -1 if agn else int(c))]['emitted']) for c in r[:, 6]])
        err = np.abs(g[:, 5].astype(np.float64) - r[:, 5]) / r[:, 5]
        print('gaussian', case, b, 'worst error / tol', float((err / tol).max()))
        assert (err <= tol).all(), (case, kw, b, float((err / tol).max()))


# ------------------------------------------------------------------------------------------ default options
@gpu
@pytest.mark.parametrize('kind', HC.POST_KINDS)
def test_default_options_are_postprocess(dev, kind):
    from yolov4_amd.yolo.util.utils import postprocess, postprocess_nms
    p, C, conf, thre, props = _post_case(kind)
    a, b = _up(p, dev), _up(p, dev)
    ga, gb = postprocess(a, C, conf, thre), postprocess_nms(b, C, conf, thre)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(b[:, :, :4].cpu().numpy().view(np.int32), props['xyxy'].view(np.int32))
    for x, y, r in zip(ga, gb, props['ref']):
        assert (x is None) == (y is None) == (r is None)
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and np.array_equal(y.cpu().numpy(), r)


@gpu
def test_postprocess_reaches_its_entries_through_lib_once_each(dev, monkeypatch):
    """postprocess() runs on the driver it shares with postprocess_nms() / postprocess_wbf() and still looks its count and
    NMS entries up on lib() when called (bench.py brackets them there): each is called once on 'four', the smallest of
    HC.POST_KINDS, and wrapping changes neither the result nor the in-place xyxy.  An empty batch: the count entry refuses
    it (Y4Error); postprocess_nms() gives []."""
    from yolov4_amd import lib, ops
    from yolov4_amd.yolo.util.utils import postprocess, postprocess_nms
    p, C, conf, thre, props = _post_case('four')
    assert any(r is not None for r in props['ref'])
    plain_in = _up(p, dev)
    plain = postprocess(plain_in, C, conf, thre)
    L = lib()
    calls = {'y4_post_count_f32': 0, 'y4_post_nms_f32': 0}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper
    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    wrapped_in = _up(p, dev)
    wrapped = postprocess(wrapped_in, C, conf, thre)
    assert calls == {'y4_post_count_f32': 1, 'y4_post_nms_f32': 1}, calls
    assert torch.equal(wrapped_in.view(torch.int32), plain_in.view(torch.int32))
    assert np.array_equal(wrapped_in[:, :, :4].cpu().numpy().view(np.int32), props['xyxy'].view(np.int32))
    assert len(wrapped) == len(plain) == len(props['ref'])
    for x, y in zip(wrapped, plain):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    empty = torch.empty((0, 8, 8), device=dev)
    with pytest.raises(ops.Y4Error):
        postprocess(empty, 3)
    assert postprocess_nms(empty, 3) == []


# ------------------------------------------------------------------------------------------ sizes x modes, exact
EXACT_MODES = {'diou': dict(metric='diou'), 'linear': dict(soft='linear'), 'linear-diou': dict(soft='linear', metric='diou'),
               'agnostic': dict(agnostic=True), 'agnostic-linear': dict(agnostic=True, soft='linear'),
               'maxdet': dict(max_det=100), 'linear-maxdet': dict(soft='linear', max_det=40),
               'agnostic-diou-maxdet': dict(agnostic=True, metric='diou', max_det=7)}
SIZED = [('R%d' % R, R) for R in NC.SEG_SIZES] + [(k, k) for k in ('big', 'n63', 'n64', 'n65')]


@gpu
@pytest.mark.parametrize('mode', sorted(EXACT_MODES))
@pytest.mark.parametrize('name,what', SIZED, ids=[n for n, _ in SIZED])
def test_sizes_exact(dev, name, what, mode):
    kw = EXACT_MODES[mode]
    if isinstance(what, int):
        case = ('seg', (what, 'image' if kw.get('agnostic') else 'class'))
    else:
        case = ('post', what)
    _assert_exact(dev, case, _freeze(kw))


@gpu
@pytest.mark.parametrize('case,kw', [('diou', dict(metric='diou')), ('diou', dict(metric='diou', soft='linear')),
                                     ('soft', dict(soft='linear')), ('agnostic', dict(agnostic=True)),
                                     ('maxdet', dict(max_det=5)), ('maxdet', dict(max_det=8)), ('maxdet', dict(max_det=9)),
                                     ('maxdet', dict(max_det=1)), ('maxdet', dict(max_det=5, soft='linear'))])
def test_property_cases_exact(dev, case, kw):
    _assert_exact(dev, (case, None), _freeze(kw))


@gpu
@pytest.mark.parametrize('kw', [dict(metric='diou', max_det=50), dict(soft='linear', max_det=30), dict(agnostic=True, max_det=20),
                                dict(agnostic=True, soft='linear', metric='diou', max_det=20)],
                         ids=['diou', 'linear', 'agnostic', 'agnostic-linear-diou'])
@pytest.mark.parametrize('kind', ('wide', 'overflow'))
def test_wide_rows_and_candidate_overflow(dev, kind, kw):
    """rows too wide for the LDS-tiled count / fill (the row-per-thread kernels run, agnostic forms included), and more
    candidates than the first buffer guess (the call repeats after its host read)"""
    _assert_exact(dev, ('wide', kind), _freeze(kw))


# ------------------------------------------------------------------------------------------ Gaussian decay
@gpu
@pytest.mark.parametrize('R', NC.SEG_SIZES + (NC.GAUSS_BIG,))
def test_gaussian_sizes(dev, R):
    _assert_gaussian(dev, ('gauss', (R, ())), _freeze(dict(soft='gaussian', sigma=NC.GAUSS_SIGMA)))


@gpu
@pytest.mark.parametrize('extra', [{}, {'max_det': 10}, {'agnostic': True}], ids=['plain', 'maxdet', 'agnostic'])
@pytest.mark.parametrize('kind', ('n63', 'n64', 'n65'))
def test_gaussian_tile_heights(dev, kind, extra):
    _assert_gaussian(dev, ('gtile', (kind, _freeze(extra))), _freeze(dict(soft='gaussian', sigma=NC.GAUSS_SIGMA, **extra)))


# ------------------------------------------------------------------------------------------ empty inputs
@gpu
@pytest.mark.parametrize('kw', [dict(metric='diou'), dict(soft='linear'), dict(soft='gaussian'), dict(agnostic=True),
                                dict(max_det=3), dict(agnostic=True, soft='linear', max_det=3)])
def test_empty_inputs(dev, kw):
    from yolov4_amd.yolo.util.utils import postprocess_nms
    p, C, conf, thre, props = _post_case('last')            # image 1 has no candidates
    assert props['images_with_candidates'] == [True, False, True]
    got = postprocess_nms(_up(p, dev), C, conf, thre, **kw)
    assert got[0] is not None and got[1] is None and got[2] is not None
    assert postprocess_nms(_up(p, dev), C, 2.0, thre, **kw) == [None, None, None]
    assert postprocess_nms(torch.zeros((2, 0, 5 + C), device=dev), C, conf, thre, **kw) == [None, None]


# ------------------------------------------------------------------------------------------ validate()
@gpu
def test_validate_takes_nms_options(dev):
    from yolov4_amd.yolo.engine.build import validate
    from yolov4_amd.yolo.util.utils import NMSOptions, detections_to_coco
    p, C, conf, thre, props = _post_case('n65')             # 3 images: batches of 2 and 1
    pred = torch.from_numpy(p)

    class Stub(torch.nn.Module):
        at = 0

        def forward(self, x):
            out = pred[self.at:self.at + x.shape[0]].clone().to(x.device)
            self.at += x.shape[0]
            return out

    info = torch.tensor([[480., 640., 96., 96., 17., 0.], [333., 500., 96., 96., 42., 0.], [96., 96., 96., 96., 7., 0.]])
    loader = [(torch.zeros(2, 3, 8, 8), {'img_info': info[:2]}), (torch.zeros(1, 3, 8, 8), {'img_info': info[2:]})]

    def records(rows):
        out = []
        for r, i in zip(rows, info):
            out.extend(detections_to_coco(None if r is None else torch.from_numpy(r), [float(v) for v in i[:4]], int(i[4])))
        return out
    assert validate(loader, Stub(), conf, thre, device=dev, num_classes=C) == (0, 0)
    assert validate.records == records(props['ref']) and len(validate.records) > 0
    kw = dict(metric='diou', soft='linear', agnostic=True, max_det=20)
    want, _ = NC.postprocess_nms_ref(p.copy(), C, conf, thre, **kw)
    for opt in (NMSOptions(**kw), kw):
        validate(loader, Stub(), conf, thre, device=dev, num_classes=C, nms_options=opt)
        assert validate.records == records(want)
    assert records(want) != records(props['ref'])


@gpu
def test_detect_images_takes_nms_options(dev):
    """two planted boxes of different classes with IoU 0.7: both per class, the higher score alone across classes"""
    import recipe
    from yolov4_amd.detect import detect_images
    from yolov4_amd.yolo.util.utils import NMSOptions
    S = 64
    cfg = {'MODEL': recipe.MODEL_CFG, 'TEST': {'IMGSIZE': S, 'CONFTHRE': 0.3, 'NMSTHRE': 0.45}}

    class Planted(torch.nn.Module):
        def forward(self, x):
            p = torch.zeros((x.shape[0], 4, 85), dtype=torch.float32)
            p[:, 0, :5] = torch.tensor([32.0, 32.0, 40.0, 40.0, 0.75])
            p[:, 0, 5 + 3] = 0.5
            p[:, 2, :5] = torch.tensor([32.0, 26.0, 40.0, 28.0, 0.75])
            p[:, 2, 5 + 17] = 0.75
            return p.to(x.device)
    src = [torch.full((40, 48, 3), 90, dtype=torch.uint8, device=dev)]
    kw = dict(draw=False, encode=False)
    assert [r['detections'][:, 6].tolist() for r in detect_images(Planted(), cfg, src, **kw)] == [[3.0, 17.0]]
    for opt in (NMSOptions(agnostic=True), dict(agnostic=True), dict(max_det=1)):
        out = detect_images(Planted(), cfg, src, nms_options=opt, **kw)
        assert [r['detections'][:, 6].tolist() for r in out] == [[17.0]]
    out = detect_images(Planted(), cfg, src, conf_thre=0.1, nms_options=dict(agnostic=True, soft='linear'), **kw)
    det = out[0]['detections']
    assert det[:, 6].tolist() == [17.0, 3.0] and det[1, 5] == np.float32(0.5) * (np.float32(1) - np.float32(28.0) / np.float32(40.0))


# ------------------------------------------------------------------------------------------ options (no GPU needed)
def test_bad_options_raise():
    from yolov4_amd.yolo.util.utils import NMSOptions, postprocess_nms
    t = torch.zeros(1, 4, 7)
    for kw in (dict(metric='giou'), dict(soft='quadratic'), dict(soft='gaussian', sigma=0.0), dict(max_det=-1)):
        with pytest.raises(ValueError):
            postprocess_nms(t, 2, **kw)
        with pytest.raises(ValueError):
            NMSOptions(**kw)
    if not torch.cuda.is_available():
        import yolov4_amd
        with pytest.raises(yolov4_amd.Y4Error):
            postprocess_nms(t, 2, metric='diou')


def test_c_entries_reject_bad_options_before_any_launch():
    import yolov4_amd
    from yolov4_amd._lib import NmsOpts
    L = yolov4_amd.lib()
    fake = 0x1000

    def call(o, B=2, N=10, C=3):
        return L.y4_post_nms_ex_f32(fake, B, N, C, 0.25, 0.45, ctypes.addressof(o), fake, 100, fake, fake, fake, 1 << 40, None)
    for o in (NmsOpts(2, 0, 0.5, 0, 0), NmsOpts(-1, 0, 0.5, 0, 0), NmsOpts(0, 3, 0.5, 0, 0), NmsOpts(0, 2, 0.0, 0, 0),
              NmsOpts(0, 2, -1.0, 0, 0), NmsOpts(0, 2, float('nan'), 0, 0), NmsOpts(0, 0, 0.5, 2, 0), NmsOpts(0, 0, 0.5, 0, -1)):
        assert call(o) == 1
        assert L.y4_post_nms_ex_workspace(100, 6, ctypes.addressof(o)) == 0
    ok = NmsOpts(1, 2, 0.5, 1, 100)
    assert call(ok, N=1 << 30, C=2) == 1                    # agnostic: N * C must stay below 2^31
    assert L.y4_post_count_ex_f32(fake, 2, 1 << 30, 2, 0.25, 1, 1, fake, None) == 1
    assert L.y4_post_count_ex_f32(fake, 2, 10, 2, 0.25, 1, 2, fake, None) == 1
    assert L.y4_post_nms_ex_f32(fake, 2, 10, 3, 0.25, 0.45, None, fake, 100, fake, fake, fake, 1 << 40, None) == 2
    assert L.y4_post_nms_ex_f32(fake, 2, 10, 3, 0.25, 0.45, ctypes.addressof(ok), fake, 100, fake, fake, fake, 16, None) == 4
    # the workspace queries run on the host; Soft-NMS adds its state behind the hard layout
    plain = NmsOpts(0, 0, 0.5, 0, 0)
    hard = L.y4_post_nms_ex_workspace(1000, 160, ctypes.addressof(plain))
    assert hard == L.y4_post_nms_workspace(1000, 160)
    assert L.y4_post_nms_ex_workspace(1000, 160, ctypes.addressof(ok)) >= hard + 1000 * 9
    assert L.y4_post_topk_workspace(1000, 160) >= 1000 * 12 + 160 * 4
    assert L.y4_post_topk_compact_f32(fake, fake, fake, 2, 3, 0, 100, fake, fake, fake, fake, 1 << 40, None) == 1
    assert L.y4_post_topk_compact_f32(fake, fake, fake, 2, 3, 5, 100, fake, fake, fake, fake, 16, None) == 4
    assert L.y4_post_topk_compact_f32(fake, fake, None, 2, 3, 5, 100, fake, fake, fake, fake, 1 << 40, None) == 2


def test_nms_options_from_cfg_and_cli():
    from yolov4_amd import detect
    from yolov4_amd.yolo.util.utils import NMSOptions
    base = {'TEST': {'IMGSIZE': 608, 'CONFTHRE': 0.001, 'NMSTHRE': 0.4}}
    assert NMSOptions.from_cfg(base) == NMSOptions() == NMSOptions('iou', None, 0.5, False, 0)
    assert NMSOptions.from_cfg({}) == NMSOptions()
    full = {'TEST': dict(base['TEST'], NMS_METRIC='DIoU', NMS_SOFT='gaussian', NMS_SIGMA=0.3, NMS_AGNOSTIC=True, MAX_DET=100)}
    o = NMSOptions.from_cfg(full)
    assert o == NMSOptions('diou', 'gaussian', 0.3, True, 100)
    assert o.kwargs() == dict(metric='diou', soft='gaussian', sigma=0.3, agnostic=True, max_det=100)
    assert NMSOptions.from_cfg({'TEST': {'NMS_SOFT': 'none'}}).soft is None
    with pytest.raises(ValueError):
        NMSOptions.from_cfg({'TEST': {'NMS_METRIC': 'ciou'}})
    ap = detect.build_parser()
    need = ['--cfg', 'c.json', '--source', 'x.jpg']
    assert detect.nms_options_from_args(ap.parse_args(need), base) is None
    assert detect.nms_options_from_args(ap.parse_args(need), full) == o
    a = ap.parse_args(need + ['--nms-metric', 'diou', '--soft-nms', 'linear', '--nms-sigma', '0.25', '--agnostic-nms',
                              '--max-det', '50'])
    assert detect.nms_options_from_args(a, base) == NMSOptions('diou', 'linear', 0.25, True, 50)
    a = ap.parse_args(need + ['--soft-nms', 'none', '--max-det', '0'])
    assert detect.nms_options_from_args(a, full) == NMSOptions('diou', None, 0.3, True, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(need + ['--nms-metric', 'giou'])
