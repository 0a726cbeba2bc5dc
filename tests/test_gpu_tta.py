# -*- coding: utf-8 -*-
"""The test-time-augmentation kernels (csrc/tta.hip) and weighted box fusion (csrc/postprocess.hip) against
tests/fusion_cases.py's float32 restatements, bit for bit: rows, order and every float.  tests/test_fusion_cases.py shows
without a GPU what each input contains.

The argument checks at the end need no GPU: they run wherever the library loads."""
import numpy as np
import pytest
import torch

import fusion_cases as FC

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


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------ view
def _view(dev, x, r, flip, stride, channels_last):
    """one y4_tta_view_f32 launch with the host's geometry; channels_last: both tensors NHWC in memory"""
    from yolov4_amd import ops
    from yolov4_amd._lib import check, lib
    B, C, H, W = x.shape
    ch, cw, Hv, Wv, ry, rx = FC.view_geometry(H, W, r, stride)
    xd = _up(x, dev)
    out = torch.full((B, C, Hv, Wv), -7.0, dtype=torch.float32, device=dev)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
        out = out.contiguous(memory_format=torch.channels_last)
    check(lib().y4_tta_view_f32(ops._ptr(xd), B, C, H, W, *xd.stride(), ops._ptr(out), Hv, Wv, *out.stride(), ch, cw,
                                float(ry), float(rx), int(flip), float(FC.FILL), ops._stream()), 'view')
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize('channels_last', (False, True), ids=('nchw', 'nhwc'))
@pytest.mark.parametrize('flip', (False, True), ids=('plain', 'flip'))
@pytest.mark.parametrize('r', FC.VIEW_SCALES)
def test_view_matches_restatement(dev, r, flip, channels_last):
    x = FC.view_input()
    assert _same_bits(_view(dev, x, r, flip, 32, channels_last), FC.view_ref(x, r, flip))


@gpu
@pytest.mark.parametrize('stride', (32, 1), ids=('padded', 'ragged'))
@pytest.mark.parametrize('flip', (False, True), ids=('plain', 'flip'))
@pytest.mark.parametrize('r', (1.0, 0.83))
def test_view_width_off_the_vector_width(dev, r, flip, stride):
    """a 70-wide input (not a multiple of the lane's four pixels); stride 1 leaves the view 70 / 58 wide as well: the last
    lane of a row stores fewer than four pixels and rows start off the 16-byte grid"""
    x = FC.view_input(70)
    assert FC.view_geometry(40, 70, r, stride)[3] % 4 == (0 if stride == 32 else 2)
    assert _same_bits(_view(dev, x, r, flip, stride, False), FC.view_ref(x, r, flip, stride))


@gpu
def test_tta_views_identity_is_the_input_and_others_match(dev):
    from yolov4_amd.yolo.util.tta import TTA_FILL, TTAOptions, tta_views
    assert TTA_FILL == float(FC.FILL)
    x = np.ascontiguousarray(FC.view_input()[:, :, :32, :64])
    xd = _up(x, dev)
    opts = TTAOptions(scales=(1.0, 1.0, 0.67), flips=(False, True, True))
    views = tta_views(xd, opts, 32)
    assert views[0][0] is xd and views[0][1]['inv_sx'] == 1.0 and not views[0][1]['flip']
    for (v, m), (r, f) in zip(views[1:], ((1.0, True), (0.67, True))):
        assert _same_bits(v.cpu().numpy(), FC.view_ref(x, r, f))
        want = FC.merge_meta(32, 64, r, f)
        assert (m['Wv'], m['flip'], F32(m['inv_sx']), F32(m['inv_sy'])) == (want['Wv'], f, want['inv_sx'], want['inv_sy'])


# ------------------------------------------------------------------------------------------ merge
@gpu
@pytest.mark.parametrize('n_ch', FC.MERGE_NCH)
@pytest.mark.parametrize('N', FC.MERGE_N)
def test_merge_matches_restatement(dev, N, n_ch):
    """three views of N, N + 1 and N rows: the identity (its bits stay), a mirrored down-scale at row_off N and an up-scale
    behind it; the rows of each view go to every image's slab"""
    from yolov4_amd.yolo.util.tta import merge_views
    preds = [FC.merge_pred(N, n_ch), FC.merge_pred(N + 1, n_ch), FC.merge_pred(N, n_ch, seed=10)]
    metas = [FC.merge_meta(64, 96, 1.0, False), FC.merge_meta(64, 96, 0.83, True), FC.merge_meta(64, 96, 1.25, False)]
    host = [dict(m, inv_sx=float(m['inv_sx']), inv_sy=float(m['inv_sy'])) for m in metas]
    got = merge_views([_up(p, dev) for p in preds], host).cpu().numpy()
    assert _same_bits(got, FC.merge_ref(preds, metas))
    assert _same_bits(got[:, :N], preds[0])


# ------------------------------------------------------------------------------------------ weighted box fusion
def _assert_wbf(dev, case, kw):
    from yolov4_amd.yolo.util.utils import postprocess_wbf
    p, C, conf, thre = FC.wbf_case(case)
    pd = _up(p, dev)
    got = postprocess_wbf(pd, C, conf, thre, **dict(kw))
    ref, _, xyxy = FC.wbf_reference(case, kw)
    after = pd.cpu().numpy()
    assert np.array_equal(after[:, :, :4].view(np.int32), xyxy.view(np.int32))
    assert np.array_equal(after[:, :, 4:], p[:, :, 4:])
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (case, kw, b)
        if r is not None:
            g = g.cpu().numpy()
            assert g.shape == r.shape, (case, kw, b, g.shape, r.shape)
            assert _same_bits(g, r), (case, kw, b, np.argwhere(g.view(np.int32) != r.view(np.int32))[:5])


def _freeze(kw):
    return tuple(sorted(kw.items()))


@gpu
@pytest.mark.parametrize('views', (1, 3))
@pytest.mark.parametrize('R', FC.WBF_SIZES)
def test_wbf_segment_sizes(dev, R, views):
    _assert_wbf(dev, ('seg', (R, 'class')), _freeze(dict(views=views)))


@gpu
@pytest.mark.parametrize('extra', [dict(views=1), dict(views=3, max_det=20)], ids=('plain', 'views3-maxdet'))
@pytest.mark.parametrize('R', FC.WBF_SIZES)
def test_wbf_agnostic_segment_sizes(dev, R, extra):
    _assert_wbf(dev, ('seg', (R, 'image')), _freeze(dict(agnostic=True, **extra)))


@gpu
@pytest.mark.parametrize('max_det', (1, 7, 100))
def test_wbf_max_det(dev, max_det):
    _assert_wbf(dev, ('seg', (513, 'class')), _freeze(dict(views=3, max_det=max_det)))


WIDE = [('wide', dict(views=3)), ('wide', dict(agnostic=True, max_det=50)), ('overflow', dict(views=3)),
        ('overflow', dict(max_det=50))]


@gpu
@pytest.mark.parametrize('kind,kw', WIDE, ids=['%s-%s' % (k, '-'.join(sorted(kw))) for k, kw in WIDE])
def test_wbf_wide_rows_and_candidate_overflow(dev, kind, kw):
    """C = 252: the row-per-thread count / fill kernels, per class and with image-sized agnostic segments; 'overflow': more
    candidates than the first buffer guess, the call repeats with room after its host read"""
    _assert_wbf(dev, ('wide', kind), _freeze(kw))


@gpu
def test_wbf_empty_inputs(dev):
    from yolov4_amd.yolo.util.utils import postprocess_wbf
    p, C, conf, thre = FC.make_wbf_seg_case(255, 'class')
    assert postprocess_wbf(_up(p, dev), C, 2.0, thre) == [None, None]
    assert postprocess_wbf(torch.zeros((2, 0, 5 + C), device=dev), C, conf, thre) == [None, None]
    host = torch.from_numpy(p.copy())
    got = postprocess_wbf(host, C, conf, thre, views=3)      # a host tensor: result and xyxy side effect on the host
    ref, _, xyxy = FC.wbf_reference(('seg', (255, 'class')), _freeze(dict(views=3)))
    assert not got[0].is_cuda and _same_bits(got[0].numpy(), ref[0]) and _same_bits(host[:, :, :4].numpy(), xyxy)


# ------------------------------------------------------------------------------------------ argument checks (no GPU needed)
def test_c_entries_reject_bad_arguments_before_any_launch():
    import yolov4_amd
    L = yolov4_amd.lib()
    fake = 0x1000
    OK, SHAPE, NULL, WS = 0, 1, 2, 4

    def view(inp=fake, out=fake, B=2, C=3, H=40, W=72, Hv=64, Wv=96, ch=33, cw=59, ry=1.2, rx=1.2, flip=1):
        return L.y4_tta_view_f32(inp, B, C, H, W, C * H * W, H * W, W, 1, out, Hv, Wv, C * Hv * Wv, Hv * Wv, Wv, 1, ch, cw,
                                 ry, rx, flip, 0.447, None)
    assert view(inp=None) == NULL and view(out=None) == NULL
    for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(Hv=0), dict(Wv=0), dict(ch=0), dict(cw=0), dict(ch=65),
                dict(cw=97), dict(flip=2), dict(flip=-1), dict(ry=0.0), dict(rx=float('nan'))):
        assert view(**bad) == SHAPE, bad

    def merge(pred=fake, out=fake, B=2, N=65, n_ch=85, n_total=200, row_off=100, flip=1):
        return L.y4_tta_merge_f32(pred, B, N, n_ch, out, n_total, row_off, 96.0, flip, 1.2, 1.2, None)
    assert merge(pred=None) == NULL and merge(out=None) == NULL
    for bad in (dict(row_off=136), dict(n_ch=4), dict(N=0), dict(B=0), dict(flip=2), dict(row_off=-1),
                dict(N=1 << 26, n_total=1 << 27, row_off=0)):
        assert merge(**bad) == SHAPE, bad

    def wbf(pred=fake, B=2, N=10, C=3, thre=0.55, agn=0, views=3, seg=fake, total=100, rows=fake, kept=fake, ws=fake,
            nbytes=1 << 40):
        return L.y4_post_wbf_f32(pred, B, N, C, 0.25, thre, agn, views, seg, total, rows, kept, ws, nbytes, None)
    for bad in (dict(views=0), dict(views=-1), dict(agn=2), dict(agn=-1), dict(thre=-0.1), dict(thre=float('nan')),
                dict(B=0), dict(N=0), dict(C=0), dict(total=-1), dict(agn=1, N=1 << 30, C=2)):
        assert wbf(**bad) == SHAPE, bad
    for name in ('pred', 'seg', 'rows', 'kept', 'ws'):
        assert wbf(**{name: None}) == NULL, name
    assert wbf(nbytes=16) == WS
    # the workspace query runs on the host: keys, gathered candidates (24 B) and cluster state (44 B) per candidate
    assert L.y4_post_wbf_workspace(1000, 160) >= 1000 * (8 + 24 + 44) + 160 * 4


def test_bad_options_raise():
    from yolov4_amd.yolo.util.tta import TTAOptions, wbf_kwargs
    from yolov4_amd.yolo.util.utils import NMSOptions, postprocess_wbf
    t = torch.zeros(1, 4, 7)
    for kw in (dict(views=0), dict(max_det=-1), dict(iou_thre=-1.0), dict(iou_thre=float('nan'))):
        with pytest.raises(ValueError):
            postprocess_wbf(t, 2, 0.25, **kw)
    if not torch.cuda.is_available():
        import yolov4_amd
        with pytest.raises(yolov4_amd.Y4Error):
            postprocess_wbf(t, 2, 0.25)
    for kw in (dict(scales=(1.0, 0.5), flips=(False,)), dict(scales=(), flips=()), dict(scales=(0.2,), flips=(False,)),
               dict(scales=(2.5,), flips=(True,)), dict(merge='soft'), dict(wbf_thre=-1.0)):
        with pytest.raises(ValueError):
            TTAOptions(**kw)
    assert wbf_kwargs(None) == {} and wbf_kwargs(NMSOptions(agnostic=True, max_det=9)) == dict(agnostic=True, max_det=9)
    assert wbf_kwargs(dict(max_det=3)) == dict(max_det=3) and wbf_kwargs(NMSOptions().kwargs()) == dict(agnostic=False, max_det=0)
    for bad in (dict(metric='diou'), NMSOptions(soft='linear'), dict(sigma=0.3), dict(max_det=-1)):
        with pytest.raises(ValueError):
            wbf_kwargs(bad)


def test_tta_options_from_cfg_and_cli():
    from yolov4_amd import detect
    from yolov4_amd.yolo.util.tta import TTAOptions
    base = {'TEST': {'IMGSIZE': 608, 'CONFTHRE': 0.001, 'NMSTHRE': 0.4}}
    assert TTAOptions.from_cfg(base) is None and TTAOptions.from_cfg({}) is None and TTAOptions.from_cfg(None) is None
    assert TTAOptions() == TTAOptions((1.0, 0.83, 0.67), (False, True, False), 'nms', 0.55)
    full = {'TEST': dict(base['TEST'], TTA={'SCALES': [1, 0.75], 'FLIPS': [0, 1], 'MERGE': 'WBF', 'WBF_THRE': 0.6})}
    o = TTAOptions.from_cfg(full)
    assert o == TTAOptions((1.0, 0.75), (False, True), 'wbf', 0.6)
    assert TTAOptions.from_cfg({'TEST': {'TTA': {'MERGE': 'wbf'}}}) == TTAOptions(merge='wbf')
    with pytest.raises(ValueError):
        TTAOptions.from_cfg({'TEST': {'TTA': {'SCALES': [1, 0.5]}}})
    ap = detect.build_parser()
    need = ['--cfg', 'c.json', '--source', 'x.jpg']
    assert detect.tta_from_args(ap.parse_args(need), base) is None
    assert detect.tta_from_args(ap.parse_args(need), full) == o
    assert detect.tta_from_args(ap.parse_args(need + ['--tta']), base) == TTAOptions()
    a = ap.parse_args(need + ['--tta', '--tta-scales', '1,0.5', '--tta-flips', '0,1', '--tta-merge', 'wbf'])
    assert detect.tta_from_args(a, base) == TTAOptions((1.0, 0.5), (False, True), 'wbf', 0.55)
    assert detect.tta_from_args(ap.parse_args(need + ['--tta-merge', 'nms']), full) == TTAOptions((1.0, 0.75), (False, True), 'nms', 0.6)
    assert detect.tta_from_args(ap.parse_args(need + ['--tta-scales', '1,0.9,0.8,0.7']), base).flips == (False,) * 4
    with pytest.raises(SystemExit):
        ap.parse_args(need + ['--tta-merge', 'soft'])
