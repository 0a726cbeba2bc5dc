# -*- coding: utf-8 -*-
"""CPU-side checks of the training augmentation: every case of tests/augment_cases.py reaches the branch it is listed for,
the fp64 reference satisfies its identities, the measured fp32-emulation error stays within K / 4, the host box arithmetic
and the sampler of yolov4_amd/yolo/data/transform.py give hand-computed values and stay in range, and the C ABI exports the
new entry points."""
import math
import random

import numpy as np
import pytest

import augment_cases as A
import yolov4_amd
from yolov4_amd import _lib
from yolov4_amd.yolo.data import transform as T

F64 = np.float64
CFG = {'AUGMENTATION': {'JITTER': 0.3, 'RANDOM_HORIZONTAL_FLIP': True, 'COLOR_DITHERING': True, 'HUE': 0.1,
                        'SATURATION': 1.5, 'EXPOSURE': 1.5, 'IS_MOSAIC': True, 'MIN_OFFSET': 0.2},
       'DATA': {'MAX_NUM_LABELS': 60}}


@pytest.fixture(scope='module')
def stats():
    out = {}
    for c in A.CASES:
        st = A.new_stats()
        A.render(c, F64, st)
        out[c['name']] = st
    return out


# ---------------------------------------------------------------------------------------------- branch reach

def test_cases_reach_their_branches(stats):
    for name in ('pad_ring', 'pad_ring_flip_noswap', 'mixed_signs', 'tiny_source', 'batch3_mixed', 'colour_hue_up'):
        assert stats[name]['pad_taps'] > 0, name
    for name in ('pure_crop', 'pure_crop_flip', 'exact_2x', 'crop_1x1'):
        assert stats[name]['pad_taps'] == 0 and stats[name]['fractional'] > 0, name
    for c in A.CASES:
        if c['exact']:
            st = stats[c['name']]
            assert st['pad_taps'] == 0 and st['fractional'] == 0 and st['hsv'] == 0, c['name']
            assert not any(s['color'] for sm in c['samples'] for s in sm['srcs'])
    assert stats['colour_identity']['hsv'] == 0                      # colour on, identity parameters: skipped
    assert any(s['color'] for s in A.BY_NAME['colour_identity']['samples'][0]['srcs'])
    assert stats['colour_hue_down']['wrap_below'] > 0 and stats['colour_hue_down']['grey'] > 0
    up = stats['colour_hue_up']
    assert up['wrap_above'] > 0 and up['clip_high'] > 0 and up['clip_low'] > 0 and up['s_over_1'] > 0
    assert up['grey'] > 0 and up['black'] > 0
    assert stats['colour_sat_only']['clip_low'] > 0 and stats['colour_mosaic']['hsv'] > 0


def test_case_list_covers_the_listed_shapes():
    shapes, sizes, layouts, swaps, pitched, flips, nsrc = set(), set(), set(), set(), False, set(), set()
    for c in A.CASES:
        sizes.add(c['S'])
        layouts.add(c['layout'])
        for sm in c['samples']:
            nsrc.add(len(sm['srcs']))
            for s in sm['srcs']:
                shapes.add((s['h'], s['w']))
                swaps.add(s['swap_rb'])
                flips.add(s['flip'])
                pitched |= s['pitch_extra'] > 0
    assert shapes >= {(2, 3), (17, 23), (37, 53), (64, 64)} and sizes == {32, 40, 64}
    assert layouts == {'nchw', 'slot', 'nhwc4'} and swaps == {0, 1} and flips == {0, 1} and nsrc == {1, 4} and pitched
    s = A.BY_NAME['exact_2x']['samples'][0]['srcs'][0]
    assert s['crop_w'] == s['crop_h'] == 2 * A.BY_NAME['exact_2x']['S']
    s = A.BY_NAME['pad_ring']['samples'][0]['srcs'][0]
    assert max(s['crop_left'], s['crop_right'], s['crop_top'], s['crop_bottom']) < 0
    s = A.BY_NAME['pure_crop']['samples'][0]['srcs'][0]
    assert min(s['crop_left'], s['crop_right'], s['crop_top'], s['crop_bottom']) > 0
    b3 = A.BY_NAME['batch3_mixed']['samples']
    assert [len(sm['srcs']) for sm in b3] == [1, 4, 1]
    assert len({(s['h'], s['w']) for sm in b3 for s in sm['srcs']}) >= 4


def test_mosaic_cuts_and_clamps():
    for S in (40, 64):
        lo, hi = int(S * 0.2), int(S * 0.8)
        cuts = {(c['samples'][0]['cut_x'], c['samples'][0]['cut_y']) for c in A.CASES
                if c['name'].startswith('mosaic_%d_' % S)}
        assert (hi, hi) in cuts and (S // 2, S // 2) in cuts
        if S == 40:
            assert {(lo, lo), (lo, hi), (0, S), (S, 0)} <= cuts
    hit = [False] * 4
    for name in ('mosaic_clamp_left_top', 'mosaic_clamp_right_bottom'):
        sm = A.BY_NAME[name]['samples'][0]
        for s in sm['srcs']:
            flags = A.shifts(s, sm['cut_x'], sm['cut_y'], A.BY_NAME[name]['S'])[4]
            hit = [a or b for a, b in zip(hit, flags)]
    assert hit == [True] * 4, hit                                      # left, top, right, bottom clamp each active
    for c in A.CASES:                                                  # every window fits its resized image
        for sm in c['samples']:
            for q, s in enumerate(sm['srcs']):
                _, _, ex, ey = (0, 0, c['S'], c['S']) if len(sm['srcs']) == 1 else A.tile_rect(q, sm['cut_x'], sm['cut_y'], c['S'])
                assert 0 <= s['win_x'] <= c['S'] - ex and 0 <= s['win_y'] <= c['S'] - ey, c['name']


def test_rejects_differ_from_the_valid_case_in_one_field():
    table, samples = A.flat_sources(A.BY_NAME['batch3_mixed'])
    assert len(table) == 6 and [s[2] for s in samples] == [1, 4, 1]
    names = [r[0] for r in A.REJECTS]
    assert len(set(names)) == len(names) and len(names) >= 20
    for _, where, idx, fld, _, code in A.REJECTS + A.REJECTS_MEANS:
        assert where in ('arg', 'src', 'sample') and code in (A.Y4_ERR_SHAPE, A.Y4_ERR_NULL)
        if where == 'src':
            assert idx < len(table) and (fld in table[idx] or fld in ('src', 'pitch'))


# ---------------------------------------------------------------------------------------------- reference identities

def test_emulation_error_is_within_a_quarter_of_the_bound():
    worst = max(A.emulation_error_units(c) for c in A.CASES)
    print('max |fp32 emulation - fp64 reference| = %.2f x 2^-24; K = %d' % (worst, A.K))
    assert worst <= A.K / 4
    assert A.K == 2 ** math.ceil(math.log2(4 * worst)), 'K is 4 x the measured error rounded up to a power of two'
    assert abs(worst - A.MEASURED_UNITS) < 0.1, 'the docstring figure is stale'


def test_exact_cases_are_u8_over_255():
    c = A.BY_NAME['identity_64']
    img = c['samples'][0]['srcs'][0]['img'][:, :, ::-1]
    want = (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]
    assert np.array_equal(A.render(c, np.float32), want)
    c = A.BY_NAME['crop_to_32_flip']
    img = c['samples'][0]['srcs'][0]['img'][2:34, 10:42, ::-1][:, ::-1]
    want = (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]
    assert np.array_equal(A.render(c, np.float32), want)


def test_hsv_identity_parameters_return_the_input():
    rgb = np.random.RandomState(5).uniform(0, 255, size=(4000, 3))
    rgb[:50] = rgb[:50, :1]                                            # grey
    rgb[50:60] = 0
    back = A.hsv_jitter(rgb.astype(F64), 0.0, 1.0, 1.0, F64)
    used = np.abs(back - rgb).max() / 255 / (A.K * A.UNIT)
    print('HSV round trip: share of the bound used %.3f' % used)
    assert used <= 1


def test_double_flip_is_the_identity():
    img = A._img(37, 53, 9)
    plain = A.case('p', 40, [A.sample(40, [A.src(img, -6, 9, 4, -7)])])
    twice = A.case('t', 40, [A.sample(40, [A.src(img[:, ::-1], 9, -6, 4, -7, flip=1)])])
    assert np.array_equal(A.render(plain), A.render(twice))


def test_mosaic_of_copies_with_zero_shifts_is_the_single_image():
    img = A._img(37, 53, 10)
    one = A.src(img, 5, 7, 3, 4, color=1, dhue=0.05, dsat=1.2, dexp=0.9)
    single = A.render(A.case('s', 40, [A.sample(40, [one])]))
    for cut in ((8, 32), (20, 20), (31, 9)):
        four = A.sample(40, [one] * 4, cut)
        assert all(A.shifts(s, cut[0], cut[1], 40)[:4] == (0, 0, 0, 0) for s in four['srcs'])
        assert np.array_equal(A.render(A.case('m', 40, [four])), single)


def test_channel_sums_reference():
    s = A.src(np.full((5, 7, 3), 255, np.uint8))
    assert A.channel_sums(s) == [5 * 7 * 255] * 3
    assert 65535 * 65535 * 255 < 2 ** 40                               # the largest accepted image cannot overflow


# ---------------------------------------------------------------------------------------------- boxes (hand-computed)

SHAPE = (100, 200)
P = T.AugParams(crop_left=10, crop_right=50, crop_top=20, crop_bottom=30)        # crop 140 x 50; S = 70: x * 0.5, y * 1.4
BOXES = np.array([[0, 30, 50, 30, 1],        # cut by the crop on the left: x -10..40 -> 0..40, y 10..40
                  [0, 30, 10, 10, 2],        # x -10..0 -> 0, 0: collapsed onto the left edge
                  [160, 30, 20, 10, 3],      # x 150..170 -> 140, 140: right edge
                  [50, 5, 10, 10, 4],        # y -15..-5 -> 0, 0: top edge
                  [50, 75, 10, 20, 5],       # y 55..75 -> 50, 50: bottom edge
                  [60, 40, 20, 10, 6]], F64)  # inside: x 50..70, y 20..30


def test_transform_boxes_cut_dropped_and_scaled():
    got = T.transform_boxes(BOXES, SHAPE, P, 70)
    assert np.allclose(got, [[0, 14, 20, 56, 1], [25, 28, 35, 42, 6]], rtol=0, atol=1e-12)
    assert BOXES[0, 0] == 0 and BOXES[0, 2] == 50                      # the input is not modified


def test_transform_boxes_flip_and_permutation():
    p = T.AugParams(crop_left=10, crop_right=50, crop_top=20, crop_bottom=30, flip=True, perm=(5, 4, 3, 2, 1, 0))
    got = T.transform_boxes(BOXES, SHAPE, p, 70)
    # mirrored in the 140-wide crop: 0..40 -> 100..140, 50..70 -> 70..90; the stored order comes first
    assert np.allclose(got, [[35, 28, 45, 42, 6], [50, 14, 70, 56, 1]], rtol=0, atol=1e-12)
    assert T.transform_boxes(np.zeros((0, 5)), SHAPE, P, 70).shape == (0, 5)


def test_mosaic_shifts_and_boxes():
    p = T.AugParams(crop_left=-40, crop_right=20, crop_top=-10, crop_bottom=0)   # crop 220 x 110
    assert T.mosaic_shifts(SHAPE, p, 60, 50, 100) == (18, 9, 0, 0)               # int(40 * 100 / 220), int(10 * 100 / 110)
    pf = T.AugParams(crop_left=-40, crop_right=20, crop_top=-10, crop_bottom=0, flip=True)
    assert T.mosaic_shifts(SHAPE, pf, 60, 50, 100) == (0, 9, 18, 0)              # left and right trade places
    assert T.tile_window(1, (0, 9, 18, 0), 60, 50, 100) == (42, 9, 40, 50, 60, 0)
    # the clamps: left <= S - cut_x, right <= cut_x, top <= S - cut_y, bottom <= cut_y
    big = T.AugParams(crop_left=-90, crop_right=-90, crop_top=-45, crop_bottom=-45)  # crop 380 x 190: 23.68 each way
    assert T.mosaic_shifts(SHAPE, big, 80, 80, 100) == (20, 20, 20, 20)          # left, top clamped to 100 - 80
    assert T.mosaic_shifts(SHAPE, big, 15, 15, 100) == (15, 15, 15, 15)          # right, bottom clamped to the cut
    box = np.array([[20, 10, 90, 40, 7], [50, 40, 80, 70, 8]], F64)
    got0 = T.mosaic_boxes(box, 0, SHAPE, p, 60, 50, 100)             # window origin (18, 9), 60 x 50, lands at (0, 0)
    assert np.allclose(got0, [[2, 1, 60, 31, 7], [32, 31, 60, 50, 8]], rtol=0, atol=1e-12)
    got3 = T.mosaic_boxes(box, 3, SHAPE, p, 60, 50, 100)             # origin (60, 50), 40 x 50, lands at (60, 50)
    assert np.allclose(got3, [[60, 50, 80, 70, 8]], rtol=0, atol=1e-12)   # the first box collapses onto the top edge
    assert box[0, 0] == 20


def test_windows_agree_with_the_case_module():
    rng = random.Random(3)
    for _ in range(200):
        S = rng.choice((32, 40, 64))
        shapes = [(rng.randint(2, 70), rng.randint(3, 70)) for _ in range(4)]
        mp = T.sample_train_params(CFG, shapes, S, rng)
        srcs = [A.src(np.zeros((h, w, 3), np.uint8), p.crop_left, p.crop_right, p.crop_top, p.crop_bottom, flip=int(p.flip))
                for (h, w), p in zip(shapes, mp.tiles)]
        sm = A.sample(S, srcs, (mp.cut_x, mp.cut_y))
        for q, (s, shp, p) in enumerate(zip(sm['srcs'], shapes, mp.tiles)):
            win = T.tile_window(q, T.mosaic_shifts(shp, p, mp.cut_x, mp.cut_y, S), mp.cut_x, mp.cut_y, S)
            assert win[:2] == (s['win_x'], s['win_y']) and win[2:] == tuple(np.roll(A.tile_rect(q, mp.cut_x, mp.cut_y, S), 2))


def test_pad_labels_truncates_and_zero_pads():
    b = np.array([[10, 20, 30, 60, 3]], F64)
    out = T.pad_labels(b, 60)
    assert out.shape == (60, 5) and out.dtype == F64
    assert out[0].tolist() == [20, 40, 20, 40, 3] and not out[1:].any()
    many = np.tile(b, (70, 1))
    many[:, 4] = np.arange(70)
    out = T.pad_labels(many, 60)
    assert out.shape == (60, 5) and out[:, 4].tolist() == list(range(60))
    assert not T.pad_labels(np.zeros((0, 5)), 60).any()
    mp = T.MosaicParams(cut_x=60, cut_y=50, tiles=[T.AugParams()] * 4)
    lab = T.sample_labels([np.array([[10, 10, 20, 20, q]], F64) for q in range(4)], [(100, 100)] * 4, mp, 100, 60)
    assert lab[0].tolist() == [20, 20, 20, 20, 0] and lab[:, 4].tolist()[:1] == [0] and not lab[1:].any()


# ---------------------------------------------------------------------------------------------- sampler

def test_sampler_ranges_and_flip_rate():
    rng = random.Random(1234)
    S, (h, w), n = 64, (37, 53), 10000
    jh, jw = int(h * 0.3), int(w * 0.3)
    lo, hi = int(S * 0.2), int(S * 0.8)
    flips, seen_cut, seen_crop = 0, set(), set()
    for i in range(n):
        mp = T.sample_train_params(CFG, [(h, w)], S, rng, num_boxes=[5])
        assert lo <= mp.cut_x <= hi and lo <= mp.cut_y <= hi and len(mp.tiles) == 1
        p = mp.tiles[0]
        assert all(isinstance(v, int) for v in (p.crop_left, p.crop_right, p.crop_top, p.crop_bottom, mp.cut_x, mp.cut_y))
        assert -jw <= p.crop_left <= jw and -jw <= p.crop_right <= jw and -jh <= p.crop_top <= jh and -jh <= p.crop_bottom <= jh
        assert -0.1 <= p.dhue <= 0.1 and 1 / 1.5 <= p.dsat <= 1.5 and 1 / 1.5 <= p.dexp <= 1.5
        assert p.color is True and isinstance(p.flip, bool) and sorted(p.perm) == [0, 1, 2, 3, 4]
        flips += p.flip
        seen_cut.add(mp.cut_x)
        seen_crop.add(p.crop_left)
    assert seen_cut == set(range(lo, hi + 1)) and seen_crop == set(range(-jw, jw + 1))     # both ends are reached
    prob = 0.5 * math.erfc(0.5 / math.sqrt(2))                        # P(N(0,1) > 0.5) = 0.3085
    sigma = math.sqrt(prob * (1 - prob) / n)
    assert abs(flips / n - prob) <= 5 * sigma, (flips / n, prob)
    assert len(T.sample_train_params(CFG, [(h, w)] * 4, S, rng).tiles) == 4
    off = dict(CFG, AUGMENTATION=dict(CFG['AUGMENTATION'], RANDOM_HORIZONTAL_FLIP=False, COLOR_DITHERING=False))
    assert not any(T.sample_train_params(off, [(h, w)], S, rng).tiles[0].flip for _ in range(200))
    assert T.sample_train_params(off, [(h, w)], S, rng).tiles[0].color is False
    T.sample_train_params(CFG, [(h, w)], S)                           # the default generators


def test_sampler_refuses_a_jitter_that_can_empty_the_crop():
    for j in (0.5, 0.7):
        bad = dict(CFG, AUGMENTATION=dict(CFG['AUGMENTATION'], JITTER=j))
        with pytest.raises(ValueError):
            T.sample_train_params(bad, [(37, 53)], 64, random.Random(0))
    with pytest.raises(ValueError):
        T.sample_train_params(CFG, [(37, 53)] * 2, 64, random.Random(0))


# ---------------------------------------------------------------------------------------------- ABI

def test_augment_symbols_are_exported_with_prototypes():
    L = yolov4_amd.lib()
    for name in ('y4_augment_means_u8', 'y4_augment_mosaic_u8_f32'):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    import ctypes
    assert ctypes.sizeof(_lib.AugSrc) == 72 and ctypes.sizeof(_lib.AugSample) == 16
    assert L.y4_augment_means_u8(None, None, 1, None, None) == A.Y4_ERR_NULL


def test_transform_keeps_the_reference_constructor():
    import inspect
    assert list(inspect.signature(T.Transform.__init__).parameters)[1:] == ['cfg', 'is_train']
    assert list(inspect.signature(T.Transform.__call__).parameters)[1:] == ['img_list', 'bboxes_list', 'img_size']
    t = T.Transform(CFG)
    assert t.is_train and t.max_num_labels == 60 and t.jitter_ratio == 0.3 and t.is_mosaic
