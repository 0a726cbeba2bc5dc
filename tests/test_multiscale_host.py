# -*- coding: utf-8 -*-
"""The multi-scale schedule (yolo/data/multiscale.py): a pure function of (seed, epoch, batch // every), no GPU."""
import pytest

from yolov4_amd.yolo.data.multiscale import MultiScale


def _seq(ms, epoch, n=200):
    return [ms.size_at(epoch, b) for b in range(n)]


def test_same_arguments_same_size_other_seed_or_epoch_other_sequence():
    a, b = MultiScale(seed=3), MultiScale(seed=3)
    assert _seq(a, 0) == _seq(b, 0) and _seq(a, 7) == _seq(b, 7)
    assert a.size_at(5, 123) == a.size_at(5, 123)
    assert _seq(a, 0) != _seq(a, 1)
    assert _seq(a, 0) != _seq(MultiScale(seed=4), 0)
    # a resumed run: epoch 2 does not depend on epochs 0 and 1 having been drawn
    fresh = MultiScale(seed=3)
    assert _seq(fresh, 2) == _seq(a, 2)


def test_the_default_is_the_references_rule():
    ms = MultiScale()
    assert ms.sizes == tuple(range(320, 609, 32)) and ms.every == 10
    seen = set()
    for e in range(20):
        seen.update(_seq(ms, e))
    assert seen == {320, 352, 384, 416, 448, 480, 512, 544, 576, 608}


@pytest.mark.parametrize('every', (1, 3, 10))
def test_constant_within_every_batches_and_inside_the_range(every):
    ms = MultiScale((100, 300, 32), every=every, seed=1)
    assert ms.sizes == (128, 160, 192, 224, 256, 288)
    s = _seq(ms, 0, 30 * every)
    for k in range(30):
        assert len(set(s[k * every:(k + 1) * every])) == 1
    assert all(100 <= v <= 300 and v % 32 == 0 for v in s)
    assert len(set(s)) > 1


def test_a_list_of_sizes():
    ms = MultiScale([64, 96], every=1, stride=32)
    assert set(_seq(ms, 0)) == {64, 96}
    with pytest.raises(ValueError):
        MultiScale([64, 100], stride=32)
    with pytest.raises(ValueError):
        MultiScale([])


def test_value_errors():
    with pytest.raises(ValueError):
        MultiScale((330, 340, 32))                             # no multiple of 32 inside
    with pytest.raises(ValueError):
        MultiScale((608, 320, 32))                             # lo > hi
    with pytest.raises(ValueError):
        MultiScale(every=0)
    with pytest.raises(ValueError):
        MultiScale((-64, 0, 32))
    cfg = {'AUGMENTATION': {'RANDOM_RESIZE': True, 'RANDOM_RESIZE_RANGE': [330, 340]}}
    with pytest.raises(ValueError):
        MultiScale.from_cfg(cfg)
    with pytest.raises(ValueError):
        MultiScale.from_cfg({'AUGMENTATION': {'RANDOM_RESIZE': True, 'RANDOM_RESIZE_EVERY': 0}})


def test_from_cfg():
    assert MultiScale.from_cfg({}) is None
    assert MultiScale.from_cfg({'AUGMENTATION': {'IS_MOSAIC': True}}) is None
    assert MultiScale.from_cfg({'AUGMENTATION': {'RANDOM_RESIZE': False}}) is None
    ms = MultiScale.from_cfg({'AUGMENTATION': {'RANDOM_RESIZE': True}}, seed=5)
    assert ms.sizes == tuple(range(320, 609, 32)) and ms.every == 10 and ms.seed == 5
    tiny = {'MODEL': {'STRIDES': [16, 32], 'ANCHOR_MASK': [[3, 4, 5], [0, 1, 2]]},
            'AUGMENTATION': {'RANDOM_RESIZE': True, 'RANDOM_RESIZE_RANGE': [64, 96], 'RANDOM_RESIZE_EVERY': 1}}
    ms = MultiScale.from_cfg(tiny)
    assert ms.sizes == (64, 96) and ms.every == 1
    # the step is the model's largest stride: 16 alone would admit 80
    tiny['MODEL'] = {'STRIDES': [8, 16], 'ANCHOR_MASK': [[3, 4, 5], [0, 1, 2]]}
    assert MultiScale.from_cfg(tiny).sizes == (64, 80, 96)


def test_the_loader_refuses_a_schedule_for_validation():
    from yolov4_amd.yolo.data.cocodataset import COCOBatchLoader

    class Val:
        is_train = False
    with pytest.raises(ValueError):
        COCOBatchLoader(Val(), 2, {}, multiscale=MultiScale())
