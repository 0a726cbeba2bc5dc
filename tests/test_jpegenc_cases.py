# -*- coding: utf-8 -*-
"""The numpy restatement of the JPEG compression arithmetic (tests/jpegenc_cases.py) against the coefficients Pillow
(libjpeg-turbo) coded into the goldens: every real block exactly, the dummy blocks by their rule, the tables by their formula."""
import numpy as np
import pytest

import jpeg_cases as J
import jpegenc_cases as E


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpegenc')


def test_the_goldens_are_the_cases_they_claim(npz):
    assert sorted(k[:-5] for k in npz.files if k.endswith('__jpg')) == E.NAMES
    for name in E.NAMES:
        c = E.CASES[name]
        p = J.parse(npz[name + '__jpg'].tobytes())
        px = npz[name + '__px']
        assert (p['width'], p['height']) == (c['width'], c['height']) == (px.shape[1], px.shape[0])
        assert p['sof'] == 0xC0 and p['restart_interval'] == 0 and not p['dqt16'] and p['n_dht'] == (2 if px.ndim == 2 else 4)
        if c['sampling'] is None:
            assert p['ncomp'] == 1 and px.ndim == 2
        else:
            assert p['ncomp'] == 3 and (p['comps'][0][1], p['comps'][0][2]) == E.SAMPLING[c['sampling']]


@pytest.mark.parametrize('name', E.NAMES)
def test_restatement_equals_pillow(npz, name):
    c = E.CASES[name]
    want, want_qt, _ = J.entropy(npz[name + '__jpg'].tobytes())
    coef, real, qt = E.coefficients(npz[name + '__px'], c['sampling'], c['quality'])
    assert np.array_equal(qt, want_qt)
    assert coef.shape == want.shape
    assert np.array_equal(coef[real], want[real]), 'a real block differs'
    assert np.array_equal(coef[~real], want[~real]), 'a dummy block is not (DC of the block before it, AC zero)'


def test_dummy_conditions_are_met(npz):
    for name in E.RIGHT_DUMMY + E.BOTTOM_DUMMY:
        c = E.CASES[name]
        hs, vs = E.SAMPLING[c['sampling']]
        _, _, grids, real = E.geometry(c['width'], c['height'], 3, hs, vs)
        if name in E.RIGHT_DUMMY:
            assert real[0][0] < grids[0][0]
        if name in E.BOTTOM_DUMMY:
            assert real[0][1] < grids[0][1]
    _, real, _ = E.coefficients(npz['e17x33_420__px'], '420', 75)
    assert 0 < (~real).sum() < real.size


def test_saturated_case_stuffs_bytes(npz):
    data = npz['esat_40x24_420__jpg'].tobytes()
    start = J.parse(data)['scan_start']
    assert b'\xff\x00' in data[start:]
    coef, _, _ = E.coefficients(npz['esat_40x24_420__px'], '420', 100)
    assert np.abs(coef.astype(np.int32)).max() >= 900
