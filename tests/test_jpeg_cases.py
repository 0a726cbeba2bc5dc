# -*- coding: utf-8 -*-
"""The JPEG fixtures are what tests/jpeg_cases.py says they are, its numpy restatement of the decode reproduces the recorded
libjpeg-turbo pixels bit for bit, and (where Pillow is present) Pillow still decodes the files to those pixels."""
import io
import os

import numpy as np
import pytest

import jpeg_cases as J


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpeg')


def test_every_fixture_is_listed_and_small(npz):
    on_disk = sorted(f[:-4] for f in os.listdir(J.JPEG_DIR) if f.endswith('.jpg'))
    assert on_disk == sorted(J.SUPPORTED + J.UNSUPPORTED)
    for name in on_disk:
        assert os.path.getsize(os.path.join(J.JPEG_DIR, name + '.jpg')) <= 3 * 1024, name
    assert sorted(npz.files) == sorted(J.SUPPORTED + [n + '__raw' for n in J.ORIENT] + ['progressive_17x33'])


@pytest.mark.parametrize('name', J.SUPPORTED)
def test_fixture_meets_its_conditions(name):
    want = J.FIXTURES[name]
    p = J.parse(J.read(name))
    hv = J.geometry(p)[0]
    assert (p['width'], p['height'], p['ncomp']) == (want['width'], want['height'], want['ncomp'])
    assert hv[0] == (want['hs'], want['vs']) and all(x == (1, 1) for x in hv[1:])
    assert p['precision'] == 8 and p['sof'] == want['sof'] and p['scan_ncomp'] == p['ncomp']
    assert (p['restart_interval'] > 0) == want['restart']
    assert p['orientation'] == want['orientation']
    assert p['dqt16'] == want['dqt16']
    if want['dqt16']:
        assert max(max(t) for t in p['qt'].values()) > 255
    if want.get('optimized'):
        std = J.parse(J.read('s48x40_420'))['huff']
        assert p['huff'] != std, 'optimised tables differ from the standard ones'


def test_edge_conditions_of_the_pixel_stage():
    def dims(name):
        c = J.FIXTURES[name]
        return c, -(-c['width'] // c['hs']), -(-c['height'] // c['vs'])
    for name in J.NARROW_CHROMA:
        c, dw, _ = dims(name)
        assert c['hs'] == 2 and dw <= 2, name
    assert {dims(n)[1] for n in J.NARROW_CHROMA} == {1, 2}
    for name in J.WIDE_CHROMA_ODD:
        c, dw, _ = dims(name)
        assert c['hs'] == 2 and dw > 2 and (c['width'] % 2 or c['height'] % 2), name
    for name in J.ODD:
        c = J.FIXTURES[name]
        assert c['width'] % 8 and c['height'] % 8 and c['width'] % 2 and c['height'] % 2, name
    rst = [n for n in J.SUPPORTED if J.FIXTURES[n]['restart']]
    assert {(J.FIXTURES[n]['ncomp'], J.FIXTURES[n]['hs']) for n in rst} == {(3, 2), (3, 1), (1, 1)}
    for n in rst:                                       # more than one interval
        p = J.parse(J.read(n))
        _, mx, my, _ = J.geometry(p)
        assert mx * my > p['restart_interval'] and J.read(n).count(b'\xff\xd0') >= 1
    assert sorted(J.FIXTURES[n]['orientation'] for n in J.ORIENT) == list(range(1, 9))
    for name, marker in (('progressive_17x33', 0xC2),):
        assert J.parse(J.read(name))['sof'] == marker
    assert J.parse(J.read('cmyk_9x5'))['ncomp'] == 4


@pytest.mark.parametrize('name', J.SUPPORTED)
def test_restatement_reproduces_the_recorded_pixels(npz, name):
    got = J.decode(J.read(name))
    assert got.dtype == np.uint8 and got.shape == npz[name].shape
    assert np.array_equal(got, npz[name])
    if name in J.ORIENT:
        assert np.array_equal(J.decode(J.read(name), apply_orientation=False), npz[name + '__raw'])
        if J.FIXTURES[name]['orientation'] >= 5:
            assert got.shape[:2] == (13, 21)


def test_orientation_fixtures_tell_the_eight_maps_apart(npz):
    seen = [npz[n].tobytes() + bytes(npz[n].shape) for n in J.ORIENT]
    assert len(set(seen)) == 8


def test_pillow_still_decodes_the_fixtures_to_the_recorded_pixels(npz):
    Image = pytest.importorskip('PIL.Image')
    ImageOps = pytest.importorskip('PIL.ImageOps')
    features = pytest.importorskip('PIL.features')
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('this Pillow is not built on libjpeg-turbo')
    for name in J.SUPPORTED + ['progressive_17x33']:
        im = Image.open(io.BytesIO(J.read(name)))
        raw = np.asarray(im.convert('RGB'))
        if name in J.ORIENT:
            assert np.array_equal(raw, npz[name + '__raw']), name
            raw = np.asarray(ImageOps.exif_transpose(im).convert('RGB'))
        assert np.array_equal(raw, npz[name]), name
