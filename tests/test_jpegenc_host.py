# -*- coding: utf-8 -*-
"""The JPEG encoder's host stage (y4_jpeg_encode_setup / _bound / _host; csrc/jpeg_enc_host.h) without a GPU: files taken apart
by the decoder's host stage come back byte for byte, the restatement's coefficients give Pillow's bytes, out_cap with canaries
behind the buffer, error codes, and the same header in a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpegenc_cases as E
import yolov4_amd
from yolov4_amd._lib import JpegInfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_FORMAT = 0, 1, 2, 4, 6
CANARY = 0xA5
GUARD = 64
# baseline, standard Huffman tables, no restart markers, no EXIF, 8-bit quantisation tables
ROUND_TRIP = [n for n in J.SUPPORTED if n.split('_')[0] in ('gray', 'narrow', 'wide', 'q30', 'q95', 'q100') or n[0] == 's']


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpegenc')


def take_apart(data):
    L = yolov4_amd.lib()
    info = JpegInfo()
    assert L.y4_jpeg_parse_host(data, len(data), ctypes.byref(info)) == OK
    coef = np.zeros(int(info.coef_count), dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    assert L.y4_jpeg_entropy_host(data, len(data), ctypes.byref(info), coef.ctypes.data, coef.size, qt.ctypes.data) == OK
    return info, coef, qt


def encode(coef, info, qt, cap=None):
    """-> (code, bytes); asserts that nothing behind the cap was written"""
    L = yolov4_amd.lib()
    cap = int(L.y4_jpeg_encode_bound(ctypes.byref(info))) if cap is None else cap
    out = np.full(cap + GUARD, CANARY, dtype=np.uint8)
    n = ctypes.c_size_t(77)
    rc = L.y4_jpeg_encode_host(coef.ctypes.data, ctypes.byref(info), qt.ctypes.data, out.ctypes.data, cap, ctypes.byref(n))
    assert (out[cap:] == CANARY).all(), 'a write past out_cap'
    assert n.value <= cap and (rc == OK or n.value == 0)
    return rc, out[:n.value].tobytes()


def poison_dummies(coef, info):
    """the blocks the encoder must not read, overwritten"""
    coef = coef.copy()
    hv = [(info.hs[c], info.vs[c]) for c in range(info.ncomp)]
    _, _, grids, real = E.geometry(info.width, info.height, info.ncomp, hv[0][0], hv[0][1])
    at = 0
    for (bw, bh), (rw, rh) in zip(grids, real):
        blocks = coef[at:at + 64 * bw * bh].reshape(bh, bw, 64)
        blocks[rh:] = 0x5A5A
        blocks[:, rw:] = 0x5A5A
        at += 64 * bw * bh
    return coef


@pytest.mark.parametrize('name', ROUND_TRIP)
def test_decoder_fixtures_come_back_byte_for_byte(name):
    data = J.read(name)
    info, coef, qt = take_apart(data)
    rc, out = encode(poison_dummies(coef, info), info, qt)
    assert rc == OK and out == data


@pytest.mark.parametrize('name', E.NAMES)
def test_goldens_come_back_byte_for_byte(npz, name):
    data = npz[name + '__jpg'].tobytes()
    info, coef, qt = take_apart(data)
    L = yolov4_amd.lib()
    assert L.y4_jpeg_encode_bound(ctypes.byref(info)) >= len(data)
    rc, out = encode(poison_dummies(coef, info), info, qt)
    assert rc == OK and out == data
    rc, out = encode(coef, info, qt, cap=len(data))                 # the exact size suffices
    assert rc == OK and out == data


@pytest.mark.parametrize('name', E.NAMES)
def test_setup_and_restatement_coefficients_give_pillows_bytes(npz, name):
    """geometry and tables from y4_jpeg_encode_setup, coefficients from the numpy restatement (dummies left zero)"""
    c = E.CASES[name]
    px = npz[name + '__px']
    hs, vs = (1, 1) if c['sampling'] is None else E.SAMPLING[c['sampling']]
    info, qt = JpegInfo(), np.zeros((3, 64), dtype=np.uint16)
    L = yolov4_amd.lib()
    assert L.y4_jpeg_encode_setup(c['width'], c['height'], 1 if px.ndim == 2 else 3, hs, vs, c['quality'], ctypes.byref(info),
                                  qt.ctypes.data) == OK
    parsed, _, parsed_qt = take_apart(npz[name + '__jpg'].tobytes())
    assert bytes(info) == bytes(parsed) and np.array_equal(qt, parsed_qt)
    coef, _, want_qt = E.coefficients(px, c['sampling'], c['quality'], fill_dummies=False)
    assert np.array_equal(qt, want_qt)
    rc, out = encode(coef, info, qt)
    assert rc == OK and out == npz[name + '__jpg'].tobytes()


@pytest.mark.parametrize('name', ['e9x5_420', 'egray_9x5'])
def test_every_cap_below_the_size_is_a_workspace_error(npz, name):
    data = npz[name + '__jpg'].tobytes()
    info, coef, qt = take_apart(data)
    for cap in range(len(data)):
        rc, out = encode(coef, info, qt, cap=cap)
        assert rc == ERR_WORKSPACE and out == b'', cap
    assert encode(coef, info, qt, cap=len(data)) == (OK, data)


def test_null_shape_and_range_errors(npz):
    L = yolov4_amd.lib()
    data = npz['e17x33_420__jpg'].tobytes()
    info, coef, qt = take_apart(data)
    out = np.zeros(4096, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    args = [coef.ctypes.data, ctypes.byref(info), qt.ctypes.data, out.ctypes.data, out.size, ctypes.byref(n)]
    for k in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[k] = None
        assert L.y4_jpeg_encode_host(*bad) == ERR_NULL
    assert L.y4_jpeg_encode_bound(None) == 0
    wrong = JpegInfo.from_buffer_copy(bytes(info))
    wrong.mcus_x += 1                                               # not the geometry of this width
    assert L.y4_jpeg_encode_bound(ctypes.byref(wrong)) == 0
    assert encode(coef, wrong, qt)[0] == ERR_SHAPE
    for bad_qt in (0, 256):
        q2 = qt.copy()
        q2[0, 5] = bad_qt
        assert encode(coef, info, q2)[0] == ERR_SHAPE
    q2 = qt.copy()
    q2[2, 0] += 1                                                   # the chroma components must share table 1
    assert encode(coef, info, q2)[0] == ERR_SHAPE
    big = coef.copy()
    big[1] = 1024                                                   # an AC value of 11 bits
    assert encode(big, info, qt)[0] == ERR_FORMAT
    big = coef.copy()
    big[0] = 3000                                                   # a DC difference of 12 bits
    assert encode(big, info, qt)[0] == ERR_FORMAT
    f, q = JpegInfo(), np.zeros((3, 64), dtype=np.uint16)
    setup = lambda *a: L.y4_jpeg_encode_setup(*a, ctypes.byref(f), q.ctypes.data)
    assert setup(17, 33, 3, 2, 2, 95) == OK and f.coef_count == info.coef_count
    assert setup(17, 33, 3, 2, 2, 0) == ERR_SHAPE and setup(17, 33, 3, 2, 2, 101) == ERR_SHAPE
    assert setup(17, 33, 3, 1, 2, 75) == ERR_SHAPE and setup(17, 33, 1, 2, 2, 75) == ERR_SHAPE
    assert setup(0, 33, 3, 2, 2, 75) == ERR_SHAPE and setup(17, 65536, 3, 2, 2, 75) == ERR_SHAPE
    assert setup(17, 33, 2, 1, 1, 75) == ERR_SHAPE
    assert L.y4_jpeg_encode_setup(17, 33, 3, 2, 2, 75, None, q.ctypes.data) == ERR_NULL


@pytest.mark.parametrize('quality', [1, 2, 10, 49, 50, 51, 75, 90, 99, 100])
def test_tables_follow_the_formula(quality):
    f, q = JpegInfo(), np.zeros((3, 64), dtype=np.uint16)
    assert yolov4_amd.lib().y4_jpeg_encode_setup(8, 8, 3, 1, 1, quality, ctypes.byref(f), q.ctypes.data) == OK
    want = E.quality_tables(quality)
    assert np.array_equal(q[0], want[0]) and np.array_equal(q[1], want[1]) and np.array_equal(q[2], want[1])


def _sanitizer_compiler(tmp):
    """a host compiler that can build and link -fsanitize=address,undefined, or None"""
    probe = os.path.join(tmp, 'probe.cpp')
    with open(probe, 'w') as f:
        f.write('int main() { return 0; }\n')
    for cxx in ('c++', 'g++', 'clang++'):
        path = shutil.which(cxx)
        if not path:
            continue
        exe = os.path.join(tmp, 'probe_' + cxx.replace('+', 'p'))
        r = subprocess.run([path, '-fsanitize=address,undefined', probe, '-o', exe], capture_output=True)
        if r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
            return path
    return None


def test_host_stage_under_address_and_ub_sanitizers(npz, tmp_path):
    cxx = _sanitizer_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip('no host compiler with the sanitizer runtime')
    files = tmp_path / 'files'
    files.mkdir()
    for name in ROUND_TRIP:
        shutil.copy(os.path.join(J.JPEG_DIR, name + '.jpg'), str(files / (name + '.jpg')))
    for name in E.NAMES:
        (files / (name + '.jpg')).write_bytes(npz[name + '__jpg'].tobytes())
    exe = str(tmp_path / 'jpegenc_host_main')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(ROOT, 'tests', 'jpegenc_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, str(files)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert '%d files' % (len(ROUND_TRIP) + len(E.NAMES)) in run.stdout and ' 0 failures' in run.stdout
