# -*- coding: utf-8 -*-
"""The JPEG host stage (y4_jpeg_parse_host, y4_jpeg_entropy_host; csrc/jpeg_host.h) without a GPU: parse records and
coefficients against the numpy restatement in tests/jpeg_cases.py, error codes, truncation and corruption with canaries
behind the coefficient cap, and the same header in a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import yolov4_amd
from yolov4_amd._lib import JpegInfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_NULL, ERR_WORKSPACE, ERR_FORMAT, ERR_UNSUPPORTED = 0, 1, 2, 4, 6, 7
CANARY = 0x5A5A
GUARD = 64


@pytest.fixture(scope='module')
def npz(golden):
    return golden('jpeg')


def parse(data):
    info = JpegInfo()
    return yolov4_amd.lib().y4_jpeg_parse_host(data, len(data), ctypes.byref(info)), info


def entropy(data, info, cap=None):
    """-> (code, coefficients [coef_count], qt [3][64]); asserts that nothing behind the cap was written"""
    cap = int(info.coef_count) if cap is None else cap
    coef = np.full(cap + GUARD, CANARY, dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    rc = yolov4_amd.lib().y4_jpeg_entropy_host(data, len(data), ctypes.byref(info), coef.ctypes.data, cap, qt.ctypes.data)
    assert (coef[cap:] == CANARY).all(), 'a write past coef_cap'
    return rc, coef[:cap], qt


def test_error_codes_and_messages():
    L = yolov4_amd.lib()
    assert L.y4_strerror(ERR_FORMAT) != L.y4_strerror(ERR_UNSUPPORTED)
    assert b'unknown' not in L.y4_strerror(ERR_FORMAT) and b'unknown' not in L.y4_strerror(ERR_UNSUPPORTED)
    assert [L.y4_strerror(c) for c in range(3)] == [b'ok', b'unsupported or inconsistent shape / pitch / alignment',
                                                    b'required pointer is NULL']
    assert ctypes.sizeof(JpegInfo) == 88
    info = JpegInfo()
    assert L.y4_jpeg_parse_host(None, 10, ctypes.byref(info)) == ERR_NULL
    assert L.y4_jpeg_parse_host(b'\xff\xd8\xff\xd9', 4, None) == ERR_NULL


@pytest.mark.parametrize('name', J.SUPPORTED)
def test_parse_fields(name):
    data = J.read(name)
    rc, info = parse(data)
    assert rc == OK
    p = J.parse(data)
    hv, mx, my, grids = J.geometry(p)
    want = J.FIXTURES[name]
    assert (info.width, info.height, info.ncomp) == (want['width'], want['height'], want['ncomp'])
    n = info.ncomp
    assert list(info.hs)[:n] == [h for h, _ in hv] and list(info.vs)[:n] == [v for _, v in hv]
    assert list(info.hs)[n:] == [0] * (3 - n) and list(info.blocks_w)[n:] == [0] * (3 - n)
    assert (info.mcus_x, info.mcus_y) == (mx, my)
    assert list(zip(info.blocks_w, info.blocks_h))[:n] == grids
    assert info.restart_interval == p['restart_interval'] and (info.restart_interval > 0) == want['restart']
    assert info.orientation == want['orientation']
    assert info.coef_count == 64 * sum(w * h for w, h in grids)


@pytest.mark.parametrize('name', J.SUPPORTED)
def test_coefficients_equal_the_restatement(npz, name):
    data = J.read(name)
    rc, info = parse(data)
    assert rc == OK
    rc, coef, qt = entropy(data, info)
    assert rc == OK
    want_coef, want_qt, _ = J.entropy(data)
    assert np.array_equal(coef, want_coef)
    assert np.array_equal(qt, want_qt)
    px = J.pixels_from_coefficients(coef, qt, info.width, info.height, info.ncomp, info.hs[0], info.vs[0], info.orientation)
    assert np.array_equal(px, npz[name])


def test_cap_and_record_are_checked():
    data = J.read('s17x33_420')
    rc, info = parse(data)
    assert entropy(data, info, cap=int(info.coef_count) - 1)[0] == ERR_WORKSPACE
    other = J.read('s9x5_420')
    assert entropy(other, info)[0] == ERR_SHAPE            # the record of another file


@pytest.mark.parametrize('name', J.UNSUPPORTED)
def test_valid_files_outside_the_subset(name):
    assert parse(J.read(name))[0] == ERR_UNSUPPORTED


def _patch_sof(data, offset, value):
    """one byte of the SOF0 payload replaced (offset from the length field's end)"""
    at = data.index(b'\xff\xc0') + 4 + offset
    return data[:at] + bytes([value]) + data[at + 1:]


def test_other_unsupported_layouts():
    data = J.read('s9x5_420')
    assert parse(_patch_sof(data, 0, 12))[0] == ERR_UNSUPPORTED                # 12-bit precision
    assert parse(_patch_sof(data, 7, 0x12))[0] == ERR_UNSUPPORTED              # h1v2 luma
    assert parse(_patch_sof(data, 10, 0x21))[0] == ERR_UNSUPPORTED             # subsampled the other way round
    at = data.index(b'\xff\xc0')
    for marker in (0xC3, 0xC9, 0xCA):                                          # lossless, arithmetic
        assert parse(data[:at + 1] + bytes([marker]) + data[at + 2:])[0] == ERR_UNSUPPORTED
    assert parse(_patch_sof(_patch_sof(data, 1, 0), 2, 0))[0] == ERR_FORMAT    # height 0


def test_fill_bytes_and_skipped_segments():
    data = J.read('rst_48x40_420')
    want = entropy(data, parse(data)[1])[1]
    at = data.index(b'\xff\xdb')
    padded = data[:at] + b'\xff\xff\xff' + data[at:]                           # fill bytes before a marker
    padded = padded[:2] + b'\xff\xfe\x00\x05abc' + b'\xff\xe5\x00\x02' + padded[2:]   # COM and an unknown APPn
    rst = padded.index(b'\xff\xd0')
    padded = padded[:rst] + b'\xff' + padded[rst:]                             # a fill byte before RST0
    rc, info = parse(padded)
    assert rc == OK
    rc, coef, _ = entropy(padded, info)
    assert rc == OK and np.array_equal(coef, want)


@pytest.mark.parametrize('name', ['s9x5_420', 'rst_gray_48x40', 'orient6_13x21'])
def test_every_truncation_returns_a_code_and_respects_the_cap(name):
    data = J.read(name)
    full = parse(data)[1]
    seen = set()
    for n in range(len(data)):
        cut = bytes(data[:n])
        rc, info = parse(cut)
        assert rc in (OK, ERR_FORMAT), (n, rc)
        if rc == OK:
            assert info.coef_count == full.coef_count
            rc, _, _ = entropy(cut, info)
            assert rc in (OK, ERR_FORMAT), (n, rc)
            if rc == OK:
                assert n >= len(data) - 2, 'only the EOI marker may be missing from a file that still decodes'
        seen.add(rc)
    assert seen == {OK, ERR_FORMAT}


def test_corruptions_are_format_errors():
    data = J.read('rst_48x40_420')
    assert parse(data)[0] == OK

    def code(bad):
        rc, info = parse(bad)
        return rc if rc != OK else entropy(bad, info)[0]

    # a DHT whose code counts and symbols are all zero: no code is in the table
    at = data.index(b'\xff\xc4')
    ln = int.from_bytes(data[at + 2:at + 4], 'big')
    assert code(data[:at + 5] + bytes(ln - 3) + data[at + 2 + ln:]) == ERR_FORMAT
    # ... and with the table's class / id byte zeroed too, so that another table is missing
    assert code(data[:at + 4] + bytes(ln - 2) + data[at + 2 + ln:]) == ERR_FORMAT
    # a segment length that runs past the end
    at = data.index(b'\xff\xdb')
    assert code(data[:at + 2] + b'\xff\xf0' + data[at + 4:]) == ERR_FORMAT
    assert code(data[:at + 2] + b'\x00\x01' + data[at + 4:]) == ERR_FORMAT
    # a wrong RSTn sequence
    at = data.index(b'\xff\xd1')
    assert code(data[:at + 1] + b'\xd3' + data[at + 2:]) == ERR_FORMAT
    # no quantisation table at all
    at = data.index(b'\xff\xdb')
    ln = int.from_bytes(data[at + 2:at + 4], 'big')
    rest = data[:at] + data[at + 2 + ln:]
    while b'\xff\xdb' in rest[:rest.index(b'\xff\xda')]:
        at = rest.index(b'\xff\xdb')
        ln = int.from_bytes(rest[at + 2:at + 4], 'big')
        rest = rest[:at] + rest[at + 2 + ln:]
    assert code(rest) == ERR_FORMAT
    # zero width
    at = data.index(b'\xff\xc0')
    assert code(data[:at + 7] + b'\x00\x00' + data[at + 9:]) == ERR_FORMAT
    # not a JPEG
    assert code(b'') == ERR_FORMAT and code(b'\x89PNG\r\n\x1a\n' + bytes(32)) == ERR_FORMAT


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


def test_host_stage_under_address_and_ub_sanitizers(tmp_path):
    cxx = _sanitizer_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip('no host compiler with the sanitizer runtime')
    exe = str(tmp_path / 'jpeg_host_main')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(ROOT, 'tests', 'jpeg_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, J.JPEG_DIR], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert ' 0 failures' in run.stdout


def test_jpeg_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'jpeg.hip'), ())
    assert sorted(r['name'].split('(')[0] for r in rows) == ['jpeg_color_kernel', 'jpeg_idct_kernel']
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 for r in rows), rows
