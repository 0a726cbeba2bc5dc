# -*- coding: utf-8 -*-
"""The batch letterbox kernel (csrc/preprocess.hip) keeps a lane's four pixels in registers: no scratch memory, no spilled
VGPRs, 16 bytes of LDS (the image's two scales), full occupancy (scripts/kernel_resources.py compiles the file for gfx950 and reads the code object's metadata; no GPU
needed).  The rectangular decode instances of csrc/yolo_decode.hip take the registers and LDS of the square ones."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

KERNELS = ['letterbox_batch_kernel', 'preprocess_kernel']
VGPRS = {'letterbox_batch_kernel': 38, 'preprocess_kernel': 20}     # as the cross-compile reports them


def test_preprocess_kernels_no_scratch_no_spills():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'preprocess.hip'), ())
    assert sorted(r['name'].split('(')[0] for r in rows) == KERNELS
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 for r in rows), rows
    for r in rows:
        name = r['name'].split('(')[0]
        assert r['agprs'] == 0 and r['vgprs'] == VGPRS[name], r          # pinned: a change either way wants a look
        assert r['lds'] == (16 if name == 'letterbox_batch_kernel' else 0) and r['occupancy'] == 8, r


def test_rect_decode_instances_cost_what_the_square_ones_do():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'yolo_decode.hip'), ('-ffp-contract=off',))
    tiled = {r['name'].split('(')[0]: r for r in rows if 'yolo_decode_tiled_kernel<true' in r['name']}
    assert len(tiled) == 8, sorted(tiled)
    for tp in (16, 32):
        for sc in ('true', 'false'):
            sq = tiled['void yolo_decode_tiled_kernel<true, %d, %s, false>' % (tp, sc)]
            rc = tiled['void yolo_decode_tiled_kernel<true, %d, %s, true>' % (tp, sc)]
            assert rc['scratch'] == 0 and rc['vgpr_spill'] == 0
            assert (rc['vgprs'], rc['lds'], rc['occupancy']) == (sq['vgprs'], sq['lds'], sq['occupancy']), (sq, rc)
