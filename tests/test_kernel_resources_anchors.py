# -*- coding: utf-8 -*-
"""The anchor-fitting kernels (csrc/anchors.hip) keep their shapes in registers and their tables in a few KB of LDS: no
scratch memory, no spilled VGPRs (scripts/kernel_resources.py compiles the file for gfx950 and reads the code object's
metadata; no GPU needed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

KERNELS = ['anchor_assign_kernel', 'anchor_fitness_kernel']
VGPRS = {'anchor_assign_kernel': 45, 'anchor_fitness_kernel': 53}     # as the cross-compile reports them


def test_no_scratch_no_spills_small_lds():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'anchors.hip'), ('-ffp-contract=off',))
    assert sorted(r['name'].split('(')[0] for r in rows) == KERNELS
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 for r in rows), rows
    for r in rows:
        assert r['lds'] <= 8192, r
        assert r['agprs'] == 0 and r['vgprs'] <= VGPRS[r['name'].split('(')[0]], r   # <= 64: eight waves per SIMD, the most there are
        assert r['occupancy'] == 8, r
