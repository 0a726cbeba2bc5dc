# -*- coding: utf-8 -*-
"""RandAugment's kernels (csrc/randaug.hip) keep everything in registers and a few KB of LDS: no scratch memory, no spilled
VGPRs (scripts/kernel_resources.py compiles the file for gfx950 and reads the code object's metadata; no GPU needed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

KERNELS = ['randaug_gather_u8_kernel', 'randaug_stats_kernel', 'void randaug_apply_kernel<false>',
           'void randaug_apply_kernel<true>']


def test_no_scratch_and_no_spills():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'randaug.hip'), ('-ffp-contract=off',))
    assert sorted(r['name'].split('(')[0] for r in rows) == KERNELS
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 for r in rows), rows
    for r in rows:
        if 'apply' in r['name'] or 'stats' in r['name']:
            assert r['vgprs'] <= 64 and r['lds'] <= 4096, r        # eight waves per SIMD; the tables and the histogram
        else:
            assert r['lds'] == 0, r                                 # the gather, as in csrc/resample.hip
