# -*- coding: utf-8 -*-
"""YOLOv4-tiny's kernels (csrc/tiny.hip) keep everything in registers: no scratch memory, no spilled VGPRs -- the filter
gradient's 27 x 4 accumulators per thread included (scripts/kernel_resources.py compiles the file for gfx950 and reads the
code object's metadata; no GPU needed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

KERNELS = ['fork_half_bwd_kernel', 'pool2_bwd_kernel', 'pool2_fwd_kernel', 'stem_s2_fwd_kernel', 'stem_s2_wgrad_fold_kernel',
           'stem_s2_wgrad_kernel']


def test_no_scratch_and_no_spills():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'tiny.hip'), ())
    assert sorted(r['name'].split('(')[0] for r in rows) == KERNELS
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 for r in rows), rows
    wgrad = [r for r in rows if r['name'].startswith('stem_s2_wgrad_kernel')][0]
    assert wgrad['vgprs'] <= 168 and wgrad['lds'] <= 64 * 1024          # three waves per SIMD, LDS of the default limit
