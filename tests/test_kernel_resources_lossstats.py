# -*- coding: utf-8 -*-
"""The loss-statistics kernels (csrc/yolo_loss.hip) hold their eleven partial sums in registers:
no scratch memory, no spilled VGPRs, 352 B of LDS for the block reduction and 22 KB for the one-block fold
(scripts/kernel_resources.py compiles the file for gfx950 and reads the code object's metadata; no GPU needed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

# as the cross-compile reports them: (VGPRs, LDS bytes)
KERNELS = {'yolo_loss_stats_kernel': (33, 352), 'yolo_loss_stats_fold_kernel': (48, 22528)}


def test_no_scratch_no_spills_and_the_stated_registers_and_lds():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'yolo_loss.hip'), ('-ffp-contract=off',))
    rows = [r for r in rows if r['name'].split('(')[0] in KERNELS]
    assert sorted(r['name'].split('(')[0] for r in rows) == sorted(KERNELS)
    for r in rows:
        vgprs, lds = KERNELS[r['name'].split('(')[0]]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, r
        assert r['agprs'] == 0 and r['vgprs'] <= vgprs and r['lds'] == lds, r
        assert r['vgprs'] <= 64, r                             # eight waves per SIMD, the most there are
