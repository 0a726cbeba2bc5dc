# -*- coding: utf-8 -*-
"""The JPEG encoder's and the box overlay's kernels keep everything in registers: no scratch memory, no spilled VGPRs
(scripts/kernel_resources.py compiles the file for gfx950 and reads the code object's metadata; no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


@pytest.mark.parametrize('source, kernels', [('jpeg_enc.hip', ['jpeg_fdct_kernel']), ('draw.hip', ['draw_boxes_kernel'])])
def test_no_scratch_and_no_spills(source, kernels):
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', source), ())
    assert sorted(r['name'].split('(')[0] for r in rows) == kernels
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 for r in rows), rows
