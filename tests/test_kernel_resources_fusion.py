# -*- coding: utf-8 -*-
"""The test-time-augmentation kernels (csrc/tta.hip) keep a lane's pixels / elements in registers: no scratch memory, no
spills, no AGPRs, no LDS, full occupancy; the weighted-box-fusion kernel of csrc/postprocess.hip uses no scratch and holds its
cluster state in 45 KB of LDS (scripts/kernel_resources.py compiles the files for gfx950 and reads the code objects'
metadata; no GPU needed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

KERNELS = ['tta_view_kernel', 'void tta_merge_kernel<false>', 'void tta_merge_kernel<true>']
VGPRS = {'tta_view_kernel': 28, 'void tta_merge_kernel<true>': 8, 'void tta_merge_kernel<false>': 16}   # as the cross-compile reports them


def test_tta_kernels_no_scratch_no_spills():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'tta.hip'), ('-ffp-contract=off',))
    assert sorted(r['name'].split('(')[0] for r in rows) == KERNELS
    assert all(r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 for r in rows), rows
    for r in rows:
        name = r['name'].split('(')[0]
        assert r['agprs'] == 0 and r['vgprs'] == VGPRS[name], r          # pinned: a change either way wants a look
        assert r['lds'] == 0 and r['occupancy'] == 8, r


def test_wbf_kernel_uses_no_scratch():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'yolov4_amd', 'csrc', 'postprocess.hip'), ('-ffp-contract=off',))
    wbf = [r for r in rows if 'post_wbf_kernel<' in r['name']]
    assert sorted(r['name'].split('(')[0] for r in wbf) == ['void post_wbf_kernel<false>', 'void post_wbf_kernel<true>']
    for r in wbf:
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['agprs'] == 0, r
        assert 1024 * 44 <= r['lds'] < 65536 and r['occupancy'] >= 2, r     # the cluster state of 1024 candidates
