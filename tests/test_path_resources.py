"""The path unit's kernels (rust-doom_amd/csrc/hip/path.hip) as shipped: the two walks and the two frontier kernels are in the
library, use no scratch memory, spill no register and leave room for four waves per SIMD; the frontier keeps its workgroup of 1024
threads and its LDS to the sixteen waves' keys and counts; the walks have four waves to a workgroup and no LDS at all."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

DESCEND = ['flood_descend_kernel', 'flood_descend_towards_kernel']
FRONTIERS = ['area_frontiers_kernel', 'worldset_area_frontiers_kernel']


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_path_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in DESCEND + FRONTIERS:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
    for name in FRONTIERS:
        assert res[name]['max_flat_workgroup_size'] == 1024, (name, res[name])
        assert 0 < res[name]['group_segment_fixed_size'] <= 256, (name, res[name])  # sixteen 64-bit keys and sixteen counts: 192 bytes
    for name in DESCEND:
        assert res[name]['max_flat_workgroup_size'] == 256, (name, res[name])
        assert res[name]['group_segment_fixed_size'] == 0, (name, res[name])
    # the units this one reads from keep their kernels
    for name in ('flood_grids_kernel', 'draw_area_planes_kernel', 'area_cells_kernel', 'reveal_area_kernel'):
        assert name in res, name
