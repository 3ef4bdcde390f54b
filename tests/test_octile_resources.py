"""The octile distance's kernels as shipped (rust-doom_amd/csrc/hip/flood.hip, path.hip): the flood and the two descents are in the library,
use no scratch memory, spill no register and leave room for four waves per SIMD; the flood keeps a workgroup of 1024 threads and
its LDS to the two flags and the waves' counts -- its distances and move bits live in global memory, whatever the grid's size.  The
kernels of the 4-neighbour calls are still there beside them."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

KERNELS = ['flood_octile_kernel', 'flood_descend_octile_kernel', 'flood_descend_octile_towards_kernel']


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_octile_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
    r = res['flood_octile_kernel']
    assert r['max_flat_workgroup_size'] == 1024, r
    assert 0 < r['group_segment_fixed_size'] <= 128, r  # the two flags and sixteen counts
    for name in KERNELS[1:]:
        assert res[name]['group_segment_fixed_size'] == 0, (name, res[name])
    for name in ('flood_grids_kernel', 'flood_maps_kernel', 'flood_descend_kernel', 'flood_descend_towards_kernel', 'area_frontiers_kernel'):
        assert name in res, name
