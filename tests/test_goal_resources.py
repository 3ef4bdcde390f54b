"""The goal distance's kernels as shipped: the flood of grids (rust-doom_amd/csrc/hip/flood.hip), the two plane kernels and the two
cell kernels (goal.hip) are in the library, use no scratch memory, spill no register and leave room for four waves per SIMD; the
flood keeps its workgroup of 1024 threads and its LDS to the two flags and the waves' counts -- its distances and move bits live in
global memory, whatever the grid's size."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

KERNELS = ['flood_grids_kernel', 'draw_area_planes_kernel', 'worldset_draw_area_planes_kernel', 'area_cells_kernel', 'worldset_area_cells_kernel']


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_goal_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
    r = res['flood_grids_kernel']
    assert r['max_flat_workgroup_size'] == 1024, r
    assert 0 < r['group_segment_fixed_size'] <= 128, r  # the two flags and sixteen counts
    for name in KERNELS[1:]:
        assert res[name]['group_segment_fixed_size'] == 0, (name, res[name])
    # the units this one reads from keep their kernels
    for name in ('flood_maps_kernel', 'reveal_area_kernel', 'draw_area_maps_kernel', 'draw_sector_maps_kernel', 'locate_players_kernel'):
        assert name in res, name
