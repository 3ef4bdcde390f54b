"""The wall distance's kernel as shipped (rust-doom_amd/csrc/hip/walls.hip): it is in the library, uses no scratch memory, spills no
register, leaves room for four waves per SIMD and keeps its static LDS -- the open bytes of a tile with a halo of the largest radius
and phase 1's vertical distances -- within 64 KiB; the kernels whose planes it reads and feeds are still there."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_wall_kernel_is_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    walls = [k for k in res if k.startswith('wall_')]
    assert walls == ['wall_distance_kernel'], walls  # one kernel, no variant
    r = res['wall_distance_kernel']
    assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    assert r['vgpr_count'] <= 128, r  # at least four waves per SIMD
    assert 1 <= r['group_segment_fixed_size'] <= 65536, r
    assert r['max_flat_workgroup_size'] == 256, r
    # the static LDS is what the header's constants say: (TX + 2R)(TY + 2R) open bytes and (TX + 2R) TY distances at R = 32
    import rust_doom_amd as rd
    tx, ty = rd.WALL_TILE
    halo = 2 * rd.WALL_MAX_RADIUS
    assert r['group_segment_fixed_size'] == (tx + halo) * (ty + halo) + (tx + halo) * ty, r
    # the floods and the goal distance keep their kernels
    for name in ('flood_maps_kernel', 'flood_grids_kernel', 'flood_descend_kernel', 'flood_descend_towards_kernel', 'area_frontiers_kernel',
                 'draw_area_planes_kernel', 'worldset_draw_area_planes_kernel', 'area_cells_kernel', 'draw_sector_maps_kernel'):
        assert name in res, name
