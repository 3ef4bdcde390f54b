"""The straight walks' kernels as shipped (rust-doom_amd/csrc/hip/line.hip): the two walk_lines kernels and the two path_straighten
kernels are in the library, use no scratch memory, spill no register, leave room for four waves per SIMD and take no LDS: a wave
works through ballots alone.  The kernels of the descents and of the frontiers are still there beside them."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

KERNELS = ['walk_lines_kernel', 'walk_lines_reversed_kernel', 'path_straighten_kernel', 'path_straighten_reversed_kernel']


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_line_kernels_are_shipped_without_scratch_spills_or_lds():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
        assert r['group_segment_fixed_size'] == 0, (name, r)
        assert r['max_flat_workgroup_size'] == 256, (name, r)
    for name in ('flood_descend_kernel', 'flood_descend_towards_kernel', 'flood_descend_octile_kernel', 'flood_descend_octile_towards_kernel',
                 'area_frontiers_kernel', 'worldset_area_frontiers_kernel'):
        assert name in res, name
