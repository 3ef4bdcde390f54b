"""The sector kernels (rust-doom_amd/csrc/hip/sectors.hip) as shipped: all four are in the library, use no scratch memory, spill no
register, leave room for four waves per SIMD and keep static LDS under 16 KiB, so that LDS never limits their occupancy
(tests/test_automap_resources.py)."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_sector_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name, threads in (('locate_players_kernel', 64), ('worldset_locate_players_kernel', 64), ('draw_sector_maps_kernel', 256),
                          ('worldset_draw_sector_maps_kernel', 256)):
        assert name in res, sorted(res)
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
        assert r['group_segment_fixed_size'] < 16 * 1024 and r['max_flat_workgroup_size'] == threads, (name, r)
