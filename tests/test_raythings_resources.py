"""The kernels of the rays that see things as shipped (rust-doom_amd/csrc/hip/raythings.hip): they are in the library, use no
scratch memory, spill no register, leave room for four waves per SIMD, keep their list and their keys in at most 16 KiB of static
LDS -- with 160 KiB per CU, ten such workgroups (40 waves) are more than a CU holds, so LDS never limits their occupancy (DESIGN
section 16) -- and run 256 threads a workgroup.  These are conditions; the register counts recorded below are what the shipped build
gave, and what DESIGN section 33 quotes.  The kernels whose helpers this one borrows are still there, with the LDS they declare."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

LIST = 512 * (16 + 8)    # raythings.hip LIST_CAP entries of (cx, cz, cc, bottom) and (top, index)
KEYS = 4 * 64 * 8        # a key per wave and ray of a pass of 64
LDS = LIST + KEYS + 4 * 4 + 4 * 4  # and the four waves' counts and reaches
RECORDED = {'cast_rays_things_kernel': dict(vgpr_count=58, sgpr_count=101), 'worldset_cast_rays_things_kernel': dict(vgpr_count=58, sgpr_count=101)}


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_ray_thing_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name, recorded in RECORDED.items():
        assert name in res, sorted(res)
        r = res[name]
        print(name, r, 'recorded', recorded)
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
        assert r['vgpr_count'] <= 128, r  # at least four waves per SIMD
        assert r['group_segment_fixed_size'] == LDS == 14368 and LDS <= 16 * 1024, r
        assert r['max_flat_workgroup_size'] == 256, r
    # the kernels whose helpers are borrowed (thingset.hpp, world_shared.hpp's append and live_height) keep their LDS
    for name in ('sense_things_kernel', 'worldset_sense_things_kernel'):
        assert name in res and res[name]['group_segment_fixed_size'] == 9640, (name, res.get(name))
    for name in ('stamp_things_kernel', 'worldset_stamp_things_kernel'):
        assert name in res and res[name]['group_segment_fixed_size'] == 15376, (name, res.get(name))
    assert res['draw_thing_maps_kernel']['group_segment_fixed_size'] == 12304, res['draw_thing_maps_kernel']
