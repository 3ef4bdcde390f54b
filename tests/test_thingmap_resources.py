"""The thing-map kernel as shipped (rust-doom_amd/csrc/hip/thingmap.hip): it is in the library, uses no scratch memory, spills no
register, leaves room for four waves per SIMD and keeps its list in at most 16 KiB of static LDS -- with 160 KiB per CU, ten such
workgroups (40 waves) are more than a CU holds, so LDS never limits its occupancy.  The three are conditions;
the figures recorded below are what the shipped build gave, and what DESIGN section 30 quotes.  The thing set's declaration moved to
a header of its own for this kernel: the sensing kernels of things.hip are still there, with the LDS they declare."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

LIST = 768 * 16  # thingmap.hip LIST_CAP entries of (x, z, r2, key)
LDS = LIST + 4 * 4  # and the four waves' counts
RECORDED = dict(vgpr_count=48, sgpr_count=50)  # of the shipped build: quoted, not required


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_thing_map_kernel_is_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    assert 'draw_thing_maps_kernel' in res, sorted(res)
    r = res['draw_thing_maps_kernel']
    print('draw_thing_maps_kernel', r, 'recorded', RECORDED)
    assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    assert r['vgpr_count'] <= 128, r  # at least four waves per SIMD
    assert r['group_segment_fixed_size'] == LDS == 12304 and LDS <= 16 * 1024, r
    assert r['max_flat_workgroup_size'] == 256, r
    for name in ('sense_things_kernel', 'worldset_sense_things_kernel'):
        assert name in res and res[name]['group_segment_fixed_size'] == 9640, (name, res.get(name))
