"""The kernels of things in the frame as shipped -- the thing plane's pair, planes.hip's instantiation for its fourth, internal plane
(PLANE_THING = 4 in kernels.hpp), and the three of rust-doom_amd/csrc/hip/framethings.hip: they are in the library, use no scratch
memory and spill no register; the thing-plane kernels use no LDS, as the other planes'; the reduction keeps its 64-slot table in
well under 8 KiB of static LDS; all run 256 threads a workgroup.  These are conditions; the register counts recorded below are what
the shipped build gave, and what DESIGN section 34 quotes.  Only the new kernels are named here."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

TABLE = 7 * 64 * 4  # framethings.hip FrameThingTable: key, count, four box words and the depth bits of 64 slots
RECORDED = {'plane_kernel<4u, false>': dict(vgpr_count=32, lds=0), 'plane_kernel<4u, true>': dict(vgpr_count=32, lds=0),
            'plane_fix_kernel<4u, false>': dict(vgpr_count=14, lds=0), 'plane_fix_kernel<4u, true>': dict(vgpr_count=14, lds=0),
            'frame_things_init_kernel': dict(vgpr_count=6, lds=0), 'frame_things_reduce_kernel': dict(vgpr_count=23, lds=TABLE),
            'frame_things_bits_kernel': dict(vgpr_count=19, lds=0)}


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_frame_thing_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name, recorded in RECORDED.items():
        assert name in res, sorted(res)
        r = res[name]
        print(name, r, 'recorded', recorded)
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
        assert r['vgpr_count'] <= 64, r  # eight waves per SIMD
        assert r['group_segment_fixed_size'] == recorded['lds'] and recorded['lds'] < 8 * 1024, r
        assert r['max_flat_workgroup_size'] == 256, r
    assert TABLE == 1792
