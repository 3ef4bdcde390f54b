"""The kernels of the clocked render as shipped (rust-doom_amd/csrc/hip/lights.hip, frames.hip): both are in the library, use no
scratch memory, spill no register and keep no static LDS; the light kernel is one wave64 per workgroup."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_light_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('light_tables_kernel', 'player_frames_kernel'):
        assert name in res, sorted(res)
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == 0 and r['max_flat_workgroup_size'] == 64, (name, r)
        assert r['vgpr_count'] <= 64, (name, r)  # eight waves per SIMD
