"""The ray-cast kernels (rust-doom_amd/csrc/hip/world.hip) as shipped: both are in the library, use no scratch memory and spill
no register -- their node stack is in dynamic LDS, sized at launch, so the static LDS is zero too."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_ray_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('cast_rays_kernel', 'worldset_cast_rays_kernel'):
        assert name in res, sorted(res)
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['group_segment_fixed_size'] == 0 and r['max_flat_workgroup_size'] == 64, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
