"""The spawn kernels (rust-doom_amd/csrc/hip/spawn.hip) as shipped: both are in the library, use no scratch memory, spill no
register, leave room for four waves per SIMD and keep nothing in LDS -- a lane's candidate, its generator and its descents live in
registers (tests/test_flood_resources.py)."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_spawn_kernels_are_shipped_without_scratch_spills_or_lds():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('spawn_players_kernel', 'worldset_spawn_players_kernel'):
        assert name in res, sorted(res)
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
        assert r['group_segment_fixed_size'] == 0, (name, r)
        assert r['max_flat_workgroup_size'] == 64, (name, r)
