"""The flood kernel (rust-doom_amd/csrc/hip/flood.hip) as shipped: it is in the library, uses no scratch memory, spills no register,
leaves room for four waves per SIMD (two workgroups of 1024 threads on a CU are two waves per SIMD more than that needs), and keeps
its static LDS to the two flags and the waves' counts, so that the static and dynamic LDS of the largest grid stay within the 64 KiB
a launch gets without raising an attribute of the function (tests/test_sectors_resources.py)."""
import importlib.util
import os
import shutil

import pytest

import rust_doom_amd as rd
from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_flood_kernel_is_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    assert 'flood_maps_kernel' in res, sorted(res)
    r = res['flood_maps_kernel']
    assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    assert r['vgpr_count'] <= 128, r  # at least four waves per SIMD
    assert r['max_flat_workgroup_size'] == 1024, r
    cells = rd.flood_max_cells()
    dynamic = ((2 * cells + 3) & ~3) + cells  # a 16-bit distance per cell, rounded up to a word, and a byte of move bits
    assert r['group_segment_fixed_size'] <= 128 and r['group_segment_fixed_size'] + dynamic <= 64 * 1024, (r, dynamic)
