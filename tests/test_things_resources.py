"""The things' kernels as shipped (rust-doom_amd/csrc/hip/things.hip): both sensing kernels are in the library, use no scratch
memory, spill no register, leave room for four waves per SIMD and take the static LDS the kernel declares -- the blocking lines, the
rays and the minima of the sight pass, the waves' counts, their nearest keys and collected counts per category, and the six values
parked for the touch test."""
import importlib.util
import os
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

KERNELS = ['sense_things_kernel', 'worldset_sense_things_kernel']
# list and rays: 256 float4 each; part: 256 floats; counts: 4 words; keys: 4 x 8 x 8 bytes; collected: 4 x 8 words; parked: 6 floats
LDS = 2 * 256 * 16 + 256 * 4 + 4 * 4 + 4 * 8 * 8 + 4 * 8 * 4 + 6 * 4


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_the_thing_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    assert LDS == 9640
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (name, r)
        assert r['vgpr_count'] <= 128, (name, r)  # at least four waves per SIMD
        assert r['group_segment_fixed_size'] == LDS, (name, r)
        assert r['max_flat_workgroup_size'] == 256, (name, r)
    for name in ('reveal_lines_kernel', 'worldset_reveal_lines_kernel'):  # the kernels whose sight pass this one shares are still there
        assert name in res, name
