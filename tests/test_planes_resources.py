"""The plane kernels (rust-doom_amd/csrc/hip/planes.hip) as shipped: every instantiation found in the library uses no scratch
memory and spills no register, and every plane has at least one -- the three of include/rdoom.h and the fourth, internal one of
the thing plane (PLANE_THING in kernels.hpp).  A bandwidth-bound pass has no excuse for either."""
import importlib.util
import os
import re
import shutil

import pytest

from util import ROOT

_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)

HEADER = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
KERNELS = open(os.path.join(ROOT, 'rust-doom_amd', 'csrc', 'hip', 'kernels.hpp')).read()


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_plane_kernels_are_shipped_without_scratch_or_spills():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    ours = {k: v for k, v in res.items() if re.match(r'plane_(fix_)?kernel<', k)}
    assert ours, sorted(res)
    for k, r in ours.items():
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (k, r)
        assert r['group_segment_fixed_size'] == 0, (k, r)  # no LDS either
    planes = {name: int(re.search(r'^#define\s+RDOOM_PLANE_%s\s+(\d+)u' % name, HEADER, flags=re.M).group(1)) for name in ('DEPTH', 'LABEL', 'PRIMITIVE')}
    planes['THING'] = int(re.search(r'^constexpr uint32_t PLANE_THING = (\d+)u;', KERNELS, flags=re.M).group(1))
    assert len(set(planes.values())) == 4 and 'PLANE_THING' not in HEADER
    for name, plane in planes.items():
        for kernel in ('plane_kernel', 'plane_fix_kernel'):
            found = [k for k in ours if re.match(r'%s<%du?, (true|false)>' % (kernel, plane), k)]
            assert found, (name, kernel, sorted(ours))
