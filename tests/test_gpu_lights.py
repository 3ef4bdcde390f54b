"""Every player its own clock, on the GPU (lights.hip light_tables_kernel, rdoom_lightset_tables, rdoom_batch_render_players_clocked,
rdoom_poses_from_players_device_clocked).  Each case runs in a child process of its own (tests/gpu_lights_child.py has what it
checks) under a time limit of its own; after a case that died of a signal or ran into its limit nothing more is started on the GPU:
the remaining cases fail at once."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
CHILD = os.path.join(ROOT, 'tests', 'gpu_lights_child.py')
# seconds: the host side of a case (the numpy restatement, the oracle's rasteriser, building levels) is most of it
LIMITS = {'tables': 420, 'one_time': 300, 'many_times': 240, 'oracle': 420, 'loop': 420, 'errors': 240}
_stopped = []


@pytest.mark.parametrize('case', list(LIMITS))
def test_clocked(case):
    assert not _stopped, 'not started: case %r ended in a fault or ran into its time limit' % _stopped[0]
    try:
        r = subprocess.run([sys.executable, CHILD, case], cwd=os.path.join(ROOT, 'tests'), capture_output=True, text=True,
                           timeout=LIMITS[case])
    except subprocess.TimeoutExpired as e:
        _stopped.append(case)
        pytest.fail('case %s ran longer than %d s\n%s' % (case, LIMITS[case], str(e.stdout or '')[-2000:]))
    print(r.stdout[-4000:])
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append(case)
    assert r.returncode == 0 and 'RESULT ok' in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
