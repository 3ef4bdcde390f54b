"""The player step on the GPU away from its default config and tick length (world.hip: step_players under player_step_kernel,
game_step_kernel and worldset_game_step_kernel): bit for bit against the restatements at every config and tick length of
tests/step_cases.py, the argument edges of the three entry points, the float64 model of tests/step_model.py and its closed forms,
and doors that rise at their speed at other tick lengths.  Each case runs in a child process of its own
(tests/gpu_step_child.py has what it checks) under a time limit of its own; after a case that died of a signal, ran into its
limit or failed otherwise than by one of its own assertions nothing more is started on the GPU: the remaining cases fail at once.  tests/test_step_configs_host.py and
tests/test_step_model_host.py hold the CPU side: that no case passes vacuously."""
import os
import subprocess
import sys

import pytest

import step_cases as sc
from util import ROOT

pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
CHILD = os.path.join(ROOT, 'tests', 'gpu_step_child.py')
ALL = list(sc.ALL_FIELDS)
THIRD = (len(sc.CONFIGS) + 2) // 3
CASES = [('step', '0'), ('step', '1'), ('edges',)]
CASES += [(kind, name, key) for kind in ('game', 'worldset') for name in ALL for key in ('35', '120')]
CASES += [('model', str(k), str(min(k + THIRD, len(sc.CONFIGS)))) for k in range(0, len(sc.CONFIGS), THIRD)]
CASES += [('doors', '35'), ('doors', '120')]
LIMIT = 240  # seconds: a case is a few; most of that is the host side (starting Python, the restatements, the model)
FAULT_WORDS = ('illegal memory access', 'HIP error', 'hipError', 'HSA_STATUS_ERROR', 'Memory access fault')
_stopped = []


@pytest.mark.parametrize('case', CASES, ids='-'.join)
def test_step(case):
    assert not _stopped, 'not started: case %r ended in a fault or ran into its time limit' % (_stopped[0],)
    try:
        r = subprocess.run([sys.executable, CHILD, *case], cwd=os.path.join(ROOT, 'tests'), capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(case)
        pytest.fail('case %s ran longer than %d s\n%s' % (case, LIMIT, str(e.stdout or '')[-2000:]))
    print(r.stdout[-12000:])
    # a fault can also come back as a Python exception of the child (HIP's 'an illegal memory access was encountered' through
    # torch or the library's status): only a case that failed one of its own assertions lets the next one start
    if r.returncode != 0 and (r.returncode < 0 or r.returncode in (124, 134, 137, 139) or 'AssertionError' not in r.stderr
                              or any(w in r.stdout + r.stderr for w in FAULT_WORDS)):
        _stopped.append(case)
    assert r.returncode == 0 and 'RESULT ok' in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
