"""Child process of tests/test_gpu_planes.py (rdoom_debug_set is process-wide; prints one RESULT line):
  hooks  the golden poses of level 0 under every equivalent-path test hook in turn, each time a dirtied batch rendered without and
         with primitive ids: depth, label and primitive planes must equal the ORACLE's composition (tests/planes_ref.py) bit for
         bit, in both row orders, and the primitive plane the id path's own read_primitive_ids."""
import json
import os
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import planes_ref
import rust_doom_amd as rd
from oracle import wad_oracle
from util import GOLDEN, META_PATH, dirtying_poses, ensure_wad

HOOKS = [{}, {'vis32': 1}, {'no_qtab': 1}, {'keep_vis': 1}, {'leak_mod': 97}, {'no_bins': 1}, {'entry_cap': 300}, {'vis32': 1, 'leak_mod': 101}]
PLANES = {'depth': rd.PLANE_DEPTH, 'label': rd.PLANE_LABEL, 'primitive': rd.PLANE_PRIMITIVE}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def hooks_case():
    lv = wad_oracle.build_level(ensure_wad(), META_PATH, 0)
    g = json.load(open(os.path.join(GOLDEN, 'digests.json')))
    rows = np.load(os.path.join(GOLDEN, 'poses.npy'))[0]
    poses = np.zeros(len(rows), rd.POSE)
    for i, p in enumerate(rows):
        poses[i]['modelview'], poses[i]['projection'], poses[i]['time'] = p[:16], p[16:32], p[32]
    lights = np.array([lv.lights.fill_buffer_at(float(p['time'])) for p in poses])
    w, h = g['width'], g['height']
    want = planes_ref.expected_batch(lv, poses, lights, w, h)
    other, olights = dirtying_poses(poses), np.roll(lights, 1, axis=0)
    level = rd.DeviceLevel(lv)
    bad, fixups, cases = 0, 0, 0
    for hooks in HOOKS:
        rd.debug_set('reset')
        for name, value in hooks.items():
            rd.debug_set(name, value)
        batch = rd.Batch(level, w, h, len(poses))  # (vis32 / entry_cap are read here)
        for ids in (False, True):
            if ids:
                batch.enable_primitive_ids()
            batch.render(other, olights)
            t = batch.render(poses, lights, timed=True)
            fixups += t['fixup_pixels']
            for name, plane in PLANES.items():
                for td in (False, True):
                    got = batch.read_plane(plane, top_down=td)
                    exp = want[name][:, ::-1] if td else want[name]
                    diff = int((bits(got) != bits(exp)).sum())
                    if ids and name == 'primitive' and not td:
                        diff += int((got != batch.read_primitive_ids()).sum())
                    if diff:
                        print('MISMATCH hooks=%r ids=%s plane=%s top_down=%s pixels=%d' % (hooks, ids, name, td, diff))
                    bad += diff
            cases += 1
        batch.close()
    rd.debug_set('reset')
    print('RESULT bad=%d fixups=%d cases=%d' % (bad, fixups, cases))
    return bad == 0


if __name__ == '__main__':
    sys.exit(0 if {'hooks': hooks_case}[sys.argv[1]]() else 1)
