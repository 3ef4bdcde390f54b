#!/usr/bin/env python3
"""Writes tests/golden/step_model_error.json: the worst absolute difference of pos, vel and last_height_diff between the binary32
restatement of the player step (tests/world_restatement.c through world_ref.RefWorld.step, on the CPU) and the float64 model
(tests/step_model.py), per config and tick length of tests/step_cases.py, over the model's cases in room A of the analytic level:
one record for the cases with clipping on and one for those with clipping off, whose landing height comes from noclip()'s
2000-unit probe, a binary32 sum about 1000 (an ulp of 6e-5).  `tick_cap` is the ticks a case runs at most there (60, fewer where
the spring is unstable: step_cases.tick_cap), `landings` the ticks in which noclip() put a head sphere on the floor.
It is binary32 rounding accumulated over a case's ticks: the tests allow the product 8 times the record (another libm, another
order of the thread chunks) and never measure it against the GPU.  A pos record above 1e-3 / 8 fails here: the bound is capped at
1e-3 world units.  tests/test_step_model_host.py recomputes this record and compares.

    python tests/golden/make_step_model_error.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    sys.path.insert(0, p)
import rust_doom_amd as rd  # noqa: E402

import step_cases as sc  # noqa: E402
import world_ref  # noqa: E402
from util import META_PATH, ensure_wad  # noqa: E402

OUT = os.path.join(HERE, 'step_model_error.json')
FACTOR, POS_CAP = 8.0, 1e-3


def record():
    ref = world_ref.RefWorld(rd.Wad(ensure_wad(), META_PATH), sc.MODEL_LEVEL)
    rows = []
    for name, values in sc.CONFIGS.items():
        for key, dt in sc.DTS.items():
            names, st, inp, ticks, final = sc.model_run(values, dt)
            got = sc.snapshots(lambda s, i: ref.step(s, i, config=sc.config(values), dt=dt), st, inp, ticks)
            row = {'config': name, 'dt': key, 'cases': len(names), 'ticks': int(ticks.sum()), 'tick_cap': sc.tick_cap(dict(zip(sc.FIELDS, values)), dt),
                   'landings': int(final['landings'].sum())}
            for cls, mask in sc.classes(st).items():
                row[cls] = sc.model_error(got, final, mask)
                if FACTOR * row[cls]['pos'] > POS_CAP:
                    raise SystemExit('%s dt %s, %s: pos differs by %g, the bound would pass %g' % (name, key, cls, row[cls]['pos'], POS_CAP))
            rows.append(row)
    return {'measure': 'worst absolute difference between the binary32 restatement and the float64 model over the cases, in world '
                       'units (pos, last_height_diff) and world units per second (vel)',
            'factor': FACTOR, 'records': rows}


if __name__ == '__main__':
    with open(OUT, 'w') as f:
        json.dump(record(), f, indent=1)
        f.write('\n')
    print(OUT)
