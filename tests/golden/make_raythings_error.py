"""Writes tests/golden/raythings_error.json: what tests/raythings_ref.py's binary32 restatement of include/rdoom_rays.h differs by
from the float64 model of the same lines on raythings_ref.random_field() -- how many rays name the same thing, and the worst
|t32 - t64| among those.  tests/test_raythings_host.py allows four times the recorded worst (other numpy builds), and the GPU is
never part of it: the yardstick is the float64 model.  Run from the repository root: python tests/golden/make_raythings_error.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import raythings_ref  # noqa: E402

if __name__ == '__main__':
    c = raythings_ref.field_comparison()
    record = dict(field=raythings_ref.FIELD, rays=c['rays'], agree=c['agree'], hits=c['hits'], worst_abs_t=c['worst'], numpy=np.__version__)
    with open(os.path.join(HERE, 'raythings_error.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print(record)
