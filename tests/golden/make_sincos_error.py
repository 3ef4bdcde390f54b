#!/usr/bin/env python3
"""Writes tests/golden/sincos_error.json: the worst error of the project's sincos (tests/sincos_restatement.h, the twin of
rust-doom_amd/csrc/hip/sincos_rd.hpp) against float64 sin / cos, per binade, over every argument of the binades 2^9 .. 2^13 --
512 <= |x| < 16384, both signs -- in the measure of tests/test_world_host.py::test_restatement_sincos_within_two_ulp, with the
first argument that attains each.  Below 512 nothing is recorded: tests/test_sincos_host.py holds every argument there to the
bound of 2.  tests/test_sincos_host.py recomputes this record and compares (relative tolerance 1e-6: another libm's last digit).

    python tests/golden/make_sincos_error.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import sincos_ref  # noqa: E402

EXPONENTS = range(9, 14)
OUT = os.path.join(HERE, 'sincos_error.json')


def record():
    rows = []
    keys = [(e, neg) for neg in (False, True) for e in EXPONENTS]
    err, at = sincos_ref.worst([sincos_ref.binade(e, neg) for e, neg in keys])
    for (e, neg), w, a in zip(keys, err, at):
        x = a.view(np.float32)
        rows.append({'binade': sincos_ref.binade(e, neg), 'from': float((-1 if neg else 1) * 2.0 ** e), 'to': float((-1 if neg else 1) * 2.0 ** (e + 1)),
                     'worst_sin': float(w[0]), 'worst_sin_at': float(x[0]), 'worst_cos': float(w[1]), 'worst_cos_at': float(x[1])})
    return {'measure': 'error in units of the last place of the binary32 nearest the float64 result where that exceeds 1e-5 in '
                       'magnitude, else the absolute error over 1e-12',
            'binades': rows}


if __name__ == '__main__':
    with open(OUT, 'w') as f:
        json.dump(record(), f, indent=1)
        f.write('\n')
    print(OUT)
