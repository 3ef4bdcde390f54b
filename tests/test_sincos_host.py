"""The project's sincos on the host, with no GPU: tests/sincos_restatement.h -- the one definition the C restatements include, the
twin of rust-doom_amd/csrc/hip/sincos_rd.hpp -- swept over whole binades by tests/sincos_sweep.c.  The sums that
tests/test_gpu_sincos.py compares with the device's notice a constant that is wrong in its last place; every argument of
|x| < 512 is within the 2 of the project's ulp measure that the headers claim; the measured error from 512 to 16384 is the
committed record's; the numpy copy (area_ref.sincos) is the same function for every class of argument; and the C is defined for
every bit pattern (a run under the undefined-behaviour sanitizer, in a program of its own)."""
import json
import os
import subprocess

import numpy as np

import area_ref
import sincos_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sums_notice_a_constant_one_ulp_off():
    """(a) -DSINCOS_VARIANT=1 moves the reduction's 2/pi to the next float: the sums of the binades 2^-1 .. 2^9 must differ"""
    binades = [sincos_ref.binade(e) for e in range(-1, 10)]
    true, variant = sincos_ref.sums(binades)[binades], sincos_ref.sums(binades, variant=1)[binades]
    assert (true != variant).any()
    assert len(set(true.tolist())) == len(binades)  # (and no two binades share a sum)


def test_within_two_ulp_below_512():
    """(b) every argument of |x| < 512, both signs, zero and the denormals included: 2^24 x 136 arguments.  The bound is the one
    the project claims (tests/test_world_host.py::test_restatement_sincos_within_two_ulp); the worst measured is 1.562 (sin, at
    480.66367) and 1.527 (cos, at 27.214437)."""
    binades = [sincos_ref.binade(e, neg) for neg in (False, True) for e in range(-127, 9)]
    err, at = sincos_ref.worst(binades)
    print('worst sin %.6f at %r, worst cos %.6f at %r' % (err[:, 0].max(), at[err[:, 0].argmax(), 0:1].view(np.float32)[0],
                                                         err[:, 1].max(), at[err[:, 1].argmax(), 1:2].view(np.float32)[0]))
    bad = [(b, e.tolist(), a.view(np.float32).tolist()) for b, e, a in zip(binades, err, at) if not (e <= 2.0).all()]
    assert not bad, bad[:4]


def test_error_from_512_to_16384_is_the_recorded_curve():
    """(c) tests/golden/sincos_error.json (tests/golden/make_sincos_error.py), recomputed: the worst errors to a relative 1e-6 --
    another libm's last digit -- and the arguments that attain them"""
    record = json.load(open(os.path.join(HERE, 'golden', 'sincos_error.json')))['binades']
    assert [r['binade'] for r in record] == [sincos_ref.binade(e, neg) for neg in (False, True) for e in range(9, 14)]
    err, at = sincos_ref.worst([r['binade'] for r in record])
    x = at.view(np.float32)
    for r, e, a in zip(record, err, x):
        assert abs(e[0] - r['worst_sin']) <= 1e-6 * r['worst_sin'] and abs(e[1] - r['worst_cos']) <= 1e-6 * r['worst_cos'], (r, e)
        assert (float(a[0]), float(a[1])) == (r['worst_sin_at'], r['worst_cos_at']), (r, a)
        assert abs(r['from']) <= abs(a[0]) < abs(r['to']) and abs(r['from']) <= abs(a[1]) < abs(r['to'])
    # what the documents say of the record: past 2 from 512 on, growing with every binade
    worst = np.maximum(err[:5], err[5:]).max(1)
    assert worst[0] > 2.0 and (np.diff(worst) > 0).all()


def test_numpy_copy_is_the_same_function():
    """(d) area_ref.sincos against the header's function: 2^16 arguments of every binade (every 128th mantissa, the last
    included), +-inf and NaNs of both signs"""
    mant = np.arange(0, 1 << 23, 128, dtype=np.uint32)
    mant[-1] = (1 << 23) - 1
    for first in range(0, 512, 64):
        bits = ((np.arange(first, first + 64, dtype=np.uint32) << 23)[:, None] | mant[None, :]).reshape(-1)
        want = sincos_ref.evaluate(bits)
        s, c = area_ref.sincos(bits.view(np.float32))
        ok = sincos_ref.same_bits(s, want[:, 0]) & sincos_ref.same_bits(c, want[:, 1])
        assert ok.all(), [hex(b) for b in bits[~ok][:4]]
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)
    want = sincos_ref.evaluate(special)
    for b, w in zip(special, want):
        s, c = area_ref.sincos(np.array(b, np.uint32).view(np.float32)[()])  # a scalar, as area_ref.bands calls it
        assert isinstance(s, np.float32) and sincos_ref.same_bits(s, w[0]) and sincos_ref.same_bits(c, w[1]), hex(b)
    assert np.isnan(want).all()


def test_defined_for_every_bit_pattern(tmp_path):
    """(e) tests/sincos_sanitized.c -- a main of its own around the header -- built with the undefined-behaviour sanitizer,
    float-cast-overflow included, any report fatal: every binade at a mantissa stride of 2^13, and every argument of the binades
    from 2^30 up, exponent 255 (inf, NaN) included, where an unguarded (int) conversion would be out of range"""
    exe = str(tmp_path / 'sincos_sanitized')
    subprocess.check_call(['gcc', '-O2', '-ffp-contract=off', '-fno-fast-math', '-fsanitize=undefined,float-cast-overflow',
                           '-fno-sanitize-recover=all', '-I', HERE, '-o', exe, os.path.join(HERE, 'sincos_sanitized.c'), '-lm'])
    whole = [b for sign in (0, 256) for b in range(sign + 127 + 30, sign + 256)]
    k = min(16, os.cpu_count() or 1)
    jobs = [['0', '512', str(1 << 13)]]
    bounds = np.linspace(0, 99, k + 1).astype(int)
    for sign in (0, 256):
        jobs += [[str(sign + 157 + a), str(sign + 157 + b), '1'] for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    covered = sorted(b for j in jobs[1:] for b in range(int(j[0]), int(j[1])))
    assert covered == whole and whole[-1] == 511 and 255 in whole
    running = []
    results = []
    for j in jobs:
        running.append((j, subprocess.Popen([exe, *j], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        if len(running) >= k:
            results.append(_finish(running.pop(0)))
    results += [_finish(r) for r in running]
    assert sum(results) == 512 * 1024 + len(whole) * (1 << 23)


def _finish(job):
    args, p = job
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0 and 'runtime error' not in err, (args, p.returncode, err[-2000:])
    return int(out.split()[1])
