"""The test side of the sincos sweep: tests/sincos_sweep.c (the restatements' one sincos, tests/sincos_restatement.h, swept over
binades) compiled like the restatements and loaded through ctypes.  A binade is bits >> 23, sign and exponent together."""
import ctypes
import os
import threading

import numpy as np

from util import restatement_lib  # (first: it puts the repository on the path)
import world_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'sincos_sweep.c')
HEADER = os.path.join(HERE, 'sincos_restatement.h')
N_BINADES, BINADE = 512, 1 << 23
NAN = 0x7FC00000
_sums = {}
_lock = threading.Lock()


def binade(exponent, negative=False):
    """the binade of 2^exponent <= |x| < 2^(exponent + 1); exponent -127: zero and the denormals"""
    assert -127 <= exponent <= 128
    return (256 if negative else 0) + exponent + 127


def _spread(n, k):
    """0 .. n - 1 reordered so that _chunked's k contiguous ranges each take every k-th index: neighbouring binades cost alike"""
    return [j for i in range(k) for j in range(i, n, k)]


def lib(variant=0):
    L = restatement_lib(SRC, [HEADER], flags=['-DSINCOS_VARIANT=%d' % variant] if variant else [], tag='_variant%d' % variant if variant else '')
    v, u = ctypes.c_void_p, ctypes.c_uint32
    for name, args in (('ss_sums', [u, u, v]), ('ss_raw', [u, v]), ('ss_eval', [v, u, v]), ('ss_worst', [u, u, v, v])):
        getattr(L, name).restype, getattr(L, name).argtypes = None, args
    return L


def sums(binades=None, variant=0, threads=16):
    """the 512 per-binade sums as a uint64 array (slots outside `binades`, a sorted list, stay 0); the whole sweep of the true
    function is computed once per process"""
    whole = binades is None
    with _lock:
        if whole and variant in _sums:
            return _sums[variant]
        todo = list(range(N_BINADES)) if whole else [int(b) for b in binades]
        todo = [todo[j] for j in _spread(len(todo), threads)]
        out = np.zeros(N_BINADES, np.uint64)
        L = lib(variant)

        def run(r):
            for b in todo[r[0]:r[1]]:
                L.ss_sums(b, b + 1, out.ctypes.data)
        world_ref._chunked(run, len(todo), threads)
        if whole:
            out.setflags(write=False)
            _sums[variant] = out
        return out


def raw(b):
    """binade b's (s, c) pairs by mantissa: float32 (2^23, 2)"""
    out = np.empty((BINADE, 2), np.float32)
    lib().ss_raw(int(b), out.ctypes.data)
    return out


def evaluate(bits):
    """the (s, c) pairs of the arguments whose bits are given: float32 (n, 2)"""
    bits = np.ascontiguousarray(bits, np.uint32).reshape(-1)
    out = np.empty((len(bits), 2), np.float32)
    lib().ss_eval(bits.ctypes.data, len(bits), out.ctypes.data)
    return out


def worst(binades, stride=1, threads=16):
    """per binade of the list: (worst sin, worst cos) float64 (n, 2) in test_restatement_sincos_within_two_ulp's measure against
    float64 sin / cos, and the bits of the arguments that attain them, uint32 (n, 2)"""
    binades = [int(b) for b in binades]
    err, at = np.zeros((len(binades), 2), np.float64), np.zeros((len(binades), 2), np.uint32)
    L = lib()

    order = _spread(len(binades), threads)

    def run(r):
        for i in order[r[0]:r[1]]:
            L.ss_worst(binades[i], stride, err[i].ctypes.data, at[i].ctypes.data)
    world_ref._chunked(run, len(binades), threads)
    return err, at


def same_bits(a, b):
    """elementwise: the same binary32, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
