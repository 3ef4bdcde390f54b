"""A numpy restatement of the device light tables' contract (include/rdoom.h "device light set"):
light_level_at, noise, fract and clamp of game/src/lights.rs:33-78 in binary32 throughout, the sine of `noise` as the binary64 sine
of the binary32 argument rounded once to binary32, and Rust's `as u8` (truncate, saturate, NaN -> 0).  Vectorised over (times,
infos); every intermediate is a float32 array, so each operation rounds once to binary32 as the kernel's does."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
GLOW, RANDOM, ALTERNATE = 0, 1, 2
# rdoom_light_info (the package's LIGHT_INFO, restated so that this file imports nothing of the library)
LIGHT_INFO = np.dtype([('level', '<f4'), ('has_effect', '<i4'), ('effect_kind', '<i4'), ('alt_level', '<f4'), ('speed', '<f4'),
                       ('duration', '<f4'), ('sync', '<f4')])


def fract(x):
    return x - np.floor(x)


def noise_arg(sync, time, speed):
    """the argument of the sine in noise(sync, floor(time * speed)) (lights.rs:46, 62-64)"""
    t = np.floor(time * speed)
    return (sync + t / F(1000.0)) * F(12.9898) + sync * F(78.233)


def sine(arg):
    """the contract's sine: binary64 sine of the binary32 argument, rounded once"""
    return np.sin(arg.astype(np.float64)).astype(np.float32)


def levels_at(infos, times):
    """light_level_at of every (time, info): float32 (len(times), len(infos))"""
    infos = np.asarray(infos, LIGHT_INFO).reshape(-1)
    t = np.asarray(times, np.float32).reshape(-1, 1)
    level, alt, speed = infos['level'][None, :], infos['alt_level'][None, :], infos['speed'][None, :]
    duration, sync = infos['duration'][None, :], infos['sync'][None, :]
    with np.errstate(all='ignore'):  # the degenerate Glow divides by zero, as the reference does
        scale = level - alt
        phase = t * speed / scale
        glow = np.abs(F(0.5) - fract(phase)) * F(2.0) * scale + alt
        n = fract(F(1.0) + sine(noise_arg(sync, t, speed)) * F(43758.547))
        random = np.where(n < duration, alt, level)
        alternate = np.where(fract(t * speed + sync * F(3.5435)) < duration, alt, level)
    kind = infos['effect_kind'][None, :]
    out = np.where(kind == GLOW, glow, np.where(kind == RANDOM, random, alternate))
    out = np.where(infos['has_effect'][None, :] != 0, out, np.broadcast_to(level, out.shape))
    assert out.dtype == np.float32
    return out


def rust_u8(v):
    """`v as u8` of Rust for float32 v: NaN -> 0, saturating, truncating"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), 0, np.trunc(np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0))).astype(np.uint8)


def tables(infos, times):
    """Lights::fill_buffer_at of every time: uint8 (len(times), 256), entries from len(infos) upwards 0"""
    lv = levels_at(infos, times)
    with np.errstate(invalid='ignore'):
        c = np.where(lv < F(0.0), F(0.0), np.where(lv > F(1.0), F(1.0), lv))  # clamp: a NaN passes through
        v = (c * F(255.0)).astype(np.float32)
    out = np.zeros((lv.shape[0], 256), np.uint8)
    out[:, :lv.shape[1]] = rust_u8(v)
    return out


def random_args(infos, times):
    """(len(times), len(infos)) float32: the sine's argument at every Random entry, NaN elsewhere"""
    infos = np.asarray(infos, LIGHT_INFO).reshape(-1)
    t = np.asarray(times, np.float32).reshape(-1, 1)
    arg = noise_arg(infos['sync'][None, :], t, infos['speed'][None, :])
    is_random = (infos['has_effect'] != 0) & (infos['effect_kind'] == RANDOM)
    return np.where(is_random[None, :], arg, F(np.nan)).astype(np.float32)


_libm = None


def libm_sinf(arg):
    """glibc sinf of one binary32 argument (what the host builder and the oracle call)"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
        _libm.sinf.restype = ctypes.c_float
        _libm.sinf.argtypes = [ctypes.c_float]
    return F(_libm.sinf(float(arg)))


def explained(infos, times, got, want):
    """The rule that relates a table computed with libm sinf (`got`: the host's, the oracle's) to the contract's (`want`): every
    differing byte must be a Random entry whose sinf differs from the contract's sine at that argument.  Returns (differing
    bytes, unexplained (time index, entry) pairs)."""
    args = random_args(infos, times)
    bad = []
    diff = np.argwhere(got[:, :args.shape[1]] != want[:, :args.shape[1]])
    for ti, e in diff:
        a = args[ti, e]
        if np.isnan(a) or libm_sinf(a) == sine(np.array([a], np.float32))[0]:
            bad.append((int(ti), int(e)))
    if (got[:, args.shape[1]:] != want[:, args.shape[1]:]).any():
        bad.append((-1, -1))
    return len(diff), bad


def near_midpoint(args, rel=2.0 ** -48):
    """args (float32) whose binary64 sine lies within `rel` (relative) of the midpoint of two neighbouring binary32 numbers: there
    a binary64 sine with an error of an ulp of its own may round to either neighbour, and the contract does not pin the entry"""
    a = np.asarray(args, np.float32)
    s = np.sin(a.astype(np.float64))
    r = s.astype(np.float32)
    other = np.nextafter(r, np.where(s > r.astype(np.float64), F(np.inf), F(-np.inf)).astype(np.float32))
    mid = (r.astype(np.float64) + other.astype(np.float64)) * 0.5
    return (s != r.astype(np.float64)) & (np.abs(s - mid) <= rel * np.abs(s))


def handwritten_infos(seed=15):
    """255 infos over the ranges wad/src/light.rs can produce: levels k / 31 (k = light >> 3), shifted by the +-2 / 31 contrast and
    clamped; alt_level another k / 31; the (speed, duration) pairs of FLASH, FLICKER, SLOW_STROBE, FAST_STROBE and GLOW; sync 0 or
    a 16-bit id hash / 15.  80 each of Glow, Random and Alternate, 15 without an effect."""
    rng = np.random.default_rng(seed)
    out = np.zeros(255, LIGHT_INFO)
    for i in range(255):
        k = int(rng.integers(0, 32))
        level = F(k) / F(31.0)
        contrast = int(rng.integers(0, 3))
        if contrast:
            level = np.clip(level + (F(2.0) / F(31.0) if contrast == 1 else F(-2.0) / F(31.0)), F(0.0), F(1.0))
        out[i]['level'] = level
        if i >= 240:
            continue
        alt_k = int(rng.integers(0, 32))
        while F(alt_k) / F(31.0) == level:  # (the degenerate Glow has a table of its own: degenerate_glow)
            alt_k = (alt_k + 1) % 32
        sync = F(float(rng.integers(0, 65536))) / F(15.0)
        kind = i % 3
        if kind == GLOW:
            speed, duration, sync = F(0.5), F(0.0), F(0.0)
        elif kind == RANDOM:
            speed, duration = [(F(20.0), F(0.06)), (F(8.0), F(0.5))][int(rng.integers(0, 2))]
        else:
            speed, duration = [(F(1.0), F(0.85)), (F(2.0), F(0.7))][int(rng.integers(0, 2))]
            if rng.integers(0, 4) == 0:
                sync = F(0.0)
        out[i] = (level, 1, kind, F(alt_k) / F(31.0), speed, duration, sync)
    return out


def degenerate_glow():
    """Glow lights with level == alt_level (light.rs never builds one; a caller's table may): the division by zero"""
    out = np.zeros(3, LIGHT_INFO)
    out[0] = (F(0.5), 1, GLOW, F(0.5), F(0.5), F(0.0), F(0.0))
    out[1] = (F(1.0), 1, GLOW, F(1.0), F(0.5), F(0.0), F(0.0))
    out[2] = (F(0.0), 1, GLOW, F(0.0), F(2.0), F(0.0), F(0.0))
    return out


def host_times(seed=7):
    """the times of the host comparison: 0, the times the existing tests render at, 200 random ones in an hour, a few near 1e5"""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array([0.0, 0.31, 0.5, 0.75, 1.25, 1.7, 12.5], np.float32),
                           rng.uniform(0.0, 3600.0, 200).astype(np.float32),
                           np.array([99999.0, 100000.0, 100000.5, 100001.37, 123456.79], np.float32)])
