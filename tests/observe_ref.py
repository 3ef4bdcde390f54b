"""What rdoom_batch_resolve_observation / rdoom_batch_read_observation must return, restated in numpy from FULL-SIZE frames: the
RGB8 frames (n, H, W, 3) uint8 and the depth planes (n, H, W) float32, bottom-up rows, which the callers take from the oracle
(test_gpu_rgb.compose, planes_ref), never from the product.  include/rdoom.h has the contract: cell (cx, cy) covers columns
[cx*fx, cx*fx + fx) and rows [cy*fy, cy*fy + fy), leftover columns and rows belong to no cell, top_down reverses the output rows
only.  A helper, not a test."""
import numpy as np

OBS_RGB8, OBS_RGB8_PLANAR, OBS_GRAY8, OBS_DEPTH_MIN = 1, 2, 3, 4
FACTORS = (1, 2, 4, 8)


def factors(factor):
    fx, fy = (factor, factor) if isinstance(factor, (int, np.integer)) else factor
    assert fx in FACTORS and fy in FACTORS, factor
    return int(fx), int(fy)


def cells(a, fx, fy):
    """(n, H, W, ...) -> (n, oh, ow, fy * fx, ...): the pixels of every cell, the leftover columns and rows cropped"""
    n, h, w = a.shape[:3]
    oh, ow = h // fy, w // fx
    assert oh > 0 and ow > 0
    rest = a.shape[3:]
    a = a[:, :oh * fy, :ow * fx].reshape((n, oh, fy, ow, fx) + rest)
    a = np.moveaxis(a, 2, 3)  # (n, oh, ow, fy, fx, ...)
    return a.reshape((n, oh, ow, fy * fx) + rest)


def mean_rgb(rgb, factor):
    """(n, H, W, 3) uint8 -> (n, oh, ow, 3) uint8: (2 S + n) / (2 n) in uint32 -- the exact mean, a half rounds up"""
    fx, fy = factors(factor)
    s = cells(np.asarray(rgb, np.uint8), fx, fy).astype(np.uint32).sum(axis=3, dtype=np.uint32)
    n = np.uint32(fx * fy)
    return ((np.uint32(2) * s + n) // (np.uint32(2) * n)).astype(np.uint8)


def gray(rgb, factor):
    """(n, H, W, 3) uint8 -> (n, oh, ow) uint8: (77 S_r + 150 S_g + 29 S_b + 128 n) / (256 n) in uint32"""
    fx, fy = factors(factor)
    s = cells(np.asarray(rgb, np.uint8), fx, fy).astype(np.uint32).sum(axis=3, dtype=np.uint32)
    n = np.uint32(fx * fy)
    v = np.uint32(77) * s[..., 0] + np.uint32(150) * s[..., 1] + np.uint32(29) * s[..., 2] + np.uint32(128) * n
    return (v // (np.uint32(256) * n)).astype(np.uint8)


def depth_min(depth, factor):
    """(n, H, W) float32 -> (n, oh, ow) float32: the smallest depth of the cell, starting at +inf; a NaN is never taken"""
    fx, fy = factors(factor)
    c = cells(np.asarray(depth, np.float32), fx, fy)
    start = np.full(c.shape[:3] + (1,), np.inf, np.float32)
    return np.fmin.reduce(np.concatenate([start, c], axis=3), axis=3).astype(np.float32)


def observation(fmt, factor, rgb=None, depth=None, top_down=False):
    """one format from the full-size frames it needs (rgb for the colour formats, depth for OBS_DEPTH_MIN)"""
    if fmt == OBS_DEPTH_MIN:
        out = depth_min(depth, factor)
    elif fmt == OBS_GRAY8:
        out = gray(rgb, factor)
    else:
        out = mean_rgb(rgb, factor)
    if top_down:
        out = out[:, ::-1]
    if fmt == OBS_RGB8_PLANAR:
        out = np.moveaxis(out, 3, 1)
    return np.ascontiguousarray(out)


def shape(fmt, width, height, factor):
    fx, fy = factors(factor)
    ow, oh = width // fx, height // fy
    return {OBS_RGB8: (oh, ow, 3), OBS_RGB8_PLANAR: (3, oh, ow)}.get(fmt, (oh, ow))
