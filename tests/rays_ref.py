"""The test side of the ray cast: tests/rays_restatement.c (the contract of include/rdoom.h "ray casts" restated on
world_restatement.c's world and traversal, with a camera eye and quaternion of its own) compiled with world_ref.py's flags
(gcc -O2 -ffp-contract=off -fno-fast-math) and loaded through ctypes."""
import ctypes
import os
import threading

import numpy as np

import rust_doom_amd as rd
import world_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'rays_restatement.c')
NO_HIT = 0xFFFFFFFF
_lib = None
_lock = threading.Lock()


def lib():
    """the restatement as a shared library, its prototypes declared"""
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [world_ref.SRC, os.path.join(HERE, 'sincos_restatement.h')])
            v, u = ctypes.c_void_p, ctypes.c_uint32
            L.ry_cast.restype = None
            L.ry_cast.argtypes = [v, v, u, u, u, v, u, ctypes.c_float, v, u, v, v, v, v, v, v]
            L.ry_eyes.restype = None
            L.ry_eyes.argtypes = [v, u, v, v]
            L.ry_view_translations.restype = None
            L.ry_view_translations.argtypes = [v, u, v]
            _lib = L
    return _lib


def eyes(states):
    """(eyes (n, 3), quaternions (n, 4) as s, x, y, z) of PLAYER_STATE records"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    e, q = np.zeros((len(states), 3), np.float32), np.zeros((len(states), 4), np.float32)
    lib().ry_eyes(states.ctypes.data, len(states), e.ctypes.data, q.ctypes.data)
    return e, q


def view_translations(states):
    """(n, 3): the translation column of the view matrix of each player's camera, computed from this restatement's own eye"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    out = np.zeros((len(states), 3), np.float32)
    lib().ry_view_translations(states.ctypes.data, len(states), out.ctypes.data)
    return out


def cast(ref_world, states, dirs, max_range, offsets=None, threads=16):
    """the rays of every player through a world_ref.RefWorld (rays_restatement.c includes world_restatement.c, so it reads
    the handle's struct as the library that built it wrote it).  Returns a dict: frac (n, R) float32, hit (n, R) uint32, raw_time / raw_hit (the
    fold before the time <= 1 cut), origin / vel (n, R, 3)."""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n, r = len(states), len(dirs)
    out = dict(frac=np.zeros((n, r), np.float32), hit=np.zeros((n, r), np.uint32), raw_time=np.zeros((n, r), np.float32),
               raw_hit=np.zeros((n, r), np.uint32), origin=np.zeros((n, r, 3), np.float32), vel=np.zeros((n, r, 3), np.float32))
    n_obj = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
        n_obj = offsets.shape[1]
    L = lib()

    def run(rng):
        a, b = rng
        L.ry_cast(ref_world.h.value, states.ctypes.data, n, a, b - a, dirs.ctypes.data, r, max_range,
                  offsets.ctypes.data if offsets is not None else None, n_obj, out['frac'].ctypes.data, out['hit'].ctypes.data,
                  out['raw_time'].ctypes.data, out['raw_hit'].ctypes.data, out['origin'].ctypes.data, out['vel'].ctypes.data)
    world_ref._chunked(run, n, threads)
    return out


# ---- the inputs the host and GPU tests share ------------------------------------------------------------------------------------
PITCH_LIMIT = float(np.float32(1.57079637) - np.float32(1e-2))  # the step's clamp (player.rs:196-201)
PITCHES = (1e-8, 0.3, -0.45, PITCH_LIMIT, -PITCH_LIMIT)
RANGES = (5.0, 30.0, 1000.0)


def odd_table():
    """a second direction table: pitched and unnormalised directions, one of them backwards, one straight down"""
    t = [(0.0, 0.0, -1.0), (0.3, 0.2, -2.5), (-1.5, -0.4, -1.0), (0.02, 0.9, -0.3), (0.0, -3.0, -0.001), (0.7, 0.1, 0.6),
         (-0.25, 0.05, -0.125)]
    return np.array(t, np.float32)


def players(built, seed, count=None, height=None):
    """PLAYER_STATE records standing at rest height above the level's floor centroids (all of them, or `count` drawn with
    replacement), with seeded yaws kept at least 0.02 rad away from the multiples of pi/2 and pitches cycling through PITCHES"""
    if height is None:
        height = float(rd.player_config_default()['height'])
    cents = np.asarray(built.floor_centroids(), np.float32).reshape(-1, 3)
    rng = np.random.RandomState(seed)
    if count is not None:
        cents = cents[rng.randint(0, len(cents), count)]
    n = len(cents)
    quarter = rng.randint(0, 8, n) - 4
    yaws = (quarter + rng.uniform(0.02 / (np.pi / 2), 1.0 - 0.02 / (np.pi / 2), n)) * (np.pi / 2)
    pos = cents.copy()
    pos[:, 1] += np.float32(height)
    pitches = np.array([PITCHES[i % len(PITCHES)] for i in range(n)], np.float32)
    return rd.player_states(pos, yaws.astype(np.float32), pitch=pitches)


# ---- the central ray against the depth plane of the same players' frames ----------------------------------------------------------
DEPTH_FRAME = (321, 201)  # odd, so that the central ray (-z) goes through the centre of pixel (160, 100)
DEPTH_RANGE = 30.0


def depth_candidates(ref_world, states, max_range=DEPTH_RANGE):
    """(indices of the players to sample, the central ray's distance per player): by the restatement alone, the players whose
    central ray ends on a static triangle within max_range"""
    out = cast(ref_world, states, np.array([[0.0, 0.0, -1.0]], np.float32), max_range)
    static = out['hit'][:, 0] < ref_world.n_static_triangles
    return np.nonzero(static)[0], (out['frac'][:, 0].astype(np.float64) * max_range)


def depth_agreement(distance, depth, label):
    """distance: the central ray's length per sampled player (+inf: nothing within range); depth, label: (n, H, W) planes of the
    same players' frames, bottom-up or top-down alike.  Returns (usable, matches, nearer): usable marks the frames whose centre
    pixel shows a flat or a wall of the static level (label kind 0 / 1, object id 0); matches those where the ray's distance
    equals the centre depth within 1e-3 relative plus the depth change across one pixel (the largest difference to the four
    neighbouring pixels); nearer those where the ray ends NEARER than that -- which must not happen, while further may: the
    collision geometry omits the non-blocking walls the frame shows.  The tolerance is geometric slack for "same surface" (the
    ray samples a point, the pixel a footprint), not a figure tuned to the library."""
    n, h, w = depth.shape
    cy, cx = h // 2, w // 2
    d0 = depth[:, cy, cx].astype(np.float64)
    lab = label[:, cy, cx].astype(np.int64)
    usable = ((lab & 0xF) <= 1) & ((lab >> 4) == 0) & (lab != 0xFFFF) & np.isfinite(d0)
    around = np.stack([depth[:, cy - 1, cx], depth[:, cy + 1, cx], depth[:, cy, cx - 1], depth[:, cy, cx + 1]], 1).astype(np.float64)
    with np.errstate(invalid='ignore'):  # (inf - inf next to the sky)
        diff = np.abs(around - d0[:, None])
    slack = np.where(np.isfinite(diff), diff, 0.0).max(1)
    tol = 1e-3 * np.abs(np.where(usable, d0, 0.0)) + slack
    dist = np.asarray(distance, np.float64)
    matches = usable & (np.abs(dist - np.where(usable, d0, 0.0)) <= tol)
    nearer = usable & (dist < np.where(usable, d0, 0.0) - tol)
    return usable, matches, nearer
