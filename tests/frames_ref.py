"""The test side of the player cameras: tests/frames_restatement.c (the device camera restated on world_restatement.c's sincos twin)
compiled with gcc -O2 -ffp-contract=off -fno-fast-math and loaded through ctypes, like tests/world_ref.py."""
import ctypes
import os
import threading

import numpy as np

import rust_doom_amd as rd
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'frames_restatement.c')
_lib = None
_lock = threading.Lock()


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [os.path.join(HERE, 'world_restatement.c'), os.path.join(HERE, 'sincos_restatement.h')])
            L.fr_cameras.restype = None
            L.fr_cameras.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p]
            L.fr_sky_angles.restype = None
            L.fr_sky_angles.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
            _lib = L
    return _lib


def projection(width, height):
    """the camera's projection (rdoom_pose_from_player's: it does not depend on the player)"""
    return np.ascontiguousarray(rd.pose_from_player((0.0, 0.0, 0.0), 0.0, 0.0, width, height)['projection'], np.float32)


def cameras(states, width, height, time=0.0, offsets=None):
    """(POSE array, (n, n_objects, 16) modelviews or None) as the device computes them"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    n = len(states)
    proj = projection(width, height)
    poses = np.zeros(n, rd.POSE)
    mvs, n_obj = None, 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32)
        n_obj = offsets.shape[1]
        mvs = np.zeros((n, n_obj, 16), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    lib().fr_cameras(p(states), n, p(proj), time, p(offsets), n_obj, p(poses), p(mvs))
    return poses, mvs


def sky_angles(projection_, modelviews):
    """per (.., 16) modelview: (host path's atan2f angle, correctly rounded angle), float32 arrays of the leading shape"""
    m = np.ascontiguousarray(modelviews, np.float32)
    shape = m.shape[:-1]
    m = m.reshape(-1, 16)
    host, cr = np.zeros(len(m), np.float32), np.zeros(len(m), np.float32)
    proj = np.ascontiguousarray(projection_, np.float32)
    lib().fr_sky_angles(proj.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p), len(m),
                        host.ctypes.data_as(ctypes.c_void_p), cr.ctypes.data_as(ctypes.c_void_p))
    return host.reshape(shape), cr.reshape(shape)
