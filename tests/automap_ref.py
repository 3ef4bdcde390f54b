"""The test side of the top-down map: tests/automap_restatement.c (the contract of include/rdoom.h "top-down maps" restated as a
brute force over every line for every pixel, with its own sincos) compiled like the other restatements and loaded through
ctypes, and the views the host and GPU tests share."""
import ctypes
import os
import threading

import numpy as np

import rust_doom_amd as rd
import world_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'automap_restatement.c')
_lib = None
_lock = threading.Lock()


class View(ctypes.Structure):
    _fields_ = [('width', ctypes.c_uint32), ('height', ctypes.c_uint32), ('scale', ctypes.c_float), ('half_width', ctypes.c_float),
                ('marker', ctypes.c_float), ('flags', ctypes.c_uint32)]


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [os.path.join(HERE, 'sincos_restatement.h')])
            v, u = ctypes.c_void_p, ctypes.c_uint32
            L.am_draw.restype = None
            L.am_draw.argtypes = [v, u, v, v, u, v, u, u, u, v, u, v, v]
            L.am_classes.restype = None
            L.am_classes.argtypes = [v, u, v, u, u, v]
            L.am_points.restype = None
            L.am_points.argtypes = [v, v, v]
            _lib = L
    return _lib


def view(width, height, scale, half_width=0.75, marker=3.0, rotate=False, show_flat=False, show_hidden=False, top_down=False):
    """the arguments of World.draw_maps as the restatement's view"""
    flags = (rd.MAP_ROTATE if rotate else 0) | (rd.MAP_SHOW_FLAT if show_flat else 0) | (rd.MAP_SHOW_HIDDEN if show_hidden else 0) | \
        (rd.MAP_TOP_DOWN if top_down else 0)
    return View(int(width), int(height), scale, half_width, marker, flags)


def draw(lines, states, offsets=None, levels=None, threads=16, **kw):
    """the maps of every player, (n, height, width) uint8.  lines: a MAP_LINE array (World.map_lines), or with `levels` (a slot
    per player) a list of them, one per slot.  offsets: None or (n, n_objects, 3).  kw: view()'s arguments."""
    v = view(**kw)
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    n = len(states)
    ranges, lv, n_slots = None, None, 0
    if levels is not None:
        n_slots = len(lines)
        starts = np.cumsum([0] + [len(t) for t in lines])
        ranges = np.ascontiguousarray(np.stack([starts[:-1], [len(t) for t in lines]], 1).astype(np.uint32))
        lines = np.concatenate(lines)
        lv = np.ascontiguousarray(np.asarray(levels).reshape(-1).astype(np.uint32))
    lines = np.ascontiguousarray(lines, rd.MAP_LINE)
    n_obj = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
        n_obj = offsets.shape[1]
    out = np.zeros((n, v.height, v.width), np.uint8)
    L = lib()

    def run(rng):
        a, b = rng
        L.am_draw(lines.ctypes.data, len(lines), ranges.ctypes.data if ranges is not None else None,
                  lv.ctypes.data if lv is not None else None, n_slots, states.ctypes.data, n, a, b - a,
                  offsets.ctypes.data if offsets is not None else None, n_obj, ctypes.addressof(v), out.ctypes.data)
    world_ref._chunked(run, n, threads)
    return out


def classes(lines, offsets=None, show_flat=True, show_hidden=True):
    """the class of every line for one player (offsets: None or (n_objects, 3)); 0 where the view does not draw it"""
    lines = np.ascontiguousarray(lines, rd.MAP_LINE)
    out = np.zeros(len(lines), np.uint8)
    n_obj = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 3)
        n_obj = len(offsets)
    flags = (rd.MAP_SHOW_FLAT if show_flat else 0) | (rd.MAP_SHOW_HIDDEN if show_hidden else 0)
    lib().am_classes(lines.ctypes.data, len(lines), offsets.ctypes.data if offsets is not None else None, n_obj, flags, out.ctypes.data)
    return out


def points(state, **kw):
    """(height, width, 2): the world (x, z) of every pixel of one player's map, rows as in the map"""
    v = view(**kw)
    st = np.ascontiguousarray(state, rd.PLAYER_STATE).reshape(1)
    out = np.zeros((v.height, v.width, 2), np.float32)
    lib().am_points(ctypes.addressof(v), st.ctypes.data, out.ctypes.data)
    return out


# ---- the views the GPU comparison runs (tests/test_gpu_automap.py): both sizes, the three scales, every flag on and off, marker 0
# and 3, both half widths -- each value in at least two views, not the full product
VIEWS = [
    dict(width=160, height=120, scale=0.05),
    dict(width=160, height=120, scale=0.12, rotate=True, show_flat=True, half_width=2.5),
    dict(width=160, height=120, scale=0.30, top_down=True, marker=0.0, half_width=0.5),
    dict(width=160, height=120, scale=0.30, rotate=True, top_down=True, show_flat=True),
    dict(width=77, height=53, scale=0.05, rotate=True, top_down=True, half_width=2.5, marker=0.0),
    dict(width=77, height=53, scale=0.12, show_flat=True, half_width=0.5),
    dict(width=77, height=53, scale=0.30, rotate=True),
    dict(width=77, height=53, scale=0.12, top_down=True, show_flat=True, rotate=True, marker=0.0),
]
