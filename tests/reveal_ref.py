"""The test side of the seen lines: tests/reveal_restatement.c (the contract of include/rdoom.h "seen lines" restated as a brute
force -- every ray against every line, twice, nothing culled, its own sincos) compiled like the other restatements and loaded
through ctypes; the expected maps drawn through a set (automap_ref.draw on the rows of the table that are seen or flagged
LINE_MAPPED); and the fans and players the host and GPU tests share."""
import ctypes
import os
import threading

import numpy as np

import automap_ref
import rust_doom_amd as rd
import world_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'reveal_restatement.c')
STOP_RANGE, STOP_ONE_SIDED, STOP_TWO_SIDED = 0, 1, 2
NO_WITNESS = 0xFFFFFFFF
_lib = None
_lock = threading.Lock()

# the fans of the GPU comparison: (rays, fov, range)
FANS = [(64, 1.6, 12.0), (200, 2 * np.pi, 40.0), (1, 0.0, 12.0)]
# the fan that takes the sight pass (sight.hpp) twice: a pass of 256 rays, then one of 3 rays that point backwards -- 85 slices of the
# list and a thread without one -- for 16 players of E1M1, whose 713 lines fill the list in three chunks
TAIL_PLAYERS, TAIL_RANGE = 16, 12.0


def tail_fan():
    return np.concatenate([rd.map_fan(256, 1.6), -rd.map_fan(3, 1.0)])


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [os.path.join(HERE, 'sincos_restatement.h')])
            v, u = ctypes.c_void_p, ctypes.c_uint32
            L.rv_reveal.restype = None
            L.rv_reveal.argtypes = [v, u, v, v, u, v, u, u, u, v, u, ctypes.c_float, v, u, v, u, v, v, v, v, v, v, u]
            _lib = L
    return _lib


def words_of(n_lines):
    return (int(n_lines) + 31) // 32


def reveal(lines, states, fan, max_range, offsets=None, levels=None, seen=None, stride=None, detail=False, threads=16):
    """the seen lines of every player.  lines: a MAP_LINE array, or with `levels` (a slot per player) a list of them, one per slot.
    seen: None (zeroed rows of `stride` words, default the largest table's) or a uint32 (n, stride) array, which is copied, not
    changed.  Returns a dict: seen (n, stride) uint32, new (n,) uint32; with detail also limit (n, R) float32 (the T_r), stop
    (n, R) uint8 (STOP_*), marks (n, R) uint32 (lines the ray sees), witness_ray / witness_t (n, most lines): the first ray that
    sees each line (NO_WITNESS: none) and its t."""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    fan = np.ascontiguousarray(fan, np.float32).reshape(-1, 2)
    n, r = len(states), len(fan)
    ranges, lv, n_slots = None, None, 0
    if levels is not None:
        n_slots = len(lines)
        most = max(len(t) for t in lines)
        starts = np.cumsum([0] + [len(t) for t in lines])
        ranges = np.ascontiguousarray(np.stack([starts[:-1], [len(t) for t in lines]], 1).astype(np.uint32))
        lines = np.concatenate(lines)
        lv = np.ascontiguousarray(np.asarray(levels).reshape(-1).astype(np.uint32))
    else:
        most = len(lines)
    lines = np.ascontiguousarray(lines, rd.MAP_LINE)
    n_obj = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
        n_obj = offsets.shape[1]
    if seen is None:
        seen = np.zeros((n, words_of(most) if stride is None else stride), np.uint32)
    else:
        seen = np.ascontiguousarray(seen).view(np.uint32).reshape(n, -1).copy()
    assert seen.shape[1] >= words_of(most)
    out = dict(seen=seen, new=np.zeros(n, np.uint32))
    if detail:
        out.update(limit=np.zeros((n, r), np.float32), stop=np.zeros((n, r), np.uint8), marks=np.zeros((n, r), np.uint32),
                   witness_ray=np.full((n, most), NO_WITNESS, np.uint32), witness_t=np.zeros((n, most), np.float32))
    ptr = lambda k: out[k].ctypes.data if k in out else None
    L = lib()

    def run(rng):
        a, b = rng
        L.rv_reveal(lines.ctypes.data, len(lines), ranges.ctypes.data if ranges is not None else None,
                    lv.ctypes.data if lv is not None else None, n_slots, states.ctypes.data, n, a, b - a, fan.ctypes.data, r, max_range,
                    offsets.ctypes.data if offsets is not None else None, n_obj, seen.ctypes.data, seen.shape[1], out['new'].ctypes.data,
                    ptr('limit'), ptr('stop'), ptr('marks'), ptr('witness_ray'), ptr('witness_t'), most)
    world_ref._chunked(run, n, threads)
    return out


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).reshape(len(words), -1).sum(1).astype(np.uint32)


def blocking(lines, offsets=None):
    """which lines block sight for one player (offsets: None or (n_objects, 3)), from the table alone, in numpy"""
    def live(side, what):
        h = lines[side][what].astype(np.float32)
        if offsets is None:
            return h
        ids = lines[side][what + '_id']
        by = np.where((ids != 0) & (ids < len(offsets)), np.asarray(offsets, np.float32)[np.minimum(ids, len(offsets) - 1), 1], np.float32(0))
        return (h + by).astype(np.float32)
    two = (lines['front']['present'] == 1) & (lines['back']['present'] == 1)
    lo = np.maximum(live('front', 'floor'), live('back', 'floor'))
    hi = np.minimum(live('front', 'ceiling'), live('back', 'ceiling'))
    return ~two | ~(hi > lo)


def draw_seen(lines, states, seen, offsets=None, levels=None, **kw):
    """the maps drawn through the sets: player p's is automap_ref.draw on the rows of its level's table whose bit is set in row p
    of `seen` or that carry LINE_MAPPED.  lines / levels as for reveal; a slot outside the set: an all-zero map"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    seen = np.ascontiguousarray(seen).view(np.uint32).reshape(len(states), -1)
    out = []
    for p in range(len(states)):
        table = lines
        if levels is not None:
            if levels[p] >= len(lines):
                v = automap_ref.view(**kw)
                out.append(np.zeros((v.height, v.width), np.uint8))
                continue
            table = lines[int(levels[p])]
        keep = rd.unpack_seen(seen[p], len(table)) | ((table['flags'] & rd.LINE_MAPPED) != 0)
        off = None if offsets is None else offsets[p:p + 1]
        out.append(automap_ref.draw(table[keep], states[p:p + 1], off, threads=1, **kw)[0])
    return np.stack(out)


def random_offsets(rng, n, n_objects):
    """per-player object offsets that shut, open and half-open doors and move lifts: y from a few values, most of them 0"""
    off = np.zeros((n, n_objects, 3), np.float32)
    off[:, 1:, 1] = rng.choice(np.array([0.0, 0.0, 0.0, 0.72, 1.28, -0.64, -0.08], np.float32), (n, n_objects - 1))
    return off
