"""The test side of the explored area: tests/area_restatement.c (the contract of include/rdoom.h "explored area" restated as a brute
force -- every ray against every line, nothing culled, every sample in turn into byte-per-cell planes of the whole grid, its own
sincos and its own grid formulas) compiled like the other restatements and loaded through ctypes; a numpy evaluation of the grid
formulas; the kernel's window and band arithmetic restated for the non-vacuity checks; and the cases the host and GPU tests share."""
import ctypes
import os
import threading

import numpy as np

import rust_doom_amd as rd
import world_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'area_restatement.c')
NONE = 0xFFFFFFFF
F = np.float32
_lib = None
_lock = threading.Lock()

# the cases of the GPU comparison: (rays, fov, range, cell)
CASES = [(64, 1.6, 12.0, 0.25), (64, 1.6, 12.0, 0.0625), (200, 2 * np.pi, 40.0, 0.0625), (1, 0.0, 12.0, 0.25)]
WINDOW_WORDS = 4096  # area.hip's LDS window, both planes


class Grid(ctypes.Structure):
    _fields_ = [('ix0', ctypes.c_int32), ('iz0', ctypes.c_int32), ('gw', ctypes.c_uint32), ('gh', ctypes.c_uint32),
                ('pitch', ctypes.c_uint32), ('words', ctypes.c_uint32)]


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [os.path.join(HERE, 'sincos_restatement.h')])
            v, u, f = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
            L.ar_grid.restype = ctypes.c_int
            L.ar_grid.argtypes = [v, u, f, v]
            L.ar_reveal.restype = None
            L.ar_reveal.argtypes = [v, u, v, v, u, v, u, u, u, v, u, f, v, u, f, u, v, u, v, v, v, v, u]
            L.ar_draw.restype = None
            L.ar_draw.argtypes = [v, u, v, v, u, v, u, u, u, u, u, f, ctypes.c_int, ctypes.c_int, f, v, u, v]
            _lib = L
    return _lib


def grid(lines, cell):
    """the restatement's grid of a table, as an rd.AreaGrid"""
    lines = np.ascontiguousarray(lines, rd.MAP_LINE)
    g = Grid()
    assert lib().ar_grid(lines.ctypes.data, len(lines), cell, ctypes.byref(g)) == 1
    return rd.AreaGrid(g.ix0, g.iz0, g.gw, g.gh, g.pitch, g.words)


def grid_numpy(lines, cell):
    """the contract's grid formulas evaluated in numpy float32, on their own"""
    xs = np.concatenate([lines['a'][:, 0], lines['b'][:, 0]]).astype(F)
    zs = np.concatenate([lines['a'][:, 1], lines['b'][:, 1]]).astype(F)
    cx = lambda x: int(np.floor(F(x) / F(cell)))
    ix0, iz0 = cx(xs.min()) - 1, cx(zs.min()) - 1
    gw, gh = cx(xs.max()) + 1 - ix0 + 1, cx(zs.max()) + 1 - iz0 + 1
    pitch = (gw + 31) // 32
    return rd.AreaGrid(ix0, iz0, gw, gh, pitch, gh * pitch)


def _tables(lines, levels):
    ranges, lv, n_slots = None, None, 0
    if levels is not None:
        n_slots = len(lines)
        starts = np.cumsum([0] + [len(t) for t in lines])
        ranges = np.ascontiguousarray(np.stack([starts[:-1], [len(t) for t in lines]], 1).astype(np.uint32))
        tables = lines
        lines = np.concatenate(lines)
        lv = np.ascontiguousarray(np.asarray(levels).reshape(-1).astype(np.uint32))
    else:
        tables = [lines]
    return np.ascontiguousarray(lines, rd.MAP_LINE), tables, ranges, lv, n_slots


def reveal(lines, states, fan, max_range, cell, n_steps=None, offsets=None, levels=None, area=None, stride=None, detail=False, threads=16):
    """the explored area of every player.  lines: a MAP_LINE array, or with `levels` (a slot per player) a list of them, one per
    slot.  area: None (zeroed rows of `stride` words, default the largest grid's) or a uint32 (n, 2, stride) array, which is copied,
    not changed.  Returns a dict: area (n, 2, stride) uint32, new (n, 2) uint32; with detail also limit (n, R) float32 (the T_r),
    free_witness (n, most cells, 2) the first (ray, step) that marked each cell FREE (NONE: none), wall_witness (n, most cells) the
    first ray that marked it WALL."""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    fan = np.ascontiguousarray(fan, np.float32).reshape(-1, 2)
    n, r = len(states), len(fan)
    lines, tables, ranges, lv, n_slots = _tables(lines, levels)
    grids = [grid(t, cell) for t in tables]
    most_words, most_cells = max(g.words for g in grids), max(g.gw * g.gh for g in grids)
    if n_steps is None:
        n_steps = rd.area_steps(max_range, cell)
    n_obj = 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
        n_obj = offsets.shape[1]
    if area is None:
        area = np.zeros((n, 2, most_words if stride is None else stride), np.uint32)
    else:
        area = np.ascontiguousarray(area).view(np.uint32).reshape(n, 2, -1).copy()
    assert area.shape[2] >= most_words
    out = dict(area=area, new=np.zeros((n, 2), np.uint32))
    if detail:
        out.update(limit=np.zeros((n, r), np.float32), free_witness=np.full((n, most_cells, 2), NONE, np.uint32),
                   wall_witness=np.full((n, most_cells), NONE, np.uint32))
    ptr = lambda k: out[k].ctypes.data if k in out else None
    L = lib()

    def run(rng):
        a, b = rng
        L.ar_reveal(lines.ctypes.data, len(lines), ranges.ctypes.data if ranges is not None else None,
                    lv.ctypes.data if lv is not None else None, n_slots, states.ctypes.data, n, a, b - a, fan.ctypes.data, r, max_range,
                    offsets.ctypes.data if offsets is not None else None, n_obj, cell, n_steps, area.ctypes.data, area.shape[2],
                    out['new'].ctypes.data, ptr('limit'), ptr('free_witness'), ptr('wall_witness'), most_cells)
    world_ref._chunked(run, n, threads)
    return out


def draw(lines, states, area, cell, width, height, scale, rotate=False, top_down=False, levels=None, threads=16):
    """the maps drawn through `area` (n, 2, stride): a uint8 (n, height, width) array"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    n = len(states)
    lines, _, ranges, lv, n_slots = _tables(lines, levels)
    area = np.ascontiguousarray(area).view(np.uint32).reshape(n, 2, -1)
    out = np.full((n, height, width), 0xEE, np.uint8)
    L = lib()

    def run(rng):
        a, b = rng
        L.ar_draw(lines.ctypes.data, len(lines), ranges.ctypes.data if ranges is not None else None, lv.ctypes.data if lv is not None else None,
                  n_slots, states.ctypes.data, n, a, b - a, width, height, scale, int(rotate), int(top_down), cell, area.ctypes.data,
                  area.shape[2], out.ctypes.data)
    world_ref._chunked(run, n, threads)
    return out


def popcount(words):
    """the set bits of each (player, plane) row of an (n, 2, stride) array: (n, 2) uint32"""
    words = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(words.view(np.uint8), axis=-1).reshape(words.shape[0], words.shape[1], -1).sum(2).astype(np.uint32)


def sincos(x):
    """the project's sincos in numpy float32, operation for operation (csrc/hip/sincos_rd.hpp, as tests/sincos_restatement.h writes
    it out), of a scalar or an array: (s, c).  The quadrant is taken as gfx950's conversion gives it -- saturated at INT_MIN and
    INT_MAX, 0 for a NaN -- so every bit pattern has a result."""
    x = np.asarray(x, F)
    with np.errstate(all='ignore'):  # (inf and NaN go through like any argument)
        k = np.floor(x * F(0.636619772) + F(0.5))
        r = ((x - k * F(1.5703125)) - k * F(4.837512969970703125e-4)) - k * F(7.54978995489188216e-8)
        z = r * r
        ps = ((F(-1.9515295891e-4) * z + F(8.3321608736e-3)) * z - F(1.6666654611e-1)) * z * r + r
        pc = ((F(2.443315711809948e-5) * z - F(1.388731625493765e-3)) * z + F(4.166664568298827e-2)) * z * z - F(0.5) * z + F(1.0)
        in_range = np.abs(k) < F(2147483648.0)  # (false for a NaN)
        q = np.where(in_range, np.where(in_range, k, F(0.0)).astype(np.int64) & 3, np.where(k >= F(2147483648.0), 3, 0))
        s = np.select([q == 0, q == 1, q == 2], [ps, pc, -ps], -pc)
        c = np.select([q == 0, q == 1, q == 2], [pc, -ps, -pc], ps)
    return (F(s), F(c)) if x.ndim == 0 else (s, c)


def bands(g, cell, states, fan, max_range):
    """how many bands area.hip's window formula (its header comment and axis_window) gives each player for a fan of at most 256
    rays, in numpy float32: the rows between the cells of pos.z -+ the largest |vel.z|, clipped to the grid, the word columns
    between those of pos.x -+ the largest |vel.x|, and WINDOW_WORDS / 2 / columns rows to a band"""
    fan = np.asarray(fan, F).reshape(-1, 2)
    assert len(fan) <= 256
    cx = lambda x: int(np.floor(F(x) / F(cell)))
    out = []
    for st in np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1):
        s, c = sincos(st['yaw'])
        vx = (c * fan[:, 0] + (-s) * fan[:, 1]) * F(max_range)
        vz = ((-s) * fan[:, 0] + (-c) * fan[:, 1]) * F(max_range)
        ax, az = np.abs(vx).max(), np.abs(vz).max()
        px, pz = F(st['pos'][0]), F(st['pos'][2])
        c_lo, c_hi = max(cx(px - ax) - g.ix0, 0), min(cx(px + ax) - g.ix0, g.gw - 1)
        r_lo, r_hi = max(cx(pz - az) - g.iz0, 0), min(cx(pz + az) - g.iz0, g.gh - 1)
        if c_lo > c_hi or r_lo > r_hi:
            out.append(0)
            continue
        band_rows = (WINDOW_WORDS // 2) // ((c_hi >> 5) - (c_lo >> 5) + 1)
        out.append((r_hi - r_lo + band_rows) // band_rows)
    return np.array(out)


def crossed64(o, q, a, b, slack):
    """float64: which of the segments a[k] -> b[k] the segment o -> q crosses, more than `slack` world units away from o, from q
    and from the ends of a -> b"""
    cross = lambda ax, az, bx, bz: ax * bz - az * bx
    d, v, w = b - a, q - o, a - o
    den = cross(v[0], v[1], d[:, 0], d[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        t = cross(w[:, 0], w[:, 1], d[:, 0], d[:, 1]) / den
        u = cross(w[:, 0], w[:, 1], v[0], v[1]) / den
        along, length = np.hypot(*v), np.hypot(d[:, 0], d[:, 1])
        return (den != 0) & (t * along > slack) & (t * along < along - slack) & (u * length > slack) & (u * length < length - slack)


def distance64(q, a, b):
    """float64: the distance of point q from each of the segments a[k] -> b[k]"""
    d = b - a
    on = np.clip(((q - a) * d).sum(1) / np.maximum((d * d).sum(1), 1e-300), 0, 1)
    return np.hypot(*(q - (a + on[:, None] * d)).T)
