"""The test side of the sectors: tests/sector_restatement.c (the contract of include/rdoom.h "sectors" restated point by point -- every
point from the root through the library's HOST arrays, nothing shared, nothing skipped) compiled like the other restatements and
loaded through ctypes, and the players and views the host and GPU tests share."""
import ctypes
import os
import threading

import numpy as np

import rust_doom_amd as rd
import world_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'sector_restatement.c')
NONE, NONE16 = 0xFFFFFFFF, 0xFFFF
_lib = None
_lock = threading.Lock()


class _Level(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('nodes', 'sectors', 'leaf_sector', 'leaf_edges', 'edges')] + \
               [(k, ctypes.c_uint32) for k in ('n_nodes', 'n_sectors', 'n_leaves', 'n_edges')]


class View(ctypes.Structure):
    _fields_ = [('width', ctypes.c_uint32), ('height', ctypes.c_uint32), ('scale', ctypes.c_float), ('half_width', ctypes.c_float),
                ('marker', ctypes.c_float), ('flags', ctypes.c_uint32)]


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [os.path.join(HERE, 'sincos_restatement.h')])
            v, u = ctypes.c_void_p, ctypes.c_uint32
            L.sr_points.restype = None
            L.sr_points.argtypes = [v, v, u, v]
            L.sr_locate.restype = None
            L.sr_locate.argtypes = [v, u, v, v, u, v, u, v, v, v, u, v]
            L.sr_draw.restype = None
            L.sr_draw.argtypes = [v, u, v, v, u, u, u, v, u, v, v, u, v, v, v]
            _lib = L
    return _lib


class Tables:
    """the host arrays of one level (a World, or a slot of a WorldSet) as the restatement reads them"""

    def __init__(self, world, slot=None):
        arrays = world.arrays() if slot is None else world.arrays(slot)
        self.nodes = np.ascontiguousarray(arrays['nodes'], rd.WORLD_NODE)
        m = world.map_sectors() if slot is None else world.map_sectors(slot)
        self.sectors = np.ascontiguousarray(m.sectors, rd.MAP_SECTOR)
        self.leaf_sector = np.ascontiguousarray(m.leaf_sector, np.uint32)
        self.leaf_edges = np.ascontiguousarray(m.leaf_edges, np.uint32).reshape(-1, 2)
        self.edges = np.ascontiguousarray(m.edges, rd.MAP_EDGE)
        self.n_chunks = len(arrays['chunks'])
        assert rd.WORLD_NODE.itemsize == 28 and len(self.leaf_sector) == len(self.leaf_edges) == max(1, self.n_chunks)

    def record(self):
        return _Level(self.nodes.ctypes.data, self.sectors.ctypes.data, self.leaf_sector.ctypes.data, self.leaf_edges.ctypes.data,
                      self.edges.ctypes.data, len(self.nodes), len(self.sectors), len(self.leaf_sector), len(self.edges))


def _records(tables):
    tables = tables if isinstance(tables, (list, tuple)) else [tables]
    return (_Level * len(tables))(*[t.record() for t in tables]), len(tables)


def words_of(n_sectors):
    return (int(n_sectors) + 31) // 32


def sector_at(tables, xz):
    """the sector at each world point (n, 2) of one level: uint32, NONE in the void"""
    xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
    out = np.zeros(len(xz), np.uint32)
    rec, _ = _records(tables)
    lib().sr_points(ctypes.addressof(rec), xz.ctypes.data, len(xz), out.ctypes.data)
    return out


def _players(states, offsets, levels):
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    n, n_obj = len(states), 0
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
        n_obj = offsets.shape[1]
    lv = None if levels is None else np.ascontiguousarray(np.asarray(levels).reshape(-1).astype(np.uint32))
    return states, n, offsets, n_obj, lv


def locate(tables, states, offsets=None, levels=None, visited=None, stride=None):
    """tables: a Tables, or with `levels` (a slot per player) a list of them.  visited: None (zeroed rows of `stride` words, default
    the largest table's) or a uint32 (n, stride) array, which is copied.  Returns a dict: sector (n,) uint32, heights (n, 2) float32,
    visited (n, stride) uint32, new (n,) uint32."""
    states, n, offsets, n_obj, lv = _players(states, offsets, levels)
    rec, n_slots = _records(tables)
    most = max(t.n_sectors for t in rec)
    if visited is None:
        visited = np.zeros((n, words_of(most) if stride is None else stride), np.uint32)
    else:
        visited = np.ascontiguousarray(visited).view(np.uint32).reshape(n, -1).copy()
    assert visited.shape[1] >= words_of(most)
    out = dict(sector=np.zeros(n, np.uint32), heights=np.zeros((n, 2), np.float32), visited=visited, new=np.zeros(n, np.uint32))
    lib().sr_locate(ctypes.addressof(rec), n_slots, lv.ctypes.data if lv is not None else None, states.ctypes.data, n,
                    offsets.ctypes.data if offsets is not None else None, n_obj, out['sector'].ctypes.data, out['heights'].ctypes.data,
                    visited.ctypes.data, visited.shape[1], out['new'].ctypes.data)
    return out


def view(width, height, scale, rotate=False, top_down=False):
    return View(int(width), int(height), scale, 0.0, 0.0, (rd.MAP_ROTATE if rotate else 0) | (rd.MAP_TOP_DOWN if top_down else 0))


def draw(tables, states, offsets=None, levels=None, visited=None, threads=16, **kw):
    """the three planes of every player: (sector (n, h, w) uint16, floor, ceiling (n, h, w) float32).  kw: view()'s arguments"""
    v = view(**kw)
    states, n, offsets, n_obj, lv = _players(states, offsets, levels)
    rec, n_slots = _records(tables)
    stride = 0
    if visited is not None:
        visited = np.ascontiguousarray(visited).view(np.uint32).reshape(n, -1)
        stride = visited.shape[1]
    sector = np.zeros((n, v.height, v.width), np.uint16)
    floor, ceiling = np.zeros(sector.shape, np.float32), np.zeros(sector.shape, np.float32)
    L = lib()

    def run(rng):
        a, b = rng
        L.sr_draw(ctypes.addressof(rec), n_slots, lv.ctypes.data if lv is not None else None, states.ctypes.data, n, a, b - a,
                  offsets.ctypes.data if offsets is not None else None, n_obj, ctypes.addressof(v),
                  visited.ctypes.data if visited is not None else None, stride, sector.ctypes.data, floor.ctypes.data, ceiling.ctypes.data)
    world_ref._chunked(run, n, threads)
    return sector, floor, ceiling


def map_to_world(pts):
    """(wad_x, wad_y) map units -> (x, z) world, float32: the inverse of mapcheck.world_to_map"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    return np.stack([-pts[:, 1] / 100.0, -pts[:, 0] / 100.0], 1).astype(np.float32)


def players(wad, index, n, rng, outside=4, nan=2):
    """(states, on_map): n players of level `index` at jittered floor centroids with random yaws; the first on_map = n - outside -
    nan of them are on or near the map, then `outside` far outside it, then `nan` on a NaN (the last one in z, the others in x)"""
    cent = wad.build_level(index).floor_centroids()
    pos = cent[rng.integers(0, len(cent), n)].astype(np.float32)
    pos[:, [0, 2]] += rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
    st = rd.player_states(pos, rng.uniform(-7, 7, n).astype(np.float32))
    on_map = n - outside - nan
    st['pos'][on_map:n - nan, 0] += np.float32(500.0)
    if nan:
        st['pos'][n - nan:, 0] = np.nan
        st['pos'][n - 1, 2] = np.nan
        st['pos'][n - 1, 0] = pos[n - 1, 0]
    return st, on_map


def random_offsets(rng, n, n_objects):
    """per-player object offsets that move floors and ceilings: y from a few values, most of them 0"""
    off = np.zeros((n, n_objects, 3), np.float32)
    if n_objects > 1:
        off[:, 1:, 1] = rng.choice(np.array([0.0, 0.0, 0.0, 0.72, 1.28, -0.64, -0.08], np.float32), (n, n_objects - 1))
    return off


def patched_wad(directory, secret, damaging, level=0):
    """a copy of the synthetic IWAD (whose generator writes no sector of type 9 or 5) in which sector `secret` of level `level` has
    type 9 and sector `damaging` type 5; returns its path"""
    import mapcheck
    from util import ensure_wad
    data, lumps = mapcheck.read_directory(ensure_wad())
    data = bytearray(data)
    marker = mapcheck.level_markers(lumps)[level]
    _, pos, size = next(l for l in lumps[marker + 1:marker + 11] if l[0] == b'SECTORS')
    for sector, kind in ((secret, 9), (damaging, 5)):
        assert sector * 26 < size
        data[pos + sector * 26 + 22:pos + sector * 26 + 24] = int(kind).to_bytes(2, 'little')
    path = os.path.join(str(directory), 'patched.wad')
    with open(path, 'wb') as f:
        f.write(bytes(data))
    return path
