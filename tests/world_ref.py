"""The test side of the collision world: tests/world_restatement.c (an independent binary32 restatement of game::world and
game::player, sharing no code with the product) compiled with gcc -O2 -ffp-contract=off -fno-fast-math and loaded through
ctypes, fed from the product's level walk (rdoom_wad_walk) by a Python visitor."""
import ctypes
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import rust_doom_amd as rd
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'world_restatement.c')
_libs = {}
_lock = threading.Lock()
CENSUS_FLAGS, CENSUS_TAG = ['-DRS_CENSUS'], '_census'  # the build that counts the step's branch outcomes (world_restatement.c)

NODE = np.dtype([('origin', '<f4', 2), ('displace', '<f4', 2), ('length', '<f4'), ('positive', '<i4'), ('negative', '<i4')])
assert NODE == rd.WORLD_NODE


def declare_census(L):
    """the prototypes of a census build's table"""
    L.rs_census_count.restype = ctypes.c_uint32
    L.rs_census_name.restype = ctypes.c_char_p
    L.rs_census_name.argtypes = [ctypes.c_uint32]
    L.rs_census_read.restype = L.rs_census_reset.restype = None
    L.rs_census_read.argtypes = [ctypes.c_void_p]


def census_read(L):
    """{outcome: count} of a census build's table"""
    n = L.rs_census_count()
    counts = np.zeros(n, np.uint64)
    L.rs_census_read(ctypes.c_void_p(counts.ctypes.data))
    return {L.rs_census_name(i).decode(): int(counts[i]) for i in range(n)}


def census(reset=False):
    """{outcome: count}: what the ticks stepped through lib(census=True) took since the last reset"""
    out = census_read(lib(census=True))
    if reset:
        lib(census=True).rs_census_reset()
    return out


def lib(census=False):
    """the restatement as a shared library, its prototypes declared; census=True: the build with the census table, a library of
    its own with the same arithmetic"""
    with _lock:
        if census not in _libs:
            deps = [os.path.join(HERE, 'sincos_restatement.h')]
            L = restatement_lib(SRC, deps, flags=CENSUS_FLAGS, tag=CENSUS_TAG) if census else restatement_lib(SRC, deps)
            if census:
                declare_census(L)
            L.wb_new.restype = ctypes.c_void_p
            for name in ('wb_free', 'wb_leaf_end', 'wb_node_end', 'wb_build', 'wb_counts', 'wb_copy', 'rs_sweep', 'rs_step'):
                getattr(L, name).restype = None
            f = ctypes.c_float
            L.wb_root.argtypes = [ctypes.c_void_p, f, f, f, f, f]
            L.wb_node.argtypes = [ctypes.c_void_p, f, f, f, f, f, ctypes.c_int]
            L.wb_leaf.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.wb_flat.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, f, ctypes.c_int]
            L.wb_flat.restype = None
            L.wb_quad.argtypes = [ctypes.c_void_p, ctypes.c_uint32, f, f, f, f, f, f]
            L.wb_quad.restype = None
            for name in ('wb_free', 'wb_leaf_end', 'wb_node_end', 'wb_build'):
                getattr(L, name).argtypes = [ctypes.c_void_p]
            L.rs_sincos.argtypes = [f, ctypes.POINTER(f), ctypes.POINTER(f)]
            L.rs_sincos.restype = None
            _libs[census] = L
    return _libs[census]


def sincos(x):
    s, c = ctypes.c_float(), ctypes.c_float()
    lib().rs_sincos(ctypes.c_float(x), ctypes.byref(s), ctypes.byref(c))
    return np.float32(s.value), np.float32(c.value)


class _Feeder:
    """LevelVisitor (rd.make_visitor) that forwards the events WorldBuilder listens to, and counts the geometry it sees"""

    def __init__(self, h, L):
        self.h, self.L, self.ok = h, L, True
        self.blocker_quads = self.sky_quads = self.other_quads = 0
        self.flat_vertex_counts = []

    def _line(self, line):
        return [line.origin[0], line.origin[1], line.displace[0], line.displace[1], line.length]

    def visit_bsp_root(self, line):
        self.ok &= bool(self.L.wb_root(self.h, *self._line(line)))

    def visit_bsp_node(self, line, branch):
        self.ok &= bool(self.L.wb_node(self.h, *self._line(line), branch))

    def visit_bsp_leaf(self, branch):
        self.ok &= bool(self.L.wb_leaf(self.h, branch))

    def visit_bsp_leaf_end(self):
        self.L.wb_leaf_end(self.h)

    def visit_bsp_node_end(self):
        self.L.wb_node_end(self.h)

    def _flat(self, p, ceiling):
        self.flat_vertex_counts.append(p.n_vertices)
        self.L.wb_flat(self.h, p.object_id, ctypes.cast(p.vertices, ctypes.c_void_p), p.n_vertices, p.height, ceiling)

    def visit_floor_poly(self, p):
        self._flat(p, 0)

    def visit_ceil_poly(self, p):
        self._flat(p, 1)

    def visit_floor_sky_poly(self, p):
        self._flat(p, 0)

    def visit_ceil_sky_poly(self, p):
        self._flat(p, 1)

    def visit_wall_quad(self, q):
        if q.blocker:
            self.blocker_quads += 1
            self.L.wb_quad(self.h, q.object_id, q.v1[0], q.v1[1], q.v2[0], q.v2[1], q.height_range[0], q.height_range[1])
        else:
            self.other_quads += 1

    def visit_sky_quad(self, q):
        self.sky_quads += 1
        self.L.wb_quad(self.h, q.object_id, q.v1[0], q.v1[1], q.v2[0], q.v2[1], q.height_range[0], q.height_range[1])


class RefWorld:
    """WorldBuilder + World + Player of the restatement, built from `wad`'s level `index` (an rd.Wad); census=True: in the build
    that counts the step's branch outcomes (read them with world_ref.census())"""

    def __init__(self, wad, index, census=False):
        L = self.L = lib(census)
        self.census = census
        self.h = ctypes.c_void_p(L.wb_new())
        self.feed = _Feeder(self.h, L)
        wad.walk(index, self.feed)
        assert self.feed.ok, 'the walk broke one of WorldBuilder\'s asserts'
        L.wb_build(self.h)
        c = (ctypes.c_uint32 * 7)()
        L.wb_counts(self.h, c)
        n_nodes, n_chunks, n_tris, n_static, n_verts, n_dyn, n_objects = list(c)
        self.nodes = np.zeros(n_nodes, NODE)
        self.chunks = np.zeros((n_chunks, 2), np.uint32)
        self.triangles = np.zeros((n_tris, 4), np.uint32)
        self.verts = np.zeros((n_verts, 3), np.float32)
        self.dynamics = np.zeros((n_dyn, 3), np.uint32)
        L.wb_copy(self.h, *[ctypes.c_void_p(a.ctypes.data) for a in (self.nodes, self.chunks, self.triangles, self.verts, self.dynamics)])
        self.n_static_triangles, self.n_objects = n_static, n_objects

    def __del__(self):
        try:
            self.L.wb_free(self.h)
        except Exception:
            pass

    def arrays(self):
        return dict(nodes=self.nodes, chunks=self.chunks, triangles=self.triangles, verts=self.verts, dynamics=self.dynamics,
                    n_static_triangles=self.n_static_triangles, n_objects=self.n_objects)

    def sweep(self, spheres, vels, offsets=None, threads=16):
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        vels = np.ascontiguousarray(vels, np.float32).reshape(-1, 3)
        n = len(spheres)
        out = np.zeros((n, 4), np.float32)
        n_obj = 0
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
            n_obj = offsets.shape[1]

        def run(r):
            a, b = r
            off = ctypes.c_void_p(offsets[a:b].ctypes.data) if offsets is not None else None
            self.L.rs_sweep(self.h, ctypes.c_void_p(spheres[a:b].ctypes.data), ctypes.c_void_p(vels[a:b].ctypes.data), b - a, off, n_obj,
                           ctypes.c_void_p(out[a:b].ctypes.data))
        _chunked(run, n, threads)
        return out

    def step(self, states, inputs, config=None, dt=1.0 / 60.0, offsets=None, threads=16):
        """a stepped copy of `states` (rd.PLAYER_STATE); inputs (n_ticks, n) rd.PLAYER_INPUT; dt 0 means 1/60 (include/rdoom.h)"""
        dt = float(np.float32(1.0) / np.float32(60.0)) if dt == 0 else dt
        states = np.array(states, rd.PLAYER_STATE).reshape(-1)
        n = len(states)
        inputs = np.ascontiguousarray(inputs, rd.PLAYER_INPUT).reshape(-1, n)
        cfg = np.ascontiguousarray(np.asarray(config if config is not None else rd.player_config_default(), rd.PLAYER_CONFIG).reshape(1))
        n_obj = 0
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 3)
            n_obj = offsets.shape[1]

        def run(r):
            a, b = r
            self.L.rs_step(self.h, ctypes.c_void_p(states.ctypes.data), ctypes.c_void_p(inputs.ctypes.data), n, a, b - a, len(inputs),
                          ctypes.c_void_p(cfg.ctypes.data), ctypes.c_float(dt),
                          ctypes.c_void_p(offsets.ctypes.data) if offsets is not None else None, n_obj)
        _chunked(run, n, threads)
        return states


def _chunked(fn, n, threads):
    if n == 0:
        return
    k = max(1, min(threads, n))
    bounds = np.linspace(0, n, k + 1).astype(int)
    ranges = [(int(bounds[i]), int(bounds[i + 1])) for i in range(k) if bounds[i + 1] > bounds[i]]
    if len(ranges) == 1:
        fn(ranges[0])
        return
    with ThreadPoolExecutor(len(ranges)) as ex:  # (ctypes releases the GIL around the calls)
        list(ex.map(fn, ranges))
