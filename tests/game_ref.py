"""The test side of doors, lifts and exits: tests/game_restatement.c (Level::poll_triggers, the move effects of Level::update and
the tick order, on top of world_restatement.c) compiled like world_ref.py's restatement, and the trigger list restated in Python
from oracle.wad_oracle's level reader and metadata (wad/src/visitor.rs:341-500) -- not from the product."""
import ctypes
import os
import struct
import threading

import numpy as np

import rust_doom_amd as rd
import world_ref
from oracle import wad_oracle as wo
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'game_restatement.c')
F = np.float32
_libs = {}
_lock = threading.Lock()
TYPES = {'WalkOver': rd.TRIGGER_WALK_OVER, 'Push': rd.TRIGGER_PUSH, 'Switch': rd.TRIGGER_SWITCH, 'Gun': rd.TRIGGER_GUN,
         'Any': rd.TRIGGER_ANY}


def census(reset=False):
    """{outcome: count}: what the ticks stepped through lib(census=True) took since the last reset (a table of its own: this
    library carries its own copy of world_restatement.c)"""
    out = world_ref.census_read(lib(census=True))
    if reset:
        lib(census=True).rs_census_reset()
    return out


def lib(census=False):
    """the restatement as a shared library, its prototypes declared; census=True: the build with world_restatement.c's census"""
    with _lock:
        if census not in _libs:
            deps = [world_ref.SRC, os.path.join(HERE, 'sincos_restatement.h')]
            L = restatement_lib(SRC, deps, flags=world_ref.CENSUS_FLAGS, tag=world_ref.CENSUS_TAG) if census else \
                restatement_lib(SRC, deps)
            if census:
                world_ref.declare_census(L)
            L.rs_game_step.restype = None
            L.rs_game_step.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32] * 4 + \
                [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4
            L.rs_object_modelview.restype = None
            L.rs_object_modelview.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
            _libs[census] = L
    return _libs[census]


def _line(a, b):  # Line2f::from_two_points (math/src/line.rs:12-33) in binary32
    dx, dy = F(b[0] - a[0]), F(b[1] - a[1])
    length = F(np.sqrt(F(F(dx * dx) + F(dy * dy))))
    if abs(length) >= F(1e-16):
        return a[0], a[1], F(dx / length), F(dy / length), length
    return a[0], a[1], F(0), F(0), F(0)


def triggers(wad_path, meta_path, index):
    """(triggers TRIGGER, effects MOVE_EFFECT, n_objects) of level `index` as compute_dynamic_sectors builds them"""
    meta = wo.Metadata(meta_path)
    level = wo.Level(wo.Archive(wad_path, meta_path), index)
    trig, effs = [], []
    tags = sorted((s[6], i) for i, s in enumerate(level.sectors) if s[6] > 0)
    if not tags:  # visitor.rs:360-364
        return np.zeros(0, rd.TRIGGER), np.zeros(0, rd.MOVE_EFFECT), 1
    info = {}
    next_id = [1]

    def update(sid, move, out):  # DynamicSectorInfo::update (visitor.rs:168-244)
        d = info.setdefault(sid, wo.DynamicSectorInfo())
        if move is None:
            return
        sector = level.sectors[sid]
        if d.neighbour_heights is None:
            d.neighbour_heights = level.neighbour_heights(sid)
            if d.neighbour_heights is None:
                return
        ff, sf = wo._option_to_heights(move.get('floor'), sector, d.neighbour_heights)
        fc, sc = wo._option_to_heights(move.get('ceiling'), sector, d.neighbour_heights)
        d.floor_range = wo._merge_range(d.floor_range, sector[0], [c for c in (ff, sf) if c is not None])
        d.ceiling_range = wo._merge_range(d.ceiling_range, sector[1], [c for c in (fc, sc) if c is not None])
        if d.ceiling_range is not None and d.ceiling_id == 0:
            d.ceiling_id, next_id[0] = next_id[0], next_id[0] + 1
        if d.floor_range is not None and d.floor_id == 0:
            d.floor_id, next_id[0] = next_id[0], next_id[0] + 1
        speed = F(F(F(move.get('speed', 0)) / F(8.0)) * F(0.7))
        wait = F(move.get('wait', 0))
        for obj, cur, first, second in ((d.floor_id, sector[0], ff, sf), (d.ceiling_id, sector[1], fc, sc)):
            if first is not None:
                out.append((obj, wo.from_wad_height(wo.i16(first - cur)),
                            wo.from_wad_height(wo.i16(second - cur)) if second is not None else F(0), speed, wait,
                            int(second is not None), int(bool(move.get('repeat', False)))))

    for ld in level.linedefs:
        start, end, _, special, tag, _, left = ld
        if special == 0:
            continue
        a, b = level.vertex(start), level.vertex(end)
        if a is None or b is None:
            continue
        m = meta.linedef.get(special)
        if m is not None:
            ttype, flags = TYPES[m['trigger']], (rd.TRIGGER_ONLY_ONCE if m.get('only_once', False) else 0) | \
                (rd.TRIGGER_EXIT if 'exit' in m else 0)
            move = m.get('move')
        else:
            ttype, flags, move = rd.TRIGGER_ANY, rd.TRIGGER_UNIMPLEMENTED, None
        out = []
        if tag == 0:
            side = level.side(left)
            if side is not None and level.sidedefs[side][5] < len(level.sectors):
                update(level.sidedefs[side][5], move, out)
        else:
            for t, sid in tags:
                if t == tag:
                    update(sid, move, out)
        ox, oy, dx, dy, length = _line(a, b)
        trig.append(((ox, oy), (dx, dy), length, ttype, flags, special, len(effs), len(effs) + len(out)))
        effs.extend(out)
    return np.array(trig, rd.TRIGGER), np.array(effs, rd.MOVE_EFFECT), max(1, next_id[0])


class RefGame:
    """N games of the restatement on a RefWorld; state arrays are numpy, advanced by step(); census=True: stepped in the build
    that counts the step's branch outcomes (read them with game_ref.census())"""

    def __init__(self, ref_world, trig, effs, n, n_objects, census=False):
        self.L = lib(census)
        self.w, self.trig, self.effs, self.n, self.n_objects = ref_world, np.ascontiguousarray(trig), np.ascontiguousarray(effs), n, n_objects
        self.order = np.tile(np.arange(len(trig), dtype=np.uint32), (n, 1)).copy()
        self.counts = np.full(n, len(trig), np.uint32)
        self.act = np.zeros((n, n_objects, 4), np.float32)
        self.aflags = np.zeros((n, n_objects), np.uint32)
        self.offsets = np.zeros((n, n_objects, 3), np.float32)

    def step(self, states, inputs, actions=None, config=None, dt=1.0 / 60.0, threads=16):
        """a stepped copy of `states`; dt 0 means 1/60 (include/rdoom.h), as in RefWorld.step"""
        dt = float(np.float32(1.0) / np.float32(60.0)) if dt == 0 else dt
        states = np.array(states, rd.PLAYER_STATE).reshape(-1)
        n = self.n
        inputs = np.ascontiguousarray(inputs, rd.PLAYER_INPUT).reshape(-1, n)
        acts = np.ascontiguousarray(actions, np.uint8).reshape(-1, n) if actions is not None else None
        cfg = np.ascontiguousarray(np.asarray(config if config is not None else rd.player_config_default(), rd.PLAYER_CONFIG).reshape(1))
        p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None

        def run(r):
            a, b = r
            self.L.rs_game_step(ctypes.c_void_p(self.w.h.value), p(self.trig), len(self.trig), p(self.effs), p(states), p(inputs), p(acts),
                               n, a, b - a, len(inputs), p(cfg), dt, p(self.offsets), self.n_objects, p(self.order), p(self.counts),
                               p(self.act), p(self.aflags))
        world_ref._chunked(run, n, threads)
        return states


def object_modelview(pos, yaw, pitch, off):
    out = np.zeros(16, np.float32)
    pos = np.ascontiguousarray(pos, np.float32)
    off = np.ascontiguousarray(off, np.float32)
    lib().rs_object_modelview(ctypes.c_void_p(pos.ctypes.data), F(yaw), F(pitch), ctypes.c_void_p(off.ctypes.data),
                              ctypes.c_void_p(out.ctypes.data))
    return out


# ---- the patched level variant: the specials the synthetic levels lack ---------------------------------------------------------
GUN_SPECIAL = 46  # (a Gun special the synthetic metadata does not define; the patched metadata adds it, opening like special 1)


def patch_linedefs(wad_bytes, level_lump, patches):
    """a copy of the IWAD with LINEDEFS entries of the level whose marker is lump `level_lump` patched: {index: (special, tag)}"""
    data = bytearray(wad_bytes)
    n_lumps, dir_off = struct.unpack_from('<ii', data, 4)
    pos, size = struct.unpack_from('<ii', data, dir_off + 16 * (level_lump + 2))
    name = bytes(data[dir_off + 16 * (level_lump + 2) + 8:dir_off + 16 * (level_lump + 2) + 16]).rstrip(b'\0')
    assert name == b'LINEDEFS', name
    for i, (special, tag) in patches.items():
        assert 14 * i + 14 <= size
        struct.pack_into('<HH', data, pos + 14 * i + 6, special, tag)
    return bytes(data)
