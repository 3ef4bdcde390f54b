"""The test side of solid things: tests/solid_restatement.c -- the game step of game_restatement.c written
out again with the contract's thing contact -- compiled like game_ref.py's restatement, a RefGame and a RefWorldSet that step with
things, the metadata lookup of the obstacle bits, and the shared cases of tests/test_solid_host.py.  Nothing here needs torch or a
device."""
import ctypes
import os
import threading

import numpy as np

import game_ref
import rust_doom_amd as rd
import world_ref
import worldset_ref
from util import restatement_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'solid_restatement.c')
F = np.float32
INF = float('inf')
_lib = None
_lock = threading.Lock()


def lib():
    """the restatement as a shared library, its prototypes declared"""
    global _lib
    with _lock:
        if _lib is None:
            L = restatement_lib(SRC, [game_ref.SRC, world_ref.SRC, os.path.join(HERE, 'sincos_restatement.h')])
            v, u, f = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
            L.rs_solid_step.restype = None
            L.rs_solid_step.argtypes = [v, v, u, v, v, v, v, u, u, u, u, v, f, v, u, v, v, v, v, v, u, v, v, u, f, f, v]
            L.rs_thing_contact.restype = ctypes.c_int32
            L.rs_thing_contact.argtypes = [v, u, v, v, f, f, v, v, v, f, v, u, v]
            _lib = L
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _rows(rows):
    """rows of thing bits as contiguous uint32 (None stays None)"""
    return None if rows is None else np.ascontiguousarray(rows).view(np.uint32)


def thing_contact(things, pos, D, body=0.19, world=(INF, 0.0, 0.0, 0.0), solid=None, hidden=None, below=INF, above=INF, offsets=None):
    """the contract's thing contact alone: (thing or -1, time, normal) after the world's contact `world` of a sweep from pos along D"""
    things = np.ascontiguousarray(things, rd.THING).reshape(-1)
    out = np.zeros(4, F)
    w, pos, D = np.asarray(world, F), np.asarray(pos, F), np.asarray(D, F)
    off = None if offsets is None else np.ascontiguousarray(offsets, F).reshape(-1, 3)
    which = lib().rs_thing_contact(_p(things), len(things), _p(_rows(solid)), _p(_rows(hidden)), below, above, _p(w), _p(pos), _p(D), body,
                                   _p(off), 0 if off is None else len(off), _p(out))
    return which, out[0], out[1:]


class SolidGame(game_ref.RefGame):
    """game_ref.RefGame stepped with the things of its level in the way.  things: THING records; solid: the level's row of bits or
    None; the rest per step"""

    def __init__(self, ref_world, trig, effs, n, n_objects, things, solid=None):
        super().__init__(ref_world, trig, effs, n, n_objects)
        self.things = np.ascontiguousarray(things, rd.THING).reshape(-1)
        self.solid = _rows(solid)
        self.bumped = np.full(n, -1, np.int32)

    def step(self, states, inputs, actions=None, config=None, dt=1.0 / 60.0, threads=16, hidden=None, below=INF, above=INF):
        """as RefGame.step; hidden: None or (n, stride) words.  self.bumped keeps the first thing each player slid along"""
        states = np.array(states, rd.PLAYER_STATE).reshape(-1)
        n = self.n
        inputs = np.ascontiguousarray(inputs, rd.PLAYER_INPUT).reshape(-1, n)
        acts = np.ascontiguousarray(actions, np.uint8).reshape(-1, n) if actions is not None else None
        cfg = np.ascontiguousarray(np.asarray(config if config is not None else rd.player_config_default(), rd.PLAYER_CONFIG).reshape(1))
        hidden = _rows(hidden)
        stride = 0 if hidden is None else hidden.reshape(n, -1).shape[1]
        assert hidden is None or stride * 32 >= len(self.things)
        assert self.solid is None or self.solid.size * 32 >= len(self.things)

        def run(r):
            a, b = r
            lib().rs_solid_step(ctypes.c_void_p(self.w.h.value), _p(self.trig), len(self.trig), _p(self.effs), _p(states), _p(inputs),
                                _p(acts), n, a, b - a, len(inputs), _p(cfg), dt, _p(self.offsets), self.n_objects, _p(self.order),
                                _p(self.counts), _p(self.act), _p(self.aflags), _p(self.things), len(self.things), _p(self.solid),
                                _p(hidden), stride, below, above, _p(self.bumped))
        world_ref._chunked(run, n, threads)
        return states


class SolidWorldSet(worldset_ref.RefWorldSet):
    """worldset_ref.RefWorldSet stepped with things: tables[slot] the THING records of the level in `slot`, solid None or
    (levels, stride) words, row `slot` the level's.  The tick of RefWorldSet.step with SolidGame in RefGame's place; bumped as
    SolidGame keeps it, over the whole run"""

    def __init__(self, wad_path, meta_path, indices, levels, tables, solid=None):
        super().__init__(wad_path, meta_path, indices, levels)
        self.tables = [np.ascontiguousarray(t, rd.THING).reshape(-1) for t in tables]
        self.solid = _rows(solid)
        self.bumped = np.full(len(self.levels), -1, np.int32)

    def step(self, states, inputs, actions=None, config=None, dt=1.0 / 60.0, threads=16, hidden=None, below=INF, above=INF):
        states = np.array(states, rd.PLAYER_STATE).reshape(-1)
        n = len(states)
        inputs = np.asarray(inputs, rd.PLAYER_INPUT).reshape(-1, n)
        hidden = _rows(hidden)
        for t in range(len(inputs)):
            exited, requested = np.nonzero(self.stage == 1)[0], np.nonzero(self.stage == 2)[0]
            self.stage[exited] = 2
            for p in requested:
                self.stage[p] = 0
                d = self.dest[self.levels[p]]
                self.levels[p] = d
                self._fresh(d, p)
                pos, yaw = self.starts[d]
                s = states[p]
                s['pos'], s['vel'], s['yaw'], s['pitch'], s['last_height_diff'] = pos, 0.0, yaw, F(1e-8), 0.0
            for slot, g in enumerate(self.games):
                sel = np.nonzero(self.levels == slot)[0]
                if not len(sel):
                    continue
                sub = SolidGame(g.w, g.trig, g.effs, len(sel), g.n_objects, self.tables[slot], None if self.solid is None else self.solid[slot])
                sub.order, sub.counts, sub.act = g.order[sel].copy(), g.counts[sel].copy(), g.act[sel].copy()
                sub.aflags, sub.offsets = g.aflags[sel].copy(), g.offsets[sel].copy()
                sub.bumped = self.bumped[sel].copy()
                before = states[sel].copy()
                before['flags'] &= ~np.uint32(rd.PLAYER_EXITED)
                act = None if actions is None else np.asarray(actions, np.uint8).reshape(-1, n)[t:t + 1, sel]
                after = sub.step(before, inputs[t:t + 1, sel], act, config=config, dt=dt, threads=threads,
                                 hidden=None if hidden is None else hidden.reshape(n, -1)[sel], below=below, above=above)
                fired = (after['flags'] & rd.PLAYER_EXITED) != 0
                after['flags'] |= states[sel]['flags']
                states[sel] = after
                g.order[sel], g.counts[sel], g.act[sel], g.aflags[sel], g.offsets[sel] = sub.order, sub.counts, sub.act, sub.aflags, sub.offsets
                self.bumped[sel] = sub.bumped
                if self.dest[slot] is not None:
                    start = sel[fired & (self.stage[sel] == 0)]
                    self.stage[start] = 1
        return states


# ---- which things are solid: the lookup the header states, from the TOML itself ------------------------------------------------
CATEGORIES = ('decorations', 'weapons', 'powerups', 'artifacts', 'ammo', 'keys', 'monsters')  # the merge order


def obstacle_types(meta_path):
    """{thing_type: obstacle} by first match in merge order, read with tomllib: a later entry of a type never counts"""
    try:
        import tomllib
    except ModuleNotFoundError:  # before Python 3.11: the same parser under its earlier name, as oracle/wad_oracle.py has it
        import tomli as tomllib
    with open(meta_path, 'rb') as f:
        meta = tomllib.load(f)
    out = {}
    for cat in CATEGORIES:
        for entry in meta['things'].get(cat, []):
            out.setdefault(int(entry['thing_type']), bool(entry.get('obstacle', False)))
    return out


def expected_obstacles(things, meta_path):
    """the bool per THING record the header promises: its type's first metadata entry says obstacle = true"""
    types = obstacle_types(meta_path)
    return np.array([types.get(int(t), False) for t in things['thing_type']], bool)


# ---- shared cases --------------------------------------------------------------------------------------------------------------
def make_things(xz, radius=0.2, base=0.0, object_id=0, category=rd.THING_DECORATION):
    """THING records at the (x, z) points: one radius / base / object for all, or one each"""
    xz = np.asarray(xz, F).reshape(-1, 2)
    t = np.zeros(len(xz), rd.THING)
    t['x'], t['z'], t['radius'], t['base'], t['object_id'], t['category'] = xz[:, 0], xz[:, 1], radius, base, object_id, category
    return t


def facing(frm, to):
    """the yaw that looks from frm to to, both (x, z): forward is (-sin yaw, -cos yaw)"""
    d = np.asarray(to, np.float64) - np.asarray(frm, np.float64)
    return np.arctan2(-d[..., 0], -d[..., 1]).astype(F)


def walk_script(n, ticks, seed, strafe_after=40):
    """the fixed script of the obstacle runs: every player walks forward; player p strafes right (p even) or left (p odd) from tick
    strafe_after + p % 16 on, so that one stopped dead at a thing slides round it; every 8th player turns a little each tick"""
    rng = np.random.default_rng(seed)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    p = np.arange(n)[None, :]
    t = np.arange(ticks)[:, None]
    inp['movement'][..., 1] = -1.0
    inp['movement'][..., 0] = np.where(t >= strafe_after + p % 16, np.where(p % 2 == 0, 1.0, -1.0), 0.0)
    inp['look'][..., 0] = np.where(p % 8 == 7, rng.normal(scale=0.01, size=(ticks, n)), 0.0).astype(F)
    return inp


def players_at_things(ref, things, targets, n, seed, dist=(0.6, 1.4)):
    """n players on the floor around the things `targets` (indices, used round-robin), each facing its thing from a random side and
    distance; the ones with no floor under them are dropped.  (states, the thing each one faces)"""
    rng = np.random.default_rng(seed)
    pick = np.asarray(targets)[np.arange(n) % len(targets)]
    ang = rng.uniform(-np.pi, np.pi, n)
    d = rng.uniform(dist[0], dist[1], n)
    centre = np.stack([things['x'][pick], things['z'][pick]], 1).astype(np.float64)
    xz = (centre + np.stack([np.cos(ang), np.sin(ang)], 1) * d[:, None]).astype(F)
    y = worldset_ref.floor_y(ref, xz)
    ok = np.isfinite(y)
    pos = np.stack([xz[:, 0], np.where(ok, y + F(0.25), F(0)), xz[:, 1]], 1).astype(F)
    yaw = facing(xz, centre) + rng.normal(scale=0.08, size=n).astype(F)
    return rd.player_states(pos, yaw)[ok], pick[ok]


def distances(states, things):
    """float64 (n, T) distances in xz from every player's centre to every thing's"""
    px, pz = states['pos'][:, 0].astype(np.float64), states['pos'][:, 2].astype(np.float64)
    return np.hypot(px[:, None] - things['x'].astype(np.float64)[None], pz[:, None] - things['z'].astype(np.float64)[None])


E1M1_PLAYERS, E1M1_TICKS, E1M1_SEED = 64, 120, 0  # seed: chosen so that tests/test_solid_host.py's three conditions hold


def e1m1_case(wad_path, meta_path, n=E1M1_PLAYERS, ticks=E1M1_TICKS, seed=E1M1_SEED):
    """E1M1's own table with the solid rows of the metadata: n players started around its obstacles and steered at them by
    walk_script (those without a floor under them are dropped).  A dict: wad, ref (RefWorld), trig, effs, n_objects, things,
    obstacles (bool), solid ((1, words) int32), states, inputs -- the test-side trigger list, no device"""
    wad = rd.Wad(wad_path, meta_path)
    world = wad.build_world(0, device=False)
    things, obstacles = world.map_things(), world.thing_obstacles()
    ref = world_ref.RefWorld(wad, 0)
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
    states, _ = players_at_things(ref, things, np.nonzero(obstacles)[0], n, seed)
    return dict(wad=wad, ref=ref, trig=trig, effs=effs, n_objects=n_obj, things=things, obstacles=obstacles,
                solid=rd.pack_things([obstacles]), states=states, inputs=walk_script(len(states), ticks, seed + 1))


def e1m1_game(case, things=None, solid='own'):
    """a SolidGame of e1m1_case's players: its own table and solid row, or another table / row (None: every thing solid)"""
    return SolidGame(case['ref'], case['trig'], case['effs'], len(case['states']), case['n_objects'],
                     case['things'] if things is None else things, case['solid'][0] if isinstance(solid, str) else solid)
