"""The test side of the spawn: include/rdoom.h "spawn" restated in numpy -- the generator in Python integers, the table in binary64,
the geometry in np.float32 operations, one per operation of the header, and the sector at a point from tests/sector_ref.py's
restatement -- and the hand-made levels and the players the host and GPU tests share.  Nothing here calls the product's spawn."""
import atexit
import functools
import os
import shutil
import sys
import tempfile

import numpy as np

import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ROOT

F = np.float32
TRIES = 8
RISE = F(0.5)
TWO_PI = F(6.2831855)
PITCH = F(1e-8)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
DEFAULTS = dict(clearance=0.56, max_step=0.24)


def philox(counter, key):
    """Philox4x32-10 in Python integers: counter four words, key two"""
    x0, x1, x2, x3 = counter
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
        p0, p1 = M0 * x0, M1 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & MASK32, (p0 >> 32) ^ x3 ^ k1, p0 & MASK32
    return x0, x1, x2, x3


def draws(seed, p, episode, t):
    """the four draws of try t of player p: binary32, exact, in [0, 1)"""
    words = philox((int(p), int(episode), int(t), 0), (seed & MASK32, (seed >> 32) & MASK32))
    return [F(w >> 8) * F(2.0 ** -24) for w in words]


def table(arrays):
    """the spawn table of World.arrays(): (corners (m, 3, 3) float32, cumulative (m,) float32)"""
    tri, verts = np.asarray(arrays['triangles']).reshape(-1, 4), np.asarray(arrays['verts'], F).reshape(-1, 3)
    corners, cumulative, total = [], [], np.float64(0.0)
    for v1, v2, v3, normal in tri:
        if not verts[normal, 1] > 0:
            continue
        a, b, c = (verts[i].astype(np.float64) for i in (v1, v2, v3))
        area = np.float64(0.5) * abs((b[0] - a[0]) * (c[2] - a[2]) - (b[2] - a[2]) * (c[0] - a[0]))
        if not area > 0:
            continue
        total = total + area
        corners.append(verts[[v1, v2, v3]])
        cumulative.append(F(total))
    return np.array(corners, F).reshape(-1, 3, 3), np.array(cumulative, F)


class Level:
    """what the spawn reads of one level (a World, or a slot of a WorldSet), from its host arrays: the sector tables, the spawn table
    restated from the triangles, and the start"""

    def __init__(self, world, slot=None):
        self.tables = sector_ref.Tables(world, slot)
        self.corners, self.cumulative = table(world.arrays() if slot is None else world.arrays(slot))
        t = world.spawn_table() if slot is None else world.spawn_table(slot)
        self.start_pos, self.start_yaw = np.asarray(t.start_pos, F), F(t.start_yaw)  # (the start is the level's, not the spawn's)


def live(tables, sector, offsets):
    """(floor, ceiling) float32 of sectors `sector` (none of them NONE) for the players of `offsets` ((m, n_objects, 3) or None)"""
    rec = tables.sectors[sector]
    out = []
    for height, obj in ((rec['floor'], rec['floor_id']), (rec['ceiling'], rec['ceiling_id'])):
        off = np.zeros(len(sector), F)
        if offsets is not None:
            ok = (obj != 0) & (obj < offsets.shape[1])
            off[ok] = offsets[np.nonzero(ok)[0], obj[ok], 1]
        out.append((height + off).astype(F))
    return out


def clear_at(level, xz, offsets, clearance):
    """(clear, floor, sector) of the points xz (m, 2) for the players of `offsets`: in a sector, with the clearance"""
    sector = sector_ref.sector_at(level.tables, xz)
    inside = sector != sector_ref.NONE
    floor, ok = np.full(len(xz), np.nan, F), np.zeros(len(xz), bool)
    if inside.any():
        f, g = live(level.tables, sector[inside], offsets[inside] if offsets is not None else None)
        floor[inside] = f
        with np.errstate(invalid='ignore'):
            ok[inside] = (g - f).astype(F) >= F(clearance)
    return ok, floor, sector


def search(cumulative, target):
    """the header's search: the first entry whose cumulative > target, the last when there is none"""
    lo, hi, steps = 0, len(cumulative), 0
    while lo < hi:
        mid = (lo + hi) >> 1
        if cumulative[mid] > target:
            hi = mid
        else:
            lo = mid + 1
        steps += 1
    assert steps <= max(1, int(np.ceil(np.log2(max(1, len(cumulative))))) + 1)
    return min(lo, len(cumulative) - 1)


def candidates(level, seed, players, episodes, t):
    """try t of `players`: (q (m, 3) float32, u3 (m,) float32, entry (m,))"""
    q, u3, entry = np.zeros((len(players), 3), F), np.zeros(len(players), F), np.zeros(len(players), np.int64)
    total = level.cumulative[-1]
    for k, (p, e) in enumerate(zip(players, episodes)):
        u0, u1, u2, u3[k] = draws(seed, p, e, t)
        entry[k] = search(level.cumulative, F(u0 * total))
        a, b, c = level.corners[entry[k]]
        if F(u1 + u2) > F(1):
            u1, u2 = F(F(1) - u1), F(F(1) - u2)
        q[k] = (a + u1 * (b - a).astype(F)).astype(F) + (u2 * (c - a).astype(F)).astype(F)
    return q, u3, entry


def valid(level, q, offsets, margin, clearance, max_step):
    """(valid (m,), floor (m,)) of the candidates q (m, 3) for the players of `offsets`"""
    margin, max_step = F(margin), F(max_step)
    ok, floor, _ = clear_at(level, q[:, [0, 2]], offsets, clearance)
    with np.errstate(invalid='ignore'):
        ok &= np.abs((floor - q[:, 1]).astype(F)) <= max_step
        k = F(margin * F(0.70710677))
        for dx, dz in ((margin, None), (-margin, None), (None, margin), (None, -margin), (k, k), (-k, k), (k, -k), (-k, -k)):
            near = np.stack([q[:, 0] if dx is None else (q[:, 0] + dx).astype(F), q[:, 2] if dz is None else (q[:, 2] + dz).astype(F)], 1)
            c, f, _ = clear_at(level, near, offsets, clearance)
            rise = (f - floor).astype(F)
            ok &= c & (np.abs(rise) <= max_step) & ~((rise > 0) & (rise < (RISE - margin).astype(F)))
    return ok, floor


def default_margin():
    return float(rd.player_config_default()['radius'])


def spawn(levels, states, seed, level_of=None, mask=None, episode=None, offsets=None, margin=None, clearance=0.56, max_step=0.24,
          flags=rd.PLAYER_CLIP, tries=None):
    """levels: a Level, or with level_of (a slot per player) a list of them.  states: PLAYER_STATE records, copied; tries: the
    contents of tries_out before the call (None: zeros).  Returns (states, tries uint32)."""
    states = np.array(states, rd.PLAYER_STATE).reshape(-1)
    n = len(states)
    levels = levels if isinstance(levels, (list, tuple)) else [levels]
    level_of = np.zeros(n, np.int64) if level_of is None else np.asarray(level_of).reshape(-1).astype(np.uint32).astype(np.int64)
    mask = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    episode = np.zeros(n, np.int64) if episode is None else np.asarray(episode).reshape(-1).astype(np.uint32).astype(np.int64)
    tries = np.zeros(n, np.uint32) if tries is None else np.array(tries).reshape(-1).view(np.uint32).copy()
    offsets = None if offsets is None else np.asarray(offsets, F).reshape(n, -1, 3)
    margin = default_margin() if margin is None else margin
    outside = mask & (level_of >= len(levels))
    tries[outside] = 0
    for slot, level in enumerate(levels):
        mine = np.nonzero(mask & (level_of == slot))[0]
        if not len(mine):
            continue
        fresh = rd.player_states(np.repeat(level.start_pos[None], len(mine), 0), level.start_yaw, pitch=PITCH, flags=flags)
        won = np.zeros(len(mine), np.uint32)
        left = np.arange(len(mine))
        for t in range(1, TRIES + 1):
            if not len(left) or not len(level.cumulative):
                break
            who = mine[left]
            q, u3, _ = candidates(level, seed, who, episode[who], t)
            ok, floor = valid(level, q, offsets[who] if offsets is not None else None, margin, clearance, max_step)
            hit = left[ok]
            fresh['pos'][hit, 0], fresh['pos'][hit, 1], fresh['pos'][hit, 2] = q[ok, 0], (floor[ok] + RISE).astype(F), q[ok, 2]
            fresh['yaw'][hit] = (u3[ok] * TWO_PI).astype(F)
            won[hit] = t
            left = left[~ok]
        states[mine] = fresh
        tries[mine] = won
    return states, tries


# ---- the hand-made levels: small enough to check by eye ------------------------------------------------------------------------------
# Each is drawn on tools/mkwad.py's 64-unit grid (0.64 world units a cell) and is two sectors, because a level needs a BSP node.
# World coordinates: x = -wad_y / 100, z = -wad_x / 100.
HAND = ['square', 'thin', 'step', 'low']
CELL = 0.64
_tmp = None


def _hand_levels(mkwad):
    def level(w, h, sectors, fills, thing, jitter=()):
        L = mkwad.GridLevel(w, h)
        ids = [L.add_sector(f, c, 'FLOOR0_1', 'CEIL3_5', 200, wall='STARTAN3') for f, c in sectors]
        for (x0, y0, x1, y1), s in fills:
            L.fill(x0, y0, x1, y1, ids[s])
        L.things.append((thing[0], thing[1], 90, 1, 7))
        for g, d in jitter:
            L.jitter[g] = d
        L.max_tag = 0
        return L
    return [
        # a square room, cells 2..6 both ways (2.56 x 2.56), one height: its two halves are sectors of equal heights
        level(8, 8, [(0, 128), (0, 128)], [((2, 2, 4, 6), 0), ((4, 2, 6, 6), 1)], (3 * 64, 4 * 64)),
        # a corridor 0.32 wide (cells 2..3 with the column x = 3 pulled 32 units in) and four cells long, in two halves
        level(6, 8, [(0, 128), (0, 128)], [((2, 2, 3, 4), 0), ((2, 4, 3, 6), 1)], (2 * 64 + 16, 3 * 64),
              jitter=[((3, y), (-32, 0)) for y in range(2, 7)]),
        # two rooms of 4 x 4 cells side by side, the second 0.5 higher
        level(12, 8, [(0, 160), (50, 210)], [((2, 2, 6, 6), 0), ((6, 2, 10, 6), 1)], (3 * 64, 4 * 64)),
        # the square room with 0.5 of headroom
        level(8, 8, [(0, 50), (0, 50)], [((2, 2, 4, 6), 0), ((4, 2, 6, 6), 1)], (3 * 64, 4 * 64)),
    ]


@functools.lru_cache(maxsize=None)
def hand_wad():
    """the path of an IWAD with the hand-made levels as E1M1 .. E1M4, generated once a process by tools/mkwad.py's own level writer"""
    global _tmp
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import mkwad
    levels = _hand_levels(mkwad)
    saved = mkwad.kat_level
    mkwad.kat_level = lambda: levels.pop(0)  # build_wad writes a ('kat',) spec from kat_level(): here, the next hand-made level
    try:
        data, _ = mkwad.build_wad(1993, specs=[('E1M%d' % (i + 1), ('kat',)) for i in range(len(HAND))])
    finally:
        mkwad.kat_level = saved
    _tmp = tempfile.mkdtemp(prefix='rdoom_spawn_')
    atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    path = os.path.join(_tmp, 'hand.wad')
    with open(path, 'wb') as f:
        f.write(data)
    return path


def hand_world(name, device=False):
    """(wad, World) of a hand-made level"""
    wad = rd.Wad(hand_wad(), META_PATH)
    return wad, wad.build_world(HAND.index(name), device=device)


def blank_states(n, byte=0xA5):
    """n records filled with a byte pattern: what a spawn must overwrite, or leave"""
    return np.frombuffer(bytes([byte]) * (n * rd.PLAYER_STATE.itemsize), rd.PLAYER_STATE).copy()


# ---- the levels of the test IWAD ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real(index):
    """(wad, the host-only World, its Level) of level `index` of the test IWAD: built once, left unchanged"""
    from util import ensure_wad
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(index, device=False)
    return wad, world, Level(world)


def entry_sectors(level):
    """the sector at the centroid of every entry of the level's table"""
    c = level.corners.astype(np.float64).mean(1)
    return sector_ref.sector_at(level.tables, c[:, [0, 2]].astype(F))


@functools.lru_cache(maxsize=None)
def door_case(n=4096, seed=77):
    """E1M4 with one manual door -- the one with the most floor -- raised by hand-written offsets in the games of the odd players only:
    (door sector, offsets (n, n_objects, 3), the reference's (states, tries), the sector of every player)"""
    _, world, level = real(3)
    t = world.triggers()
    sectors = level.tables.sectors
    area = np.diff(np.concatenate([[0.0], level.cumulative.astype(np.float64)]))
    at = entry_sectors(level)
    best = None
    for i in np.nonzero(t['triggers']['special_type'] == 1)[0]:
        e = t['effects'][t['triggers']['effect_start'][i]:t['triggers']['effect_end'][i]]
        if len(e) != 1 or e[0]['first_height_offset'] < 0.9:
            continue
        for s in np.nonzero((sectors['ceiling_id'] == e[0]['object_id']) & (sectors['ceiling'] == sectors['floor']))[0]:
            if best is None or area[at == s].sum() > best[0]:
                best = (area[at == s].sum(), int(s), int(e[0]['object_id']), F(e[0]['first_height_offset']))
    assert best is not None, 'E1M4 has no shut manual door'
    _, door, obj, lift = best
    offsets = np.zeros((n, world.game_objects, 3), F)
    offsets[1::2, obj, 1] = lift
    states, tries = spawn(level, blank_states(n), seed, offsets=offsets)
    return door, offsets, (states, tries), sector_ref.sector_at(level.tables, states['pos'][:, [0, 2]])
