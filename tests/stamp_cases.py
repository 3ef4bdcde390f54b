"""What the host and the GPU tests of the solid things on the grid share: one-room levels whose grid has a wanted size (a level
made by tools/mkwad.py in a temporary directory, so that a real world handle has it), thing tables written out by hand with the
cells they close, random tables, and the end-to-end case on E1M1 -- each computed once by tests/stamp_ref.py and left unchanged."""
import functools
import os
import sys
import tempfile

import numpy as np

import flood_ref
import goal_ref
import rust_doom_amd as rd
import sector_ref
import stamp_ref
import walls_ref
from util import META_PATH, ROOT, ensure_wad

F = np.float32
U = np.uint32
INF = F(np.inf)
UNIT = 0.64  # a cell of tools/mkwad.py's authoring grid in world units
BODY, E2E_CELL, E2E_STEP, E2E_SEED = 0.19, 0.125, 0.32, (29, 103)
E1M1_BARRELS = (0, 1, 4, 15, 24, 28, 33)

_tmp = tempfile.TemporaryDirectory(prefix='rdoom_stamp_')


def things_at(points, radius=0.0, base=0.0, object_id=0):
    t = np.zeros(len(points), rd.THING)
    if len(points):
        t['x'], t['z'] = np.asarray(points, F).reshape(-1, 2).T
    t['radius'], t['base'], t['object_id'] = radius, base, object_id
    return t


def bit_rows(rows, stride=1):
    """rows of thing bits from lists of indices: [[0, 2], []] -> a (2, stride) uint32 array"""
    out = np.zeros((len(rows), stride), U)
    for r, row in enumerate(rows):
        for i in row:
            out[r, i // 32] |= U(1) << U(i % 32)
    return out


# ---- one-room levels ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def room_wad(across, down):
    """a Wad of one level: a flat room `across` x `down` authoring cells, x in [-(2 + across) * 0.64, -1.28] and z in
    [-(2 + down) * 0.64, -1.28], floor 0, ceiling 1.28, in two sectors (a level needs a BSP node), with no thing of its own"""
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import mkwad

    def level():
        L = mkwad.GridLevel(down + 4, across + 4)  # the authoring grid's x is the world's z
        a = L.add_sector(0, 128, 'FLOOR0_1', 'CEIL3_5', 255, wall='STARTAN3')
        b = L.add_sector(0, 128, 'FLOOR0_1', 'CEIL3_5', 255, wall='STARTAN3')
        L.fill(2, 2, 3, 2 + across, a)
        L.fill(3, 2, 2 + down, 2 + across, b) if down > 1 else L.fill(2, 3, 3, 2 + across, b)
        L.things.append((2 * mkwad.CELL + 32, 2 * mkwad.CELL + 32, 0, 1, 7))  # the player's start: a marker, not in the thing table
        L.max_tag = 0
        return L

    saved = mkwad.kat_level
    mkwad.kat_level = level
    try:
        data, _ = mkwad.build_wad(1993, specs=[('E1M1', ('kat',))])
    finally:
        mkwad.kat_level = saved
    path = os.path.join(_tmp.name, 'room_%d_%d.wad' % (across, down))
    with open(path, 'wb') as f:
        f.write(data)
    return rd.Wad(path, META_PATH)


def _span(lo, hi, cell):
    with np.errstate(all='ignore'):
        return int(np.floor(F(hi) / F(cell))) - int(np.floor(F(lo) / F(cell))) + 3


@functools.lru_cache(maxsize=None)
def room_of_grid(gw, gh):
    """(wad, host world, cell, grid) of a one-room level whose explored-area grid at `cell` is gw x gh: a search over the room's
    size and the cell with the contract's own formula, checked against rdoom_world_area_grid"""
    for across in range(1, 17):
        for down in range(1, 17):
            if across == 1 and down == 1:
                continue
            for k in range(-30, 31):
                cell = float(F(UNIT * across / (gw - 3 + 0.5) * (1.0 + 0.002 * k))) if gw > 3 else 100.0
                if _span(-(2 + across) * UNIT, -2 * UNIT, cell) == gw and _span(-(2 + down) * UNIT, -2 * UNIT, cell) == gh:
                    wad = room_wad(across, down)
                    host = wad.build_world(0, device=False)
                    grid = host.area_grid(cell)
                    assert (grid.gw, grid.gh) == (gw, gh), (grid, gw, gh)
                    return wad, host, cell, grid
    raise AssertionError('no room has a grid of %d x %d' % (gw, gh))


def flat(n, grid, shape=None, floor=0.0, ceiling=1.28):
    """n rows of flat open planes over the whole extent (the level's grid, or a larger shape)"""
    h, w = shape if shape is not None else (grid.gh, grid.gw)
    return np.full((n, h, w), floor, F), np.full((n, h, w), ceiling, F)


def centre(grid, cell, ix, iz):
    """the centre of cell (ix, iz), as the contract computes it"""
    x, z = goal_ref.centres(grid, cell)
    return float(x[ix]), float(z[iz])


# ---- cases written out by hand --------------------------------------------------------------------------------------------------------
# The grid of room_wad(2, 2) at cell 0.25: 8 x 8 cells from (-12, -12), so that cell (ix, iz) has the centre
# ((ix - 11.5) * 0.25, (iz - 11.5) * 0.25) and every number below is exact in binary32.
HAND_CELL = 0.25
HAND_GRID = stamp_ref.grid_of(-12, -12, 8, 8)
HAND_OBJECTS = 4
WIDE = (0.0, np.inf, np.inf)  # grow, block_below, block_above: the wrapper's default
NARROW = (0.0, 0.25, 0.5)
SHORT = (0.0, float(np.nextafter(F(0.25), F(0))), float(np.nextafter(F(0.5), F(0))))  # a hair inside NARROW's two bounds


def at(ix, iz, dx=0.0, dz=0.0):
    return ((ix - 11.5) * 0.25 + dx, (iz - 11.5) * 0.25 + dz)


def plus(ix, iz, index=0):
    return {(ix, iz): index, (ix - 1, iz): index, (ix + 1, iz): index, (ix, iz - 1): index, (ix, iz + 1): index}


def hand_cases():
    """a list of dicts: name, table, solid / hidden (lists of thing indices, or None), floors ({(ix, iz): floor} over a flat floor
    of 0 under a ceiling of 1.28; a floor of +inf is a void cell with a ceiling of -inf), offsets ({object: y} or None), window (grow,
    block_below, block_above), want ({(ix, iz): the lowest blocking index}, every other cell -1), written out by hand"""
    out = []

    def add(name, table, want, solid=None, hidden=None, floors=None, offsets=None, window=WIDE):
        out.append(dict(name=name, table=table, want=want, solid=solid, hidden=hidden, floors=floors or {}, offsets=offsets, window=window))

    hair = float(np.nextafter(F(0.25), F(0)))
    everywhere = {(ix, iz): 0 for ix in range(8) for iz in range(8)}
    add('at a centre, radius 0', things_at([at(3, 4)]), {(3, 4): 0})
    add('a radius of exactly one cell', things_at([at(3, 4)], radius=0.25), plus(3, 4))
    add('a radius a hair below one cell', things_at([at(3, 4)], radius=hair), {(3, 4): 0})
    add('the disc reaches no centre: the own cell', things_at([at(3, 4, 0.1, 0.1)], radius=0.05), {(3, 4): 0})
    add('on the corner of its own cell, radius 0', things_at([at(3, 4, -0.125, -0.125)]), {(3, 4): 0})  # floorf: the lower corner belongs
    add('outside the grid, the disc reaches in', things_at([at(-1, 4)], radius=0.25), {(0, 4): 0})
    add('outside the grid, the disc a hair short', things_at([at(-1, 4)], radius=hair), {})
    add('in no cell', things_at([(1.0e6, -1.0e6), (3.0e30, 0.0)]), {})
    add('r * r overflows', things_at([(-1.0e30, 2.0e30)], radius=3.0e19), everywhere)
    three = things_at([at(1, 1), at(3, 3), at(5, 5)])
    add('solid and hidden bits', three, {(1, 1): 0}, solid=[0, 2], hidden=[2])
    add('both rows null', three, {(1, 1): 0, (3, 3): 1, (5, 5): 2})
    add('everything hidden', three, {}, hidden=[0, 1, 2])
    add('nothing solid', three, {}, solid=[])
    add('the lower index', things_at([at(3, 4), at(3, 4), at(3, 4)], radius=[0.0, 0.25, 0.0]), {**plus(3, 4, 1), (3, 4): 0})
    add('the lower index, the wide one first', things_at([at(3, 4), at(3, 4)], radius=[0.25, 0.0]), plus(3, 4, 0))
    # the window: dy = floor - (base + off); -0.25 <= dy <= 0.5 blocks
    lifted = things_at([at(3, 4)], radius=0.25, base=0.5)
    steps = {(3, 4): 0.5, (2, 4): 0.25, (4, 4): 1.0, (3, 3): 0.125, (3, 5): 1.125}  # dy 0, -0.25, 0.5, -0.375, 0.625
    add('the window, bounds inclusive', lifted, {(3, 4): 0, (2, 4): 0, (4, 4): 0}, floors=steps, window=NARROW)
    add('the window, a hair narrower', lifted, {(3, 4): 0}, floors=steps, window=SHORT)
    on_lift = things_at([at(3, 4)], base=0.5, object_id=2)
    add('a thing on a lift carried 2 up', on_lift, {(3, 4): 0}, floors={(3, 4): 2.5}, offsets={2: 2.0}, window=NARROW)
    add('the lift at rest', on_lift, {}, floors={(3, 4): 2.5}, window=NARROW)
    # (the library refuses offsets whose row ends at or below the set's largest object_id: this one is for the restatement alone)
    add('an object beyond the row', things_at([at(3, 4)], base=0.5, object_id=9), {(3, 4): 0}, floors={(3, 4): 0.5}, offsets={2: 2.0, 3: 7.0},
        window=NARROW)
    add('object 0 does not move', things_at([at(3, 4)], base=0.5), {(3, 4): 0}, floors={(3, 4): 0.5}, offsets={0: 5.0}, window=NARROW)
    add('a NaN floor, a finite window', things_at([at(3, 4)], radius=0.25), {**plus(3, 4), (2, 4): None}, floors={(2, 4): np.nan}, window=NARROW)
    add('a NaN floor, an infinite window', things_at([at(3, 4)], radius=0.25), {**plus(3, 4), (2, 4): None}, floors={(2, 4): np.nan})
    add('a void cell, an infinite window', things_at([at(3, 4)], radius=0.25), plus(3, 4), floors={(2, 4): np.inf})
    add('a void cell, a finite window', things_at([at(3, 4)], radius=0.25), {**plus(3, 4), (2, 4): None}, floors={(2, 4): np.inf}, window=NARROW)
    add('-0 and a NaN payload pass through', things_at([at(6, 6)]), {(6, 6): 0}, floors={(0, 0): -0.0, (1, 0): 'payload', (7, 7): -0.0})
    for c in out:
        c['want'] = {k: v for k, v in c['want'].items() if v is not None}
    return out


PAYLOAD = 0x7FC12345  # a quiet NaN with a payload


def hand_planes(case, shape=(8, 8)):
    """(floor, ceiling) (1, H, W) float32 of a hand case"""
    floor, ceiling = flat(1, HAND_GRID, shape)
    for (ix, iz), f in case['floors'].items():
        if isinstance(f, str):
            floor.view(U)[0, iz, ix] = PAYLOAD
        else:
            floor[0, iz, ix] = f
            if f == np.inf:
                ceiling[0, iz, ix] = -np.inf
    return floor, ceiling


def hand_offsets(case):
    """(1, HAND_OBJECTS, 3) float32: the case's row of offsets, zeros where it has none"""
    off = np.zeros((1, HAND_OBJECTS, 3), F)
    for o, y in (case['offsets'] or {}).items():
        off[0, o, 1] = y
    return off


def hand_index(case, shape=(8, 8), first=0):
    """(H, W) int32: the index plane a hand case wants, its indices counted from `first`"""
    index = np.full(shape, -1, np.int32)
    for (ix, iz), i in case['want'].items():
        index[iz, ix] = first + i
    return index


def planes_of(floor, ceiling, index):
    """the contract's output planes from the inputs and an index plane: +inf / -inf where a thing blocks, the input's words elsewhere"""
    f, c = np.ascontiguousarray(floor, F).view(U).copy(), np.ascontiguousarray(ceiling, F).view(U).copy()
    f[index >= 0], c[index >= 0] = stamp_ref.PLUS_INF, stamp_ref.MINUS_INF
    return f.view(F), c.view(F)


# ---- random tables ------------------------------------------------------------------------------------------------------------------

POISON = 0xA5A5A5A5
SIZES = (1, 31, 32, 33, 255, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def random_case(gw, gh, size, grow):
    """8 rows on a gw x gh grid: a random table of `size` things over the grid and a little beyond, radii from 0 to three cells,
    objects 0 .. 5, a random solid row, random hidden rows, a stride two words wider with the extra words poisoned, floors of
    several heights with a NaN, a void cell and a -0 among them, random offsets and a finite window"""
    wad, host, cell, grid = room_of_grid(gw, gh)
    rng = np.random.default_rng(9000 + 7 * size + gw + int(grow * 100))
    n = 8
    x, z = goal_ref.centres(grid, cell)
    table = np.zeros(size, rd.THING)
    table['x'] = rng.uniform(x[0] - 2 * cell, x[-1] + 2 * cell, size).astype(F)
    table['z'] = rng.uniform(z[0] - 2 * cell, z[-1] + 2 * cell, size).astype(F)
    table['radius'] = (rng.uniform(0, 3 * cell, size) * (rng.random(size) < 0.7)).astype(F)
    table['base'] = rng.choice(F([0.0, 0.25, 0.5, 1.0]), size)
    table['object_id'] = rng.integers(0, 6, size)
    words = max(1, (size + 31) // 32)
    stride = words + 2
    solid = rd.pack_things(rng.random(stride * 32) < min(0.75, 24.0 / size)).view(U)[None].copy()  # some two dozen solid things at the most
    hidden = rng.integers(0, 1 << 32, (n, stride), dtype=np.uint64).astype(U) & rng.integers(0, 1 << 32, (n, stride), dtype=np.uint64).astype(U)
    # thing 0 blocks in row 0 whatever was drawn: inside the grid, solid, not hidden there, at a height most floors are in the window of
    table['x'][0], table['z'][0], table['base'][0], table['object_id'][0] = x[gw // 3], z[gh // 2], 0.25, 0
    solid[0, 0] |= U(1)
    hidden[0, 0] &= ~U(1)
    solid[:, words:], hidden[:, words:] = ~U(POISON), POISON  # the words beyond the set's are not read
    floor = rng.choice(F([0.0, 0.25, 0.5, 1.0, -0.0]), (n, gh, gw))
    ceiling = np.full((n, gh, gw), 1.28, F) + floor
    spots = rng.integers(0, gh * gw, (3, n))
    rows = np.arange(n)
    floor.reshape(n, -1)[rows, spots[0]] = np.nan
    floor.reshape(n, -1)[rows, spots[1]], ceiling.reshape(n, -1)[rows, spots[1]] = INF, -INF
    floor.reshape(n, -1).view(U)[rows, spots[2]] = 0x7FC12345  # a NaN with a payload
    floor[0, gh // 2, gw // 3], ceiling[0, gh // 2, gw // 3] = 0.25, 1.53  # thing 0's own cell in row 0
    offsets = np.zeros((n, max(6, host.game_objects), 3), F)
    offsets[:, :, 1] = rng.choice(F([0.0, 0.25, -0.25, 2.0]), offsets.shape[:2])
    window = dict(grow=grow, block_below=0.25, block_above=0.5)
    want = stamp_ref.stamp(table, grid, cell, floor, ceiling, solid=solid, hidden=hidden, offsets=offsets, **window)
    return dict(wad=wad, cell=cell, grid=grid, table=table, solid=solid, hidden=hidden, floor=floor, ceiling=ceiling, offsets=offsets,
                window=window, want=want, stride=stride)


# ---- the end-to-end case on E1M1 ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def e1m1_wad():
    return rd.Wad(ensure_wad(), META_PATH)


def flood_to_start(floor, ceiling, seeds):
    """inflate_grids(0.19, 0.125), then flood_grids(towards=True, max_step=0.32), on the restatements: (planes, (dist, count))"""
    fi, ci, _ = walls_ref.inflate_grids(floor, ceiling, BODY, E2E_CELL)
    return (fi, ci), goal_ref.flood_grids(fi, ci, seeds, True, max_step=E2E_STEP)


@functools.lru_cache(maxsize=None)
def e1m1_case():
    """four rows of E1M1 at cell 0.125: row 0 with nothing hidden, row 1 with all seven barrels hidden, row 2 with thing 0 hidden,
    row 3 with rng 25's offsets; every stage of draw_area_planes, stamp_things, inflate_grids and flood_grids by the restatements,
    stamped and unstamped"""
    host = e1m1_wad().build_world(0, device=False)
    cell, n = E2E_CELL, 4
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    table, obstacles = host.map_things(), host.thing_obstacles()
    off = sector_ref.random_offsets(np.random.default_rng(25), n, host.game_objects)
    off[:3] = 0
    _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off)
    seeds = np.tile(np.array([E2E_SEED], np.int32), (n, 1))
    solid = rd.pack_things(obstacles).view(U)[None]
    hidden = bit_rows([[], list(E1M1_BARRELS), [0], []], solid.shape[1])
    stamped = stamp_ref.stamp(table, g, cell, floor, ceiling, solid=solid, hidden=hidden, offsets=off)
    return dict(host=host, grid=g, table=table, obstacles=obstacles, offsets=off, floor=floor, ceiling=ceiling, seeds=seeds, solid=solid,
                hidden=hidden, stamped=stamped, plain=flood_to_start(floor, ceiling, seeds), after=flood_to_start(stamped[0], stamped[1], seeds))


def open_cells(floor, ceiling):
    return np.stack([flood_ref.open_cells(floor[p], ceiling[p], 0.56) for p in range(len(floor))])
