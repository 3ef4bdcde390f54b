"""The test side of the goal distance (include/rdoom.h "goal distance"): a deque breadth-first search over flood_ref.moves -- forwards
as flood_ref.flood walks it, and for RDOOM_FLOOD_TOWARDS over the reversed relation built from the same comparisons; a level's planes
on its area grid from sector_ref.sector_at at the cell centres and the live heights, all in numpy float32; and the cell of a point by
the explored-area contract's formulas."""
import collections

import numpy as np

import flood_ref
import rust_doom_amd as rd
import sector_ref

F = np.float32
INF = F(np.inf)
UNREACHED = 0xFFFFFFFF
FROM_LEFT, FROM_RIGHT, FROM_ABOVE, FROM_BELOW = flood_ref.FROM_LEFT, flood_ref.FROM_RIGHT, flood_ref.FROM_ABOVE, flood_ref.FROM_BELOW


def reversed_moves(bits):
    """flood_ref.moves' bits of the relation followed backwards: FROM_LEFT of a cell now says that the move from the cell INTO its
    left neighbour is allowed -- which flood_ref.moves records at that neighbour as FROM_RIGHT -- and so on"""
    out = np.zeros_like(bits)
    out[:, 1:] |= np.where(bits[:, :-1] & FROM_RIGHT, FROM_LEFT, 0).astype(np.uint8)
    out[:, :-1] |= np.where(bits[:, 1:] & FROM_LEFT, FROM_RIGHT, 0).astype(np.uint8)
    out[1:, :] |= np.where(bits[:-1, :] & FROM_BELOW, FROM_ABOVE, 0).astype(np.uint8)
    out[:-1, :] |= np.where(bits[1:, :] & FROM_ABOVE, FROM_BELOW, 0).astype(np.uint8)
    return out


def flood(floor, ceiling, seed=None, towards=False, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """distances (H, W) uint32 of one grid: from seed = (column, row), None: (W // 2, H // 2), to every cell, or with `towards` from
    every cell to the seed"""
    h, w = np.asarray(floor).shape
    is_open, bits = flood_ref.moves(floor, ceiling, max_step, max_drop, clearance)
    if towards:
        bits = reversed_moves(bits)
    dist = np.full(h * w, UNREACHED, np.uint32)
    c, r = (w // 2, h // 2) if seed is None else (int(seed[0]), int(seed[1]))
    if 0 <= c < w and 0 <= r < h and is_open[r, c]:
        m = bits.reshape(-1).tolist()
        seen = {r * w + c: 0}
        queue = collections.deque([r * w + c])
        while queue:
            a = queue.popleft()
            d, col = seen[a] + 1, a % w
            for ok, b, bit in ((col + 1 < w, a + 1, FROM_LEFT), (col > 0, a - 1, FROM_RIGHT), (a + w < h * w, a + w, FROM_ABOVE),
                               (a >= w, a - w, FROM_BELOW)):
                if ok and (m[b] & bit) and b not in seen:
                    seen[b] = d
                    queue.append(b)
        dist[np.fromiter(seen.keys(), np.int64, len(seen))] = np.fromiter(seen.values(), np.int64, len(seen)).astype(np.uint32)
    return dist.reshape(h, w)


def flood_grids(floor, ceiling, seeds=None, towards=False, **kw):
    """(distances (n, H, W) uint32, counts (n,) uint32) of n grids; seeds: None or (n, 2) of (column, row)"""
    dist = np.stack([flood(floor[p], ceiling[p], None if seeds is None else seeds[p], towards, **kw) for p in range(len(floor))])
    return dist, (dist != UNREACHED).reshape(len(dist), -1).sum(1).astype(np.uint32)


def widen(dist16):
    """flood_maps' distances as flood_grids gives them: 0xFFFF widened to 0xFFFFFFFF"""
    d = np.asarray(dist16).view(np.uint16).astype(np.uint32)
    return np.where(d == flood_ref.UNREACHED, np.uint32(UNREACHED), d)


# ---- the planes of a level on its area grid ----------------------------------------------------------------------------------------

def centres(grid, cell):
    """(x of every column (gw,), z of every row (gh,)) float32: the contract's ((float)(ix0 + ix) + 0.5f) * cell"""
    x = ((np.arange(grid.gw, dtype=np.int32) + np.int32(grid.ix0)).astype(F) + F(0.5)) * F(cell)
    z = ((np.arange(grid.gh, dtype=np.int32) + np.int32(grid.iz0)).astype(F) + F(0.5)) * F(cell)
    return x, z


def live_heights(sectors, s, offsets):
    """(floor, ceiling) float32 of sectors s (uint32, NONE for none) in the game of `offsets` ((n_objects, 3) or None): height + the y
    of the object's row, 0 for object 0 and objects beyond the row; +inf / -inf for none"""
    none = s == sector_ref.NONE
    at = np.where(none, 0, s).astype(np.int64)
    out = []
    for height, ident, void in (('floor', 'floor_id', INF), ('ceiling', 'ceiling_id', -INF)):
        obj = sectors[ident][at].astype(np.int64)
        add = np.zeros(at.shape, F)
        if offsets is not None:
            moved = (obj != 0) & (obj < len(offsets))
            add[moved] = np.asarray(offsets, F)[obj[moved], 1]
        out.append(np.where(none, void, sectors[height][at].astype(F) + add).astype(F))
    return out


def level_sectors(tables, grid, cell):
    """(gh, gw) uint32: the sector at every cell centre of the level's grid"""
    x, z = centres(grid, cell)
    pts = np.stack(np.broadcast_arrays(x[None, :], z[:, None]), 2).reshape(-1, 2)
    return sector_ref.sector_at(tables, pts).reshape(grid.gh, grid.gw)


def planes(tables, grids, cell, n, levels=None, offsets=None, area=None, shape=None, at_centres=None):
    """the three planes of n rows: (sector (n, H, W) uint16, floor, ceiling (n, H, W) float32).  tables, grids: one level's Tables and
    AreaGrid, or with `levels` (a slot per row) lists of them; offsets: None or (n, n_objects, 3); area: None or (n, 2, stride)
    uint32 rows of reveal_area; shape: (H, W), None: the largest gh and gw; at_centres: level_sectors of every level, if the caller
    has them already"""
    tables = tables if isinstance(tables, (list, tuple)) else [tables]
    grids = [grids] if isinstance(grids, rd.AreaGrid) else list(grids)
    h, w = shape if shape is not None else (max(g.gh for g in grids), max(g.gw for g in grids))
    if at_centres is None:
        at_centres = [level_sectors(t, g, cell) for t, g in zip(tables, grids)]
    sector = np.full((n, h, w), sector_ref.NONE16, np.uint16)
    floor, ceiling = np.full((n, h, w), INF, F), np.full((n, h, w), -INF, F)
    for p in range(n):
        slot = 0 if levels is None else int(levels[p])
        if not 0 <= slot < len(tables):
            continue
        g, s = grids[slot], at_centres[slot].copy()
        if area is not None:
            bits = rd.unpack_area(np.ascontiguousarray(area[p]), g)
            s[~(bits[0] & ~bits[1])] = sector_ref.NONE
        f, c = live_heights(tables[slot].sectors, s, None if offsets is None else offsets[p])
        sector[p, :g.gh, :g.gw] = np.where(s >= sector_ref.NONE16, sector_ref.NONE16, s).astype(np.uint16)
        floor[p, :g.gh, :g.gw], ceiling[p, :g.gh, :g.gw] = f, c
    return sector, floor, ceiling


def cells(grids, cell, states, levels=None):
    """(n, 2) int32 (ix, iz) of every player's (pos.x, pos.z) in the grid of its level, (-1, -1) where it lies in none: the
    explored-area contract's "point (x, z) lies in cell", in numpy float32"""
    grids = [grids] if isinstance(grids, rd.AreaGrid) else list(grids)
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    out = np.full((len(states), 2), -1, np.int32)
    for p, st in enumerate(states):
        slot = 0 if levels is None else int(levels[p])
        if not 0 <= slot < len(grids):
            continue
        g = grids[slot]
        with np.errstate(all='ignore'):
            q = np.array([st['pos'][0], st['pos'][2]], F) / F(cell)
        if not (np.isfinite(q).all() and (np.abs(q) < F(2.0 ** 30)).all()):
            continue
        ix, iz = int(np.floor(q[0])) - g.ix0, int(np.floor(q[1])) - g.iz0
        if 0 <= ix < g.gw and 0 <= iz < g.gh:
            out[p] = ix, iz
    return out
