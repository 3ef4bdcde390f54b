"""The test side of the solid things on the grid: the contract of include/rdoom.h "solid things on the grid" restated in numpy
binary32 from the header's text alone -- every float an np.float32, one rounded operation per line, every thing against every cell,
no cull, no tiles, no list.  The cell centres are goal_ref.centres', the cell of a point is goal_ref.cells' rule (a thing is
located as a player at its (x, z) would be) and off() is things_ref._off."""
import numpy as np

import goal_ref
import rust_doom_amd as rd
import things_ref

F = np.float32
U = np.uint32
INF = F(np.inf)
PLUS_INF, MINUS_INF = U(0x7F800000), U(0xFF800000)


def grid_of(ix0, iz0, gw, gh):
    """an rd.AreaGrid written out by hand"""
    pitch = (gw + 31) // 32
    return rd.AreaGrid(ix0, iz0, gw, gh, pitch, gh * pitch)


def bits(row, n):
    """bit i % 32 of word i / 32 of a row, for i < n"""
    return rd.unpack_things(np.ascontiguousarray(row).view(U), n)


def own_cells(table, grid, cell):
    """(T, 2) int32: the cell (ix, iz) each thing's point lies in, (-1, -1) where it lies in none"""
    if not len(table):
        return np.zeros((0, 2), np.int32)
    at = np.stack([table['x'], np.zeros(len(table), F), table['z']], 1).astype(F)
    return goal_ref.cells(grid, cell, rd.player_states(at, np.zeros(len(table), F)))


def blocking(table, grid, cell, floor, solid_row=None, hidden_row=None, offsets=None, grow=0.0, block_below=np.inf, block_above=np.inf):
    """(gh, gw) int64: the lowest index of a thing that blocks each cell of the level's grid, -1 where none does.  floor: the
    (gh, gw) float32 input floors of those cells; offsets: None or this row's (n_objects, 3)"""
    t_n = len(table)
    best = np.full((grid.gh, grid.gw), -1, np.int64)
    candidate = np.ones(t_n, bool) if solid_row is None else bits(solid_row, t_n)
    if hidden_row is not None:
        candidate &= ~bits(hidden_row, t_n)
    xc, zc = goal_ref.centres(grid, cell)
    own = own_cells(table, grid, cell)
    y = table['base'].astype(F) + things_ref._off(offsets, table['object_id'].astype(np.int64)) if t_n else np.zeros(0, F)
    low, high = -F(block_below), F(block_above)
    f = np.asarray(floor, F)
    with np.errstate(all='ignore'):
        for i in np.nonzero(candidate)[0][::-1]:  # from the last to the first: the lowest index is written last
            r = F(table['radius'][i]) + F(grow)
            r2 = r * r
            ex = xc - F(table['x'][i])
            ez = zc - F(table['z'][i])
            exex = ex * ex
            ezez = ez * ez
            d2 = exex[None, :] + ezez[:, None]
            covers = d2 <= r2
            if own[i, 0] >= 0:
                covers[own[i, 1], own[i, 0]] = True
            dy = f - y[i]
            best[covers & (dy >= low) & (dy <= high)] = i
    return best


def stamp(tables, grids, cell, floor, ceiling, levels=None, solid=None, hidden=None, offsets=None, **window):
    """every row: (floor_out, ceiling_out (n, H, W) float32 whose words are the contract's, index_out (n, H, W) int32).  tables,
    grids: one level's THING array and AreaGrid, or with `levels` (a slot per row) lists of them; floor, ceiling: (n, H, W) float32;
    solid: None or (levels, stride) uint32; hidden: None or (n, stride) uint32; offsets: None or (n, n_objects, 3); window: grow,
    block_below, block_above"""
    floor, ceiling = np.ascontiguousarray(floor, F), np.ascontiguousarray(ceiling, F)
    n = len(floor)
    if levels is None:
        tables, grids, levels = [tables], [grids], np.zeros(n, U)
    tables = [np.ascontiguousarray(t, rd.THING).reshape(-1) for t in tables]
    fo, co = floor.view(U).copy(), ceiling.view(U).copy()
    index = np.full(floor.shape, -1, np.int32)
    for p in range(n):
        lv = int(levels[p])
        if lv >= len(tables):  # a slot outside the set: passed through
            continue
        g = grids[lv]
        best = blocking(tables[lv], g, cell, floor[p, :g.gh, :g.gw], None if solid is None else solid[lv], None if hidden is None else hidden[p],
                        None if offsets is None else offsets[p], **window)
        index[p, :g.gh, :g.gw] = best
        fo[p, :g.gh, :g.gw][best >= 0] = PLUS_INF
        co[p, :g.gh, :g.gw][best >= 0] = MINUS_INF
    return fo.view(F), co.view(F), index
