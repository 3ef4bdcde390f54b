"""The test side of waypoints and frontiers (include/rdoom.h "waypoints and frontiers"): the walk down a field written from the
contract over flood_ref.moves' bits (goal_ref.reversed_moves' for RDOOM_FLOOD_TOWARDS), and the frontier of an explored area from
rd.unpack_area's booleans and a distance array.  Plain numpy and Python."""
import numpy as np

import flood_ref
import goal_ref
import rust_doom_amd as rd

UNREACHED = goal_ref.UNREACHED
NO_LIMIT = 0xFFFFFFFF
# the contract's neighbour order (column - 1, column + 1, row - 1, row + 1), and the bit that says "the cell may be entered from
# that neighbour" -- for a TOWARDS field, in goal_ref.reversed_moves' bits, "the cell may be left for that neighbour"
NEIGHBOURS = ((-1, 0, flood_ref.FROM_LEFT), (1, 0, flood_ref.FROM_RIGHT), (0, -1, flood_ref.FROM_ABOVE), (0, 1, flood_ref.FROM_BELOW))


def descend(floor, ceiling, dist, start, towards=False, max_moves=NO_LIMIT, stop_dist=0, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """(cell (column, row), moves, path [(column, row), ...]) of one grid: the contract's walk from `start` down `dist` (H, W)"""
    h, w = np.asarray(floor).shape
    dist = np.asarray(dist).view(np.uint32) if np.asarray(dist).dtype.itemsize == 4 else np.asarray(dist, np.uint32)
    _, bits = flood_ref.moves(floor, ceiling, max_step, max_drop, clearance)
    if towards:
        bits = goal_ref.reversed_moves(bits)
    c, r = int(start[0]), int(start[1])
    if not (0 <= c < w and 0 <= r < h) or int(dist[r, c]) == UNREACHED:
        return (-1, -1), 0, []
    m, path = 0, []
    while int(dist[r, c]) > stop_dist and m < max_moves:
        d = int(dist[r, c])
        for dc, dr, bit in NEIGHBOURS:
            bc, br = c + dc, r + dr
            # the move between a = (c, r) and b: forwards b -> a, which enters a from b's side; towards a -> b, which the reversed
            # bits record at a under the same name
            if 0 <= bc < w and 0 <= br < h and int(dist[br, bc]) == d - 1 and bits[r, c] & bit:
                c, r = bc, br
                break
        else:
            break
        m += 1
        path.append((c, r))
    return (c, r), m, path


def descend_grids(floor, ceiling, dist, starts, path_len=None, **kw):
    """(cells (n, 2) int32, moves (n,) uint32, path (n, path_len, 2) int32 or None) of n grids"""
    n = len(floor)
    cells, moves = np.zeros((n, 2), np.int32), np.zeros(n, np.uint32)
    path = None if path_len is None else np.full((n, path_len, 2), -1, np.int32)
    for p in range(n):
        cell, m, walked = descend(floor[p], ceiling[p], dist[p], starts[p], **kw)
        cells[p], moves[p] = cell, m
        if path is not None and walked:
            k = min(m, path_len)
            path[p, :k] = walked[:k]
    return cells, moves, path


def frontiers(rows, grid, dist):
    """one row's frontier: (cell (ix, iz), its distance, the count, the mask (H, W) uint8) from reveal_area's `rows` ((2, stride)
    words) of `grid` (None: a slot outside the set) and the (H, W) distances"""
    dist = np.asarray(dist)
    dist = dist.view(np.uint32) if dist.dtype.itemsize == 4 else dist.astype(np.uint32)
    mask = np.zeros(dist.shape, np.uint8)
    if grid is None:
        return (-1, -1), UNREACHED, 0, mask
    free, wall = rd.unpack_area(rows, grid)  # (gh, gw) booleans: bits beyond gw and cells beyond the grid are not there at all
    unknown = ~free & ~wall
    near = np.zeros_like(unknown)
    near[:, 1:] |= unknown[:, :-1]
    near[:, :-1] |= unknown[:, 1:]
    near[1:, :] |= unknown[:-1, :]
    near[:-1, :] |= unknown[1:, :]
    front = near & (dist[:grid.gh, :grid.gw] != UNREACHED)
    mask[:grid.gh, :grid.gw] = front
    iz, ix = np.nonzero(front)  # row-major: iz ascending, then ix
    if len(iz) == 0:
        return (-1, -1), UNREACHED, 0, mask
    d = dist[iz, ix]
    k = int(np.argmin(d))  # the first of the smallest: the smallest iz, then ix
    return (int(ix[k]), int(iz[k])), int(d[k]), len(iz), mask


def area_frontiers(area, grids, dist, levels=None):
    """(cells (n, 2) int32, dists (n,) uint32, counts (n,) uint32, masks (n, H, W) uint8) of n rows; grids: one AreaGrid, or with
    `levels` (a slot per row) a list of them"""
    grids = [grids] if isinstance(grids, rd.AreaGrid) else list(grids)
    n = len(dist)
    cells, dists, counts = np.zeros((n, 2), np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    masks = np.zeros(np.asarray(dist).shape, np.uint8)
    for p in range(n):
        slot = 0 if levels is None else int(levels[p])
        g = grids[slot] if 0 <= slot < len(grids) else None
        cells[p], dists[p], counts[p], masks[p] = frontiers(np.ascontiguousarray(area[p]), g, dist[p])
    return cells, dists, counts, masks
