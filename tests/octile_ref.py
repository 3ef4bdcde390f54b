"""The test side of the octile distance (include/rdoom.h "octile distance"): a heapq Dijkstra over flood_ref.moves' axial bits
(goal_ref.reversed_moves' for RDOOM_FLOOD_TOWARDS) and the diagonal bits the contract's rule makes of them, the walk down such a
field written from the contract, and the grids the host and GPU tests share.  Plain numpy and Python."""
import heapq

import numpy as np

import flood_ref
import goal_ref

F = np.float32
UNREACHED = goal_ref.UNREACHED
NO_LIMIT = 0xFFFFFFFF
FROM_LEFT, FROM_RIGHT, FROM_ABOVE, FROM_BELOW = flood_ref.FROM_LEFT, flood_ref.FROM_RIGHT, flood_ref.FROM_ABOVE, flood_ref.FROM_BELOW
FROM_UP_LEFT, FROM_UP_RIGHT, FROM_DOWN_LEFT, FROM_DOWN_RIGHT = 16, 32, 64, 128
# (column offset, row offset, the bit "the cell may be entered from the neighbour at that offset", axial?) in the descent's order
NEIGHBOURS = ((-1, 0, FROM_LEFT, True), (1, 0, FROM_RIGHT, True), (0, -1, FROM_ABOVE, True), (0, 1, FROM_BELOW, True),
              (-1, -1, FROM_UP_LEFT, False), (1, -1, FROM_UP_RIGHT, False), (-1, 1, FROM_DOWN_LEFT, False), (1, 1, FROM_DOWN_RIGHT, False))


def octile_moves(floor, ceiling, towards, max_step, max_drop, clearance):
    """(open, bits) of one (H, W) grid: bits, uint8, the four axial bits of the relation that is followed and the four diagonal
    bits: the move from a = (c + dc, r + dr) into d = (c, r) is allowed exactly when a -> s1, s1 -> d, a -> s2 and s2 -> d are, with
    s1 = (c, r + dr) and s2 = (c + dc, r)"""
    is_open, bits = flood_ref.moves(floor, ceiling, max_step, max_drop, clearance)
    if towards:
        bits = goal_ref.reversed_moves(bits)
    out = bits.copy()
    for dc, dr, bit, axial in NEIGHBOURS:
        if axial:
            continue
        from_side = FROM_LEFT if dc < 0 else FROM_RIGHT   # entered from column + dc
        from_row = FROM_ABOVE if dr < 0 else FROM_BELOW   # entered from row + dr
        here = lambda k: slice(1, None) if k < 0 else slice(None, -1)   # the cells with a neighbour at offset k, and
        there = lambda k: slice(None, -1) if k < 0 else slice(1, None)  # those neighbours
        d, s1, s2 = bits[here(dr), here(dc)], bits[there(dr), here(dc)], bits[here(dr), there(dc)]
        ok = ((s1 & from_side) != 0) & ((d & from_row) != 0) & ((s2 & from_row) != 0) & ((d & from_side) != 0)
        out[here(dr), here(dc)] |= np.where(ok, bit, 0).astype(np.uint8)
    return is_open, out


def flood(floor, ceiling, seed=None, towards=False, axial_cost=5, diagonal_cost=7, max_step=0.24, max_drop=float('inf'), clearance=0.56,
          moves=None):
    """costs (H, W) uint32 of one grid: the cheapest from seed = (column, row), None: (W // 2, H // 2), to every cell, or with
    `towards` from every cell to the seed.  moves: octile_moves of the same arguments, if the caller has them already"""
    h, w = np.asarray(floor).shape
    is_open, bits = moves if moves is not None else octile_moves(floor, ceiling, towards, max_step, max_drop, clearance)
    dist = np.full((h, w), UNREACHED, np.uint32)
    c, r = (w // 2, h // 2) if seed is None else (int(seed[0]), int(seed[1]))
    if 0 <= c < w and 0 <= r < h and is_open[r, c]:
        m = bits.tolist()
        best = {(c, r): 0}
        heap = [(0, c, r)]
        while heap:
            d, c, r = heapq.heappop(heap)
            if d > best[(c, r)]:
                continue
            for dc, dr, bit, axial in NEIGHBOURS:
                # the cell entered from (c, r) lies at the opposite offset, and has (c, r) at (dc, dr)
                bc, br = c - dc, r - dr
                if 0 <= bc < w and 0 <= br < h and (m[br][bc] & bit):
                    nd = d + (axial_cost if axial else diagonal_cost)
                    if nd < best.get((bc, br), 1 << 62):
                        best[(bc, br)] = nd
                        heapq.heappush(heap, (nd, bc, br))
        for (c, r), d in best.items():
            dist[r, c] = d
    return dist


def flood_grids(floor, ceiling, seeds=None, towards=False, **kw):
    """(costs (n, H, W) uint32, counts (n,) uint32) of n grids; seeds: None or (n, 2) of (column, row)"""
    dist = np.stack([flood(floor[p], ceiling[p], None if seeds is None else seeds[p], towards, **kw) for p in range(len(floor))])
    return dist, (dist != UNREACHED).reshape(len(dist), -1).sum(1).astype(np.uint32)


def descend(floor, ceiling, dist, start, towards=False, axial_cost=5, diagonal_cost=7, max_moves=NO_LIMIT, stop_dist=0, max_step=0.24,
            max_drop=float('inf'), clearance=0.56, moves=None):
    """(cell (column, row), moves, path [(column, row), ...]) of one grid: the contract's walk from `start` down `dist` (H, W).
    moves: octile_moves of the same arguments, if the caller has them already"""
    h, w = np.asarray(floor).shape
    dist = np.asarray(dist).view(np.uint32) if np.asarray(dist).dtype.itemsize == 4 else np.asarray(dist, np.uint32)
    _, bits = moves if moves is not None else octile_moves(floor, ceiling, towards, max_step, max_drop, clearance)
    c, r = int(start[0]), int(start[1])
    if not (0 <= c < w and 0 <= r < h) or int(dist[r, c]) == UNREACHED:
        return (-1, -1), 0, []
    m, path = 0, []
    while int(dist[r, c]) > stop_dist and m < max_moves:
        d = int(dist[r, c])
        for dc, dr, bit, axial in NEIGHBOURS:
            bc, br = c + dc, r + dr
            # the move between a = (c, r) and b, in the relation that is followed, enters a from b's side
            if 0 <= bc < w and 0 <= br < h and int(dist[br, bc]) + (axial_cost if axial else diagonal_cost) == d and bits[r, c] & bit:
                c, r = bc, br
                break
        else:
            break
        m += 1
        path.append((c, r))
    return (c, r), m, path


def walk_cost(bits, start, path, axial_cost=5, diagonal_cost=7):
    """the cost of the walk start, path[0], path[1], ... with every step checked to be an allowed move of octile_moves' `bits`:
    written apart from `descend`, from the move bits alone"""
    by_offset = {(dc, dr): (bit, axial) for dc, dr, bit, axial in NEIGHBOURS}
    cost, (c, r) = 0, (int(start[0]), int(start[1]))
    for bc, br in path:
        bit, axial = by_offset[(int(bc) - c, int(br) - r)]  # KeyError: not a neighbour
        assert bits[r, c] & bit, ('a move that is not allowed', (c, r), (bc, br))
        cost, c, r = cost + (axial_cost if axial else diagonal_cost), int(bc), int(br)
    return cost


def descend_grids(floor, ceiling, dist, starts, path_len=None, moves=None, **kw):
    """(cells (n, 2) int32, moves (n,) uint32, path (n, path_len, 2) int32 or None) of n grids; moves: None or octile_moves of
    every grid"""
    n = len(floor)
    cells, counts = np.zeros((n, 2), np.int32), np.zeros(n, np.uint32)
    moves = [None] * n if moves is None else moves
    path = None if path_len is None else np.full((n, path_len, 2), -1, np.int32)
    for p in range(n):
        cell, m, walked = descend(floor[p], ceiling[p], dist[p], starts[p], moves=moves[p], **kw)
        cells[p], counts[p] = cell, m
        if path is not None and walked:
            k = min(m, path_len)
            path[p, :k] = walked[:k]
    return cells, counts, path


def lower_bound(w, h, seed, axial_cost, diagonal_cost):
    """property 4's bound (H, W): the octile cost of the offset from the seed in free space"""
    dc, dr = np.abs(np.arange(w) - seed[0])[None, :], np.abs(np.arange(h) - seed[1])[:, None]
    return axial_cost * (np.maximum(dc, dr) - np.minimum(dc, dr)) + diagonal_cost * np.minimum(dc, dr)


# ---- grids ---------------------------------------------------------------------------------------------------------------------------

def pillar():
    """the 3 x 3 room with its centre closed"""
    f, g = flood_ref.room(3, 3)
    f[1, 1], g[1, 1] = np.inf, -np.inf
    return f, g


def random_room(w, h, seed):
    """a room with steps (some climbed, some dropped from only), ledges and closed cells.  Returns (floor, ceiling)"""
    rng = np.random.default_rng(seed)
    f = (rng.integers(0, 4, (h, w)) * F(0.12)).astype(F)   # neighbours differ by up to 0.36: rises of 0.36 are not climbed
    f[rng.random((h, w)) < 0.06] = F(0.96)                  # ledges: dropped from, not climbed
    g = np.full((h, w), 3.0, F)
    closed = rng.random((h, w)) < 0.18
    f[closed], g[closed] = np.inf, -np.inf
    g[rng.random((h, w)) < 0.03] = F(0.5)                   # too low to stand in
    return f, g


def band(n, anti=False):
    """a band of open cells three wide along the main diagonal of an n x n grid, or its mirror image along the anti-diagonal"""
    c, r = np.arange(n)[None, :], np.arange(n)[:, None]
    is_open = np.abs(c - r) <= 1
    f, g = flood_ref.room(n, n, np.inf, -np.inf)
    f[is_open], g[is_open] = 0, 1
    return (f[:, ::-1].copy(), g[:, ::-1].copy()) if anti else (f, g)
