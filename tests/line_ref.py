"""The test side of the straight walks (include/rdoom.h "straight walks"): the chain of grid moves of a segment between two cell
centres by the contract's sequential definition -- two counters and one comparison of integer products a move, no closed form --
each move looked up in flood_ref.moves' axial bits and octile_ref.octile_moves' diagonal bits; walk_lines and straighten_paths over
n grids written from the contract; and the sparse rooms the host and GPU tests share.  Plain numpy and Python."""
import numpy as np

import flood_ref
import octile_ref

F = np.float32
LIMITS = dict(max_step=0.24, max_drop=float('inf'), clearance=0.56)
# the bit "the cell may be entered from the neighbour at that offset" by the (column, row) offset of that neighbour
BIT = {(dc, dr): bit for dc, dr, bit, _ in octile_ref.NEIGHBOURS}


def chain(a, b):
    """the cells after each move of the chain from a to b, both (column, row): [] for a == b, b last otherwise"""
    (c, r), (cb, rb) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = abs(cb - c), abs(rb - r)
    sx, sy = (cb > c) - (cb < c), (rb > r) - (rb < r)
    i = j = 0
    out = []
    while i < dx or j < dy:
        if j == dy or (i < dx and (2 * i + 1) * dy < (2 * j + 1) * dx):
            c, i = c + sx, i + 1
        elif i == dx or (2 * i + 1) * dy > (2 * j + 1) * dx:
            r, j = r + sy, j + 1
        else:
            c, r, i, j = c + sx, r + sy, i + 1, j + 1
        out.append((c, r))
    return out


def moves_of(floor, ceiling, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """(open, bits) of one (H, W) grid, the forward relation with its diagonal bits, as nested lists: what walk_line looks moves up in"""
    is_open, bits = octile_ref.octile_moves(floor, ceiling, False, max_step, max_drop, clearance)
    return is_open.tolist(), bits.tolist()


def move_allowed(bits, x, y):
    """the move from cell x to its 8-neighbour y: y may be entered from x"""
    return bool(bits[y[1]][y[0]] & BIT[(x[0] - y[0], x[1] - y[1])])


def walk_line(moves, a, b, reversed=False):
    """(clear, stop (column, row), moves made) of the line from a to b on the grid of `moves` (moves_of's pair)"""
    is_open, bits = moves
    h, w = len(bits), len(bits[0])
    a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    if not (0 <= a[0] < w and 0 <= a[1] < h and 0 <= b[0] < w and 0 <= b[1] < h):
        return False, (-1, -1), 0
    if not is_open[a[1]][a[0]]:
        return False, a, 0
    x, made = a, 0
    for y in chain(a, b):
        if not (move_allowed(bits, y, x) if reversed else move_allowed(bits, x, y)):
            return False, x, made
        x, made = y, made + 1
    return True, x, made


def walk_lines(floor, ceiling, starts, targets, reversed=False, moves=None, **kw):
    """(clear (n, q) uint8, stop (n, q, 2) int32, made (n, q) the moves made before the end or the first refusal) of n grids;
    moves: None or moves_of every grid"""
    targets = np.asarray(targets)
    n, q = targets.shape[:2]
    clear, stop, made = np.zeros((n, q), np.uint8), np.zeros((n, q, 2), np.int32), np.zeros((n, q), np.int64)
    for p in range(n):
        m = moves[p] if moves is not None else moves_of(floor[p], ceiling[p], **kw)
        for k in range(q):
            clear[p, k], stop[p, k], made[p, k] = walk_line(m, starts[p], targets[p, k], reversed)
    return clear, stop, made


def straighten(moves, start, path, towards=False, max_look=64, corner_len=8):
    """(corners [(column, row), ...], length binary32) of one row; path: (path_len, 2)"""
    is_open, bits = moves
    h, w = len(bits), len(bits[0])
    inside = lambda c: 0 <= int(c[0]) < w and 0 <= int(c[1]) < h
    m = next((k for k, c in enumerate(path) if not inside(c)), len(path))
    corners, length = [], F(0)
    if not inside(start):
        return corners, length
    a, i = (int(start[0]), int(start[1])), 0
    while i < m and len(corners) < corner_len:
        look = min(max_look, m - i)
        best = next((k for k in range(look - 1, -1, -1) if walk_line(moves, a, path[i + k], not towards)[0]), None)
        if best is None:
            break
        corner = (int(path[i + best][0]), int(path[i + best][1]))
        dc, dr = corner[0] - a[0], corner[1] - a[1]
        length = F(length + np.sqrt(F(dc * dc + dr * dr)))  # the integer converted once, an IEEE square root, one rounded add
        corners.append(corner)
        a, i = corner, i + best + 1
    return corners, length


def straighten_paths(floor, ceiling, starts, path, towards=False, max_look=64, corner_len=8, moves=None, **kw):
    """(corners (n, corner_len, 2) int32, count (n,) uint32, length (n,) float32) of n grids; moves: None or moves_of every grid"""
    n = len(path)
    corners, count, length = np.full((n, corner_len, 2), -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, F)
    for p in range(n):
        m = moves[p] if moves is not None else moves_of(floor[p], ceiling[p], **kw)
        found, length[p] = straighten(m, starts[p], np.asarray(path[p]).tolist(), towards, max_look, corner_len)
        count[p] = len(found)
        if found:
            corners[p, :len(found)] = found
    return corners, count, length


def sparse_room(w, h, seed, p):
    """a flat floor with a share p of closed cells and a share p of pedestals at 0.96 (dropped from, not climbed).  Returns
    (floor, ceiling)"""
    rng = np.random.default_rng(seed)
    f, g = flood_ref.room(w, h, 0.0, 3.0)
    f[rng.random((h, w)) < p] = F(0.96)
    closed = rng.random((h, w)) < p
    f[closed], g[closed] = np.inf, -np.inf
    return f, g
