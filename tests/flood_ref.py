"""The test side of the flood (include/rdoom.h "flood"): a deque breadth-first search over float32 numpy planes, the contract's four
comparisons computed with np.float32 operations, and the hand-made grids the host and GPU tests share."""
import collections

import numpy as np

F = np.float32
INF = F(np.inf)
UNREACHED = 0xFFFF
FROM_LEFT, FROM_RIGHT, FROM_ABOVE, FROM_BELOW = 1, 2, 4, 8
DEFAULTS = dict(max_step=0.24, max_drop=float('inf'), clearance=0.56)


def open_cells(floor, ceiling, clearance):
    f, g = np.asarray(floor, F), np.asarray(ceiling, F)
    with np.errstate(invalid='ignore', over='ignore'):
        return (f < INF) & (f > -INF) & ((g - f) >= F(clearance))


def moves(floor, ceiling, max_step, max_drop, clearance):
    """(open, bits) of one (H, W) map: bits, uint8, has FROM_LEFT when the move from the left neighbour INTO the cell is allowed,
    and so on; `above` is the stored row before"""
    f, g = np.asarray(floor, F), np.asarray(ceiling, F)
    step, drop, clear = F(max_step), F(max_drop), F(clearance)
    is_open = open_cells(f, g, clear)
    bits = np.zeros(f.shape, np.uint8)

    def enters(a, b):  # a, b: slices of the source cells and of the cells entered
        with np.errstate(invalid='ignore', over='ignore'):
            return is_open[a] & is_open[b] & ((f[b] - f[a]) <= step) & ((f[a] - f[b]) <= drop) & \
                ((np.fmin(g[a], g[b]) - np.fmax(f[a], f[b])) >= clear)
    lo, hi, all_ = slice(None, -1), slice(1, None), slice(None)
    bits[:, 1:] |= np.where(enters((all_, lo), (all_, hi)), FROM_LEFT, 0).astype(np.uint8)
    bits[:, :-1] |= np.where(enters((all_, hi), (all_, lo)), FROM_RIGHT, 0).astype(np.uint8)
    bits[1:, :] |= np.where(enters((lo, all_), (hi, all_)), FROM_ABOVE, 0).astype(np.uint8)
    bits[:-1, :] |= np.where(enters((hi, all_), (lo, all_)), FROM_BELOW, 0).astype(np.uint8)
    return is_open, bits


def flood(floor, ceiling, seed=None, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """distances (H, W) uint16 of one map from seed = (column, row), None: (W // 2, H // 2)"""
    h, w = np.asarray(floor).shape
    is_open, bits = moves(floor, ceiling, max_step, max_drop, clearance)
    dist = [UNREACHED] * (h * w)
    c, r = (w // 2, h // 2) if seed is None else (int(seed[0]), int(seed[1]))
    if 0 <= c < w and 0 <= r < h and is_open[r, c]:
        m = bits.reshape(-1).tolist()
        dist[r * w + c] = 0
        queue = collections.deque([r * w + c])
        while queue:
            a = queue.popleft()
            d, col = dist[a] + 1, a % w
            for ok, b, bit in ((col + 1 < w, a + 1, FROM_LEFT), (col > 0, a - 1, FROM_RIGHT), (a + w < h * w, a + w, FROM_ABOVE),
                               (a >= w, a - w, FROM_BELOW)):
                if ok and (m[b] & bit) and dist[b] == UNREACHED:
                    dist[b] = d
                    queue.append(b)
    return np.array(dist, np.uint16).reshape(h, w)


def flood_maps(floor, ceiling, seeds=None, **kw):
    """(distances (n, H, W) uint16, counts (n,) uint32) of n maps; seeds: None or (n, 2) of (column, row)"""
    dist = np.stack([flood(floor[p], ceiling[p], None if seeds is None else seeds[p], **kw) for p in range(len(floor))])
    return dist, (dist != UNREACHED).reshape(len(dist), -1).sum(1).astype(np.uint32)


# ---- hand-made grids -------------------------------------------------------------------------------------------------------------

def room(w, h, floor=0.0, ceiling=1.0):
    return np.full((h, w), floor, F), np.full((h, w), ceiling, F)


def hand_cases():
    """a list of dicts: name, floor, ceiling (H, W) float32, seed (column, row) or None, kw (the limits, {} for the defaults), and
    where the distances are written out by hand, want (H, W) with U for UNREACHED"""
    U = UNREACHED
    out = []

    def add(name, fg, seed, want=None, **kw):
        out.append(dict(name=name, floor=fg[0], ceiling=fg[1], seed=seed, kw=kw, want=None if want is None else np.array(want, np.uint16)))

    add('1x1', room(1, 1), None, [[0]])
    add('1x1 closed', room(1, 1, 0.0, 0.5), None, [[U]])
    add('1x9 from the left', room(9, 1), (0, 0), [list(range(9))])
    add('1x9 default seed', room(9, 1), None, [[4, 3, 2, 1, 0, 1, 2, 3, 4]])
    add('9x1 from the bottom', room(1, 9), (0, 8), [[8 - k] for k in range(9)])
    add('9x1 default seed', room(1, 9), None, [[abs(k - 4)] for k in range(9)])

    # 7 x 5 ledge: columns 0-2 at 0.48, columns 3-6 at 0; a drop of 0.48 is taken, a rise of 0.48 is not
    f, g = room(7, 5, 0.0, 2.0)
    f[:, :3] = F(0.48)
    add('ledge from the top', (f, g), (0, 0), [[c + r for c in range(7)] for r in range(5)])
    add('ledge from below', (f, g), (6, 0), [[U, U, U] + [6 - c + r for c in range(3, 7)] for r in range(5)])
    add('ledge, drop limited', (f, g), (0, 0), [[c + r if c < 3 else U for c in range(7)] for r in range(5)], max_drop=0.3)
    # the same with one stair cell of 0.24 at column 3 of the last row: the plateau is climbed there, and there only
    f2 = f.copy()
    f2[4, 3] = F(0.24)  # 0.48 - 0.24 == 0.24 in binary32: a rise exactly equal to max_step passes
    assert F(0.48) - F(0.24) == F(0.24)
    want = [[(6 - 3) + (4 - 0) + 1 + (2 - c) + (4 - r) if c < 3 else 6 - c + r for c in range(7)] for r in range(5)]
    want[4][3] = 3 + 4
    add('ledge with a stair from below', (f2, g), (6, 0), want)

    # own height suffices, the shared opening does not: a (0, 0.6) and b (0.2, 0.8), 0.4 in common
    f, g = room(7, 5, 0.0, 0.6)
    f[:, 3:], g[:, 3:] = F(0.2), F(0.8)
    assert F(0.8) - F(0.2) >= F(0.56) and F(0.6) - F(0.2) < F(0.56)
    add('shared opening too low', (f, g), (0, 2), [[c + abs(r - 2) if c < 3 else U for c in range(7)] for r in range(5)])
    add('shared opening too low, from the other side', (f, g), (6, 2), [[6 - c + abs(r - 2) if c >= 3 else U for c in range(7)] for r in range(5)])

    # cells that are not numbers, or not finite: all closed but the one with a ceiling of +inf
    f, g = room(7, 5)
    f[0, 1], g[0, 3] = np.nan, np.nan
    f[1, 1], f[1, 3] = np.inf, -np.inf
    g[2, 1], g[2, 3] = -np.inf, np.inf
    f[3, 1], g[3, 1] = np.inf, -np.inf  # the void of a sector map
    f[3, 3], g[3, 3] = np.nan, np.nan
    want = flood_by_hand_blocked(7, 5, (0, 0), {(1, 0), (3, 0), (1, 1), (3, 1), (1, 2), (1, 3), (3, 3)})
    add('cells that are not numbers', (f, g), (0, 0), want)
    add('a closed seed', (f, g), (1, 1), [[U] * 7] * 5)
    add('a seed on a NaN', (f, g), (3, 3), [[U] * 7] * 5)
    for k, seed in enumerate(((-1, 2), (7, 2), (3, -1), (3, 5), (-2 ** 31, 2 ** 31 - 1))):
        add('a seed outside the grid %d' % k, room(7, 5), seed, [[U] * 7] * 5)

    # exactly at the limits: g - f == clearance and f_b - f_a == max_step pass, one ulp beyond does not
    f, g = room(7, 5, 0.0, 0.56)
    add('clearance met exactly', (f, g), None, [[abs(c - 3) + abs(r - 2) for c in range(7)] for r in range(5)])
    g2 = g.copy()
    g2[:, 5] = np.nextafter(F(0.56), F(0))
    add('clearance missed by an ulp', (f, g2), None, [[abs(c - 3) + abs(r - 2) if c < 5 else U for c in range(7)] for r in range(5)])
    f, g = room(7, 5, 0.0, 9.0)
    for c in range(7):
        f[:, c] = F(0.24) * F(c)  # 0, 0.24, 0.48, 0.72 (= 3 * 0.24 rounded), ...: not every difference is 0.24 again
    step = float(max(f[0, c + 1] - f[0, c] for c in range(6)))
    add('a rise exactly max_step', (f, g), (0, 2), [[c + abs(r - 2) for c in range(7)] for r in range(5)], max_step=step)
    below = float(np.nextafter(F(step), F(0)))
    first = min(c for c in range(6) if f[0, c + 1] - f[0, c] > F(below))
    add('a rise an ulp above max_step', (f, g), (0, 2), [[c + abs(r - 2) if c <= first else U for c in range(7)] for r in range(5)],
        max_step=below)
    return out


def flood_by_hand_blocked(w, h, seed, blocked):
    """Manhattan-grid distances around blocked cells {(column, row)} by plain relaxation to a fixed point: an independent way to
    the same numbers for a flat room with holes"""
    d = np.full((h, w), UNREACHED, np.int64)
    d[seed[1], seed[0]] = 0
    for _ in range(w * h):
        for r in range(h):
            for c in range(w):
                if (c, r) in blocked or (c, r) == tuple(seed):
                    continue
                near = [d[rr, cc] for cc, rr in ((c - 1, r), (c + 1, r), (c, r - 1), (c, r + 1))
                        if 0 <= cc < w and 0 <= rr < h and (cc, rr) not in blocked]
                if near and min(near) + 1 < d[r, c]:
                    d[r, c] = min(near) + 1
    return d.tolist()


# ---- grids that take many passes -------------------------------------------------------------------------------------------------

def serpentine(w=33, h=31):
    """every even row open, the odd rows shut but for one cell at alternating ends: one corridor of about half the cells, an end at
    (0, 0).  Returns (floor, ceiling)"""
    f, g = room(w, h, np.inf, -np.inf)
    f[0::2], g[0::2] = 0, 1
    for r in range(1, h, 2):
        c = w - 1 if (r // 2) % 2 == 0 else 0
        f[r, c], g[r, c] = 0, 1
    return f, g


def spiral(w, h):
    """a corridor one cell wide wound inwards from (0, 0), walls one cell wide.  Returns (floor, ceiling)"""
    is_open = np.zeros((h, w), bool)
    inside = lambda r, c: 0 <= r < h and 0 <= c < w
    r = c = 0
    dr, dc = 0, 1
    is_open[0, 0] = True
    while True:
        for _ in range(2):
            nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if inside(nr, nc) and not is_open[nr, nc] and not (inside(fr, fc) and is_open[fr, fc]):
                break
            dr, dc = dc, -dr  # turn right
        else:
            break
        r, c = nr, nc
        is_open[r, c] = True
    f, g = room(w, h, np.inf, -np.inf)
    f[is_open], g[is_open] = 0, 1
    return f, g


def staircase(w=350, h=60):
    """a path from the bottom right corner to the top left one that only goes left and up, every move a drop of 0.5: it can be
    walked in that direction only.  Returns (floor, ceiling, seed)"""
    f, g = room(w, h, np.inf, -np.inf)
    r, c, k = h - 1, w - 1, 0
    while True:
        f[r, c], g[r, c] = F(-0.5) * F(k), F(-0.5) * F(k) + F(2)
        k += 1
        if r == 0 and c == 0:
            break
        # keep to the diagonal: up when that is due, else left
        if r > 0 and (c == 0 or (h - 1 - r) * (w - 1) < (w - 1 - c) * (h - 1)):
            r -= 1
        else:
            c -= 1
    return f, g, (w - 1, h - 1)
