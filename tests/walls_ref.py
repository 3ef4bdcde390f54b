"""The test side of the wall distance (include/rdoom.h "wall distance"): two independent statements of D2 in numpy over
flood_ref.open_cells -- `brute`, the definition itself, a minimum over all blocking cells, for small grids; `capped`, a two-phase
shifted-minimum form usable at a level's size -- the plane rule on the 32-bit words (`inflate`), and the hand-made grids the host
and GPU tests share, their distances written out as literals."""
import math

import numpy as np

import flood_ref

F = np.float32
FAR = 0xFFFF
MAX_RADIUS = 32
NONE = np.iinfo(np.int64).max  # exact_d2 of a grid with no blocking cell anywhere


def close_d2(radius, cell):
    return int(math.floor((float(radius) / float(cell)) ** 2))


def radius_of(d2):
    """the smallest R >= 1 with R * R >= d2"""
    r = 1
    while r * r < d2:
        r += 1
    return r


def exact_d2(is_open, edge_open=False):
    """the definition on one (H, W) grid of open cells, uncapped, int64: the minimum over every blocking cell of the squared
    distance; NONE where there is no blocking cell.  Of the cell positions outside the grid only the ring next to it is listed: an
    outside position clamped to that ring stays outside and is no farther from any cell inside, so the minimum is the same."""
    is_open = np.asarray(is_open, bool)
    h, w = is_open.shape
    rows, cols = np.nonzero(~is_open)
    if not edge_open:
        ring_c = np.concatenate([np.arange(-1, w + 1), np.arange(-1, w + 1), np.full(h, -1), np.full(h, w)])
        ring_r = np.concatenate([np.full(w + 2, -1), np.full(w + 2, h), np.arange(h), np.arange(h)])
        rows, cols = np.concatenate([rows, ring_r]), np.concatenate([cols, ring_c])
    if len(rows) == 0:
        return np.full((h, w), NONE, np.int64)
    r, c = np.mgrid[0:h, 0:w].astype(np.int64)
    d = (c.reshape(-1, 1) - cols.astype(np.int64)[None, :]) ** 2 + (r.reshape(-1, 1) - rows.astype(np.int64)[None, :]) ** 2
    return d.min(1).reshape(h, w)


def report(d2, radius):
    """what d_dist2_out holds of exact distances: D2 where D2 <= R * R, FAR elsewhere"""
    return np.where(d2 <= radius * radius, d2, FAR).astype(np.uint16)


def _rows(one, floor, ceiling, clearance):
    f, g = np.asarray(floor, F), np.asarray(ceiling, F)
    if f.ndim == 2:
        return one(flood_ref.open_cells(f, g, clearance))
    return np.stack([one(flood_ref.open_cells(f[p], g[p], clearance)) for p in range(len(f))])


def brute(floor, ceiling, radius, clearance=0.56, edge_open=False):
    """d_dist2_out, uint16, of (H, W) or (n, H, W) planes by the definition"""
    return _rows(lambda o: report(exact_d2(o, edge_open), radius), floor, ceiling, clearance)


def capped_open(is_open, radius, edge_open=False):
    """d_dist2_out of one grid of open cells in two phases of shifted minima: g, the vertical distance to the nearest blocking cell
    within R of every cell of the grid padded by R, then the minimum over |dx| <= R of dx * dx + g * g"""
    R = int(radius)
    h, w = is_open.shape
    blocked = np.pad(~np.asarray(is_open, bool), R, constant_values=not edge_open)  # (h + 2R, w + 2R)
    big = 1 << 20
    g = np.full((h, w + 2 * R), big, np.int64)
    for dy in range(-R, R + 1):
        g = np.minimum(g, np.where(blocked[R + dy:R + dy + h, :], abs(dy), big))
    d2 = np.full((h, w), big * big, np.int64)
    for dx in range(-R, R + 1):
        d2 = np.minimum(d2, dx * dx + g[:, R + dx:R + dx + w] ** 2)
    return report(d2, R)


def capped(floor, ceiling, radius, clearance=0.56, edge_open=False):
    """d_dist2_out, uint16, of (H, W) or (n, H, W) planes by the two-phase form"""
    return _rows(lambda o: capped_open(o, radius, edge_open), floor, ceiling, clearance)


def inflate(floor, ceiling, d2, shut_d2):
    """d_floor_out, d_ceiling_out: the inputs' 32-bit words where D2 > shut_d2, +inf / -inf where D2 <= shut_d2.  d2: the reported
    distances of a radius with R * R >= shut_d2 (FAR is above every such value)"""
    f, g = np.ascontiguousarray(floor, F).view(np.uint32), np.ascontiguousarray(ceiling, F).view(np.uint32)
    shut = np.asarray(d2).astype(np.int64) <= shut_d2
    return np.where(shut, np.uint32(0x7F800000), f).view(F), np.where(shut, np.uint32(0xFF800000), g).view(F)


def inflate_grids(floor, ceiling, radius, cell, clearance=0.56, edge_open=False):
    """rd.inflate_grids by `capped`: (floor, ceiling, dist2)"""
    shut = close_d2(radius, cell)
    d2 = capped(floor, ceiling, radius_of(shut), clearance, edge_open)
    return inflate(floor, ceiling, d2, shut) + (d2,)


# ---- hand-made grids -------------------------------------------------------------------------------------------------------------

def hand_cases():
    """a list of dicts: name, floor, ceiling (H, W) float32, radius, edge_open, want (H, W) written out by hand with X for FAR.
    Every number is a sum of two small squares"""
    X = FAR
    out = []

    def add(name, fg, radius, edge_open, want):
        out.append(dict(name=name, floor=fg[0], ceiling=fg[1], radius=radius, edge_open=edge_open, want=np.array(want, np.uint16)))

    room = flood_ref.room
    add('1x1 open', room(1, 1), 1, False, [[1]])
    add('1x1 open, edge open', room(1, 1), 1, True, [[X]])
    add('1x1 open, edge open, R 32', room(1, 1), 32, True, [[X]])
    add('1x1 closed', room(1, 1, 0.0, 0.5), 1, False, [[0]])
    add('1x1 closed, edge open', room(1, 1, 0.0, 0.5), 1, True, [[0]])

    f, g = room(7, 7)
    g[3, 3] = F(0.5)  # the centre: too low to stand in
    add('7x7 centre closed, edge open, R 2', (f, g), 2, True, [
        [X, X, X, X, X, X, X],
        [X, X, X, 4, X, X, X],  # the corners of the 5 x 5 window are 8, the cells next to them 5: both above 4
        [X, X, 2, 1, 2, X, X],
        [X, 4, 1, 0, 1, 4, X],
        [X, X, 2, 1, 2, X, X],
        [X, X, X, 4, X, X, X],
        [X, X, X, X, X, X, X]])
    add('7x7 centre closed, R 2', (f, g), 2, False, [  # the edge wins on the outer ring, and ties the disc's axis cells at 4
        [1, 1, 1, 1, 1, 1, 1],
        [1, 4, 4, 4, 4, 4, 1],
        [1, 4, 2, 1, 2, 4, 1],
        [1, 4, 1, 0, 1, 4, 1],
        [1, 4, 2, 1, 2, 4, 1],
        [1, 4, 4, 4, 4, 4, 1],
        [1, 1, 1, 1, 1, 1, 1]])
    add('7x7 centre closed, R 1', (f, g), 1, False, [
        [1, 1, 1, 1, 1, 1, 1],
        [1, X, X, X, X, X, 1],
        [1, X, X, 1, X, X, 1],
        [1, X, 1, 0, 1, X, 1],
        [1, X, X, 1, X, X, 1],
        [1, X, X, X, X, X, 1],
        [1, 1, 1, 1, 1, 1, 1]])
    add('7x7 centre closed, edge open, R 3', (f, g), 3, True, [
        [X, X, X, 9, X, X, X],  # 3 * 3 + 1 = 10 next to the 9s, 8 = 2 * 2 + 2 * 2 on the diagonal, 5 = 2 * 2 + 1
        [X, 8, 5, 4, 5, 8, X],
        [X, 5, 2, 1, 2, 5, X],
        [9, 4, 1, 0, 1, 4, 9],
        [X, 5, 2, 1, 2, 5, X],
        [X, 8, 5, 4, 5, 8, X],
        [X, X, X, 9, X, X, X]])

    f, g = room(7, 7)
    f[3, 3] = np.nan  # a floor that is not a number closes the cell
    add('7x7 centre NaN, edge open, R 2', (f, g), 2, True, out[5]['want'].tolist())
    f, g = room(5, 3)
    g[1, 0] = np.nan
    f[1, 4], g[1, 4] = np.inf, -np.inf  # the void of the planes
    add('5x3 two closed ends, edge open, R 2', (f, g), 2, True, [
        [1, 2, X, 2, 1],
        [0, 1, 4, 1, 0],
        [1, 2, X, 2, 1]])
    return out
