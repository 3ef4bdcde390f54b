"""The test side of the things: the contract of include/rdoom.h "things" ("Sensing") restated in numpy binary32 from the header's
text alone -- every float an np.float32, one rounded operation per line, no closed form, every thing against every line, nothing
culled, nothing compacted.  The yaw's sine and cosine are the restatements' one sincos (world_ref.sincos); which lines block a
game's sight comes from reveal_ref.blocking, which the seen-lines tests pin.  Also the tables and players the host and GPU tests
share."""
import numpy as np

import reveal_ref
import rust_doom_amd as rd
import world_ref

F = np.float32
U = np.uint32
INF = F(np.inf)
CATEGORIES = 8


def words_of(n_things):
    return (int(n_things) + 31) // 32


def set_words(tables):
    return max(1, max(words_of(len(t)) for t in tables))


def params(max_range, fov=None, touch_radius=0.19, touch_below=np.inf, touch_above=np.inf, collect=()):
    """the rdoom_thing_sense of World.sense_things' arguments: cos_half_fov is one math.cos on the host, -1 for None"""
    import math
    mask = 0
    for c in collect:
        mask |= 1 << int(c)
    return dict(max_range=F(max_range), cos_half_fov=F(-1.0 if fov is None else math.cos(0.5 * float(fov))), touch_radius=F(touch_radius),
                touch_below=F(touch_below), touch_above=F(touch_above), collect_mask=mask)


def _off(offsets, ids):
    """the map contract's off(o) on one player's row (None: every object at rest)"""
    if offsets is None:
        return np.zeros(len(ids), F)
    offsets = np.asarray(offsets, F).reshape(-1, 3)
    ok = (ids != 0) & (ids < len(offsets))
    return np.where(ok, offsets[np.minimum(ids, len(offsets) - 1), 1], F(0)).astype(F)


def limits(lines, block, ox, oz, vx, vz):
    """T_r of the rays o + t * (vx[k], vz[k]): the seen-lines contract's "Ray against line" over the lines that block"""
    ax, az = lines['a'][:, 0].astype(F), lines['a'][:, 1].astype(F)
    bx, bz = lines['b'][:, 0].astype(F), lines['b'][:, 1].astype(F)
    dx = bx - ax
    dz = bz - az
    dxdx = dx * dx
    dzdz = dz * dz
    len2 = dxdx + dzdz
    wx = ax - ox
    wz = az - oz
    out = np.ones(len(vx), F)
    with np.errstate(all='ignore'):
        for k in range(len(vx)):
            velx, velz = vx[k], vz[k]
            m1 = velx * dz
            m2 = velz * dx
            den = m1 - m2
            n1 = wx * dz
            n2 = wz * dx
            num_t = n1 - n2
            t = num_t / den
            q1 = wx * velz
            q2 = wz * velx
            num_u = q1 - q2
            u = num_u / den
            hit = (len2 > 0) & (den != 0) & (u >= 0) & (u <= 1) & (t >= 0) & (t <= 1) & block
            if hit.any():
                least = t[hit].min()
                out[k] = least if least < out[k] else out[k]
    return out


def sense_player(lines, table, state, prm, offsets=None, collected_row=None):
    """one player against one level: (visible, touched, collects) bool arrays of T, nearest (8,) THING_NEAREST, new (8,) uint32"""
    t_n = len(table)
    px, py, pz = F(state['pos'][0]), F(state['pos'][1]), F(state['pos'][2])
    s, c = world_ref.sincos(float(state['yaw']))
    rx, rz = c, F(-s)
    fx, fz = F(-s), F(-c)
    gone = np.zeros(t_n, bool) if collected_row is None else rd.unpack_things(collected_row, t_n)
    with np.errstate(all='ignore'):
        dx = table['x'].astype(F) - px
        dz = table['z'].astype(F) - pz
        dxdx = dx * dx
        dzdz = dz * dz
        d2 = dxdx + dzdz
        y = table['base'].astype(F) + _off(offsets, table['object_id'])
        dy = py - y
        tr = prm['touch_radius'] + table['radius'].astype(F)
        trtr = tr * tr
        touched = ~gone & (d2 <= trtr) & (dy >= -prm['touch_below']) & (dy <= prm['touch_above'])
        rr = prm['max_range'] * prm['max_range']
        in_range = d2 <= rr
        fwd1 = dx * fx
        fwd2 = dz * fz
        fwd = fwd1 + fwd2
        root = np.sqrt(d2)
        edge = prm['cos_half_fov'] * root
        in_view = (fwd >= edge) if not prm['cos_half_fov'] <= -1 else np.ones(t_n, bool)
        cand = ~gone & in_range & in_view
        visible = np.zeros(t_n, bool)
        idx = np.nonzero(cand)[0]
        if len(idx):
            block = reveal_ref.blocking(lines, None if offsets is None else np.asarray(offsets, F).reshape(-1, 3))
            visible[idx] = limits(lines, block, px, pz, dx[idx], dz[idx]) == F(1)
        r1 = dx * rx
        r2 = dz * rz
        right = r1 + r2
    cat = (table['category'] & 0xFF).astype(np.int64)
    collects = touched & (((prm['collect_mask'] >> cat) & 1) != 0)
    nearest = np.zeros(CATEGORIES, rd.THING_NEAREST)
    new = np.zeros(CATEGORIES, U)
    for k in range(CATEGORIES):
        new[k] = (collects & (cat == k)).sum()
        best = -1
        for i in np.nonzero(visible & (cat == k))[0]:  # ascending: a tie keeps the lower index
            if best < 0 or d2[i] < d2[best]:
                best = int(i)
        nearest[k] = (best, d2[best], right[best], fwd[best]) if best >= 0 else (-1, INF, 0, 0)
    return visible, touched, collects, nearest, new


def pack(bits):
    """a bool array as the words [0, ceil(T / 32)) of a row"""
    out = np.zeros(words_of(len(bits)), U)
    i = np.nonzero(bits)[0]
    np.bitwise_or.at(out, i >> 5, (U(1) << (i & 31).astype(U)))
    return out


def sense(lines, tables, states, prm, offsets=None, levels=None, collected=None, visible=None, touched=None, stride=None):
    """every player.  lines / tables: a MAP_LINE and a THING array, or with `levels` (a slot per player) lists of them, one per
    slot.  collected / visible / touched: None (zeroed rows of `stride` words, default the set's words) or uint32 (n, stride)
    arrays as they stand before the call, which are copied, not changed.  Returns a dict: collected, visible, touched (n, stride)
    uint32, nearest (n, 8) THING_NEAREST, new (n, 8) uint32, and for the tests visible_bits / touched_bits, lists of bool arrays."""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    n = len(states)
    if levels is None:
        lines, tables, levels = [lines], [tables], np.zeros(n, U)
    tables = [np.ascontiguousarray(t, rd.THING).reshape(-1) for t in tables]
    words = set_words(tables)
    stride = words if stride is None else int(stride)
    assert stride >= words
    rows = {}
    for name, given in (('collected', collected), ('visible', visible), ('touched', touched)):
        rows[name] = np.zeros((n, stride), U) if given is None else np.ascontiguousarray(given).view(U).reshape(n, stride).copy()
    out = dict(rows, nearest=np.zeros((n, CATEGORIES), rd.THING_NEAREST), new=np.zeros((n, CATEGORIES), U), visible_bits=[], touched_bits=[])
    out['nearest']['index'], out['nearest']['d2'] = -1, INF
    for p in range(n):
        lv = int(levels[p])
        if lv >= len(tables):  # seen on the device only: rows untouched, nearest none, counts 0
            out['visible_bits'].append(np.zeros(0, bool)), out['touched_bits'].append(np.zeros(0, bool))
            continue
        off = None if offsets is None else offsets[p]
        w = words_of(len(tables[lv]))
        vis, tch, col, nearest, new = sense_player(lines[lv], tables[lv], states[p], prm, off, rows['collected'][p].copy())
        rows['visible'][p, :w], rows['touched'][p, :w] = pack(vis), pack(tch)
        rows['collected'][p, :w] |= pack(col)
        out['nearest'][p], out['new'][p] = nearest, new
        out['visible_bits'].append(vis), out['touched_bits'].append(tch)
    return out


def same_records(got, want):
    """rdoom_thing_nearest records compared bit for bit"""
    return np.array_equal(np.ascontiguousarray(got).view(U).reshape(-1), np.ascontiguousarray(want).view(U).reshape(-1))


# ---- the tables and players the tests share ----
def make_table(rng, n, bounds, near, sectors=1):
    """n things: half drawn uniformly over the bounding box (minx, maxx, minz, maxz), half within 3 units of one of the points
    `near` (k, 2); categories cycled, radii 0 .. 0.3, bases around 0"""
    t = np.zeros(n, rd.THING)
    k = n // 2
    t['x'][:k] = rng.uniform(bounds[0], bounds[1], k)
    t['z'][:k] = rng.uniform(bounds[2], bounds[3], k)
    at = near[rng.integers(0, len(near), n - k)]
    t['x'][k:] = at[:, 0] + rng.uniform(-3, 3, n - k)
    t['z'][k:] = at[:, 1] + rng.uniform(-3, 3, n - k)
    t['base'] = rng.choice(np.array([0.0, 0.0, 0.64, -0.32], F), n)
    t['radius'] = rng.uniform(0, 0.3, n)
    t['category'] = np.arange(n) % CATEGORIES
    t['thing_type'] = 2000 + np.arange(n) % 50
    return t


def bounds_of(lines):
    x = np.concatenate([lines['a'][:, 0], lines['b'][:, 0]])
    z = np.concatenate([lines['a'][:, 1], lines['b'][:, 1]])
    return float(x.min()), float(x.max()), float(z.min()), float(z.max())


def players_near(table, n, rng, spread=1.5):
    """n players near things of the table (the first n of a shuffle), on the floor, with random yaws"""
    pick = rng.permutation(len(table))[:n]
    pick = np.resize(pick, n)
    pos = np.stack([table['x'][pick] + rng.uniform(-spread, spread, n), table['base'][pick] + 0.41,
                    table['z'][pick] + rng.uniform(-spread, spread, n)], 1).astype(F)
    return rd.player_states(pos, rng.uniform(-7, 7, n).astype(F))
