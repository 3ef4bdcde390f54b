"""The test side of the rays that see things: the contract of include/rdoom_rays.h restated in numpy binary32 from the header's
text alone -- every float an np.float32, one rounded operation per line, every ray against every thing, no cull, no list, the
key's minimum by brute force.  The rays are rays_ref's: its eye and quaternion (rays_restatement.c), its turn of a direction
written out in numpy, times max_range -- tests/test_raythings_host.py shows they are rays_ref.cast's origin and vel bit for bit --
or the origin / vel arrays a caller hands in.  off() is things_ref._off.  With dtype=np.float64 the same lines are the float64
model the binary32 restatement is measured against."""
import numpy as np

import rays_ref
import rust_doom_amd as rd
import things_ref

F = np.float32
U = np.uint32
INF = F(np.inf)
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
HANGING = rd.THING_HANGING


def bits(row, n):
    """bit i % 32 of word i / 32 of a row, for i < n"""
    return rd.unpack_things(np.ascontiguousarray(row).view(U), n)


def rays(states, dirs, max_range):
    """(origin (n, 3), vel (n, R, 3)) float32: cast_rays' ray of every (player, direction)"""
    states = np.ascontiguousarray(states, rd.PLAYER_STATE).reshape(-1)
    dirs = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    eye, q = rays_ref.eyes(states)
    re, qi, qj, qk = (q[:, k][:, None] for k in range(4))
    v0, v1, v2 = (dirs[:, k][None, :] for k in range(3))
    # q * v: tmp = q.v x v + v * q.s; q.v x tmp * 2 + v (rays_restatement.c ry_turn), one rounded operation a line
    ax = qj * v2 - qk * v1
    ay = qk * v0 - qi * v2
    az = qi * v1 - qj * v0
    tx = ax + v0 * re
    ty = ay + v1 * re
    tz = az + v2 * re
    bx = qj * tz - qk * ty
    by = qk * tx - qi * tz
    bz = qi * ty - qj * tx
    turned = np.stack([bx * F(2) + v0, by * F(2) + v1, bz * F(2) + v2], -1).astype(F)
    return eye, (turned * F(max_range)).astype(F)


def heights_of(heights):
    return np.full(8, heights, F) if np.isscalar(heights) else np.asarray(heights, F).reshape(8)


def thing_times(o, v, table, heights, grow=0.0, categories=0xFF, select_row=None, hidden_row=None, offsets=None, dtype=F):
    """(R, T) of `dtype`: the contract's t of every ray o + s * v[r] against every thing of the table, +inf where the thing is not
    tried or not hit.  o: (3,), v: (R, 3); offsets: None or this player's (n_objects, 3)"""
    D = dtype
    t_n = len(table)
    o32, v32 = np.asarray(o, F), np.asarray(v, F).reshape(-1, 3)
    out = np.full((len(v32), t_n), np.inf, D)
    if not t_n:
        return out
    cat = table['category'].astype(np.int64)
    tried = np.ones(t_n, bool) if select_row is None else bits(select_row, t_n)
    if hidden_row is not None:
        tried = tried & ~bits(hidden_row, t_n)
    tried = tried & (((int(categories) >> (cat & 0xFF)) & 1) == 1)
    with np.errstate(all='ignore'):
        R = table['radius'].astype(D) + D(grow)
        tried = tried & (R > 0)
        y = table['base'].astype(D) + things_ref._off(offsets, table['object_id'].astype(np.int64)).astype(D)
        h = heights_of(heights).astype(D)[cat & 0xFF]
        hanging = (cat & HANGING) != 0
        bottom = np.where(hanging, y - h, y)
        top = np.where(hanging, y, y + h)
        ox, oy, oz = (D(o32[k]) for k in range(3))
        vx, vy, vz = (v32[:, k].astype(D)[:, None] for k in range(3))
        ray_ok = np.isfinite(o32).all() & np.isfinite(v32).all(1) & (v32 != 0).any(1)
        cx = (ox - table['x'].astype(D))[None, :]
        cz = (oz - table['z'].astype(D))[None, :]
        vxvx = vx * vx
        vzvz = vz * vz
        a = vxvx + vzvz
        cxvx = cx * vx
        czvz = cz * vz
        b = cxvx + czvz
        cxcx = cx * cx
        czcz = cz * cz
        d2 = cxcx + czcz
        RR = (R * R)[None, :]
        cc = d2 - RR
        bb = b * b
        acc = a * cc
        disc = bb - acc
        s = np.sqrt(disc)
        nb = -b
        n0 = nb - s
        n1 = nb + s
        slanted = a > 0
        h0 = np.where(slanted, n0 / a, D(-np.inf))
        h1 = np.where(slanted, n1 / a, D(np.inf))
        plan = np.where(slanted, disc >= 0, cc <= 0)
        db = (bottom - oy)[None, :]
        dt = (top - oy)[None, :]
        u0 = db / vy
        u1 = dt / vy
        rising = vy != 0
        swap = u1 < u0
        v0 = np.where(rising, np.where(swap, u1, u0), D(-np.inf))
        v1 = np.where(rising, np.where(swap, u0, u1), D(np.inf))
        in_height = rising | ((oy >= bottom) & (oy <= top))[None, :]
        t = np.where(h0 < v0, v0, h0)
        t = np.where(t > 0, t, D(0.0))
        e = np.where(v1 < h1, v1, h1)
        hit = plan & in_height & (t <= e) & (t <= 1) & tried[None, :] & ray_ok[:, None]
    return np.where(hit, t, D(np.inf)).astype(D)


def fold(times, current):
    """(frac_out float32 (R,), thing int32 (R,)): the key's minimum over a ray's things against `current`.  times: (R, T) float32"""
    r_n, t_n = times.shape
    current = np.asarray(current, F).reshape(r_n)
    frac, thing = current.copy(), np.full(r_n, -1, np.int32)
    if not t_n:
        return frac, thing
    hit = times <= F(1)
    keys = np.where(hit, times.astype(F).view(U).astype(np.uint64) << np.uint64(32) | np.arange(t_n, dtype=np.uint64)[None, :], NO_KEY)
    best = keys.min(1)
    t = (best >> np.uint64(32)).astype(U).view(F)
    with np.errstate(invalid='ignore'):
        replaces = (best != NO_KEY) & (t < current)
    frac.view(U)[replaces] = t.view(U)[replaces]
    thing[replaces] = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)[replaces]
    return frac, thing


def cast(tables, states, dirs, max_range, heights=0.56, grow=0.0, categories=0xFF, levels=None, select=None, hidden=None, offsets=None,
         frac=None, origin=None, vel=None):
    """every player: (frac_out (n, R) float32 whose words are the contract's, thing_out (n, R) int32).  tables: one level's THING
    array, or with `levels` (a slot per player) a list of them; select: None or (levels, stride) words; hidden: None or (n, stride)
    words; offsets: None or (n, n_objects, 3); frac: None (+inf) or (n, R) float32; origin (n, 3) or (n, R, 3) and vel (n, R, 3):
    the rays to use in place of rays(states, dirs, max_range)"""
    if origin is None:
        origin, vel = rays(states, dirs, max_range)
    origin, vel = np.asarray(origin, F), np.asarray(vel, F)
    n, r_n = vel.shape[0], vel.shape[1]
    if origin.ndim == 3:  # cast_rays' origin_out: one per ray, the same for every ray of a player
        assert (origin.view(U) == origin[:, :1].view(U)).all()
        origin = origin[:, 0]
    if levels is None:
        tables, levels = [tables], np.zeros(n, U)
    tables = [np.ascontiguousarray(t, rd.THING).reshape(-1) for t in tables]
    current = np.full((n, r_n), INF, F) if frac is None else np.array(frac, F).reshape(n, r_n)
    out, thing = current.copy(), np.full((n, r_n), -1, np.int32)
    for p in range(n):
        lv = int(levels[p])
        if lv >= len(tables):  # a slot outside the set: current and -1
            continue
        times = thing_times(origin[p], vel[p], tables[lv], heights, grow, categories, None if select is None else select[lv],
                            None if hidden is None else hidden[p], None if offsets is None else offsets[p])
        out[p], thing[p] = fold(times, current[p])
    return out, thing


# ---- the random field the float64 comparison and the recorded error share -----------------------------------------------------------
FIELD = dict(players=400, n_rays=64, things=64, side=20.0, max_range=10.0, pitch=0.4, seed=20261)


def table_of(x, z, base, radius, category, object_id=None):
    t = np.zeros(len(x), rd.THING)
    t['x'], t['z'], t['base'], t['radius'], t['category'] = x, z, base, radius, category
    if object_id is not None:
        t['object_id'] = object_id
    return t


def random_field(seed=FIELD['seed'], players=FIELD['players'], things=FIELD['things'], side=FIELD['side'], pitch=FIELD['pitch']):
    """(states, dirs, table, heights): players scattered over a side x side field of things of radius 0.08 .. 0.3, categories at
    random with heights 0.16 .. 1.0, a quarter of the things hanging from 1.2; eyes between 0.12 and 1.1 up, pitches within `pitch`"""
    rng = np.random.RandomState(seed)
    pos = np.stack([rng.uniform(0, side, players), rng.uniform(0.0, 1.0, players), rng.uniform(0, side, players)], 1).astype(F)
    states = rd.player_states(pos, rng.uniform(-np.pi, np.pi, players).astype(F), pitch=rng.uniform(-pitch, pitch, players).astype(F))
    dirs = rd.ray_fan(FIELD['n_rays'], 2.0)
    cat = rng.randint(0, 8, things)
    hang = rng.rand(things) < 0.25
    table = table_of(rng.uniform(0, side, things), rng.uniform(0, side, things), np.where(hang, 1.2, rng.uniform(0.0, 0.3, things)),
                     rng.uniform(0.08, 0.3, things), cat | np.where(hang, HANGING, 0))
    heights = rng.uniform(0.16, 1.0, 8).astype(F)
    return states, dirs, table, heights


def field_comparison():
    """the field through the binary32 restatement and through the float64 model of the same lines: a dict of the rays, how many
    name the same thing (or none), the worst |t32 - t64| among those that hit, and what the hit-point test needs"""
    states, dirs, table, heights = random_field()
    origin, vel = rays(states, dirs, FIELD['max_range'])
    n, r_n = vel.shape[:2]
    i32, i64 = np.zeros((n, r_n), np.int64), np.zeros((n, r_n), np.int64)
    t32, t64 = np.zeros((n, r_n), np.float64), np.zeros((n, r_n), np.float64)
    for p in range(n):
        a = thing_times(origin[p], vel[p], table, heights)
        b = thing_times(origin[p], vel[p], table, heights, dtype=np.float64)
        f, i32[p] = fold(a, np.full(r_n, INF, F))
        t32[p] = f
        i64[p] = np.where(np.isfinite(b.min(1)), b.argmin(1), -1)  # the first of equal minima: the lowest index
        t64[p] = b.min(1)
    agree = i32 == i64
    both = agree & (i32 >= 0)
    worst = float(np.abs(t32[both] - t64[both]).max())
    return dict(rays=n * r_n, agree=int(agree.sum()), hits=int(both.sum()), worst=worst, origin=origin, vel=vel, table=table, heights=heights,
                thing=i32, t=t32)
