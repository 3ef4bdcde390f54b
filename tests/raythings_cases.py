"""Hand cases of the rays that see things (include/rdoom_rays.h), with numbers binary32 holds exactly, that the host test puts
through tests/raythings_ref.py and the GPU test through the kernel as well.  Every player looks along yaw 0, pitch 0, where the
quaternion is the identity, and stands at y = -0.12f, so that its eye is at y = 0 exactly.  The cases share one launch: case k
lives 64 units along z from case k - 1, far beyond the range of 1, in one table, one select row, one row of offsets, hidden bits
and world fractions per player, and one set of parameters -- the categories carry the heights (0: 2, 1: 1, 2: 0.5, 3: +inf), and
category 5 is masked out.  The directions are the same for every player; a case names the one it is about."""
import numpy as np

import raythings_ref as rt
import rust_doom_amd as rd

F = np.float32
U = np.uint32
INF = float('inf')
NAN = float('nan')
MAX_RANGE = 1.0
DIRS = np.array([(-1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, 0), (NAN, 0, 0)], F)  # along -x, down, up, the zero ray, a NaN ray
WEST, DOWN, UP, ZERO, BAD = range(5)
HEIGHTS = np.array([2.0, 1.0, 0.5, INF, 1.0, 2.0, 1.0, 1.0], F)
CATEGORIES = 0xFF & ~(1 << rd.THING_KEY)  # category 5 is not seen
N_OBJECTS = 2
SPACING = 64.0
HANG = rd.THING_HANGING


def _case(name, things, dir=WEST, eye=(1.0, 0.0), frac=None, want=(INF, -1), hidden=(), unselected=(), lift=0.0, gpu=True):
    """things: (dx, dz, base, radius, category, object_id) relative to the case's origin; eye: the player's (x, z) there; want:
    (fraction, local index or -1) of ray `dir`; frac: the world's fraction of every ray of the player, or None; lift: the y of
    object 1 in the player's row of offsets"""
    return dict(name=name, things=things, dir=dir, eye=eye, frac=frac, want=want, hidden=hidden, unselected=unselected, lift=lift, gpu=gpu)


def hand_cases():
    post = (0.0, 0.0, -1.0, 0.5, 0, 0)  # at the origin, radius 0.5, from y = -1 to y = 1
    return [
        _case('head on', [post], want=(0.5, 0)),
        _case('a miss beside the thing', [(0.0, 0.75, -1.0, 0.5, 0, 0)]),
        _case('a tangent ray', [(0.0, 0.5, -1.0, 0.5, 0, 0)], want=(1.0, 0)),
        _case('an eye inside the thing', [(1.0, 0.0, -1.0, 0.5, 0, 0)], want=(0.0, 0)),
        _case('the zero ray of an eye inside', [(1.0, 0.0, -1.0, 0.5, 0, 0)], dir=ZERO),
        _case('a NaN ray', [(1.0, 0.0, -1.0, 0.5, 0, 0)], dir=BAD, frac=0.75, want=(0.75, -1)),
        _case('straight down onto the top cap', [(1.0, 0.0, -1.0, 0.5, 2, 0)], dir=DOWN, want=(0.5, 0)),
        _case('up onto the bottom of a hanging thing', [(1.0, 0.0, 1.0, 0.5, 2 | HANG, 0)], dir=UP, want=(0.5, 0)),
        _case('down misses a hanging thing above', [(1.0, 0.0, 1.0, 0.5, 2 | HANG, 0)], dir=DOWN),
        _case('a horizontal ray just over the top', [(0.0, 0.0, -1.0, 0.5, 2, 0)]),
        _case('a horizontal ray along the top cap', [(0.0, 0.0, -0.5, 0.5, 2, 0)], want=(0.5, 0)),
        _case('no top', [(0.0, 0.0, -5.0, 0.5, 3, 0)], want=(0.5, 0)),
        _case('no bottom when hanging', [(0.0, 0.0, 5.0, 0.5, 3 | HANG, 0)], want=(0.5, 0)),
        _case('two equal things', [post, post], want=(0.5, 0)),
        _case('a strictly earlier thing', [post, (0.25, 0.0, -1.0, 0.5, 0, 0)], want=(0.25, 1)),
        _case('the world at the same fraction', [post], frac=0.5, want=(0.5, -1)),
        _case('the world later', [post], frac=0.75, want=(0.5, 0)),
        _case('the world earlier', [post], frac=0.25, want=(0.25, -1)),
        _case('a NaN fraction passes through', [post], frac=NAN, want=(NAN, -1)),
        _case('a thing that is not selected', [post], unselected=(0,)),
        _case('a hidden thing, and the one behind it', [(0.25, 0.0, -1.0, 0.5, 0, 0), post], hidden=(0,), want=(0.5, 1)),
        _case('a masked category', [(0.0, 0.0, -1.0, 0.5, rd.THING_KEY, 0)]),
        _case('R == 0', [(0.0, 0.0, -1.0, 0.0, 0, 0)]),
        _case('a NaN eye', [post], eye=(NAN, 0.0), frac=0.75, want=(0.75, -1)),
        _case('below the ray at rest', [(0.0, 0.0, -3.0, 0.5, 1, 1)]),
        _case('carried 2 up by its object', [(0.0, 0.0, -3.0, 0.5, 1, 1)], lift=2.0, want=(0.5, 0)),
        _case('an object beyond the row stays at rest', [(0.0, 0.0, -3.0, 0.5, 1, 5)], lift=2.0, gpu=False),
    ]


def assemble(cases):
    """the cases as one launch: a dict of states, dirs, table, select (1, words), hidden (n, words), offsets (n, N_OBJECTS, 3), frac
    (n, R), and want: a list of (player, ray, fraction, index in the table or -1)"""
    n = len(cases)
    pos = np.zeros((n, 3), F)
    rows, want = [], []
    hidden_bits, unselected = np.zeros((n, 0), bool), []
    frac = np.full((n, len(DIRS)), INF, F)
    offsets = np.zeros((n, N_OBJECTS, 3), F)
    first = []
    for k, c in enumerate(cases):
        z0 = SPACING * k
        pos[k] = (c['eye'][0], -F(0.12), z0 + c['eye'][1])
        first.append(len(rows))
        rows += [(dx, z0 + dz, base, radius, cat, obj) for dx, dz, base, radius, cat, obj in c['things']]
        if c['frac'] is not None:
            frac[k] = c['frac']
        offsets[k, 1, 1] = c['lift']
        t, i = c['want']
        want.append((k, c['dir'], t, i if i < 0 else first[k] + i))
    cols = list(zip(*rows))
    table = rt.table_of(np.array(cols[0], F), np.array(cols[1], F), np.array(cols[2], F), np.array(cols[3], F), np.array(cols[4]),
                        np.array(cols[5]))
    t_n = len(table)
    hidden_bits = np.zeros((n, t_n), bool)
    chosen = np.ones(t_n, bool)
    for k, c in enumerate(cases):
        for i in c['hidden']:
            hidden_bits[k, first[k] + i] = True
        for i in c['unselected']:
            chosen[first[k] + i] = False
    words = (t_n + 31) // 32
    return dict(states=rd.player_states(pos, np.zeros(n, F), pitch=np.zeros(n, F)), dirs=DIRS, table=table,
                select=rd.pack_things(chosen, words).view(U).reshape(1, words),
                hidden=np.stack([rd.pack_things(h, words) for h in hidden_bits]).view(U), offsets=offsets, frac=frac, want=want)


# ---- random tables --------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 31, 32, 33, 64, 65, 255, 256, 257)  # the word, wave and pass boundaries
LIST_CAPACITY = 512  # raythings.hip LIST_CAP: the things a workgroup's LDS list holds; it is folded when fewer than 256 slots are free
RAY_COUNTS = (1, 7, 64, 100, 257)
RANDOM_HEIGHTS = np.array([0.56, 0.3, 1.0, INF, 0.16, 0.42, 0.0, 0.8], F)


def random_table(rng, size, around, spread, n_objects, base=0.0):
    """`size` things within `spread` of the (x, z) points `around`, drawn in turn: radii 0 .. 0.4 (a tenth of them 0), bases within
    0.5 of `base` (per point or one number), categories and objects at random, a fifth hanging from 1 above"""
    around = np.asarray(around, F).reshape(-1, 2)
    at = around[np.arange(size) % len(around)] if size else np.zeros((0, 2), F)
    low = np.broadcast_to(np.asarray(base, F), (len(around),))[np.arange(size) % len(around)] if size else np.zeros(0, F)
    hang = rng.random(size) < 0.2
    radius = np.where(rng.random(size) < 0.1, 0.0, rng.uniform(0.0, 0.4, size))
    return rt.table_of(at[:, 0] + rng.uniform(-spread, spread, size), at[:, 1] + rng.uniform(-spread, spread, size),
                       low + np.where(hang, 1.0, 0.0) + rng.uniform(-0.5, 0.5, size), radius,
                       rng.integers(0, 8, size) | np.where(hang, HANG, 0), rng.integers(0, n_objects, size))


def random_rows(rng, rows, size, stride, density=0.5):
    """(rows, stride) uint32 of random thing bits: the words at and beyond ceil(size / 32) are poison, as are the bits at and
    beyond `size` of the last word"""
    out = np.full((rows, stride), 0xDEADBEEF, U)
    words = (size + 31) // 32
    for r in range(rows):
        if words:
            bits = rng.random(words * 32) < density
            bits[size:] = rng.random(words * 32 - size) < 0.5
            out[r, :words] = rd.pack_things(bits, words).view(U)
    return out


def random_frac(rng, shape):
    """world fractions with +inf and NaN entries among them"""
    f = rng.uniform(0.0, 1.0, shape).astype(F)
    pick = rng.random(shape)
    f[pick < 0.3] = INF
    f[pick > 0.9] = NAN
    return f


def check(want, frac, thing):
    """the hand-written expectations against (n, R) outputs, words and all"""
    for p, r, t, i in want:
        assert F(frac[p, r]).view(U) == F(t).view(U) or (t != t and frac[p, r] != frac[p, r]), (p, r, frac[p, r], t)
        assert thing[p, r] == i, (p, r, thing[p, r], i)
