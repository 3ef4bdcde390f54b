"""The spawn on the host, with no GPU: the generator pinned on known answers and on a second implementation, the library's spawn table
against the triangles, the reference (tests/spawn_ref.py) on levels small enough to check by eye and on E1M1 and E1M4 of the test
IWAD -- the share of fallbacks, every accepted point checked again through tests/sector_ref.py, the sectors reached, the seed, the
batch size, and thirty idle ticks of the host step -- and the surface: header, exported symbols, the Python names, the structs'
sizes, and every argument error of the two entry points, none of which touches a device."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
import sector_ref
import spawn_ref
import world_ref
from util import META_PATH, ROOT

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
MARGIN = F(spawn_ref.default_margin())
N_REAL = 4096


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def _philox_numpy(counters, key):
    """Philox4x32-10 a second time, not sharing a line with spawn_ref.philox: numpy uint64 over rows of counters, the ten round keys
    laid out first"""
    x = np.array(counters, np.uint64).reshape(-1, 4)
    keys = [((key[0] + r * 0x9E3779B9) % 2 ** 32, (key[1] + r * 0xBB67AE85) % 2 ** 32) for r in range(10)]
    low = np.uint64(0xFFFFFFFF)
    for k0, k1 in keys:
        a, b = x[:, 0] * np.uint64(0xD2511F53), x[:, 2] * np.uint64(0xCD9E8D57)
        x = np.stack([(b >> np.uint64(32)) ^ x[:, 1] ^ np.uint64(k0), b & low, (a >> np.uint64(32)) ^ x[:, 3] ^ np.uint64(k1), a & low], 1)
    return x


KNOWN = [  # Random123's known answers for philox4x32 with 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('counter,key,want', KNOWN)
def test_the_generator_gives_the_known_answers(counter, key, want):
    assert spawn_ref.philox(counter, key) == want, ['%08x' % w for w in spawn_ref.philox(counter, key)]
    assert tuple(int(w) for w in _philox_numpy([counter], key)[0]) == want


def test_two_implementations_of_the_generator_agree_and_the_draws_are_exact():
    rng = np.random.default_rng(3)
    counters = rng.integers(0, 2 ** 32, (500, 4), dtype=np.uint64)
    counters[:, 3] = 0
    key = (int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)))
    got = _philox_numpy(counters, key)
    for c, g in zip(counters[:200], got):
        assert spawn_ref.philox(tuple(int(v) for v in c), key) == tuple(int(v) for v in g)
    seed = key[0] | key[1] << 32
    for c, g in zip(counters[:50], got):
        u = spawn_ref.draws(seed, c[0], c[1], c[2])
        assert all(x.dtype == F and 0 <= x < 1 for x in u)
        assert [float(x) * 2 ** 24 for x in u] == [int(w) >> 8 for w in g]  # exact: a 24-bit integer over 2^24
    # the largest draw times a total can round to the total: the search's last clause is needed, and it is all it needs
    assert F(F(1 - 2.0 ** -24) * F(6.5536)) <= F(6.5536)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def _same_table(t, level):
    assert t.entries.dtype == rd.SPAWN_ENTRY and rd.SPAWN_ENTRY.itemsize == 40
    assert np.array_equal(np.stack([t.entries['a'], t.entries['b'], t.entries['c']], 1).reshape(-1, 3, 3), level.corners)
    assert np.array_equal(t.entries['cumulative'], level.cumulative)


@pytest.mark.parametrize('index', [0, 3])
def test_the_table_is_the_floor_triangles_of_the_world(index):
    wad, world, level = spawn_ref.real(index)
    t = world.spawn_table()
    _same_table(t, level)
    arrays = world.arrays()
    verts, tri = arrays['verts'], arrays['triangles']
    up = verts[tri[:, 3], 1] > 0
    assert 100 < len(t.entries) <= up.sum() < len(tri)
    assert (np.diff(t.entries['cumulative'].astype(np.float64)) >= 0).all() and t.entries['cumulative'][0] > 0
    assert (t.entries['a'][:, 1] == t.entries['b'][:, 1]).all() and (t.entries['a'][:, 1] == t.entries['c'][:, 1]).all()
    # the binary64 sum, rounded once: not the binary32 running sum
    a, b, c = (t.entries[k].astype(np.float64) for k in 'abc')
    area = 0.5 * np.abs((b[:, 0] - a[:, 0]) * (c[:, 2] - a[:, 2]) - (b[:, 2] - a[:, 2]) * (c[:, 0] - a[:, 0]))
    assert np.array_equal(np.cumsum(area).astype(F), t.entries['cumulative'])
    assert not np.array_equal(np.cumsum(area.astype(F), dtype=F), t.entries['cumulative'])
    # dynamic floors (lifts) are in it, after the statics
    assert (np.nonzero(up)[0] >= arrays['n_static_triangles']).any()
    # the start is the level's
    pos, yaw = wad.build_level(index).start()
    assert np.array_equal(t.start_pos, np.asarray(pos, F)) and t.start_yaw == F(yaw)


def test_a_set_lends_each_level_its_own_table():
    wad, world, level = spawn_ref.real(3)
    ws = wad.build_world_set([0, 3, 1], device=False)
    _same_table(ws.spawn_table(1), level)
    _same_table(ws.spawn_table(0), spawn_ref.real(0)[2])
    assert len(ws.spawn_table(2).entries) < 40
    table = ws.levels()
    for slot in range(3):
        t = ws.spawn_table(slot)
        assert np.array_equal(t.start_pos, table['start_pos'][slot]) and t.start_yaw == table['start_yaw'][slot]
    with pytest.raises(rd.RdoomError) as e:
        ws.spawn_table(3)
    assert e.value.status == BAD and 'slot 3' in str(e.value)


# ---- the hand-made levels ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand(name):
    wad, world = spawn_ref.hand_world(name)
    return wad, world, spawn_ref.Level(world)


def _first_try(level, n, seed=11, **kw):
    """the first candidate of n players and whether it is valid"""
    q, _, _ = spawn_ref.candidates(level, seed, np.arange(n), np.zeros(n, np.int64), 1)
    args = dict(margin=MARGIN, clearance=0.56, max_step=0.24)
    args.update(kw)
    return q, spawn_ref.valid(level, q, None, **args)[0]


def _inside(q, x0, x1, z0, z1):
    """the distance of each point from the walls of the room x0 .. x1, z0 .. z1 (negative: outside)"""
    return np.minimum(np.minimum(q[:, 0] - x0, x1 - q[:, 0]), np.minimum(q[:, 2] - z0, z1 - q[:, 2]))


def test_a_square_room_takes_the_points_a_margin_from_its_walls():
    _, world, level = _hand('square')
    assert len(level.cumulative) >= 2 and abs(float(level.cumulative[-1]) - 2.56 * 2.56) < 0.01  # (the walk's polygons overlap the walls by a hair)
    q, ok = _first_try(level, 600)
    assert (q[:, 1] == 0).all()
    d = _inside(q.astype(np.float64), -3.84, -1.28, -3.84, -1.28)
    assert (d > -0.01).all()
    sure = np.abs(d - float(MARGIN)) > 1e-5
    assert np.array_equal(ok[sure], d[sure] > float(MARGIN)) and ok.sum() > 300 and (~ok).sum() > 100
    # the states: on the floor plus the rise, at rest, everyone placed within the tries
    st, tries = spawn_ref.spawn(level, spawn_ref.blank_states(600), 11)
    assert (tries >= 1).all() and (tries <= spawn_ref.TRIES).all() and np.array_equal(tries == 1, ok)
    first = tries == 1
    assert np.array_equal(st['pos'][first][:, [0, 2]], q[first][:, [0, 2]]) and (st['pos'][:, 1] == F(0.5)).all()
    assert (st['vel'] == 0).all() and (st['pitch'] == F(1e-8)).all() and (st['last_height_diff'] == 0).all()
    assert (st['flags'] == rd.PLAYER_CLIP).all() and (st['yaw'] >= 0).all() and (st['yaw'] < F(6.2831855)).all() and len(set(st['yaw'])) > 500
    assert (_inside(st['pos'].astype(np.float64), -3.84, -1.28, -3.84, -1.28) > float(MARGIN) - 1e-5).all()


def test_a_room_thinner_than_two_margins_sends_everyone_to_the_start():
    wad, world, level = _hand('thin')
    c = level.corners
    assert len(c) >= 2 and c[:, :, 2].max() - c[:, :, 2].min() < 2 * MARGIN  # every floor triangle is thinner than 2 * margin
    _, ok = _first_try(level, 200)
    assert not ok.any()
    st, tries = spawn_ref.spawn(level, spawn_ref.blank_states(50), 5, flags=rd.PLAYER_CLIP | rd.PLAYER_FLY)
    assert (tries == 0).all()
    ws = wad.build_world_set([spawn_ref.HAND.index('thin')], device=False)
    want = ws.start_states(np.zeros(50, np.int64), flags=rd.PLAYER_CLIP | rd.PLAYER_FLY)
    assert st.tobytes() == want.tobytes()
    # with a margin that fits, the corridor is used
    assert (spawn_ref.spawn(level, spawn_ref.blank_states(50), 5, margin=0.1)[1] > 0).mean() > 0.8


def test_a_step_keeps_its_margin_clear_until_max_step_allows_it():
    _, world, level = _hand('step')
    n = 800
    q, ok = _first_try(level, n)
    q64 = q.astype(np.float64)
    walls = _inside(q64, -3.84, -1.28, -6.40, -1.28)  # both rooms as one
    to_step = np.abs(q64[:, 2] + 3.84)
    assert set(q[:, 1].tolist()) == {0.0, 0.5}
    off = to_step > 0.01  # (the walk's polygons overlap by a hair)
    assert np.array_equal((q[:, 1] == F(0.5))[off], (q64[:, 2] < -3.84)[off])
    sure = (np.abs(walls - float(MARGIN)) > 1e-5) & (np.abs(to_step - float(MARGIN)) > 1e-5) & off
    near = to_step < float(MARGIN)
    assert np.array_equal(ok[sure], ((walls > float(MARGIN)) & ~near)[sure])
    assert (near & sure & (walls > float(MARGIN))).sum() > 40
    for side in (q[:, 1] == 0, q[:, 1] == F(0.5)):  # rejected on the low side and on the high side
        assert (near & sure & side & (walls > float(MARGIN))).sum() > 10
    _, wide = _first_try(level, n, max_step=0.6)
    assert np.array_equal(wide[sure], (walls > float(MARGIN))[sure]) and (wide & near).sum() > 40
    st, tries = spawn_ref.spawn(level, spawn_ref.blank_states(n), 11, max_step=0.6)
    high = st['pos'][:, 2].astype(np.float64) < -3.84
    assert (tries > 0).all() and np.array_equal(st['pos'][:, 1] == F(1.0), high) and (st['pos'][~high, 1] == F(0.5)).all()
    # the landing rule: a floor 0.2 higher beside the candidate is within a max_step of 0.24 and is still refused, from below only
    rise = spawn_ref.RISE - MARGIN
    assert F(0.2) < rise < F(0.5)
    level.tables.sectors['floor'][1] = F(0.2)
    try:
        q, low = _first_try(level, n)
        near = np.abs(q.astype(np.float64)[:, 2] + 3.84) < float(MARGIN)
        below = q.astype(np.float64)[:, 2] > -3.84
        assert (near & below & sure & (walls > float(MARGIN))).sum() > 10 and not low[near & below & sure].any()
        assert low[~near & below & sure & (walls > float(MARGIN))].all()
        assert not low[~below].any()  # and the triangles of the other room, still 0.5 high, are no longer the floor there
    finally:
        level.tables.sectors['floor'][1] = F(0.5)


def test_a_room_without_headroom_is_never_chosen():
    _, world, level = _hand('low')
    s = level.tables.sectors
    assert ((s['ceiling'] - s['floor']) == F(0.5)).all()
    _, ok = _first_try(level, 300)
    assert not ok.any()
    st, tries = spawn_ref.spawn(level, spawn_ref.blank_states(40), 9)
    assert (tries == 0).all() and (st['pos'] == level.start_pos).all()
    assert (spawn_ref.spawn(level, spawn_ref.blank_states(40), 9, clearance=0.5)[1] > 0).all()


def test_masks_episodes_and_slots_on_the_reference():
    _, world, level = _hand('square')
    n = 40
    blank = spawn_ref.blank_states(n)
    mask = np.arange(n) % 2 == 0
    st, tries = spawn_ref.spawn(level, blank, 3, mask=mask, tries=np.full(n, 9, np.uint32))
    assert st[~mask].tobytes() == blank[~mask].tobytes() and (tries[~mask] == 9).all() and (tries[mask] > 0).all()
    full, _ = spawn_ref.spawn(level, blank, 3)
    assert st[mask].tobytes() == full[mask].tobytes()  # a player's point does not depend on who else is reset
    ep, _ = spawn_ref.spawn(level, blank, 3, episode=np.arange(n) % 3)
    same = np.arange(n) % 3 == 0
    assert ep[same].tobytes() == full[same].tobytes() and (ep['pos'][~same] != full['pos'][~same]).any(1).all()
    out, tries = spawn_ref.spawn([level, level], blank, 3, level_of=np.where(np.arange(n) == 7, 2, 1), tries=np.full(n, 9, np.uint32))
    assert out[7].tobytes() == blank[7].tobytes() and tries[7] == 0 and (tries[np.arange(n) != 7] > 0).all()


# ---- E1M1 and E1M4 -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spawned(index, seed=1993):
    level = spawn_ref.real(index)[2]
    return spawn_ref.spawn(level, spawn_ref.blank_states(N_REAL), seed)


def _valid_again(tables, pos, margin=MARGIN, clearance=F(0.56), max_step=F(0.24)):
    """the validity rule of the header for points that were accepted, written again on tests/sector_ref.py alone: y is the floor + rise"""
    ok = np.ones(len(pos), bool)
    rec = tables.sectors
    centre = sector_ref.sector_at(tables, pos[:, [0, 2]])
    ok &= centre != sector_ref.NONE
    f0 = rec['floor'][np.minimum(centre, len(rec) - 1)]
    ok &= pos[:, 1] == (f0 + F(0.5)).astype(F)
    d = F(margin * F(0.70710677))
    for dx, dz in ((0, 0), (margin, 0), (-margin, 0), (0, margin), (0, -margin), (d, d), (-d, d), (d, -d), (-d, -d)):
        pts = np.stack([(pos[:, 0] + F(dx)).astype(F), (pos[:, 2] + F(dz)).astype(F)], 1)
        s = sector_ref.sector_at(tables, pts)
        ok &= s != sector_ref.NONE
        r = rec[np.minimum(s, len(rec) - 1)]
        ok &= (r['ceiling'] - r['floor']).astype(F) >= clearance
        rise = (r['floor'] - f0).astype(F)
        ok &= (np.abs(rise) <= max_step) & ~((rise > 0) & (rise < F(F(0.5) - margin)))
    return ok


@pytest.mark.parametrize('index', [0, 3])
def test_a_real_level_places_nearly_everyone_on_valid_floor(index):
    _, world, level = spawn_ref.real(index)
    st, tries = _spawned(index)
    share = float((tries == 0).mean())
    print('level %d: fallback share %.4f of %d, tries %s' % (index, share, N_REAL, np.bincount(tries, minlength=9).tolist()))
    assert share <= 0.10
    accepted = tries > 0
    assert _valid_again(level.tables, st['pos'][accepted]).all()
    assert (st['vel'] == 0).all() and (st['pitch'] == F(1e-8)).all() and (st['flags'] == rd.PLAYER_CLIP).all()
    start = rd.player_states([level.start_pos], level.start_yaw)[0]
    assert all(s.tobytes() == start.tobytes() for s in st[~accepted])
    # every sector with more than 2 % of the table's valid area is reached: the area by 40 000 points of numpy's own generator
    rng = np.random.default_rng(8)
    area = np.diff(np.concatenate([[0.0], level.cumulative.astype(np.float64)]))
    pick = rng.choice(len(area), 40000, p=area / area.sum())
    u, v = rng.random(40000), rng.random(40000)
    fold = u + v > 1
    u[fold], v[fold] = 1 - u[fold], 1 - v[fold]
    a, b, c = (level.corners[pick, k].astype(np.float64) for k in range(3))
    pts = (a + u[:, None] * (b - a) + v[:, None] * (c - a)).astype(F)
    pts[:, 1] += F(0.5)
    good = _valid_again(level.tables, pts)
    where = sector_ref.sector_at(level.tables, pts[:, [0, 2]])[good]
    shares = np.bincount(where, minlength=len(level.tables.sectors)) / good.sum()
    big = np.nonzero(shares > 0.02)[0]
    reached = set(sector_ref.sector_at(level.tables, st['pos'][accepted][:, [0, 2]]).tolist())
    assert len(big) >= 5 and set(big.tolist()) <= reached, (big, sorted(reached))
    assert 0.3 < good.mean() < 0.95  # the rule refuses a good part of the floor, and not most of it


@pytest.mark.parametrize('index', [0, 3])
def test_seeds_differ_and_a_state_does_not_depend_on_the_batch(index):
    level = spawn_ref.real(index)[2]
    st, tries = _spawned(index)
    other, _ = spawn_ref.spawn(level, spawn_ref.blank_states(N_REAL), 1994)
    assert (other['pos'][:, [0, 2]] != st['pos'][:, [0, 2]]).any(1).mean() > 0.99
    high, _ = spawn_ref.spawn(level, spawn_ref.blank_states(64), 1993 | 1 << 40)  # the high word of the seed is part of the key
    assert (high['pos'][:, [0, 2]] != st['pos'][:64, [0, 2]]).any(1).mean() > 0.9
    one, t1 = spawn_ref.spawn(level, spawn_ref.blank_states(1), 1993)
    assert one[0].tobytes() == st[0].tobytes() and t1[0] == tries[0]
    some, ts = spawn_ref.spawn(level, spawn_ref.blank_states(100), 1993)
    assert some.tobytes() == st[:100].tobytes() and np.array_equal(ts, tries[:100])
    ep, _ = spawn_ref.spawn(level, spawn_ref.blank_states(64), 1993, episode=np.ones(64, np.uint32))
    assert (ep['pos'][:, [0, 2]] != st['pos'][:64, [0, 2]]).any(1).all()


@pytest.mark.parametrize('index', [0, 3])
def test_thirty_idle_ticks_move_no_spawned_player_by_more_than_the_margin(index):
    wad, world, level = spawn_ref.real(index)
    st, tries = _spawned(index)
    t = world.triggers()
    game = game_ref.RefGame(world_ref.RefWorld(wad, index), t['triggers'], t['effects'], len(st), world.game_objects)
    out = game.step(st, np.zeros((30, len(st)), rd.PLAYER_INPUT))
    moved = np.hypot(out['pos'][:, 0] - st['pos'][:, 0], out['pos'][:, 2] - st['pos'][:, 2])[tries > 0]
    print('level %d: largest idle move %.4f, margin %.4f' % (index, moved.max(), MARGIN))
    assert moved.max() <= MARGIN
    assert not (out['flags'] & rd.PLAYER_DIVERGED).any() and (out['pos'][:, 1] > st['pos'][:, 1] - F(0.3)).all()  # nobody fell through


def test_a_door_takes_players_in_the_games_that_opened_it_only():
    door, offsets, (st, tries), sector = spawn_ref.door_case()
    inside = (tries > 0) & (sector == door)
    assert inside[1::2].any() and not inside[0::2].any()
    assert (offsets[0::2] == 0).all() and (offsets[1::2, :, 1] > 0.9).sum() == len(offsets) // 2


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_spawn():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- spawn:' in text and '(DESIGN section 21)' in text
    assert '#define RDOOM_SPAWN_TRIES 8u' in text and '#define RDOOM_SPAWN_RISE 0.5f' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'typedef struct rdoom_spawn_params \{\s*float margin, clearance, max_step;\s*uint32_t flags;\s*\} rdoom_spawn_params;', code)
    assert re.search(r'typedef struct rdoom_spawn_entry \{\s*float a\[3\], b\[3\], c\[3\];\s*float cumulative;\s*\} rdoom_spawn_entry;', code)
    tail = ['const float *d_object_offsets', 'uint32_t n_objects', 'const uint8_t *d_mask', 'uint64_t seed', 'const uint32_t *d_episode',
            'const rdoom_spawn_params *params', 'uint32_t *d_tries_out', 'void *stream']
    proto = re.search(r'rdoom_status rdoom_world_spawn_players\((.*?)\);', code, flags=re.S).group(1)
    assert [' '.join(a.split()) for a in proto.split(',')] == ['const rdoom_world *world', 'rdoom_player_state *d_states', 'uint32_t n'] + tail
    proto = re.search(r'rdoom_status rdoom_worldset_spawn_players\((.*?)\);', code, flags=re.S).group(1)
    assert [' '.join(a.split()) for a in proto.split(',')] == ['const rdoom_worldset *set', 'rdoom_player_state *d_states',
                                                               'const uint32_t *d_levels', 'uint32_t n'] + tail
    assert re.search(r'rdoom_status rdoom_world_spawn_table\(const rdoom_world \*world, rdoom_spawn_table \*out\);', code)
    assert re.search(r'rdoom_status rdoom_worldset_level_spawn_table\(const rdoom_worldset \*set, uint32_t slot, rdoom_spawn_table \*out\);', code)
    for words in ('Philox4x32-10', '0xD2511F53', '0xCD9E8D57', '0x9E3779B9', '0xBB67AE85', 'x = (p, e, t, 0)', '(float)(x_i >> 8) * 0x1p-24f',
                  'mid = (lo + hi) >> 1', 'n_entries - 1 when lo == n_entries', 'q = (a + u1 * (b - a)) + u2 * (c - a)', 'g - f >= clearance',
                  'fabsf(rise) <= max_step', 'rise < RDOOM_SPAWN_RISE - margin', 'u3 * 6.2831855f', 'has no counterpart', 'binary64',
                  'captured into a graph', 'n == 0 queues nothing'):
        assert words in text, words


def test_the_library_and_the_package_export_the_spawn():
    L = ctypes.CDLL(rd.LIB_PATH)
    names = {'rdoom_world_spawn_table', 'rdoom_worldset_level_spawn_table', 'rdoom_world_spawn_players', 'rdoom_worldset_spawn_players'}
    assert all(hasattr(L, n) for n in names) and names <= set(rd.API_SYMBOLS)
    assert rd.SPAWN_TRIES == 8 == spawn_ref.TRIES and rd.SPAWN_RISE == 0.5
    assert ctypes.sizeof(rd.SpawnParams) == 16 and [f[0] for f in rd.SpawnParams._fields_] == ['margin', 'clearance', 'max_step', 'flags']
    assert ctypes.sizeof(rd.SpawnTableArrays) == 32 and rd.SPAWN_ENTRY.itemsize == 40
    sig = inspect.signature(rd.World.spawn_players)
    assert list(sig.parameters) == ['self', 'states', 'seed', 'mask', 'episode', 'offsets', 'margin', 'clearance', 'max_step', 'flags',
                                    'tries_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['margin'], d['clearance'], d['max_step'], d['flags']) == (None, 0.56, 0.24, rd.PLAYER_CLIP)
    assert d['mask'] is None and d['episode'] is None and d['tries_out'] is None
    sig = inspect.signature(rd.WorldSet.spawn_players)
    assert list(sig.parameters)[:4] == ['self', 'states', 'levels', 'seed'] and list(sig.parameters)[4:] == list(d)[3:]
    assert float(rd.player_config_default()['radius']) == spawn_ref.default_margin() == float(F(0.19))
    assert rd.lib().rdoom_world_spawn_table(None, None) == BAD and b'null' in rd.lib().rdoom_last_error()
    assert rd.lib().rdoom_worldset_level_spawn_table(None, 0, None) == BAD and b'null' in rd.lib().rdoom_last_error()


def test_the_spawn_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    wad, world, _ = spawn_ref.real(0)
    ws = wad.build_world_set([0, 3], device=False)
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks
    nan, inf = float('nan'), float('inf')

    def call_world(h=world._h, st=fake, n=4, off=None, n_obj=0, params=(0.19, 0.56, 0.24, rd.PLAYER_CLIP)):
        p = ctypes.byref(rd.SpawnParams(*params)) if params is not None else None
        return L.rdoom_world_spawn_players(h, st, n, off, n_obj, None, ctypes.c_uint64(1), None, p, None, None)

    def call_set(h=ws._h, st=fake, lv=fake, n=4, off=None, n_obj=0, params=(0.19, 0.56, 0.24, rd.PLAYER_CLIP)):
        p = ctypes.byref(rd.SpawnParams(*params)) if params is not None else None
        return L.rdoom_worldset_spawn_players(h, st, lv, n, off, n_obj, None, ctypes.c_uint64(1), None, p, None, None)

    for call, noun in ((call_world, 'world'), (call_set, 'world set')):
        def fails(word, **kw):
            assert call(**kw) == BAD, kw
            assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

        fails('null ' + noun, h=None)
        fails('null params', params=None)
        fails('null states', st=None)
        for k, name in enumerate(('margin', 'clearance', 'max_step')):
            for bad in (nan, -1.0, -inf, -1e-30):
                params = [0.19, 0.56, 0.24, 0]
                params[k] = bad
                fails(name, params=tuple(params))
        fails('n_objects 1 is smaller', off=fake, n_obj=1)
        # every argument valid: the handle has no device copy, and n == 0 is not a way round that or round the checks
        fails('RDOOM_WORLD_HOST_ONLY')
        fails('RDOOM_WORLD_HOST_ONLY', n=0, st=None)
        fails('RDOOM_WORLD_HOST_ONLY', params=(0.0, 0.0, inf, 0xFFFFFFFF))
        fails('null params', n=0, params=None)
        fails('margin', n=0, params=(nan, 0.56, 0.24, 0))
    assert call_set(lv=None) == BAD and 'null levels' in L.rdoom_last_error().decode()
    assert world.game_objects > 1 and ws.n_objects > 1
