"""The things on the GPU (things.hip sense_things_kernel / worldset_sense_things_kernel) against tests/things_ref.py, the header's
"Sensing" restated in numpy: every word of every row and every record, bit for bit.  E1M1's own table with players inside, outside
and on NaNs and random door offsets; custom tables at the word, wave and pass boundaries; a door that hides a thing from the player
who has not opened it; collection along a scripted walk; a world set with a slot out of range and poisoned rows; every output
alone; the argument errors that need a thing set; streams, raw pointers and a captured graph in a child process."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import reveal_ref
import rust_doom_amd as rd
import sector_ref
import things_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0xA5A5A5A5
SIZES = (1, 31, 32, 33, 64, 255, 256, 257, 600)
CUSTOM_SEED = 3  # picked on the CPU so that the reference meets custom_case's two bounds at 600
ROUND, CONE = dict(max_range=40.0), dict(max_range=10.0, fov=1.6)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _rows(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(U)


def _same(got, want, what):
    got = _u32(got)
    want = np.ascontiguousarray(want).view(U).reshape(got.shape)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:8], want[bad][:8])


@functools.lru_cache(maxsize=None)
def level(index=0):
    wad = rd.Wad(ensure_wad(), META_PATH)
    host = wad.build_world(index, device=False)
    return dict(wad=wad, index=index, host=host, lines=host.map_lines(), things=host.map_things(), n_objects=host.game_objects)


def run(world, things, states, want, kw, offsets=None, levels=None, collected=None, stride=None, what=''):
    """one launch with all five outputs, poisoned, against the reference's result `want`"""
    n = len(states)
    stride = things.words() if stride is None else stride
    rows = [torch.full((n, stride), -1515870811, dtype=torch.int32, device='cuda') for _ in range(2)]  # 0xA5A5A5A5
    col = _rows(np.zeros((n, stride), U) if collected is None else collected)
    nearest = torch.full((n, 8, 4), 7.0, dtype=torch.float32, device='cuda')
    new = torch.full((n, 8), 77, dtype=torch.int32, device='cuda')
    off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, F)).cuda()
    args = (_dev(states),) + (() if levels is None else (_rows(np.asarray(levels, U)),))
    out = world.sense_things(*args, things, offsets=off, collected=col, visible_out=rows[0], touched_out=rows[1], nearest_out=nearest,
                             new_out=new, **kw)
    assert out.collected is col and out.visible is rows[0] and out.nearest is nearest
    torch.cuda.synchronize()
    _same(rows[0], want['visible'], (what, 'visible'))
    _same(rows[1], want['touched'], (what, 'touched'))
    _same(col, want['collected'], (what, 'collected'))
    _same(new, want['new'], (what, 'new'))
    _same(nearest, want['nearest'], (what, 'nearest'))
    return col


def poisoned(n, stride):
    return np.full((n, stride), POISON, U)


# ---- 1. the level's own table ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def own_case():
    d = level()
    rng = np.random.default_rng(11)
    st, on_map = sector_ref.players(d['wad'], d['index'], 64, rng)
    off = reveal_ref.random_offsets(np.random.RandomState(11), 64, d['n_objects'])
    words = things_ref.words_of(len(d['things']))
    want = {}
    for name, kw in (('round', ROUND), ('cone', CONE)):
        prm = things_ref.params(collect=(rd.THING_AMMO,), **kw)
        for moved in (False, True):
            want[name, moved] = things_ref.sense(d['lines'], d['things'], st, prm, off if moved else None,
                                                 visible=poisoned(64, words), touched=poisoned(64, words))
    return dict(states=st, on_map=on_map, offsets=off, want=want)


def check_own_case():
    """on the reference's own result (runs on the CPU)"""
    d, c = level(), own_case()
    t_n = len(d['things'])
    assert t_n >= 33 and c['on_map'] == 58
    for (name, moved), w in c['want'].items():
        seen = np.array([v.sum() for v in w['visible_bits']])
        assert (seen[:c['on_map']] > 0).mean() > (0.5 if name == 'round' else 0.15) and (seen < t_n).all(), (name, moved, seen)
        assert not seen[c['on_map']:].any() and not w['touched'][c['on_map']:].any()  # outside the map and on NaNs: nothing
        assert (w['nearest']['index'][c['on_map']:] == -1).all()
        assert np.array_equal((w['nearest']['index'] >= 0).any(1), seen > 0)
    assert (c['want']['round', False]['visible'] != c['want']['round', True]['visible']).any()  # the doors count
    assert (c['want']['round', False]['visible'] != c['want']['cone', False]['visible']).any()  # and the cone


def test_the_levels_own_things():
    check_own_case()
    rd.set_device(0)
    d, c = level(), own_case()
    world = d['wad'].build_world(d['index'])
    things = rd.DeviceThings(d['things'])
    assert things.info() == (1, things_ref.words_of(len(d['things'])), int(d['things']['object_id'].max()))
    for (name, moved), want in c['want'].items():
        run(world, things, c['states'], want, dict(collect=(rd.THING_AMMO,), **(ROUND if name == 'round' else CONE)),
            offsets=c['offsets'] if moved else None, what=(name, moved))


# ---- 2. custom tables at the word, wave and pass boundaries -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def custom_case(size):
    d = level()
    rng = np.random.default_rng(CUSTOM_SEED * 1000 + size)
    st = things_ref.players_near(d['things'], 16, rng)
    table = things_ref.make_table(rng, size, things_ref.bounds_of(d['lines']), np.stack([st['pos'][:, 0], st['pos'][:, 2]], 1))
    off = reveal_ref.random_offsets(np.random.RandomState(size), 16, d['n_objects'])
    prm = things_ref.params(20.0, touch_radius=0.4, collect=(1, 4, 6))
    words = things_ref.words_of(size)
    want = things_ref.sense(d['lines'], table, st, prm, off, visible=poisoned(16, words), touched=poisoned(16, words))
    return dict(states=st, table=table, offsets=off, want=want, kw=dict(max_range=20.0, touch_radius=0.4, collect=(1, 4, 6)))


def check_custom_600():
    """asserted on the reference per launch at 600: at least 4 % of the (player, thing) pairs visible and at least 12 % in range but
    blocked (runs on the CPU)"""
    c = custom_case(600)
    vis = np.stack(c['want']['visible_bits'])
    st, table = c['states'], c['table']
    dx = table['x'][None, :] - st['pos'][:, 0][:, None]
    dz = table['z'][None, :] - st['pos'][:, 2][:, None]
    in_range = (dx * dx + dz * dz) <= F(20.0) * F(20.0)  # the launch looks all round: in range and not visible is blocked
    blocked = in_range & ~vis
    assert vis.mean() >= 0.04, vis.mean()
    assert blocked.mean() >= 0.12, blocked.mean()
    assert c['want']['touched'].any() and c['want']['new'].any()


@pytest.mark.parametrize('size', SIZES)
def test_custom_tables(size):
    if size == 600:
        check_custom_600()
    rd.set_device(0)
    d, c = level(), custom_case(size)
    world = d['wad'].build_world(d['index'])
    things = rd.DeviceThings(c['table'])
    assert things.words() == things_ref.words_of(size)
    run(world, things, c['states'], c['want'], c['kw'], offsets=c['offsets'], what=size)


# ---- 3. a door ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def door_case():
    """a thing 1.5 units behind the middle of E1M1's first push door, two players half a unit in front of it: player 0's game has the
    door at rest, player 1's has its object at the trigger's first height offset"""
    d = level()
    trig = d['host'].triggers()
    k = int(np.nonzero(trig['triggers']['trigger_type'] == rd.TRIGGER_PUSH)[0][0])
    t = trig['triggers'][k]
    effect = trig['effects'][t['effect_start']]
    assert t['effect_end'] > t['effect_start'] and effect['object_id'] > 0 and effect['first_height_offset'] > 0
    mid = t['origin'] + t['displace'] * F(0.5 * t['length'])
    normal = np.array([t['displace'][1], -t['displace'][0]], F)
    off = np.zeros((2, d['n_objects'], 3), F)
    off[1, effect['object_id'], 1] = effect['first_height_offset']
    for side in (1.0, -1.0):
        thing = np.zeros(1, rd.THING)
        thing['x'], thing['z'] = mid + normal * F(1.5 * side)
        thing['category'] = rd.THING_KEY
        eye = mid - normal * F(0.5 * side)
        st = rd.player_states(np.array([[eye[0], 0.0, eye[1]]] * 2, F), np.zeros(2, F))
        want = things_ref.sense(d['lines'], thing, st, things_ref.params(10.0), off)
        if want['visible'][:, 0].tolist() == [0, 1]:
            return dict(states=st, table=thing, offsets=off, want=want)
    raise AssertionError('neither side of the door hides the thing at rest and shows it when open')


def test_a_shut_door_hides_a_thing_from_the_player_who_has_not_opened_it():
    c = door_case()
    assert c['want']['nearest']['index'][:, rd.THING_KEY].tolist() == [-1, 0]
    rd.set_device(0)
    d = level()
    world = d['wad'].build_world(d['index'])
    run(world, rd.DeviceThings(c['table']), c['states'], c['want'], dict(max_range=10.0), offsets=c['offsets'], what='door')
    # with NULL offsets every object is at rest: both players' games have the door shut
    rest = things_ref.sense(d['lines'], c['table'], c['states'], things_ref.params(10.0))
    assert not rest['visible'].any()
    run(world, rd.DeviceThings(c['table']), c['states'], rest, dict(max_range=10.0), what='door at rest')


# ---- 4. collection ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def walk_case():
    """two candles (ammo) and a barrel (decoration) in a row from E1M1's start, 35 idle things behind them so that bit 37 is the last,
    and three stops: on candle 0, on the barrel, on candle 2.  Row word 1 carries a pre-set bit beyond T."""
    d = level()
    pos, yaw = d['wad'].build_level(d['index']).start()
    table = np.zeros(38, rd.THING)
    table['x'], table['z'], table['base'] = pos[0] + 500.0, pos[2], pos[1]
    table['category'] = rd.THING_UNKNOWN
    table['x'][:3] = pos[0] + F([0.0, 0.3, 0.6])
    table['z'][:3] = pos[2]
    table['base'][:3] = pos[1] - F(0.41)
    table['category'][:3] = (rd.THING_AMMO, rd.THING_DECORATION, rd.THING_AMMO)
    table['radius'][:3] = (0.08, 0.1, 0.08)
    stops = [0.0, 0.25, 0.6]
    prm = things_ref.params(8.0, collect=(rd.THING_AMMO,), touch_below=1.0, touch_above=1.0)
    row = np.zeros((1, 3), U)
    row[0, 1] = 1 << 20  # thing 52 of a table of 38: beyond T, preserved
    row[0, 2] = 0xDEAD
    calls, free = [], []
    for x in stops:
        st = rd.player_states(np.array([[pos[0] + F(x), pos[1], pos[2]]], F), np.array([yaw], F))
        want = things_ref.sense(d['lines'], table, st, prm, collected=row, visible=poisoned(1, 3), touched=poisoned(1, 3), stride=3)
        free.append(things_ref.sense(d['lines'], table, st, prm, stride=3))  # the same stop with nothing collected
        calls.append((st, row, want))
        row = want['collected']
    return dict(table=table, calls=calls, free=free, kw=dict(max_range=8.0, collect=(rd.THING_AMMO,), touch_below=1.0, touch_above=1.0))


def check_walk_case():
    c = walk_case()
    (_, _, w0), (_, _, w1), (_, _, w2) = c['calls']
    bit = lambda w, key, i: int(w[key][0, i >> 5] >> (i & 31)) & 1
    # stop 0: on candle 0 -- touched, collected, and still reported visible and nearest by this call
    assert bit(w0, 'touched', 0) and bit(w0, 'visible', 0) and w0['nearest']['index'][0, rd.THING_AMMO] == 0
    assert w0['new'][0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and w0['collected'][0].tolist() == [1, 1 << 20, 0xDEAD]
    # stop 1: candle 0 would be seen and touched, but it is gone; the barrel is touched and not collected
    assert bit(c['free'][1], 'visible', 0) and bit(c['free'][1], 'touched', 0)
    assert not bit(w1, 'visible', 0) and not bit(w1, 'touched', 0) and w1['nearest']['index'][0, rd.THING_AMMO] == 2
    assert bit(w1, 'touched', 1) and not w1['new'].any() and w1['collected'][0].tolist() == [1, 1 << 20, 0xDEAD]
    # stop 2: candle 2
    assert bit(w2, 'touched', 2) and w2['new'][0, rd.THING_AMMO] == 1 and w2['collected'][0].tolist() == [5, 1 << 20, 0xDEAD]
    assert not bit(w2, 'touched', 1)
    assert all(w['nearest']['index'][0, rd.THING_DECORATION] == 1 for w in (w0, w1, w2))  # the barrel is never collected
    assert all(w[key][0, 2] == POISON for w in (w0, w1, w2) for key in ('visible', 'touched'))  # a word beyond the level's is not written


def test_collection_along_a_walk():
    check_walk_case()
    rd.set_device(0)
    d, c = level(), walk_case()
    world = d['wad'].build_world(d['index'])
    things = rd.DeviceThings(c['table'])
    assert things.words() == 2
    for k, (st, before, want) in enumerate(c['calls']):
        run(world, things, st, want, c['kw'], collected=before, stride=3, what=('walk', k))


# ---- 5. a world set -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def set_case():
    wad = level()['wad']
    slots = [0, 2, 7]
    hosts = [wad.build_world(i, device=False) for i in slots]
    rng = np.random.default_rng(5)
    tables = [hosts[0].map_things(), things_ref.make_table(rng, 70, things_ref.bounds_of(hosts[1].map_lines()),
                                                           np.stack([hosts[1].map_things()['x'], hosts[1].map_things()['z']], 1)),
              hosts[2].map_things()[:9]]
    lv = np.array([0, 1, 2, 3, 1, 0, 2, 0xFFFFFFFF, 1, 2], U)
    st = np.concatenate([things_ref.players_near(hosts[min(int(s), 2)].map_things(), 1, rng) for s in lv])
    n_obj = max(h.game_objects for h in hosts)
    off = reveal_ref.random_offsets(np.random.RandomState(5), len(lv), n_obj)
    stride = things_ref.set_words(tables) + 2
    prm = things_ref.params(15.0, collect=range(8), touch_radius=0.5)
    want = things_ref.sense([h.map_lines() for h in hosts], tables, st, prm, off, lv, collected=poisoned(len(lv), stride) & U(0xFFFF0000),
                            visible=poisoned(len(lv), stride), touched=poisoned(len(lv), stride), stride=stride)
    return dict(slots=slots, tables=tables, levels=lv, states=st, offsets=off, stride=stride, want=want,
                kw=dict(max_range=15.0, collect=range(8), touch_radius=0.5))


def check_set_case():
    c = set_case()
    w, stride = c['want'], c['stride']
    assert [things_ref.words_of(len(t)) for t in c['tables']] == [2, 3, 1] and stride == 5
    for p, lv in enumerate(c['levels']):
        used = things_ref.words_of(len(c['tables'][lv])) if lv < 3 else 0
        assert (w['visible'][p, used:] == POISON).all() and (w['touched'][p, used:] == POISON).all()
        assert (w['collected'][p, used:] == POISON & 0xFFFF0000).all()
        if lv >= 3:
            assert (w['nearest']['index'][p] == -1).all() and not w['new'][p].any()
        else:
            assert (w['visible'][p, :used] != POISON).all()
    assert sum(bool(v.any()) for v in w['visible_bits']) >= 6 and w['new'].any()


def test_a_world_set_with_a_slot_out_of_range():
    check_set_case()
    rd.set_device(0)
    c = set_case()
    ws = level()['wad'].build_world_set(c['slots'])
    things = rd.DeviceThings(c['tables'])
    assert things.info()[:2] == (3, 3)
    run(ws, things, c['states'], c['want'], c['kw'], offsets=c['offsets'], levels=c['levels'],
        collected=poisoned(len(c['levels']), c['stride']) & U(0xFFFF0000), stride=c['stride'], what='set')


# ---- 6. every output alone ----------------------------------------------------------------------------------------------------------

def test_every_output_alone():
    rd.set_device(0)
    d, c = level(), custom_case(257)
    world = d['wad'].build_world(d['index'])
    things = rd.DeviceThings(c['table'])
    n, words = 16, things.words()
    off = torch.from_numpy(c['offsets']).cuda()
    states = _dev(c['states'])
    for name in ('collected', 'visible', 'touched', 'nearest', 'new'):
        if name == 'nearest':
            t = torch.full((n, 8, 4), 7.0, dtype=torch.float32, device='cuda')
        else:
            t = torch.zeros((n, words if name != 'new' else 8), dtype=torch.int32, device='cuda')
        key = name if name == 'collected' else name + '_out'
        out = world.sense_things(states, things, offsets=off, **{key: t}, **c['kw'])
        assert [o is not None for o in out] == [f == name for f in out._fields]
        _same(t, c['want'][name], name)


# ---- the errors that need a thing set -----------------------------------------------------------------------------------------------

def test_the_argument_errors_that_read_the_thing_set():
    rd.set_device(0)
    d = level()
    wad = d['wad']
    world, ws = wad.build_world(0), wad.build_world_set([0, 7])
    one, two = rd.DeviceThings(d['things']), rd.DeviceThings([d['things'], d['things'][:3]])
    moved = d['things'].copy()
    moved['object_id'][0] = d['n_objects'] + 5
    high = rd.DeviceThings(moved)
    assert high.info()[2] == d['n_objects'] + 5
    L = rd.lib()
    buf = torch.zeros(4096, dtype=torch.int32, device='cuda')  # two players at the origin, and room for what the good calls write
    ptr, rows_at, new_at = (ctypes.c_void_p(buf.data_ptr() + 4 * k) for k in (0, 1024, 2048))
    prm = rd.ThingSense(10.0, -1.0, 0.19, float('inf'), float('inf'), 0, 0)

    def sense(h, things, n=2, off=None, no=0, stride=2, rows=True, lv=ptr):
        r = rows_at if rows else None
        if h is ws:
            return L.rdoom_worldset_sense_things(h._h, things._h, ptr, lv, n, off, no, ctypes.byref(prm), None, r, None, stride, None, new_at, None)
        return L.rdoom_world_sense_things(h._h, things._h, ptr, n, off, no, ctypes.byref(prm), None, r, None, stride, None, new_at, None)

    def fails(word, *a, **kw):
        assert sense(*a, **kw) == -1, (a, kw)
        assert word in L.rdoom_last_error().decode(), L.rdoom_last_error()

    fails('levels', world, two)
    fails('levels', ws, one)
    fails('stride', world, one, stride=1)
    assert sense(world, one, stride=1, rows=False) == 0  # without a bit row the stride is not looked at
    fails('n_objects', world, one, off=ptr, no=1)
    fails('object_id', world, high, off=ptr, no=d['n_objects'])
    assert sense(world, high, no=0) == 0  # NULL offsets: every object at rest, whatever its id
    assert sense(world, one, n=0) == 0 and sense(ws, two, n=0, lv=None) == 0  # n == 0 queues nothing
    fails('null', ws, two, lv=None)
    torch.cuda.synchronize()
    empty = rd.DeviceThings([np.zeros(0, rd.THING)])  # a level may hold no thing
    assert empty.info() == (1, 1, 0)
    out = world.sense_things(_dev(rd.player_states(np.zeros((1, 3), F), np.zeros(1, F))), empty, 10.0)
    assert (_u32(out.nearest.view(torch.int32))[:, :, 0] == 0xFFFFFFFF).all() and not _u32(out.new).any()
    for t in (one, two, high, empty):
        t.close()


# ---- 7. streams, tensors, pointers, a graph -----------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_things_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_things_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
