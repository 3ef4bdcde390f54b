"""The rays that see things on the GPU (raythings.hip: cast_rays_things_kernel and its world-set twin) against
tests/raythings_ref.py, include/rdoom_rays.h restated in numpy with no cull and no list: every word of frac_out as a uint32 pattern
and every thing_out, with no tolerance.  The hand cases of tests/raythings_cases.py, one player a case in one launch; random tables
at the word, wave and pass boundaries and one longer than the kernel's list, with 1 to 257 rays, random select and hidden rows in a
wider, poisoned stride, offsets, hanging things, and fractions from World.cast_rays, from NULL and from a tensor with +inf and NaN;
in place against out of place, thing_out NULL; cast_rays' own origin and vel through the reference; the synthetic E1M1's barrels
and a collected thing; a set of three levels against the three single worlds; the argument errors that read a handle; streams, raw
pointers, a stepping loop and a captured graph in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_ref
import raythings_cases as rc
import raythings_ref as rt
import rust_doom_amd as rd
import stamp_cases as sc

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
POISON_F, POISON_I = 7.0, 0x5EEEEEEE


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).cuda()


def _rows(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _states(st):
    return torch.from_numpy(np.ascontiguousarray(st, rd.PLAYER_STATE).view(np.uint8).reshape(-1).copy()).cuda()


def same(got, want, what):
    a, b = got.cpu().numpy().view(U), np.ascontiguousarray(want).view(U)  # words, not values
    bad = a != b
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], a[bad][:6], b[bad][:6])


def check(cast, frac, want, what, **kw):
    """one launch out of place into poisoned tensors, one allocated without the indices, one in place; each against the
    reference's (frac, thing).  cast(**kw) is the bound call; frac: the world's fractions as a host array, or None"""
    shape = want[0].shape
    f = None if frac is None else _dev(frac, F)
    out = torch.full(shape, POISON_F, device='cuda')
    thing = torch.full(shape, POISON_I, dtype=torch.int32, device='cuda')
    got = cast(frac=f, frac_out=out, thing_out=thing, **kw)
    assert got[0] is out and got[1] is thing
    same(out, want[0], (what, 'frac')), same(thing, want[1], (what, 'thing'))
    if f is not None:
        same(f, frac, (what, 'the input fractions'))  # out of place: the input stands
    got = cast(frac=f, **kw)  # allocated, thing_out NULL
    assert got[1] is None and got[0].dtype == torch.float32 and tuple(got[0].shape) == shape
    same(got[0], want[0], (what, 'frac alone'))
    if f is not None:
        got = cast(frac=f, frac_out=f, thing_out=True, **kw)
        assert got[0] is f and got[1].dtype == torch.int32
        same(f, want[0], (what, 'frac in place')), same(got[1], want[1], (what, 'thing in place'))


@pytest.fixture(scope='module')
def e1m1():
    rd.set_device(0)
    wad = sc.e1m1_wad()
    world = wad.build_world(0)
    yield wad, world
    world.close()


# ---- the hand cases -------------------------------------------------------------------------------------------------------------------

def test_the_hand_cases_one_player_a_case_in_one_launch():
    rd.set_device(0)
    world = sc.room_wad(2, 2).build_world(0)
    assert world.game_objects <= rc.N_OBJECTS
    cases = [c for c in rc.hand_cases() if c['gpu']]  # (the library refuses offsets whose row ends at or below an object_id: below)
    a = rc.assemble(cases)
    want = rt.cast(a['table'], a['states'], a['dirs'], rc.MAX_RANGE, heights=rc.HEIGHTS, categories=rc.CATEGORIES, select=a['select'],
                   hidden=a['hidden'], offsets=a['offsets'], frac=a['frac'])
    rc.check(a['want'], *want)
    things = rd.DeviceThings(a['table'])
    st, dirs = _states(a['states']), _dev(a['dirs'])
    cats = [c for c in range(8) if (rc.CATEGORIES >> c) & 1]
    kw = dict(heights=rc.HEIGHTS, categories=cats, select=_rows(a['select']), hidden=_rows(a['hidden']), offsets=_dev(a['offsets']))
    check(lambda **k: world.cast_rays_things(st, things, dirs, rc.MAX_RANGE, **k), a['frac'], want, 'hand cases', **kw)
    out, thing = world.cast_rays_things(st, things, dirs, rc.MAX_RANGE, frac=_dev(a['frac']), thing_out=True, **kw)
    rc.check(a['want'], out.cpu().numpy(), thing.cpu().numpy())
    things.close()
    beyond = rd.DeviceThings(rt.table_of([0.0], [0.0], [0.0], [0.5], [0], object_id=[5]))
    with pytest.raises(rd.RdoomError) as e:
        world.cast_rays_things(st, beyond, dirs, rc.MAX_RANGE, offsets=_dev(np.zeros((len(cases), 5, 3), F)))
    assert e.value.status == -1 and 'object_id' in str(e.value)
    beyond.close(), world.close()


# ---- random tables ----------------------------------------------------------------------------------------------------------------------

N = 5  # players of a random launch
RANGE = 5.0


def field_of(e1m1, size, seed, spread=3.0):
    """(states, table, offsets): N players of E1M1 at rest height over floor centroids, `size` things scattered about them at about
    their height, and a row of offsets per player"""
    wad, world = e1m1
    rng = np.random.default_rng(seed)
    st = np.array(rays_ref.players(wad.build_level(0), seed, count=N), rd.PLAYER_STATE)
    n_obj = world.game_objects + 1
    table = rc.random_table(rng, size, st['pos'][:, [0, 2]], spread, n_obj, base=st['pos'][:, 1] - F(0.33))
    offsets = np.zeros((N, n_obj, 3), F)
    offsets[:, :, 1] = rng.choice(F([0.0, 0.0, 0.25, -0.5]), (N, n_obj))
    return st, table, offsets, rng


@pytest.mark.parametrize('size', rc.SIZES + (700,))
def test_random_tables_at_the_word_wave_and_pass_boundaries_and_beyond_the_list(e1m1, size):
    """every ray count of RAY_COUNTS, the world's fractions taken in turn from World.cast_rays on the same rays, from NULL and from a
    tensor with +inf and NaN entries.  At 700 every thing is within reach of every player (spread 1, range 5): the list is folded
    and emptied once, and things of both parts win rays"""
    wad, world = e1m1
    st, table, offsets, rng = field_of(e1m1, size, 9000 + size, spread=1.0 if size > rc.LIST_CAPACITY else 3.0)
    if size > rc.LIST_CAPACITY:
        table['base'][50:600] += F(3.0)  # in reach and in the list, but over the rays' heads: they leave rays to the things behind the fold
    things = rd.DeviceThings(table)
    stride = things.words() + 1
    select, hidden = rc.random_rows(rng, 1, size, stride, 0.8), rc.random_rows(rng, N, size, stride, 0.2)
    states, off = _states(st), _dev(offsets)
    cats = [0, 1, 2, 3, 4, 5, 7]
    named = set()
    for k, n_rays in enumerate(rc.RAY_COUNTS):
        dirs = rd.ray_fan(n_rays, 2.5, pitch=0.05 * (k - 2))
        d = _dev(dirs)
        mode = ('world', None, 'mixed')[(k + size) % 3]
        if mode == 'world':
            frac = world.cast_rays(states, d, RANGE, offsets=off[:, :world.game_objects].contiguous()).cpu().numpy()
        else:
            frac = None if mode is None else rc.random_frac(rng, (N, n_rays))
        ref = dict(heights=rc.RANDOM_HEIGHTS, grow=0.05, categories=sum(1 << c for c in cats), select=select, hidden=hidden, offsets=offsets)
        want = rt.cast(table, st, dirs, RANGE, frac=frac, **ref)
        named |= set(want[1][want[1] >= 0].tolist())
        kw = dict(heights=rc.RANDOM_HEIGHTS, grow=0.05, categories=cats, select=_rows(select), hidden=_rows(hidden), offsets=off)
        check(lambda **q: world.cast_rays_things(states, things, d, RANGE, **q), frac, want, (size, n_rays, mode), **kw)
    if size >= 64:
        assert len(named) >= 5, named  # the rays end on things
    if size > rc.LIST_CAPACITY:
        assert max(named) >= rc.LIST_CAPACITY and min(named) < rc.LIST_CAPACITY  # on both sides of the fold
    things.close()


def test_without_rows_offsets_or_parameters_and_a_fold_at_every_pass(e1m1):
    """the defaults -- every thing, nothing hidden, at rest, heights 0.56 -- on 1300 things about one point: five passes, two folds"""
    wad, world = e1m1
    st, table, _, rng = field_of(e1m1, 1300, 77, spread=0.8)
    table['base'][40:1100] += F(3.0)  # over the rays' heads
    things = rd.DeviceThings(table)
    dirs = rd.ray_fan(64, 6.0)
    want = rt.cast(table, st, dirs, RANGE)
    assert (want[1] >= 2 * rc.LIST_CAPACITY).any() and (want[1] >= 0).mean() > 0.5
    check(lambda **k: world.cast_rays_things(_states(st), things, _dev(dirs), RANGE, **k), None, want, 'defaults')
    things.close()


def test_cast_rays_own_origin_and_vel_through_the_reference(e1m1):
    """both kernels use the same ray: the reference fed with what cast_rays wrote as origin_out and vel_out, not with its own rays"""
    wad, world = e1m1
    st, table, offsets, rng = field_of(e1m1, 200, 4242)
    for dirs, rng_ in ((rays_ref.odd_table(), 4.0), (rd.ray_fan(33, 3.0, pitch=-0.3), 30.0)):
        states, d = _states(st), _dev(dirs)
        shape = (len(st), len(dirs), 3)
        origin, vel = torch.zeros(shape, device='cuda'), torch.zeros(shape, device='cuda')
        frac = world.cast_rays(states, d, rng_, origin_out=origin, vel_out=vel)
        things = rd.DeviceThings(table)
        want = rt.cast(table, None, None, rng_, frac=frac.cpu().numpy(), origin=origin.cpu().numpy(), vel=vel.cpu().numpy())
        assert (want[1] >= 0).any()
        got = world.cast_rays_things(states, things, d, rng_, frac=frac, thing_out=True)
        same(got[0], want[0], 'frac of cast_rays\' rays'), same(got[1], want[1], 'thing of cast_rays\' rays')
        own = rt.rays(st, dirs, rng_)  # and the reference's own rays are those
        same(vel, own[1], 'vel'), same(origin, np.broadcast_to(own[0][:, None, :], shape), 'origin')
        things.close()


# ---- the synthetic E1M1 -------------------------------------------------------------------------------------------------------------------

def test_e1m1_rays_end_on_the_barrels_and_pass_what_their_player_collected(e1m1):
    wad, world = e1m1
    table = world.map_things()
    things = rd.DeviceThings(table)
    solid = rd.pack_things(world.thing_obstacles()).view(U)[None]
    barrels = list(sc.E1M1_BARRELS)
    assert rd.unpack_things(solid[0], len(table))[barrels].all()
    # a player 0.7 from each barrel, at rest height above its base, with a fan all round
    pos = np.stack([table['x'][barrels] - F(0.7), table['base'][barrels] + F(0.33), table['z'][barrels]], 1).astype(F)
    st = rd.player_states(pos, np.linspace(0.0, 3.0, len(barrels)).astype(F))
    dirs = rd.ray_fan(64, 2 * np.pi, pitch=-0.3)  # looking down a little: the eye, 0.45 up, is above a barrel's 0.42
    states, d = _states(st), _dev(dirs)
    frac, hit = world.cast_rays(states, d, 30.0, hit_out=True)
    before = frac.cpu().numpy().copy()
    want = rt.cast(table, st, dirs, 30.0, heights=0.42, select=solid, frac=before)
    out, thing = world.cast_rays_things(states, things, d, 30.0, heights=0.42, select=_rows(solid), frac=frac, frac_out=frac, thing_out=True)
    same(out, want[0], 'E1M1 frac'), same(thing, want[1], 'E1M1 thing')
    got_t, got_f = thing.cpu().numpy(), out.cpu().numpy()
    for p, b in enumerate(barrels):  # every player's fan ends on its barrel somewhere, nearer than the world was
        on = got_t[p] == b
        assert on.any() and (got_f[p][on] < before[p][on]).all() and (got_f[p][on] * 30.0 < 0.7).all(), (p, b)
    assert set(got_t[got_t >= 0].tolist()) <= set(np.nonzero(rd.unpack_things(solid[0], len(table)))[0].tolist())
    # two players: one stands on the candle and collects it, the other 0.8 away does not
    candle = 17
    assert (table['category'][candle] & 0xFF) == rd.THING_AMMO
    t = table[candle]
    pos = F([[t['x'], t['base'] + 0.33, t['z']], [t['x'], t['base'] + 0.33, t['z'] + 0.8]])
    st = rd.player_states(pos, F([0.0, 0.0]))
    states = _states(st)
    collected = torch.zeros((2, things.words()), dtype=torch.int32, device='cuda')
    seen = lambda **k: world.cast_rays_things(states, things, d, 30.0, heights=0.56, categories=[rd.THING_AMMO], thing_out=True, **k)
    _, first = seen(hidden=collected)
    first = first.cpu().numpy()
    assert (first[0] == candle).all() and (first[1] == candle).any()  # an eye inside the candle: every ray ends at 0
    world.sense_things(states, things, max_range=10.0, touch_below=1.0, touch_above=1.0, collect=(rd.THING_AMMO,), collected=collected)
    rows = collected.cpu().numpy().view(U)
    assert (rows[0, candle >> 5] >> (candle & 31)) & 1 and not (rows[1, candle >> 5] >> (candle & 31)) & 1
    out, after = seen(hidden=collected)
    want = rt.cast(table, st, dirs, 30.0, heights=0.56, categories=1 << rd.THING_AMMO, hidden=rows)
    same(out, want[0], 'after the pick-up, frac'), same(after, want[1], 'after the pick-up, thing')
    after = after.cpu().numpy()
    assert not (after[0] == candle).any() and np.array_equal(after[1] == candle, first[1] == candle)
    things.close()


# ---- a set ----------------------------------------------------------------------------------------------------------------------------------

def test_a_set_of_three_levels_against_the_three_single_worlds():
    """players grouped by level, then shuffled, one of them on a slot outside the set: per player what the single world of its level
    gives with that level's table and select row; the outsider keeps its fractions, index -1"""
    rd.set_device(0)
    wad, indices = sc.e1m1_wad(), [1, 6, 2]
    ws = wad.build_world_set(indices)
    rng = np.random.default_rng(336)
    per = 3
    sts, tables, n_obj = [], [], ws.n_objects + 1
    for slot, i in enumerate(indices):
        st = np.array(rays_ref.players(wad.build_level(i), 50 + slot, count=per), rd.PLAYER_STATE)
        sts.append(st)
        tables.append(rc.random_table(rng, (40, 300, 65)[slot], st['pos'][:, [0, 2]], 2.0, n_obj, base=st['pos'][:, 1] - F(0.33)))
    things = rd.DeviceThings(tables)
    stride = things.words() + 2
    select = np.concatenate([rc.random_rows(rng, 1, len(t), stride, 0.8) for t in tables])
    dirs = rd.ray_fan(100, 3.0)
    d = _dev(dirs)
    for order in ('grouped', 'shuffled'):
        levels = np.repeat(np.arange(3, dtype=U), per)
        st = np.concatenate(sts)
        outsider = rays_ref.players(wad.build_level(1), 9, count=1)
        levels, st = np.concatenate([levels, U([7])]), np.concatenate([st, np.array(outsider, rd.PLAYER_STATE)])
        if order == 'shuffled':
            perm = rng.permutation(len(st))
            levels, st = levels[perm], st[perm]
        n = len(st)
        hidden = np.stack([rc.random_rows(rng, 1, len(tables[lv]) if lv < 3 else 0, stride, 0.2)[0] for lv in levels])
        offsets = np.zeros((n, n_obj, 3), F)
        offsets[:, :, 1] = rng.choice(F([0.0, 0.25]), (n, n_obj))
        frac = rc.random_frac(rng, (n, len(dirs)))
        kw = dict(heights=rc.RANDOM_HEIGHTS, grow=0.1)
        want = rt.cast(tables, st, dirs, RANGE, levels=levels, select=select, hidden=hidden, offsets=offsets, frac=frac, **kw)
        out_p = int(np.nonzero(levels == 7)[0][0])
        assert (want[1][out_p] == -1).all() and np.array_equal(want[0][out_p].view(U), frac[out_p].view(U))
        assert all((want[1][levels == lv] >= 0).any() for lv in range(3))
        lv_t, states = _rows(levels), _states(st)
        dev_kw = dict(select=_rows(select), hidden=_rows(hidden), offsets=_dev(offsets), **kw)
        check(lambda **k: ws.cast_rays_things(states, lv_t, things, d, RANGE, **k), frac, want, ('a set', order), **dev_kw)
        if order == 'shuffled':
            for slot, i in enumerate(indices):  # the single worlds
                mine = np.nonzero(levels == slot)[0]
                world, single = wad.build_world(i), rd.DeviceThings(tables[slot])
                got = world.cast_rays_things(_states(st[mine]), single, d, RANGE, select=_rows(select[slot:slot + 1]), hidden=_rows(hidden[mine]),
                                             offsets=_dev(offsets[mine]), frac=_dev(frac[mine]), thing_out=True, **kw)
                same(got[0], want[0][mine], ('single world', slot, 'frac')), same(got[1], want[1][mine], ('single world', slot, 'thing'))
                single.close(), world.close()
    things.close(), ws.close()


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------

def test_the_errors_that_read_a_handle_and_what_queues_nothing(e1m1):
    wad, world = e1m1
    st, table, offsets, rng = field_of(e1m1, 40, 5)
    table['object_id'][3] = world.game_objects  # the set's largest object
    things, two = rd.DeviceThings(table), rd.DeviceThings([table, table])
    states, d = _states(st), _dev(rd.ray_fan(8, 1.0))
    frac = torch.full((N, 8), 0.5, device='cuda')
    rows = torch.zeros((N, 1), dtype=torch.int32, device='cuda')

    def refused(word, handle=world, th=things, **kw):
        with pytest.raises(rd.RdoomError) as e:
            handle.cast_rays_things(states, th, d, RANGE, frac=frac, **kw)
        assert e.value.status == -1 and word in str(e.value), e.value

    refused('HOST_ONLY', handle=wad.build_world(0, device=False))
    refused('thing set of 2 levels', th=two)
    refused('stride', hidden=rows.data_ptr(), stride=1)  # 40 things take two words
    refused('stride', select=rows.data_ptr(), stride=0)
    refused('n_objects', offsets=torch.zeros((N, world.game_objects, 3), device='cuda'))  # not above the largest object_id
    refused('n_objects', offsets=torch.zeros((N, 1, 3), device='cuda'))
    refused('overlap in part', frac_out=frac.data_ptr() + 4)
    refused('overlap in part', frac_out=frac.data_ptr() - 4 * (N * 8 - 1))
    for word, bad in (('height', dict(heights=-1.0)), ('height', dict(heights=float('nan'))), ('grow', dict(grow=-0.1)), ('grow', dict(grow=float('inf')))):
        refused(word, **bad)
    torch.cuda.synchronize()
    assert (frac.cpu().numpy() == 0.5).all()  # nothing was queued
    # the set form: null levels, and a thing set of another size
    ws = wad.build_world_set([1, 6])
    with pytest.raises(rd.RdoomError) as e:
        ws.cast_rays_things(states, None, two, d, RANGE)
    assert 'levels' in str(e.value)
    with pytest.raises(rd.RdoomError) as e:
        ws.cast_rays_things(states, torch.zeros(N, dtype=torch.int32, device='cuda'), things, d, RANGE)
    assert 'thing set of 1 levels' in str(e.value)
    # n == 0 queues nothing and writes nothing
    got = world.cast_rays_things(states, things, d, RANGE, n=0, frac=frac, frac_out=frac, thing_out=rows)
    torch.cuda.synchronize()
    assert got[0] is frac and (frac.cpu().numpy() == 0.5).all() and (rows.cpu().numpy() == 0).all()
    for t in (things, two, ws):
        t.close()


# ---- streams, tensors, pointers, a stepping loop, a graph ---------------------------------------------------------------------------------

def test_streams_raw_pointers_a_stepping_loop_and_a_graph_in_one_child():
    """tests/gpu_raythings_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_raythings_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
