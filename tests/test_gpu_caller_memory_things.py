"""GPU: WHERE rdoom_world_sense_things and rdoom_worldset_sense_things write.  Every array -- states, level slots, offsets and the
collected rows going in, the collected, visible and touched rows, the nearest records and the counts coming out -- is a carving of a
guarded arena (tests/guarded.py) at the least alignment the header allows, 4 and 12 mod 16.  After the call every byte outside the
outputs, the inputs included, must be what it was, and the outputs must equal tests/things_ref.py bit for bit, with the arena
poisoned 0xFF and 0x00.  Tables of 33 things (two words, one bit in the second) and 257 (a second pass of one thing), three players
a launch."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import reveal_ref
import rust_doom_amd as rd
import things_ref
from guarded import GUARD, run_guarded
from util import META_PATH, ensure_wad

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
N = 3
KW = dict(max_range=20.0, fov=3.0, touch_radius=0.5, collect=(0, 2, 4, 6))
SEEDS = {33: 33, 257: 257}  # picked on the CPU so that the reference's world result touches and collects something at both sizes


@functools.lru_cache(maxsize=None)
def case(size):
    """computed once and left unchanged: the tables of two levels, three players next to things of theirs, offsets, rows in which
    some things are collected already, and the reference's results for the world (level 0) and for the set (slots 1, 0 and 5)"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    hosts = [wad.build_world(i, device=False) for i in (0, 2)]
    rng = np.random.default_rng(SEEDS[size])
    own = [h.map_things() for h in hosts]
    tables = [things_ref.make_table(rng, size if k == 0 else 40, things_ref.bounds_of(h.map_lines()), np.stack([t['x'], t['z']], 1))
              for k, (h, t) in enumerate(zip(hosts, own))]
    n_obj = max(h.game_objects for h in hosts)
    off = reveal_ref.random_offsets(np.random.RandomState(size), N, n_obj)
    words = things_ref.set_words(tables)
    before = rng.integers(0, 1 << 32, (N, words), dtype=np.uint64).astype(U) & rng.integers(0, 1 << 32, (N, words), dtype=np.uint64).astype(U)
    prm = things_ref.params(**KW)
    st = things_ref.players_near(tables[0], N, rng, spread=0.25)
    world = things_ref.sense(hosts[0].map_lines(), tables[0], st, prm, off, collected=before)
    lv = np.array([1, 0, 5], U)
    st_set = np.concatenate([things_ref.players_near(tables[min(int(s), 1)], 1, rng, spread=0.25) for s in lv])
    return dict(wad=wad, tables=tables, offsets=off, before=before, words=words, states=st, world=world, levels=lv, set_states=st_set,
                lines=[h.map_lines() for h in hosts], prm=prm)


def place_inputs(arena, c, states, residue):
    other = 16 - residue
    s = arena.place(states, 16, residue, 'states')
    o = arena.place(c['offsets'], 16, other, 'offsets', torch.float32)
    col = arena.place(c['before'].view(np.int32), 16, residue, 'collected', torch.int32)
    vis = arena.carve((N, c['words']), torch.int32, 16, other, 'visible_out')
    tch = arena.carve((N, c['words']), torch.int32, 16, residue, 'touched_out')
    near = arena.carve((N, 8, 4), torch.float32, 16, other, 'nearest_out')
    new = arena.carve((N, 8), torch.int32, 16, residue, 'new_out')
    assert {t.data_ptr() % 16 for t in (s, o, col, vis, tch, near, new)} == {4, 12}
    return s, o, col, vis, tch, near, new


@pytest.mark.parametrize('size', [33, 257])
@pytest.mark.parametrize('residue', [4, 12])
def test_world_sense_things(size, residue):
    rd.set_device(0)
    c = case(size)
    want = c['world']
    assert want['visible'].any() and want['touched'].any() and want['new'].any() and (want['collected'] != c['before']).any()
    world = c['wad'].build_world(0)
    things = rd.DeviceThings(c['tables'][0])
    assert things.words() == c['words'] == (size + 31) // 32

    def setup(arena):
        s, o, col, vis, tch, near, new = place_inputs(arena, c, c['states'], residue)
        call = lambda: world.sense_things(s, things, offsets=o, collected=col, visible_out=vis, touched_out=tch, nearest_out=near, new_out=new,
                                          **KW)
        return call, [('collected', col, want['collected']), ('visible', vis, want['visible']), ('touched', tch, want['touched']),
                      ('nearest', near, want['nearest'].view(U).reshape(N, 8, 4)), ('new', new, want['new'])]
    run_guarded(16 * (GUARD + 4096), setup, 'sense_things %d at %d' % (size, residue))


@pytest.mark.parametrize('size', [33, 257])
@pytest.mark.parametrize('residue', [4, 12])
def test_worldset_sense_things(size, residue):
    """slots 1, 0 and one outside the set: the rows of the player outside, and the words beyond the 40 things of slot 1, keep the
    arena's poison, so the reference starts from it too"""
    rd.set_device(0)
    c = case(size)
    ws = c['wad'].build_world_set([0, 2])
    things = rd.DeviceThings(c['tables'])
    words = c['words']

    def setup(arena):
        s, o, col, vis, tch, near, new = place_inputs(arena, c, c['set_states'], residue)
        lv = arena.place(c['levels'].view(np.int32), 16, 16 - residue, 'levels', torch.int32)
        poison = np.full((N, words), arena.poison * 0x01010101, U)
        want = things_ref.sense(c['lines'], c['tables'], c['set_states'], c['prm'], c['offsets'], c['levels'], collected=c['before'],
                                visible=poison, touched=poison)
        assert (want['visible'][:2] != poison[:2]).any() and (want['visible'][2] == poison[2]).all() and not want['new'][2].any()
        call = lambda: ws.sense_things(s, lv, things, offsets=o, collected=col, visible_out=vis, touched_out=tch, nearest_out=near,
                                       new_out=new, **KW)
        # the rows that keep poison differ between the runs by design: their extents are checked, their values against this run's
        check = lambda: [np.array_equal(t.cpu().numpy().view(U), want[k]) for k, t in (('collected', col), ('visible', vis), ('touched', tch))]
        setup.checks.append(check)
        return call, [('collected', col, None), ('visible', vis, None), ('touched', tch, None), ('nearest', near, want['nearest'].view(U).reshape(N, 8, 4)),
                      ('new', new, want['new'])]
    setup.checks = []
    run_guarded(16 * (GUARD + 4096), setup, 'worldset sense_things %d at %d' % (size, residue))
    assert len(setup.checks) == 2 and all(all(check()) for check in setup.checks)
