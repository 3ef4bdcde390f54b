"""GPU: WHERE rdoom_world_cast_rays_things writes.  Every array -- the states, the directions, the select and hidden rows, the
offsets and the world's fractions going in, the fractions and the indices coming out -- is a carving of a guarded arena
(tests/guarded.py) at the least alignment the header allows, 4 and 12 mod 16.  After the call every byte outside the outputs, the
inputs included, must be what it was, and the outputs must equal tests/raythings_ref.py word for word and index for index, with the
arena poisoned 0xFF and 0x00.  Tables of 33 things (two words, one bit in the second) and 257 (a second pass of one thing), 7 rays
and 3 players a launch, out of place and in place."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import raythings_cases as rc
import raythings_ref as rt
import rust_doom_amd as rd
import stamp_cases as sc
from guarded import GUARD, run_guarded

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
N, RAYS, RANGE = 3, 7, 4.0


@functools.lru_cache(maxsize=None)
def case(size):
    """computed once and left unchanged: three players in a one-room level, a random table about them whose last thing stands in
    front of player 0, a select row and three hidden rows, offsets, world fractions with +inf and NaN, and the reference's results"""
    wad = sc.room_wad(4, 4)
    host = wad.build_world(0, device=False)
    rng = np.random.default_rng(330 + size)
    pos = np.stack([rng.uniform(-3.5, -1.5, N), np.full(N, 0.33), rng.uniform(-3.5, -1.5, N)], 1).astype(F)
    st = rd.player_states(pos, rng.uniform(-3, 3, N).astype(F), pitch=rng.uniform(-0.2, 0.2, N).astype(F))
    n_obj = max(4, host.game_objects)
    table = rc.random_table(rng, size, pos[:, [0, 2]], 2.0, n_obj)
    dirs = rd.ray_fan(RAYS, 2.0)
    origin, vel = rt.rays(st, dirs, RANGE)
    last = size - 1  # alone in its word or its pass: on player 0's middle ray, a quarter of the way along
    at = origin[0] + F(0.25) * vel[0, RAYS // 2]
    table['x'][last], table['z'][last], table['base'][last], table['radius'][last] = at[0], at[2], at[1] - F(0.3), 0.05
    table['category'][last], table['object_id'][last] = 0, 0
    words = (size + 31) // 32
    select = rc.random_rows(rng, 1, size, words, 0.8)
    select[0, last // 32] |= U(1) << U(last % 32)
    hidden = rc.random_rows(rng, N, size, words, 0.2)
    hidden[0] = U(0xFFFFFFFF)  # player 0 sees the last thing alone
    hidden[0, last // 32] = ~(U(1) << U(last % 32))
    offsets = np.zeros((N, n_obj, 3), F)
    offsets[:, 1:, 1] = rng.choice(F([0.0, 0.25]), (N, n_obj - 1))
    frac = rc.random_frac(rng, (N, RAYS))
    frac[0, RAYS // 2] = np.inf
    kw = dict(heights=rc.RANDOM_HEIGHTS, grow=0.02)
    want = rt.cast(table, st, dirs, RANGE, select=select, hidden=hidden, offsets=offsets, frac=frac, **kw)
    return dict(wad=wad, states=st, dirs=dirs, table=table, words=words, select=select, hidden=hidden, offsets=offsets, frac=frac, kw=kw, want=want)


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('size', [33, 257])
@pytest.mark.parametrize('residue', [4, 12])
def test_world_cast_rays_things(residue, size, in_place):
    rd.set_device(0)
    c = case(size)
    want_f, want_t = c['want']
    assert (want_t >= 0).any(1).all() and (want_t < 0).any() and want_t[0, RAYS // 2] == size - 1
    world, things = c['wad'].build_world(0), rd.DeviceThings(c['table'])
    assert things.words() == c['words']

    def setup(arena):
        at, other = residue, 16 - residue
        st = arena.place(np.ascontiguousarray(c['states'], rd.PLAYER_STATE), 16, at, 'states')
        dirs = arena.place(c['dirs'], 16, other, 'dirs', torch.float32)
        sel = arena.place(c['select'].view(np.int32), 16, at, 'select', torch.int32)
        hid = arena.place(c['hidden'].view(np.int32), 16, other, 'hidden', torch.int32)
        off = arena.place(c['offsets'], 16, at, 'offsets', torch.float32)
        frac = arena.place(c['frac'], 16, other, 'frac', torch.float32)
        thing = arena.carve((N, RAYS), torch.int32, 16, at, 'thing_out')
        out = frac if in_place else arena.carve((N, RAYS), torch.float32, 16, at, 'frac_out')
        assert {t.data_ptr() % 16 for t in (st, dirs, sel, hid, off, frac, thing, out)} == {4, 12}
        call = lambda: world.cast_rays_things(st, things, dirs, RANGE, select=sel, hidden=hid, offsets=off, frac=frac, frac_out=out, thing_out=thing,
                                              **c['kw'])
        return call, [('frac', out, want_f), ('thing', thing, want_t)]
    run_guarded(16 * (2 * GUARD + 4096), setup, 'rays against %d things at %d mod 16, in_place=%s' % (size, residue, in_place))
    things.close(), world.close()
