"""GPU: WHERE rdoom_world_stamp_things writes.  Every array -- the planes, the solid and hidden rows and the offsets going in, the
planes and the index plane coming out -- is a carving of a guarded arena (tests/guarded.py) at the least alignment the header
allows, 4 and 12 mod 16.  After the call every byte outside the outputs, the inputs included, must be what it was, and the outputs
must equal tests/stamp_ref.py word for word and index for index, with the arena poisoned 0xFF and 0x00.  Tables of 33 things (two
words, one bit in the second) and 257 (a second pass of one thing), three rows a launch at 77 x 53 (two tiles by four, the last
column 13 cells wide, the last row 5 high), out of place and in place."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import goal_ref
import rust_doom_amd as rd
import stamp_cases as sc
import stamp_ref
from guarded import GUARD, run_guarded

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
N = 3
SHAPE = (N, 53, 77)


@functools.lru_cache(maxsize=None)
def case(size):
    """computed once and left unchanged: a random table over a one-room level whose grid is 77 x 53, a solid row and three hidden
    rows, floors of several heights, offsets, a finite window, and the reference's results"""
    wad, host, cell, grid = sc.room_of_grid(77, 53)
    rng = np.random.default_rng(770 + size)
    x, z = goal_ref.centres(grid, cell)
    table = np.zeros(size, rd.THING)
    table['x'], table['z'] = rng.uniform(x[0], x[-1], size).astype(F), rng.uniform(z[0], z[-1], size).astype(F)
    table['radius'] = rng.uniform(0, 3 * cell, size).astype(F)
    table['base'] = rng.choice(F([0.0, 0.25, 0.5]), size)
    table['object_id'] = rng.integers(0, 4, size)
    words = (size + 31) // 32
    solid = rd.pack_things(rng.random(words * 32) < 40.0 / size).view(U)[None].copy()
    solid[0, (size - 1) // 32] |= U(1) << U((size - 1) % 32)  # the last thing, alone in its word or its pass, is solid
    hidden = (rng.integers(0, 1 << 32, (N, words), dtype=np.uint64) & rng.integers(0, 1 << 32, (N, words), dtype=np.uint64)).astype(U)
    hidden[0] = 0
    floor = rng.choice(F([0.0, 0.25, 0.5]), SHAPE)
    ceiling = floor + F(1.28)
    offsets = np.zeros((N, max(4, host.game_objects), 3), F)
    offsets[:, :, 1] = rng.choice(F([0.0, 0.25]), offsets.shape[:2])
    window = dict(grow=0.01, block_below=0.25, block_above=0.25)
    want = stamp_ref.stamp(table, grid, cell, floor, ceiling, solid=solid, hidden=hidden, offsets=offsets, **window)
    return dict(wad=wad, cell=cell, table=table, words=words, solid=solid, hidden=hidden, floor=floor, ceiling=ceiling, offsets=offsets,
                window=window, want=want)


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('size', [33, 257])
@pytest.mark.parametrize('residue', [4, 12])
def test_world_stamp_things(residue, size, in_place):
    rd.set_device(0)
    c = case(size)
    want_f, want_c, want_i = c['want']
    blocked = want_i >= 0
    assert blocked.reshape(N, -1).any(1).all() and not blocked.all() and (want_i == size - 1).any()
    world, things = c['wad'].build_world(0), rd.DeviceThings(c['table'])
    assert things.words() == c['words']

    def setup(arena):
        at, other = residue, 16 - residue
        f = arena.place(c['floor'], 16, at, 'floor', torch.float32)
        g = arena.place(c['ceiling'], 16, other, 'ceiling', torch.float32)
        sol = arena.place(c['solid'].view(np.int32), 16, at, 'solid', torch.int32)
        hid = arena.place(c['hidden'].view(np.int32), 16, other, 'hidden', torch.int32)
        off = arena.place(c['offsets'], 16, at, 'offsets', torch.float32)
        index = arena.carve(SHAPE, torch.int32, 16, other, 'index_out')
        fo, go = (f, g) if in_place else (arena.carve(SHAPE, torch.float32, 16, other, 'floor_out'), arena.carve(SHAPE, torch.float32, 16, at, 'ceiling_out'))
        assert {t.data_ptr() % 16 for t in (f, g, sol, hid, off, index, fo, go)} == {4, 12}
        call = lambda: world.stamp_things(f, g, things, c['cell'], solid=sol, hidden=hid, offsets=off, floor_out=fo, ceiling_out=go, index_out=index,
                                          **c['window'])
        return call, [('floor', fo, want_f), ('ceiling', go, want_c), ('index', index, want_i)]
    run_guarded(8 * (2 * GUARD + N * 53 * 77 * 4), setup, 'stamp of %d things at %d mod 16, in_place=%s' % (size, residue, in_place))
    things.close(), world.close()
