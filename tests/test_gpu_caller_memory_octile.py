"""GPU: WHERE the octile calls write (rdoom_flood_grids_octile, rdoom_flood_descend_octile).  Every array -- floor, ceiling, seeds,
starts and distances going in, distances, counts, cells, moves and paths coming out -- is a carving of a guarded arena
(tests/guarded.py) at the least alignment the header allows, 4 and 12 mod 16.  After the call every byte outside the outputs, the
inputs included, must be what it was, and the outputs must equal octile_ref bit for bit, with the arena poisoned 0xFF
(FLOOD_GRID_UNREACHED, -1, a NaN) and 0x00.  The flood keeps its move bits in the distance words while it runs: the poison must
not show through them.  tests/test_gpu_caller_memory_grids.py's rooms: 37 x 21 (rows change alignment) and 130 x 19 (more than two
waves a row), three rows a launch."""
import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import octile_ref
import rust_doom_amd as rd
from guarded import run_guarded
from test_gpu_caller_memory_grids import GRIDS, N, arena_bytes, grid_ids, place_planes, rooms

pytestmark = pytest.mark.gpu
U = octile_ref.UNREACHED


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('towards', [False, True])
def test_flood_grids_octile(grid, residue, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    want, counts = octile_ref.flood_grids(floor, ceiling, seeds, towards=towards)
    assert (want != U).any() and (want == U).any() and (counts > 20).all()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling, residue)
        s = arena.place(seeds, 16, residue, 'seeds', torch.int32)
        dist = arena.carve((N, h, w), torch.int32, 16, residue, 'dist_out')
        count = arena.carve((N,), torch.int32, 16, residue, 'count_out')
        assert dist.data_ptr() % 16 == count.data_ptr() % 16 == s.data_ptr() % 16 == residue
        return (lambda: rd.flood_grids_octile(f, c, s, towards=towards, dist_out=dist, count_out=count)), [('dist', dist, want), ('count', count, counts)]
    run_guarded(arena_bytes(w, h, 3), setup, 'flood_grids_octile %dx%d at %d towards=%s' % (w, h, residue, towards))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('towards', [False, True])
def test_descend_grids_octile(grid, residue, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    field, _ = octile_ref.flood_grids(floor, ceiling, seeds, towards=towards)
    starts = np.zeros((N, 2), np.int32)
    for p in range(N - 1):  # the farthest reached cell; the last row starts outside the grid
        d = np.where(field[p] == U, 0, field[p])
        r, c = np.unravel_index(np.argmax(d), d.shape)
        starts[p] = c, r
    starts[N - 1] = w, 0
    length = 7
    cells, moves, path = octile_ref.descend_grids(floor, ceiling, field, starts, path_len=length, towards=towards, max_moves=5)
    assert (moves[:N - 1] == 5).all() and moves[N - 1] == 0 and (path[:, 5:] == -1).all() and (path[:N - 1, :5] >= 0).all()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling, residue)
        d = arena.place(field, 16, residue, 'dist', torch.int32)
        s = arena.place(starts, 16, residue, 'starts', torch.int32)
        cells_out = arena.carve((N, 2), torch.int32, 16, residue, 'cells_out')
        moves_out = arena.carve((N,), torch.int32, 16, residue, 'moves_out')
        path_out = arena.carve((N, length, 2), torch.int32, 16, residue, 'path_out')
        assert cells_out.data_ptr() % 16 == moves_out.data_ptr() % 16 == path_out.data_ptr() % 16 == d.data_ptr() % 16 == residue

        def call():
            rd.descend_grids_octile(f, c, d, s, towards=towards, max_moves=5, cells_out=cells_out, moves_out=moves_out, path_out=path_out)
        return call, [('cells', cells_out, cells), ('moves', moves_out, moves), ('path', path_out, path)]
    run_guarded(arena_bytes(w, h, 3), setup, 'descend_grids_octile %dx%d at %d towards=%s' % (w, h, residue, towards))
