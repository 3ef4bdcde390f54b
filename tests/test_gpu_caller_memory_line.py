"""GPU: WHERE the straight walks write (rdoom_grid_walk_lines, rdoom_path_straighten).  Every array -- floor, ceiling, starts, targets
and paths going in, flags, stops, corners, counts and lengths coming out -- is a carving of a guarded arena (tests/guarded.py) at the
least alignment the header allows, 32-bit data at 4 and 12 mod 16, the bytes of the flags at an odd address with an odd number of
targets a row, so that the output ends off a word.  After the call every byte outside the outputs, the inputs included, must be what it
was, and the outputs must equal line_ref bit for bit, with the arena poisoned 0xFF and 0x00.  The 37 x 21 and 130 x 19 rooms of
tests/test_gpu_caller_memory_grids.py, three rows a launch."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import line_ref
import octile_ref
import rust_doom_amd as rd
from guarded import run_guarded
from test_gpu_caller_memory_grids import GRIDS, N, arena_bytes, grid_ids, place_planes, rooms

pytestmark = pytest.mark.gpu
Q = 7  # targets a row: N * Q = 21 bytes of flags


@functools.lru_cache(maxsize=None)
def cases(w, h):
    """the rooms' moves, 7 targets a row from the row's seed -- one outside the grid, the seed itself, the rest anywhere -- and the
    octile descent from the farthest reached cell to the seed, down the field towards it: computed once, left unchanged"""
    floor, ceiling, seeds = rooms(w, h)
    rng = np.random.default_rng(w + h)
    moves = [line_ref.moves_of(floor[p], ceiling[p]) for p in range(N)]
    targets = np.stack([rng.integers(0, w, (N, Q)), rng.integers(0, h, (N, Q))], 2).astype(np.int32)
    targets[:, 0], targets[:, 1] = (w, 0), seeds
    near = seeds[:, None] + rng.integers(-3, 4, (N, 3, 2))  # short lines: some are clear in these dense rooms
    targets[:, 2:5] = np.clip(near, 0, (w - 1, h - 1))
    field, _ = octile_ref.flood_grids(floor, ceiling, seeds, True)
    starts = np.zeros((N, 2), np.int32)
    for p in range(N):
        d = np.where(field[p] == octile_ref.UNREACHED, 0, field[p])
        r, c = np.unravel_index(np.argmax(d), d.shape)
        starts[p] = c, r
    _, made, path = octile_ref.descend_grids(floor, ceiling, field, starts, path_len=40, towards=True)
    assert (made > 8).all()
    for a in (targets, starts, path):
        a.setflags(write=False)
    return moves, targets, starts, path


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('rev', [False, True])
def test_walk_lines(grid, residue, rev):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    moves, targets, _, _ = cases(w, h)
    clear, stop, _ = line_ref.walk_lines(None, None, seeds, targets, rev, moves=moves)
    assert clear.any() and (clear == 0).any() and (stop[:, 0] == -1).all() and clear.size % 4 == 1

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling, residue)
        s = arena.place(seeds, 16, residue, 'starts', torch.int32)
        t = arena.place(targets, 16, residue, 'targets', torch.int32)
        clear_out = arena.carve((N, Q), torch.uint8, 16, residue + 1, 'clear_out')
        stop_out = arena.carve((N, Q, 2), torch.int32, 16, residue, 'stop_out')
        assert clear_out.data_ptr() % 4 == 1 and stop_out.data_ptr() % 16 == t.data_ptr() % 16 == residue
        return (lambda: rd.walk_lines(f, c, s, t, reversed=rev, clear_out=clear_out, stop_out=stop_out)), [('clear', clear_out, clear),
                                                                                                            ('stop', stop_out, stop)]
    run_guarded(arena_bytes(w, h, 2), setup, 'walk_lines %dx%d at %d reversed=%s' % (w, h, residue, rev))

    def setup(arena):  # without the stops: the flags alone are written
        f, c = place_planes(arena, floor, ceiling, residue)
        s = arena.place(seeds, 16, residue, 'starts', torch.int32)
        t = arena.place(targets, 16, residue, 'targets', torch.int32)
        clear_out = arena.carve((N, Q), torch.uint8, 16, residue + 3, 'clear_out')
        return (lambda: rd.walk_lines(f, c, s, t, reversed=rev, clear_out=clear_out)), [('clear', clear_out, clear)]
    run_guarded(arena_bytes(w, h, 2), setup, 'walk_lines %dx%d at %d reversed=%s, no stops' % (w, h, residue, rev))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('with_length', [False, True])
def test_straighten_paths(grid, residue, with_length):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, _ = rooms(w, h)
    moves, _, starts, path = cases(w, h)
    corner_len = 48  # more than the path's 40 cells: the last entries are the (-1, -1) fill
    corners, count, length = line_ref.straighten_paths(None, None, starts, path, True, 64, corner_len, moves=moves)
    assert (count >= 2).all() and (count <= 40).all() and (corners[:, 40:] == -1).all() and (length > 0).all()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling, residue)
        s = arena.place(starts, 16, residue, 'starts', torch.int32)
        p = arena.place(path, 16, residue, 'path', torch.int32)
        corners_out = arena.carve((N, corner_len, 2), torch.int32, 16, residue, 'corners_out')
        count_out = arena.carve((N,), torch.int32, 16, residue, 'count_out')
        outputs = [('corners', corners_out, corners), ('count', count_out, count)]
        length_out = None
        if with_length:
            length_out = arena.carve((N,), torch.float32, 16, residue, 'length_out')
            outputs.append(('length', length_out, length))
        assert corners_out.data_ptr() % 16 == count_out.data_ptr() % 16 == p.data_ptr() % 16 == residue

        def call():
            rd.straighten_paths(f, c, s, p, towards=True, corners=corners_out, count_out=count_out, length_out=length_out)
        return call, outputs
    run_guarded(arena_bytes(w, h, 2), setup, 'straighten_paths %dx%d at %d length=%s' % (w, h, residue, with_length))
