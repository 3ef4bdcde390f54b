"""GPU: WHERE the grid functions write (rdoom_flood_maps, rdoom_flood_grids, rdoom_flood_descend, rdoom_wall_distance).  Every
array -- floor, ceiling, seeds, starts and distances going in, distances, counts, cells, moves, paths and planes coming out -- is a
carving of a guarded arena (tests/guarded.py) at the least alignment the header allows: 16-bit distances at 2 and 6 mod 16, 32-bit
data at 4 and 12.  After the call every byte outside the outputs, the inputs included, must be what it was, and the outputs must
equal flood_ref / goal_ref / path_ref / walls_ref bit for bit, with the arena poisoned 0xFF (FLOOD_UNREACHED, -1, a NaN) and 0x00.
Grids of 37 x 21 (rows change alignment) and 130 x 19 (more than two waves a row), three rows a launch."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import flood_ref
import goal_ref
import path_ref
import rust_doom_amd as rd
import walls_ref
from guarded import GUARD, run_guarded
from test_gpu_walls import _random_planes

pytestmark = pytest.mark.gpu
F = np.float32
N = 3
GRIDS = [(37, 21), (130, 19)]  # (width, height)
grid_ids = dict(ids=lambda g: '%dx%d' % g)


@functools.lru_cache(maxsize=None)
def rooms(w, h):
    """N rooms with closed cells, steps that are climbed (0.2) and ledges that are only dropped from (0.5), and a seed on an open
    cell near the middle of each: (floor, ceiling, seeds), computed once and left unchanged"""
    rng = np.random.default_rng(w * 100 + h)
    floor, ceiling = (np.repeat(a[None], N, 0).copy() for a in flood_ref.room(w, h, 0.0, 2.0))
    floor += rng.choice(np.array([0.0, 0.0, 0.0, 0.2, 0.5], F), floor.shape)
    ceiling[rng.random(ceiling.shape) < 0.15] = F(0.5)  # closed: lower than a body
    seeds = np.zeros((N, 2), np.int32)
    for p in range(N):
        rows, cols = np.nonzero(flood_ref.open_cells(floor[p], ceiling[p], 0.56))
        for k in np.argsort((rows - h // 2) ** 2 + (cols - (w // 2 + 3 * p)) ** 2):  # the nearest that is in no pocket, either way
            seeds[p] = cols[k], rows[k]
            if all((goal_ref.flood(floor[p], ceiling[p], seeds[p], towards=t) != goal_ref.UNREACHED).sum() > w * h // 8 for t in (False, True)):
                break
        else:
            raise AssertionError('no seed of row %d reaches an eighth of the grid' % p)
    for a in (floor, ceiling, seeds):
        a.setflags(write=False)
    return floor, ceiling, seeds


@functools.lru_cache(maxsize=None)
def random_planes(w, h):
    floor, ceiling, _ = _random_planes(np.random.default_rng(w * 1000 + h), N, h, w, 0.9)
    return floor, ceiling


def arena_bytes(w, h, planes):
    return planes * (N * w * h * 4 + GUARD + 64) + 8 * (GUARD + 64) + N * 4096


def place_planes(arena, floor, ceiling, residue=4):
    f = arena.place(floor, 16, residue, 'floor', torch.float32)
    c = arena.place(ceiling, 16, residue, 'ceiling', torch.float32)
    assert f.data_ptr() % 16 == c.data_ptr() % 16 == residue
    return f, c


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [2, 6])
def test_flood_maps(grid, residue):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    want, counts = flood_ref.flood_maps(floor, ceiling, seeds)
    assert (want != rd.FLOOD_UNREACHED).any() and (want == rd.FLOOD_UNREACHED).any() and (counts > 20).all()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling)
        s = arena.place(seeds, 16, 4, 'seeds', torch.int32)
        dist = arena.carve((N, h, w), torch.int16, 16, residue, 'dist_out')
        count = arena.carve((N,), torch.int32, 16, 4 if residue == 2 else 12, 'count_out')
        assert dist.data_ptr() % 4 == 2 and count.data_ptr() % 16 in (4, 12)
        return (lambda: rd.flood_maps(f, c, s, dist_out=dist, count_out=count)), [('dist', dist, want), ('count', count, counts)]
    run_guarded(arena_bytes(w, h, 3), setup, 'flood_maps %dx%d at %d' % (w, h, residue))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('towards', [False, True])
def test_flood_grids(grid, residue, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    want, counts = goal_ref.flood_grids(floor, ceiling, seeds, towards=towards)
    assert (want != goal_ref.UNREACHED).any() and (want == goal_ref.UNREACHED).any()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling)
        s = arena.place(seeds, 16, 4, 'seeds', torch.int32)
        dist = arena.carve((N, h, w), torch.int32, 16, residue, 'dist_out')
        count = arena.carve((N,), torch.int32, 16, residue, 'count_out')
        assert dist.data_ptr() % 16 == count.data_ptr() % 16 == residue
        return (lambda: rd.flood_grids(f, c, s, towards=towards, dist_out=dist, count_out=count)), [('dist', dist, want), ('count', count, counts)]
    run_guarded(arena_bytes(w, h, 3), setup, 'flood_grids %dx%d at %d towards=%s' % (w, h, residue, towards))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('towards', [False, True])
def test_descend_grids(grid, residue, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds = rooms(w, h)
    field, _ = goal_ref.flood_grids(floor, ceiling, seeds, towards=towards)
    starts = np.zeros((N, 2), np.int32)
    for p in range(N - 1):  # the farthest reached cell; the last row starts outside the grid
        d = np.where(field[p] == goal_ref.UNREACHED, 0, field[p])
        r, c = np.unravel_index(np.argmax(d), d.shape)
        starts[p] = c, r
    starts[N - 1] = w, 0
    length = 7
    cells, moves, path = path_ref.descend_grids(floor, ceiling, field, starts, path_len=length, towards=towards, max_moves=5)
    assert (moves[:N - 1] == 5).all() and moves[N - 1] == 0 and (path[:, 5:] == -1).all() and (path[:N - 1, :5] >= 0).all()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling)
        d = arena.place(field, 16, 4, 'dist', torch.int32)
        s = arena.place(starts, 16, 4, 'starts', torch.int32)
        cells_out = arena.carve((N, 2), torch.int32, 16, residue, 'cells_out')
        moves_out = arena.carve((N,), torch.int32, 16, residue, 'moves_out')
        path_out = arena.carve((N, length, 2), torch.int32, 16, residue, 'path_out')
        assert cells_out.data_ptr() % 16 == moves_out.data_ptr() % 16 == path_out.data_ptr() % 16 == residue

        def call():
            rd.descend_grids(f, c, d, s, towards=towards, max_moves=5, cells_out=cells_out, moves_out=moves_out, path_out=path_out)
        return call, [('cells', cells_out, cells), ('moves', moves_out, moves), ('path', path_out, path)]
    run_guarded(arena_bytes(w, h, 3), setup, 'descend_grids %dx%d at %d towards=%s' % (w, h, residue, towards))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [2, 6])
@pytest.mark.parametrize('edge_open', [False, True])
def test_wall_distances(grid, residue, edge_open):
    rd.set_device(0)
    w, h = grid
    floor, ceiling = random_planes(w, h)
    want = walls_ref.brute(floor, ceiling, 3, edge_open=edge_open)
    assert (want == walls_ref.FAR).any() and (want == 0).any() and ((want > 0) & (want <= 9)).any()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling)
        dist2 = arena.carve((N, h, w), torch.int16, 16, residue, 'dist2_out')
        assert dist2.data_ptr() % 4 == 2
        return (lambda: rd.wall_distances(f, c, 3, edge_open=edge_open, dist2_out=dist2)), [('dist2', dist2, want)]
    run_guarded(arena_bytes(w, h, 3), setup, 'wall_distances %dx%d at %d edge_open=%s' % (w, h, residue, edge_open))


@pytest.mark.parametrize('grid', GRIDS, **grid_ids)
@pytest.mark.parametrize('residue', [2, 6])
@pytest.mark.parametrize('with_dist2', [False, True])
def test_inflate_grids(grid, residue, with_dist2):
    """the caller's floor_out / ceiling_out at 4 (and 12) mod 16, the inputs' words -- NaN payloads, the sign of a zero -- as they were"""
    rd.set_device(0)
    w, h = grid
    floor, ceiling = random_planes(w, h)
    want_f, want_c, want_d = walls_ref.inflate_grids(floor, ceiling, 0.5, 0.25)
    shut = np.isposinf(want_f) & ~np.isposinf(floor)
    assert shut.any() and (~shut).any()

    def setup(arena):
        f, c = place_planes(arena, floor, ceiling)
        plane_residue = 4 if residue == 2 else 12
        f_out = arena.carve((N, h, w), torch.float32, 16, plane_residue, 'floor_out')
        c_out = arena.carve((N, h, w), torch.float32, 16, plane_residue, 'ceiling_out')
        outputs = [('floor', f_out, want_f), ('ceiling', c_out, want_c)]
        dist2 = None
        if with_dist2:
            dist2 = arena.carve((N, h, w), torch.int16, 16, residue, 'dist2_out')
            assert dist2.data_ptr() % 4 == 2
            outputs.append(('dist2', dist2, want_d))
        assert f_out.data_ptr() % 16 == c_out.data_ptr() % 16 == plane_residue
        return (lambda: rd.inflate_grids(f, c, 0.5, 0.25, floor_out=f_out, ceiling_out=c_out, dist2_out=dist2)), outputs
    run_guarded(arena_bytes(w, h, 5), setup, 'inflate_grids %dx%d at %d dist2=%s' % (w, h, residue, with_dist2))
