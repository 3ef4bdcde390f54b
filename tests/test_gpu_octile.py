"""The octile distance on the GPU (flood.hip: flood_octile_kernel; path.hip: the two flood_descend_octile kernels) against
tests/octile_ref.py, every element of every output, bit for bit.  The grids written out by hand; every 7 x 5 hand grid from each of
its 35 seeds in both directions, fifteen rows a launch, with four pairs of costs; costs (5, 10) against five times flood_grids on the
grids that take many passes; 1 x 1, and the longest single runs from either end; random rooms whose rows, columns and diagonals are
ragged runs; a band three cells wide along either diagonal of a 300 x 300 grid, which crosses the runs' ends; the descent on all of
these, every step an allowed move and the walked cost the field's difference; area_frontiers fed an octile field; E1M1 end to end;
streams, the caller's tensors, raw pointers and a captured graph, in a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flood_ref
import goal_ref
import octile_ref
import path_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = octile_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 15  # rows a launch of the hand-made grids
COSTS = [(5, 7), (1, 1), (2, 3), (3, 4)]
LIMITS = dict(max_step=0.24, max_drop=float('inf'), clearance=0.56)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _states(st):
    return torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()


def _u32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(floor, ceiling, seeds=None, rows=None, **kw):
    """flood_grids_octile of numpy planes on the device, `rows` grids a launch (None: all in one): (distances, counts) as numpy"""
    n = len(floor)
    rows = n if rows is None else rows
    dist, count = [], []
    for a in range(0, n, rows):
        s = _dev(seeds[a:a + rows], np.int32) if seeds is not None else None
        d, c = rd.flood_grids_octile(_dev(floor[a:a + rows], F), _dev(ceiling[a:a + rows], F), s, count_out=True, **kw)
        assert d.dtype == torch.int32 and c.dtype == torch.int32
        dist.append(d.cpu().numpy().view(np.uint32))
        count.append(c.cpu().numpy().view(np.uint32))
    return np.concatenate(dist), np.concatenate(count)


def _same(got, want, what):
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    bad = got[0] != want[0]
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[0][bad][:3], want[0][bad][:3])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def _walk(floor, ceiling, dist, starts, rows=None, path_len=None, **kw):
    """descend_grids_octile of device tensors, `rows` rows a launch (None: all in one): (cells, moves, path or None) as numpy"""
    n = len(floor)
    rows = n if rows is None else rows
    cells = torch.full((n, 2), 7, dtype=torch.int32, device='cuda')
    moves = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    path = torch.full((n, path_len, 2), 7, dtype=torch.int32, device='cuda') if path_len is not None else None
    for a in range(0, n, rows):
        b = a + rows
        got = rd.descend_grids_octile(floor[a:b], ceiling[a:b], dist[a:b], starts[a:b], cells_out=cells[a:b], moves_out=moves[a:b],
                                      path_out=path[a:b] if path is not None else None, **kw)
        assert len(got) == (2 if path is None else 3)
    return cells.cpu().numpy(), moves.cpu().numpy().view(np.uint32), path.cpu().numpy() if path is not None else None


def _same_walk(got, want, what):
    for k, name in enumerate(('cells', 'moves', 'path')):
        if want[k] is None:
            assert got[k] is None, (what, name)
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name, got[k].shape, want[k].shape, got[k].dtype)
        bad = got[k] != want[k]
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:6], want[k][bad][:6])


def _checked_walks(got, field, starts, moves, costs, stop_dist=0, max_moves=octile_ref.NO_LIMIT):
    """the device's walks (cells, moves, path with room for every move) against the contract, without the descent's reference:
    every step an allowed move of octile_moves' bits, the walked cost D(start) - D(end), the end at or below stop_dist unless
    max_moves ended the walk, and the unreached or outside start (-1, -1) with no move.  Returns the number of rows that walked"""
    cells, made, path = got
    walked = 0
    for p, (c, r) in enumerate(np.asarray(starts).tolist()):
        h, w = field[p].shape
        if not (0 <= c < w and 0 <= r < h) or field[p][r, c] == U:
            assert cells[p].tolist() == [-1, -1] and made[p] == 0 and (path[p] == -1).all(), p
            continue
        m = int(made[p])
        assert m <= path.shape[1] and (path[p, m:] == -1).all() and m <= max_moves, p
        cost = octile_ref.walk_cost(moves[p][1], (c, r), path[p, :m].tolist(), *costs)
        end = path[p, m - 1] if m else (c, r)
        assert cells[p].tolist() == list(end), p
        assert cost == int(field[p][r, c]) - int(field[p][end[1], end[0]]), p
        assert int(field[p][end[1], end[0]]) <= stop_dist or m == max_moves, p
        if m:  # the move before the last began above stop_dist
            before = path[p, m - 2] if m > 1 else (c, r)
            assert int(field[p][before[1], before[0]]) > stop_dist, p
        walked += m > 0
    return walked


# ---- grids written out by hand ---------------------------------------------------------------------------------------------------------

def test_the_open_room_and_the_pillar_written_out_by_hand():
    rd.set_device(0)
    f, g = flood_ref.room(7, 5)
    want = np.array([[0, 5, 10, 15, 20, 25, 30],
                     [5, 7, 12, 17, 22, 27, 32],
                     [10, 12, 14, 19, 24, 29, 34],
                     [15, 17, 19, 21, 26, 31, 36],
                     [20, 22, 24, 26, 28, 33, 38]], np.uint32)
    seeds = np.array([(0, 0), (0, 0)], np.int32)
    for towards in (False, True):
        _same(_run(np.stack([f, f]), np.stack([g, g]), seeds, towards=towards), (np.stack([want, want]), np.array([35, 35], np.uint32)), 'room')
    f, g = octile_ref.pillar()
    want = np.array([[5, 10, 15], [0, U, 20], [5, 10, 15]], np.uint32)
    for towards in (False, True):
        _same(_run(f[None], g[None], np.array([(0, 1)], np.int32), towards=towards), (want[None], np.array([8], np.uint32)), 'pillar')
    # the default seed is (W // 2, H // 2): the pillar itself, closed
    _same(_run(f[None], g[None]), (np.full((1, 3, 3), U, np.uint32), np.zeros(1, np.uint32)), 'pillar, default seed')
    f, g = flood_ref.room(7, 5)
    _same(_run(f[None], g[None]), (octile_ref.lower_bound(7, 5, (3, 2), 5, 7).astype(np.uint32)[None], np.array([35], np.uint32)), 'default seed')


SEEDS_7x5 = np.array([(col, row) for row in range(5) for col in range(7)], np.int32)
CASES_7x5 = [c for c in flood_ref.hand_cases() if c['floor'].shape == (5, 7)]


@functools.lru_cache(maxsize=None)
def _moves_7x5(k, towards):
    c = CASES_7x5[k]
    return octile_ref.octile_moves(c['floor'], c['ceiling'], towards, **dict(LIMITS, **c['kw']))


@pytest.mark.parametrize('costs', COSTS, ids=lambda c: '%d-%d' % c)
def test_the_7x5_grids_from_each_of_their_35_seeds_in_both_directions_fifteen_rows_a_launch(costs):
    rd.set_device(0)
    assert len(CASES_7x5) >= 15
    differ = 0
    for k, c in enumerate(CASES_7x5):
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        for towards in (False, True):
            moves = _moves_7x5(k, towards)
            want = np.stack([octile_ref.flood(c['floor'], c['ceiling'], s, towards, *costs, moves=moves) for s in SEEDS_7x5])
            counts = (want != U).reshape(35, -1).sum(1).astype(np.uint32)
            _same(_run(floor, ceiling, SEEDS_7x5, rows=ROWS, towards=towards, axial_cost=costs[0], diagonal_cost=costs[1], **c['kw']),
                  (want, counts), (c['name'], towards, costs))
            differ += towards and not np.array_equal(want, np.stack(
                [octile_ref.flood(c['floor'], c['ceiling'], s, False, *costs, moves=_moves_7x5(k, False)) for s in SEEDS_7x5]))
    assert differ >= 3  # the ledges: the two directions are two fields


@pytest.mark.parametrize('seed', [(0, 0), (6, 0), (3, 4)], ids=['from the top left', 'from the top right', 'from the stair'])
def test_the_walk_on_the_7x5_grids_from_every_start(seed):
    rd.set_device(0)
    walked = shorter = longer = 0
    for k, c in enumerate(CASES_7x5):
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        f_t, g_t, s_t = _dev(floor), _dev(ceiling), _dev(SEEDS_7x5)
        for towards in (False, True):
            for costs in ((5, 7), (2, 3)):
                moves = [_moves_7x5(k, towards)] * 35
                field = np.repeat(octile_ref.flood(c['floor'], c['ceiling'], seed, towards, *costs, moves=moves[0])[None], 35, 0)
                d_t = _dev(_u32(field))
                for max_moves, stop, path_len in ((None, 0, 20), (None, 0, 2), (0, 0, 20), (1, 0, 20), (3, 0, 20), (None, 2 * costs[0], 20),
                                                  (3, costs[1], 2), (None, None, None)):
                    kw = dict(towards=towards, axial_cost=costs[0], diagonal_cost=costs[1], **c['kw'])
                    if stop is not None:
                        kw.update(max_moves=octile_ref.NO_LIMIT if max_moves is None else max_moves, stop_dist=stop)
                    want = octile_ref.descend_grids(floor, ceiling, field, SEEDS_7x5, path_len=path_len, moves=moves, **kw)
                    if stop is not None:
                        kw['max_moves'] = max_moves
                    got = _walk(f_t, g_t, d_t, s_t, rows=ROWS, path_len=path_len, **kw)
                    _same_walk(got, want, (c['name'], seed, kw, path_len))
                    if path_len == 20:
                        walked += _checked_walks(got, field, SEEDS_7x5, moves, costs, stop, octile_ref.NO_LIMIT if max_moves is None else max_moves)
                        longer += int((want[1] < path_len).sum())
                    elif path_len == 2:
                        shorter += int((want[1] > path_len).sum())
    assert walked > 1000 and shorter > 100 and longer > 100


# ---- against the 4-neighbour flood -----------------------------------------------------------------------------------------------------

def test_costs_5_and_10_are_five_times_flood_grids():
    """property 2 on the device: the hand cases, the serpentine and the 255 x 85 spiral, which take many passes"""
    rd.set_device(0)
    grids = [(c['name'], c['floor'], c['ceiling'], c['seed'], c['kw']) for c in flood_ref.hand_cases()]
    grids += [('serpentine', *flood_ref.serpentine(), (0, 0), {}), ('spiral', *flood_ref.spiral(255, 85), (0, 0), {})]
    some = 0
    for name, f, g, seed, kw in grids:
        seeds = None if seed is None else _dev(np.array([seed], np.int32))
        for towards in (False, True):
            four = rd.flood_grids(_dev(f[None]), _dev(g[None]), seeds, towards=towards, **kw).cpu().numpy().view(np.uint32)
            eight = rd.flood_grids_octile(_dev(f[None]), _dev(g[None]), seeds, towards=towards, axial_cost=5, diagonal_cost=10, **kw)
            eight = eight.cpu().numpy().view(np.uint32)
            assert np.array_equal(eight, np.where(four == U, U, 5 * four.astype(np.uint64)).astype(np.uint32)), (name, towards)
            some += int((four != U).sum() > 1)
    assert some > 30 and np.where(four == U, 0, four).max() > 5000  # the spiral: thousands of moves along one corridor


# ---- the smallest grid and the longest runs ----------------------------------------------------------------------------------------------

def test_the_smallest_grid_and_the_longest_single_runs_from_either_end():
    rd.set_device(0)
    f, g = flood_ref.room(1, 1)
    _same(_run(f[None], g[None]), (np.zeros((1, 1, 1), np.uint32), np.ones(1, np.uint32)), '1 x 1')
    got = _walk(_dev(f[None]), _dev(g[None]), torch.zeros((1, 1, 1), dtype=torch.int32, device='cuda'),
                torch.zeros((1, 2), dtype=torch.int32, device='cuda'), path_len=1)
    _same_walk(got, (np.zeros((1, 2), np.int32), np.zeros(1, np.uint32), np.full((1, 1, 2), -1, np.int32)), '1 x 1')
    line = np.arange(8192, dtype=np.uint32)
    for w, h in ((8192, 1), (1, 8192)):
        f, g = flood_ref.room(w, h)
        floor, ceiling = np.stack([f, f]), np.stack([g, g])
        seeds = np.array([(0, 0), (w - 1, h - 1)], np.int32)
        for towards in (False, True):
            for costs in ((5, 7), (3, 4)):
                want = np.stack([costs[0] * line, costs[0] * line[::-1]]).reshape(2, h, w)
                assert want.max() == 8191 * costs[0]
                kw = dict(towards=towards, axial_cost=costs[0], diagonal_cost=costs[1])
                _same(_run(floor, ceiling, seeds, **kw), (want, np.array([8192, 8192], np.uint32)), (w, h, kw))
        # the walk from the far end to the seed: 8191 moves, every one in the path (kw: the last of the loop)
        starts = seeds[::-1].copy()
        got = _walk(_dev(floor), _dev(ceiling), _dev(_u32(want)), _dev(starts), path_len=8191, **kw)
        along = np.stack([np.arange(8190, -1, -1), np.arange(1, 8192)])  # the coordinate that changes
        path = np.zeros((2, 8191, 2), np.int32)
        path[:, :, 0 if h == 1 else 1] = along
        _same_walk(got, (seeds, np.array([8191, 8191], np.uint32), path), (w, h, 'walk'))


# ---- ragged runs -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_rooms(w, h):
    """three random rooms of w x h with a seed that reaches a good part of each, and 24 starts, some of them none: computed once,
    left unchanged"""
    rng = np.random.default_rng(w * 1000 + h)
    n = 3
    floor, ceiling = (np.stack(a) for a in zip(*[octile_ref.random_room(w, h, w + h + p) for p in range(n)]))
    seeds = np.zeros((n, 2), np.int32)
    for p in range(n):
        rows, cols = np.nonzero(flood_ref.open_cells(floor[p], ceiling[p], 0.56))
        for k in rng.permutation(len(rows)):
            seeds[p] = cols[k], rows[k]
            if all((goal_ref.flood(floor[p], ceiling[p], seeds[p], towards=t) != U).sum() > w * h // 4 for t in (False, True)):
                break
        else:
            raise AssertionError('no seed of row %d reaches a quarter of the grid' % p)
    starts = np.stack([rng.integers(0, w, 24), rng.integers(0, h, 24)], 1).astype(np.int32)
    starts[:6] = [(-1, -1), (w, 5), (5, h), (-1, 5), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 0)]
    return floor, ceiling, seeds, starts


@pytest.mark.parametrize('grid', [(257, 131), (130, 19)], ids=lambda g: '%dx%d' % g)
@pytest.mark.parametrize('towards', [False, True], ids=['forwards', 'towards'])
def test_random_rooms_whose_rows_columns_and_diagonals_are_ragged_runs(grid, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, seeds, starts = _random_rooms(w, h)
    moves = [octile_ref.octile_moves(floor[p], ceiling[p], towards, **LIMITS) for p in range(3)]
    f_t, g_t = _dev(floor), _dev(ceiling)
    for costs in ((5, 7), (3, 4)):
        want = np.stack([octile_ref.flood(floor[p], ceiling[p], seeds[p], towards, *costs, moves=moves[p]) for p in range(3)])
        counts = (want != U).reshape(3, -1).sum(1).astype(np.uint32)
        four = goal_ref.flood_grids(floor, ceiling, seeds, towards)[0]
        assert np.array_equal(want != U, four != U) and (want[want != U] < costs[0] * four[want != U].astype(np.int64)).sum() > w * h // 16
        dist_t, count_t = rd.flood_grids_octile(f_t, g_t, _dev(seeds), towards=towards, axial_cost=costs[0], diagonal_cost=costs[1], count_out=True)
        _same((dist_t.cpu().numpy().view(np.uint32), count_t.cpu().numpy().view(np.uint32)), (want, counts), (grid, towards, costs))
        # the walk from 24 starts, eight a row
        which = np.arange(24) % 3
        wf, wg, wd, wm = floor[which], ceiling[which], want[which], [moves[p] for p in which]
        kw = dict(towards=towards, axial_cost=costs[0], diagonal_cost=costs[1])
        path_len = 2 * (w + h)
        ref = octile_ref.descend_grids(wf, wg, wd, starts, path_len=path_len, moves=wm, **kw)
        got = _walk(_dev(wf), _dev(wg), _dev(_u32(wd)), _dev(starts), path_len=path_len, **kw)
        _same_walk(got, ref, (grid, towards, costs, 'walk'))
        assert _checked_walks(got, wd, starts, wm, costs) >= 8 and (ref[1] == 0).sum() >= 6 and ref[1].max() < path_len
        assert all(ref[0][p].tolist() == seeds[which[p]].tolist() for p in range(24) if ref[1][p])
        limited = octile_ref.descend_grids(wf, wg, wd, starts, moves=wm, max_moves=8, stop_dist=5 * costs[1], **kw)
        _same_walk(_walk(_dev(wf), _dev(wg), _dev(_u32(wd)), _dev(starts), max_moves=8, stop_dist=5 * costs[1], **kw), limited, (grid, 'limited'))


# ---- the diagonal band -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('anti', [False, True], ids=['main diagonal', 'anti-diagonal'])
def test_a_band_three_wide_along_a_diagonal_of_a_300_x_300_grid_from_either_end(anti):
    """90 000 cells: the host picks its longest run, 64, and the band crosses a run's end every 64 rows.  Stride width + 1 carries
    the main diagonal, width - 1 its mirror image"""
    rd.set_device(0)
    n = 300
    f, g = octile_ref.band(n, anti)
    ends = np.array([(n - 1, 0), (0, n - 1)] if anti else [(0, 0), (n - 1, n - 1)], np.int32)
    floor, ceiling = np.stack([f, f]), np.stack([g, g])
    moves = octile_ref.octile_moves(f, g, False, **LIMITS)
    for costs in ((5, 7), (1, 1)):
        want = np.stack([octile_ref.flood(f, g, s, False, *costs, moves=moves) for s in ends])
        far = [want[0][ends[1][1], ends[1][0]], want[1][ends[0][1], ends[0][0]]]
        assert far == [299 * costs[1]] * 2 and (want != U).sum() == 2 * (3 * n - 2)
        for towards in (False, True):  # every move has its reverse: one field
            kw = dict(towards=towards, axial_cost=costs[0], diagonal_cost=costs[1])
            _same(_run(floor, ceiling, ends, **kw), (want, np.full(2, 3 * n - 2, np.uint32)), (anti, kw))
    # the walk from the far end (costs (1, 1), towards: the last of the loops): no axial neighbour is nearer, so every one of the
    # 299 moves is the diagonal one -- the four rows of the two grids take the four diagonal offsets
    starts = ends[::-1].copy()
    got = _walk(_dev(floor), _dev(ceiling), _dev(_u32(want)), _dev(starts), path_len=n, **kw)
    _same_walk(got, octile_ref.descend_grids(floor, ceiling, want, starts, path_len=n, moves=[moves, moves], **kw), (anti, 'walk'))
    assert _checked_walks(got, want, starts, [moves, moves], costs) == 2 and got[1].tolist() == [299, 299] and np.array_equal(got[0], ends)


# ---- frontiers of an octile field, and E1M1 end to end -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wad():
    return rd.Wad(ensure_wad(), META_PATH)


@functools.lru_cache(maxsize=None)
def _level(index, cell):
    host = _wad().build_world(index, device=False)
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    return host, tables, g, goal_ref.level_sectors(tables, g, cell)


def test_area_frontiers_fed_an_octile_field():
    """tests/test_gpu_path.py's explored area of E1M1, flooded forwards from the players' cells over the eight neighbours: the
    frontier call, unchanged, picks the cell nearest by octile cost, and the walk back stops 10 cost units from the player"""
    rd.set_device(0)
    index, cell, n = 0, 0.25, 8
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    st, _ = sector_ref.players(_wad(), index, n, np.random.default_rng(34), outside=1, nan=1)
    fan = torch.from_numpy(rd.map_fan(64, 1.6)).cuda()
    turned = st.copy()
    area = world.reveal_area(_states(turned), fan=fan, max_range=12.0, cell=cell)
    for _ in range(3):
        turned['yaw'] += F(1.6)
        world.reveal_area(_states(turned), fan=fan, max_range=12.0, cell=cell, area=area)
    floor, ceiling = world.draw_area_planes(cell, area=area, floor=True, ceiling=True)
    cells = world.area_cells(_states(st), cell)
    dist = rd.flood_grids_octile(floor, ceiling, cells)
    front, front_dist, count, mask = world.area_frontiers(area, dist, cell, dist_out=True, count_out=True, mask_out=True)
    step, made = rd.descend_grids_octile(floor, ceiling, dist, front, stop_dist=10)
    # the reference, from the explored area the device revealed (tests/test_gpu_area.py pins it)
    rows = area.cpu().numpy().view(np.uint32)
    _, w_floor, w_ceiling = goal_ref.planes(tables, g, cell, n, area=rows, at_centres=[at])
    w_cells = goal_ref.cells(g, cell, st)
    w_dist, _ = octile_ref.flood_grids(w_floor, w_ceiling, w_cells)
    want = path_ref.area_frontiers(rows, g, w_dist)
    four = path_ref.area_frontiers(rows, g, goal_ref.flood_grids(w_floor, w_ceiling, w_cells)[0])
    assert ((want[2][:n - 2] > 10).sum() >= 4) and (want[2][n - 2:] == 0).all() and (want[0][n - 2:] == -1).all(), want[2]
    assert np.array_equal(want[2], four[2]) and np.array_equal(want[3], four[3])  # property 1: the same frontier,
    has = want[2] > 0
    assert (want[1][has].astype(np.int64) < 5 * four[1][has].astype(np.int64)).any()  # nearer by the diagonals
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), w_dist)
    for k, (got, name) in enumerate(((front, 'cell'), (front_dist, 'dist'), (count, 'count'), (mask, 'mask'))):
        got = got.cpu().numpy()
        assert np.array_equal(got.view(want[k].dtype) if got.dtype.itemsize == want[k].dtype.itemsize else got, want[k]), name
    w_step, w_made, _ = octile_ref.descend_grids(w_floor, w_ceiling, w_dist, want[0], stop_dist=10)
    _same_walk((step.cpu().numpy(), made.cpu().numpy().view(np.uint32), None), (w_step, w_made, None), 'E1M1')
    # where to walk now: a cell within 10 cost units of the player -- two cells at the most -- on the way to the frontier
    far = has & (np.where(has, want[1], 0) > 10)
    assert far.sum() >= 4 and (np.abs(w_step[far] - w_cells[far]).max(1) <= 2).all() and (w_made[far] > 0).all()
    assert (w_step[~has] == -1).all() and (w_made[~has] == 0).all()


E2E_STEP = 0.32  # tests/test_gpu_goal.py: the synthetic E1M1 joins most of its sectors by steps of 0.32


def test_planes_cells_a_flood_towards_the_start_of_e1m1_and_the_walk_of_64_players():
    rd.set_device(0)
    index, cell, n = 0, 0.125, 4
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    pos, yaw = _wad().build_level(index).start()
    st = rd.player_states(np.repeat(np.asarray(pos, F)[None], n, 0), np.full(n, yaw, F))
    off = sector_ref.random_offsets(np.random.default_rng(7), n, host.game_objects)
    off[0] = 0  # row 0: all at rest
    _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    seeds = goal_ref.cells(g, cell, st)
    moves = [octile_ref.octile_moves(floor[p], ceiling[p], True, E2E_STEP, float('inf'), 0.56) for p in range(n)]
    want = np.stack([octile_ref.flood(floor[p], ceiling[p], seeds[p], True, moves=moves[p]) for p in range(n)])
    counts = (want != U).reshape(n, -1).sum(1).astype(np.uint32)
    is_open = np.stack([m[0] for m in moves])
    assert (2 * counts > is_open.reshape(n, -1).sum(1)).all(), (counts, is_open.reshape(n, -1).sum(1))  # a field worth having
    f_t, c_t = world.draw_area_planes(cell, offsets=_dev(off), floor=True, ceiling=True)
    cells = world.area_cells(_states(st), cell)
    dist, count = rd.flood_grids_octile(f_t, c_t, cells, towards=True, max_step=E2E_STEP, count_out=True)
    _same((dist.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)), (want, counts), 'end to end')
    # 64 players spread over the level, sixteen a row of planes: the waypoint 12 moves ahead, then the whole way
    rng = np.random.default_rng(5)
    which = np.arange(64) % n
    starts = np.zeros((64, 2), np.int32)
    for k, p in enumerate(which):
        rows, cols = np.nonzero(want[p] != U)
        at_k = rng.integers(len(rows))
        starts[k] = cols[at_k], rows[at_k]
    starts[:3] = [(-1, -1), tuple(np.argwhere(~is_open[0])[0][::-1]), (g.gw, 0)]
    wf, wg, wd, wm = floor[which], ceiling[which], want[which], [moves[p] for p in which]
    big = lambda t: t[torch.from_numpy(which).cuda()].contiguous()
    kw = dict(towards=True, max_step=E2E_STEP)
    ref = octile_ref.descend_grids(wf, wg, wd, starts, moves=wm, max_moves=12, **kw)
    _same_walk(_walk(big(f_t), big(c_t), big(dist), _dev(starts), max_moves=12, **kw), ref, 'waypoints')
    assert (ref[1] == 12).sum() > 40 and (ref[1][:3] == 0).all() and (ref[0][:3] == -1).all()
    longest = int(np.where(wd == U, 0, wd).max()) // 5 + 1
    got = _walk(big(f_t), big(c_t), big(dist), _dev(starts), path_len=longest, **kw)
    _same_walk(got, octile_ref.descend_grids(wf, wg, wd, starts, path_len=longest, moves=wm, **kw), 'the whole way')
    assert _checked_walks(got, wd, starts, wm, (5, 7)) >= 55 and all(got[0][k].tolist() == seeds[which[k]].tolist() for k in range(3, 64))


# ---- streams, tensors, pointers, a graph -------------------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_octile_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_octile_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
