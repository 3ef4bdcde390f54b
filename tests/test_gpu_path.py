"""Waypoints and frontiers on the GPU (path.hip: the two flood_descend kernels, the two area_frontiers kernels) against
tests/path_ref.py, every element of every output, bit for bit.  The walk on the 7 x 5 hand-made grids from every start, for three
seeds, in both directions, fifteen rows a launch, with and without limits and with paths shorter and longer than the walk; on 1 x 1,
on 1 x 8192 from end to end, on random 257 x 131 grids, from starts that are none, down a field that is not the planes', and past the
foot of a ledge.  The frontier of hand-made areas on grids whose width straddles the word edges, padded, with a longer stride, with
all bits set and all clear.  Explored area, planes, flood, frontier and walk of E1M1 end to end, and in a three-level set; streams,
the caller's tensors, raw pointers and a captured graph, in a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flood_ref
import goal_ref
import path_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = path_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 15  # rows a launch of the hand-made grids


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _states(st):
    return torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()


def _u32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _walk(floor, ceiling, dist, starts, rows=None, path_len=None, **kw):
    """descend_grids of device tensors, `rows` rows a launch (None: all in one): (cells, moves, path or None) as numpy"""
    n = len(floor)
    rows = n if rows is None else rows
    cells = torch.full((n, 2), 7, dtype=torch.int32, device='cuda')
    moves = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    path = torch.full((n, path_len, 2), 7, dtype=torch.int32, device='cuda') if path_len is not None else None
    for a in range(0, n, rows):
        b = a + rows
        got = rd.descend_grids(floor[a:b], ceiling[a:b], dist[a:b], starts[a:b], cells_out=cells[a:b], moves_out=moves[a:b],
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


# ---- the walk on hand-made grids -------------------------------------------------------------------------------------------------------

STARTS_7x5 = np.array([(col, row) for row in range(5) for col in range(7)], np.int32)


@pytest.mark.parametrize('seed', [(0, 0), (6, 0), (3, 4)], ids=['from the top left', 'from the top right', 'from the stair'])
def test_the_7x5_grids_from_every_start_in_both_directions_fifteen_rows_a_launch(seed):
    rd.set_device(0)
    cases = [c for c in flood_ref.hand_cases() if c['floor'].shape == (5, 7)]
    assert len(cases) >= 15
    walked = shorter = longer = stopped = 0
    for c in cases:
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        f_t, g_t, s_t = _dev(floor), _dev(ceiling), _dev(STARTS_7x5)
        for towards in (False, True):
            field = np.repeat(goal_ref.flood(c['floor'], c['ceiling'], seed, towards, **c['kw'])[None], 35, 0)
            d_t = _dev(_u32(field))
            for max_moves in (0, 1, 3, None):
                for stop in (0, 2):
                    for path_len in ((2, 20) if max_moves is None else ((2,) if stop else (20,))):
                        kw = dict(towards=towards, max_moves=path_ref.NO_LIMIT if max_moves is None else max_moves, stop_dist=stop, **c['kw'])
                        want = path_ref.descend_grids(floor, ceiling, field, STARTS_7x5, path_len=path_len, **kw)
                        kw['max_moves'] = max_moves
                        _same_walk(_walk(f_t, g_t, d_t, s_t, rows=ROWS, path_len=path_len, **kw), want, (c['name'], seed, kw, path_len))
                        walked += int((want[1] > 0).sum())
                        shorter, longer = shorter + int((want[1] > path_len).sum()), longer + int((want[1] < path_len).sum())
                        stopped += int(((want[0] >= 0).all(1) & (want[0] != np.array(seed)).any(1)).sum())
            # without a path, and with the defaults: no limit, down to the seed
            want = path_ref.descend_grids(floor, ceiling, field, STARTS_7x5, towards=towards, **c['kw'])
            _same_walk(_walk(f_t, g_t, d_t, s_t, rows=ROWS, towards=towards, **c['kw']), want, (c['name'], seed, towards, 'defaults'))
    assert walked > 1000 and shorter > 100 and longer > 100 and stopped > 100


def test_the_smallest_grid_the_longest_walk_and_the_foot_of_a_ledge():
    rd.set_device(0)
    f, g = flood_ref.room(1, 1)
    zero = torch.zeros((1, 1, 1), dtype=torch.int32, device='cuda')
    got = _walk(_dev(f[None]), _dev(g[None]), zero, torch.zeros((1, 2), dtype=torch.int32, device='cuda'), path_len=1)
    _same_walk(got, (np.zeros((1, 2), np.int32), np.zeros(1, np.uint32), np.full((1, 1, 2), -1, np.int32)), '1 x 1')
    # 1 x 8192 from end to end, in both directions and both senses: 8191 moves, every one in the path
    f, g = flood_ref.room(8192, 1)
    line = np.arange(8192, dtype=np.uint32)
    for towards in (False, True):
        for flip in (False, True):
            field = (line[::-1] if flip else line).reshape(1, 1, 8192)
            start = np.array([[0 if flip else 8191, 0]], np.int32)
            path = np.zeros((1, 8191, 2), np.int32)
            path[0, :, 0] = np.arange(1, 8192) if flip else np.arange(8190, -1, -1)
            want = (np.array([[8191 if flip else 0, 0]], np.int32), np.array([8191], np.uint32), path)
            ref = path_ref.descend_grids(f[None], g[None], field, start, path_len=8191, towards=towards)
            assert all(np.array_equal(a, b) for a, b in zip(ref, want))
            _same_walk(_walk(_dev(f[None]), _dev(g[None]), _dev(_u32(field)), _dev(start), path_len=8191, towards=towards), want,
                       ('1 x 8192', towards, flip))
    # the distances alone lead into the foot of a ledge (tests/test_path_host.py writes this walk out): row 0 as flooded, row 1 with
    # the stair taken away after the flood -- nothing allowed is one less, the walk stops where it stands
    f, g = flood_ref.room(2, 5, 0.0, 2.0)
    f[:3, 1], f[3, 1] = F(0.48), F(0.24)
    field = goal_ref.flood(f, g, (0, 4))
    no_stair = f.copy()
    no_stair[3, 1] = 0
    floor, ceiling, fields, starts = np.stack([f, no_stair]), np.stack([g, g]), np.stack([field, field]), np.array([(1, 2), (1, 2)], np.int32)
    want = path_ref.descend_grids(floor, ceiling, fields, starts, path_len=4)
    assert want[0].tolist() == [[0, 4], [1, 2]] and want[1].tolist() == [3, 0] and want[2][0].tolist() == [[1, 3], [0, 3], [0, 4], [-1, -1]]
    _same_walk(_walk(_dev(floor), _dev(ceiling), _dev(_u32(fields)), _dev(starts), path_len=4), want, 'the foot of a ledge')


@functools.lru_cache(maxsize=None)
def _random_grids():
    """the 257 x 131 grids of tests/test_gpu_goal.py's recipe, 64 rows of them with random starts, some of them none: computed once,
    left unchanged"""
    rng = np.random.default_rng(11)
    f = np.where(rng.random((3, 131, 257)) < 0.15, 0.3, 0.0).astype(F)  # rooms with pillars and raised cells
    g = np.where(rng.random((3, 131, 257)) < 0.1, 0.2, 1.5).astype(F)
    seeds = np.array([(128, 65), (0, 0), (256, 130)], np.int32)
    f[np.arange(3), seeds[:, 1], seeds[:, 0]], g[np.arange(3), seeds[:, 1], seeds[:, 0]] = 0.0, 1.5
    n = 64
    which = np.arange(n) % 3
    starts = np.stack([rng.integers(0, 257, n), rng.integers(0, 131, n)], 1).astype(np.int32)
    starts[:8] = [(-1, -1), (257, 5), (5, 131), (-1, 5), (5, -1), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 0), (256, 130)]
    return f[which], g[which], seeds[which], starts


@pytest.mark.parametrize('towards', [False, True], ids=['forwards', 'towards'])
def test_random_grids_from_64_starts_and_a_field_that_is_not_the_planes(towards):
    rd.set_device(0)
    floor, ceiling, seeds, starts = _random_grids()
    f_t, g_t = _dev(floor), _dev(ceiling)
    for flooded, walked in ((0.32, 0.32), (0.32, 0.24)):  # the second: flooded over steps of 0.3 the walk may not take
        dist_t = rd.flood_grids(f_t, g_t, _dev(seeds), towards=towards, max_step=flooded)  # (tests/test_gpu_goal.py pins this flood)
        dist = dist_t.cpu().numpy().view(np.uint32)
        path_len = 300
        want = path_ref.descend_grids(floor, ceiling, dist, starts, path_len=path_len, towards=towards, max_step=walked)
        at_start = np.array([dist[p, z, x] if 0 <= x < 257 and 0 <= z < 131 else U for p, (x, z) in enumerate(starts.tolist())], np.uint32)
        none = at_start == U
        assert none[:7].all() and 7 < none.sum() < 30 and (want[0][none] == -1).all() and (want[1][none] == 0).all()
        if flooded == walked:
            assert np.array_equal(want[1][~none], at_start[~none]) and np.array_equal(want[0][~none], seeds[~none])
            assert (want[1] > 100).sum() > 10 and (want[1] > path_len).any()  # some walks outrun the path
        else:
            assert (want[1][~none] < at_start[~none]).sum() > 20  # stopped early
        _same_walk(_walk(f_t, g_t, dist_t, _dev(starts), path_len=path_len, towards=towards, max_step=walked), want, (towards, flooded, walked))
        limited = path_ref.descend_grids(floor, ceiling, dist, starts, towards=towards, max_step=walked, max_moves=8, stop_dist=5)
        _same_walk(_walk(f_t, g_t, dist_t, _dev(starts), towards=towards, max_step=walked, max_moves=8, stop_dist=5), limited, (towards, 'limited'))


# ---- the frontier of hand-made areas -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wad():
    return rd.Wad(ensure_wad(), META_PATH)


@functools.lru_cache(maxsize=None)
def _cell_for(index, gw):
    """a cell size at which the level's grid is gw cells wide"""
    host = _wad().build_world(index, device=False)
    for k in range(200, 10000):
        if host.area_grid(k / 10000.0).gw == gw:
            return k / 10000.0
    raise AssertionError('no cell size gives E1M%d a grid %d wide' % (index + 1, gw))


def _front(call, area, dist, cell, **kw):
    """area_frontiers with every output: (cells, dists, counts, masks) as numpy"""
    cells, dists, counts, masks = call(area=area, dist=dist, cell=cell, dist_out=True, count_out=True, mask_out=True, **kw)
    assert cells.dtype == dists.dtype == counts.dtype == torch.int32 and masks.dtype == torch.uint8
    return cells.cpu().numpy(), dists.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32), masks.cpu().numpy()


def _same_front(got, want, what):
    for k, name in enumerate(('cell', 'dist', 'count', 'mask')):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        bad = got[k] != want[k]
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:6], want[k][bad][:6])


PICTURE = ['.........',   # tests/test_path_host.py's 9 x 6 area: '.' unknown, 'F' free, 'W' wall, 'B' both
           '.FFFW....',
           '.FFFW....',
           '.FFFFF...',
           '.WWWB....',
           '.........']


def _hand_made_rows(g, stride, rng):
    """six rows of area for grid g: the picture in a corner and again across the first word edge; random bits; FREE all ones; all
    zero; a known block with single unknown cells at the grid's right edge and at the word edges; random bits with every bit beyond
    gw, and every word beyond the grid's, set at random too"""
    n = 6
    free, wall = np.zeros((n, g.gh, g.gw), bool), np.zeros((n, g.gh, g.gw), bool)
    for x0, z0 in ((0, 0), (28, 7)):
        for iz, line in enumerate(PICTURE):
            for ix, ch in enumerate(line):
                if x0 + ix < g.gw:
                    free[0, z0 + iz, x0 + ix] |= ch in 'FB'
                    wall[0, z0 + iz, x0 + ix] |= ch in 'WB'
    free[1], wall[1] = rng.random((g.gh, g.gw)) < 0.7, rng.random((g.gh, g.gw)) < 0.15
    free[2] = True
    free[4] = True
    for ix, iz in ((g.gw - 1, 3), (31 if g.gw > 31 else 5, 9), (32 if g.gw > 32 else 6, 12), (0, 15), (63 if g.gw > 63 else 7, 18), (g.gw - 1, g.gh - 1)):
        free[4, iz, ix] = False
    free[5], wall[5] = rng.random((g.gh, g.gw)) < 0.8, rng.random((g.gh, g.gw)) < 0.1
    rows = np.zeros((n, 2, stride), np.uint32)
    rows[5] = rng.integers(0, 2 ** 32, (2, stride), dtype=np.uint64).astype(np.uint32)
    ix = np.arange(g.gw)
    for p in range(n):
        for plane, bits in ((0, free[p]), (1, wall[p])):
            words = rows[p, plane, :g.words].reshape(g.gh, g.pitch)
            inside = np.zeros((g.gh, g.pitch), np.uint32)
            np.bitwise_or.at(inside, (np.repeat(np.arange(g.gh), g.gw), np.tile(ix >> 5, g.gh)), (bits.astype(np.uint32) << (ix & 31).astype(np.uint32)).reshape(-1))
            keep = np.zeros(g.pitch, np.uint32)  # the bits beyond gw stay as they are
            np.bitwise_or.at(keep, ix >> 5, np.uint32(1) << (ix & 31).astype(np.uint32))
            words[:] = (words & ~keep) | inside
    for p in range(n):
        got = rd.unpack_area(rows[p], g)
        assert np.array_equal(got[0], free[p]) and np.array_equal(got[1], wall[p])
    return rows


@pytest.mark.parametrize('gw', [31, 32, 33, 70])
def test_the_frontier_of_hand_made_areas_across_the_word_edges(gw):
    rd.set_device(0)
    index = 1  # E1M2, the small level
    cell = _cell_for(index, gw)
    world = _wad().build_world(index)
    g = world.area_grid(cell)
    assert g.gw == gw and g.gh > 20 and g.pitch == (gw + 31) // 32
    rng = np.random.default_rng(gw)
    for stride, (h, w) in ((g.words, (g.gh, g.gw)), (g.words + 5, (g.gh + 2, g.gw + 37))):  # exact; a longer stride and padded planes
        rows = _hand_made_rows(g, stride, rng)
        n = len(rows)
        dist = np.where(rng.random((n, h, w)) < 0.6, rng.integers(0, 40, (n, h, w)), U).astype(np.uint32)  # many ties; the padding reached too
        dist[0] = U
        for x0, z0 in ((0, 0), (28, 7)):  # row 0: the picture's free cells reached, as tests/test_path_host.py has them
            for iz, line in enumerate(PICTURE):
                for ix, ch in enumerate(line):
                    if ch == 'F' and x0 + ix < g.gw:
                        dist[0, z0 + iz, x0 + ix] = abs(ix - 2) + abs(iz - 2)
        dist[2], dist[3], dist[4] = 5, U, 9
        dist[3, 11, g.gw - 2] = 77  # all unknown, one cell reached: that cell
        want = path_ref.area_frontiers(rows, g, dist)
        assert want[0][0].tolist() == [2, 1] and want[1][0] == 1 and want[2][0] >= 6 and want[3][0, 1:4, 1].all() and not want[3][0, 2, 2]
        assert want[2][2] == 0 and want[0][2].tolist() == [-1, -1] and want[1][2] == U  # FREE all ones: no frontier
        assert want[2][3] == 1 and want[0][3].tolist() == [g.gw - 2, 11] and want[1][3] == 77
        assert 6 * 2 <= want[2][4] <= 6 * 4 and want[0][4].tolist() == [g.gw - 1, 2]  # the neighbours of six single cells, all as near: the first
        assert want[2][1] > 100 and want[2][5] > 100 and not want[3][:, g.gh:].any() and not want[3][:, :, g.gw:].any()
        got = _front(world.area_frontiers, _dev(_u32(rows)), _dev(_u32(dist)), cell)
        _same_front(got, want, (gw, stride, h, w))
        # the cells alone, into the caller's tensor
        mine = torch.full((n, 2), 7, dtype=torch.int32, device='cuda')
        assert world.area_frontiers(_dev(_u32(rows)), _dev(_u32(dist)), cell, cell_out=mine) is mine and np.array_equal(mine.cpu().numpy(), want[0])


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

E2E_ROWS = 8


@functools.lru_cache(maxsize=None)
def _level(index, cell):
    host = _wad().build_world(index, device=False)
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    return host, tables, g, goal_ref.level_sectors(tables, g, cell)


def _look_around(reveal, st, cell, **kw):
    """tests/test_gpu_goal.py's explored area: four looks around, a quarter turn and a bit apart"""
    fan = torch.from_numpy(rd.map_fan(64, 1.6)).cuda()
    st = st.copy()
    area = reveal(_states(st), fan=fan, max_range=12.0, cell=cell, **kw)
    for _ in range(3):
        st['yaw'] += F(1.6)
        reveal(_states(st), fan=fan, max_range=12.0, cell=cell, area=area, **kw)
    return area


def test_explored_area_planes_flood_frontier_and_walk_of_e1m1_end_to_end():
    rd.set_device(0)
    index, cell, n = 0, 0.25, E2E_ROWS
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    # (seed 34: each of its six players on the map stands where it sees something; the last two are off the map and on a NaN)
    st, _ = sector_ref.players(_wad(), index, n, np.random.default_rng(34), outside=1, nan=1)
    area = _look_around(world.reveal_area, st, cell)
    states = _states(st)
    floor, ceiling = world.draw_area_planes(cell, area=area, floor=True, ceiling=True)
    cells = world.area_cells(states, cell)
    dist = rd.flood_grids(floor, ceiling, cells)
    front, front_dist, count, mask = world.area_frontiers(area, dist, cell, dist_out=True, count_out=True, mask_out=True)
    step, moves = rd.descend_grids(floor, ceiling, dist, front, stop_dist=1)
    # the reference, from the explored area the device revealed (tests/test_gpu_area.py pins it)
    rows = area.cpu().numpy().view(np.uint32)
    _, w_floor, w_ceiling = goal_ref.planes(tables, g, cell, n, area=rows, at_centres=[at])
    w_cells = goal_ref.cells(g, cell, st)
    w_dist, _ = goal_ref.flood_grids(w_floor, w_ceiling, w_cells)
    want = path_ref.area_frontiers(rows, g, w_dist)
    w_step, w_moves, _ = path_ref.descend_grids(w_floor, w_ceiling, w_dist, want[0], stop_dist=1)
    # its preconditions: most of the six rows on the map have a frontier worth the name, the two off it have none
    assert ((want[2][:n - 2] > 10).sum() >= 4) and (want[2][n - 2:] == 0).all() and (want[0][n - 2:] == -1).all(), want[2]
    assert (want[1][:n - 2] > 1).sum() >= 4 and len({tuple(c) for c in want[0].tolist()}) >= 5
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), w_dist)
    _same_front((front.cpu().numpy(), front_dist.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32), mask.cpu().numpy()), want, 'E1M1')
    _same_walk((step.cpu().numpy(), moves.cpu().numpy().view(np.uint32), None), (w_step, w_moves, None), 'E1M1')
    # where to walk now: a 4-neighbour of the player's own cell, one move from it on the way to the frontier
    got, on = step.cpu().numpy(), want[2] > 0
    assert on.sum() >= 4 and (np.abs(got[on] - w_cells[on]).sum(1) == 1).all() and (w_moves[on] == want[1][on] - 1).all()
    assert (got[~on] == -1).all() and (w_moves[~on] == 0).all()


def test_the_same_in_a_three_level_set_with_a_slot_out_of_range():
    rd.set_device(0)
    cell, slots = 0.25, [1, 0, 7]  # E1M2, E1M1, E1M8
    levels = [_level(i, cell) for i in slots]
    tables, grids, at = [l[1] for l in levels], [l[2] for l in levels], [l[3] for l in levels]
    ws = _wad().build_world_set(slots)
    lv = np.array([0, 1, 2, 3, 1, 0xFFFFFFFF, 2, 0], np.uint32)
    n = len(lv)
    # (seeds 60 ..: each of the six players in the set stands where it sees something and has somewhere left to explore)
    st = np.concatenate([sector_ref.players(_wad(), slots[min(int(s), 2)], 1, np.random.default_rng(60 + k), outside=0, nan=0)[0] for k, s in enumerate(lv)])
    levels_t = _dev(lv.view(np.int32))
    area = _look_around(lambda states, **kw: ws.reveal_area(states, levels_t, **kw), st, cell)
    states = _states(st)
    floor, ceiling = ws.draw_area_planes(levels_t, cell, area=area, floor=True, ceiling=True)
    cells = ws.area_cells(states, levels_t, cell)
    dist = rd.flood_grids(floor, ceiling, cells, max_step=0.32)
    got = _front(ws.area_frontiers, area, dist, cell, levels=levels_t)
    step, moves = rd.descend_grids(floor, ceiling, dist, _dev(got[0]), stop_dist=1, max_step=0.32)
    rows = area.cpu().numpy().view(np.uint32)
    _, w_floor, w_ceiling = goal_ref.planes(tables, grids, cell, n, levels=lv, area=rows, at_centres=at)
    w_dist, _ = goal_ref.flood_grids(w_floor, w_ceiling, goal_ref.cells(grids, cell, st, levels=lv), max_step=0.32)
    want = path_ref.area_frontiers(rows, grids, w_dist, levels=lv)
    assert (want[2][[3, 5]] == 0).all() and (want[0][[3, 5]] == -1).all() and (want[2][[0, 1, 2, 4, 6, 7]] > 0).all(), want[2]
    assert (want[2] > 10).sum() >= 4, want[2]
    assert len({(g.gh, g.gw) for g in grids}) == 3 and tuple(dist.shape[1:]) == ws.area_plane_shape(cell)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), w_dist)
    _same_front(got, want, 'set')
    w_step, w_moves, _ = path_ref.descend_grids(w_floor, w_ceiling, w_dist, want[0], stop_dist=1, max_step=0.32)
    _same_walk((step.cpu().numpy(), moves.cpu().numpy().view(np.uint32), None), (w_step, w_moves, None), 'set')
    # a slot outside the set with bits in its rows and a field that reaches everything: still none, and its mask is written
    area[3] = -1
    area[5, 0] = 0x55555555
    everywhere = torch.zeros_like(dist)
    got = _front(ws.area_frontiers, area, everywhere, cell, levels=levels_t)
    rows = area.cpu().numpy().view(np.uint32)
    _same_front(got, path_ref.area_frontiers(rows, grids, np.zeros_like(w_dist), levels=lv), 'set, everything reached')
    assert (got[2][[3, 5]] == 0).all() and not got[3][[3, 5]].any() and (got[2][[0, 1, 2, 4, 6, 7]] > 100).all()


# ---- streams, tensors, pointers, a graph -----------------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_path_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_path_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
