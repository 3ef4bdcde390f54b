"""The goal distance on the GPU (flood.hip: flood_grids_kernel; goal.hip: the two plane kernels, the two cell kernels) against
tests/goal_ref.py, every element of every output, bit for bit.  The flood on hand-made grids in both directions, fifteen rows a
launch, on the longest single runs, against flood_maps where that takes the grid -- once on a grid whose rows and columns are both
ragged runs -- and on shapes it cannot take; the planes of E1M2 and E1M1 against sector_at at the cell centres, at rest and with
offsets, padded, in a set, and through explored-area rows; planes, cells and a TOWARDS flood of the whole of E1M1 end to end; a door
of E1M4 open in one row only; area_cells against the grid's arithmetic and as seeds; streams, the caller's tensors, raw pointers and
a captured graph, in a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flood_ref
import goal_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = goal_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 15  # rows a launch of the hand-made grids


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _states(st):
    return torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()


def _run(floor, ceiling, seeds=None, towards=False, rows=None, **kw):
    """flood_grids of numpy planes on the device, `rows` grids a launch (None: all in one): (distances, counts) as numpy"""
    n = len(floor)
    rows = n if rows is None else rows
    dist, count = [], []
    for a in range(0, n, rows):
        s = _dev(seeds[a:a + rows], np.int32) if seeds is not None else None
        d, c = rd.flood_grids(_dev(floor[a:a + rows], F), _dev(ceiling[a:a + rows], F), s, towards=towards, count_out=True, **kw)
        assert d.dtype == torch.int32 and c.dtype == torch.int32
        dist.append(d.cpu().numpy().view(np.uint32))
        count.append(c.cpu().numpy().view(np.uint32))
    return np.concatenate(dist), np.concatenate(count)


def _same(got, want, what):
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    bad = got[0] != want[0]
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[0][bad][:3], want[0][bad][:3])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def _maps(floor, ceiling, seeds=None, **kw):
    """flood_maps of the same planes, widened"""
    s = _dev(seeds, np.int32) if seeds is not None else None
    dist, count = rd.flood_maps(_dev(floor, F), _dev(ceiling, F), s, count_out=True, **kw)
    return goal_ref.widen(dist.cpu().numpy()), count.cpu().numpy().view(np.uint32)


# ---- the flood on hand-made grids ----------------------------------------------------------------------------------------------------

def _groups():
    groups = {}
    for c in flood_ref.hand_cases():  # the cases of one shape and one set of limits share their launches
        groups.setdefault((c['floor'].shape, tuple(sorted(c['kw'].items()))), []).append(c)
    return groups


def test_hand_made_grids_in_both_directions_fifteen_rows_a_launch():
    rd.set_device(0)
    groups = _groups()
    assert len(groups) >= 6 and max(len(g) for g in groups.values()) >= 10
    for (shape, kw), group in groups.items():
        floor, ceiling = np.stack([c['floor'] for c in group]), np.stack([c['ceiling'] for c in group])
        h, w = shape
        seeds = np.array([c['seed'] if c['seed'] is not None else (w // 2, h // 2) for c in group], np.int64).astype(np.int32)
        want = np.stack([goal_ref.widen(c['want']) for c in group])
        want = (want, (want != U).reshape(len(group), -1).sum(1).astype(np.uint32))
        _same(_run(floor, ceiling, seeds, rows=ROWS, **dict(kw)), want, (shape, kw, [c['name'] for c in group]))
        if all(c['seed'] is None for c in group):
            _same(_run(floor, ceiling, None, **dict(kw)), want, (shape, kw, 'default seeds'))
        _same(_run(floor, ceiling, seeds, towards=True, rows=ROWS, **dict(kw)), goal_ref.flood_grids(floor, ceiling, seeds, True, **dict(kw)),
              (shape, kw, 'towards'))
        # the property of the header: where flood_maps takes the grid, the two agree
        _same(_run(floor, ceiling, seeds, **dict(kw)), _maps(floor, ceiling, seeds, **dict(kw)), (shape, kw, 'flood_maps'))
    # the 7 x 5 grids again, each from every cell of it, in both directions
    seeds = np.array([(col, row) for row in range(5) for col in range(7)], np.int32)
    differ = 0
    for c in flood_ref.hand_cases():
        if c['floor'].shape != (5, 7):
            continue
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        fwd, back = goal_ref.flood_grids(floor, ceiling, seeds, **c['kw']), goal_ref.flood_grids(floor, ceiling, seeds, True, **c['kw'])
        differ += int((fwd[0] != back[0]).any())
        _same(_run(floor, ceiling, seeds, rows=ROWS, **c['kw']), fwd, c['name'])
        _same(_run(floor, ceiling, seeds, towards=True, rows=ROWS, **c['kw']), back, (c['name'], 'towards'))
    assert differ >= 4  # the ledges: the direction matters


def test_the_sides_and_the_longest_single_runs():
    rd.set_device(0)
    _same(_run(*[a[None] for a in flood_ref.room(1, 1)]), (np.zeros((1, 1, 1), np.uint32), np.ones(1, np.uint32)), '1 x 1')
    for shape in ((1, 1, 70000), (1, 70000, 1)):  # refused by the side limit, not by the number of cells
        assert 70000 < rd.flood_grid_max_cells()
        with pytest.raises(rd.RdoomError) as e:
            rd.flood_grids(torch.zeros(shape, device='cuda'), torch.ones(shape, device='cuda'))
        assert e.value.status == -1 and 'a side' in str(e.value)
    line = np.arange(8192, dtype=np.uint32)
    for towards in (False, True):
        for flip in (False, True):
            want = line[::-1] if flip else line
            seed = 8191 if flip else 0
            f, g = flood_ref.room(8192, 1)
            got = _run(f[None], g[None], np.array([[seed, 0]]), towards=towards)
            _same(got, (want.reshape(1, 1, 8192), np.array([8192], np.uint32)), ('1 x 8192', towards, flip))
            f, g = flood_ref.room(1, 8192)
            got = _run(f[None], g[None], np.array([[0, seed]]), towards=towards)
            _same(got, (want.reshape(1, 8192, 1), np.array([8192], np.uint32)), ('8192 x 1', towards, flip))
    assert line.max() == 8191


def _run_length(w, h):
    """the cells of a row or column one thread sweeps at a time, as flood.hip's run_length chooses them for a w x h grid of either
    flood: the shortest run from 2 to 64 that gives each of the 1024 threads at most one run of a phase, else 64"""
    seg = 2
    while seg < 64 and (h * -(-w // seg) > 1024 or w * -(-h // seg) > 1024):
        seg += 1
    return seg


@functools.lru_cache(maxsize=None)
def _long_grids():
    """name -> (floor, ceiling, seeds, towards, the search's result): computed once, left unchanged"""
    out = {}
    f, g = flood_ref.serpentine()
    far = flood_ref.flood(f, g, (0, 0))
    r, c = np.unravel_index(np.argmax(np.where(far == flood_ref.UNREACHED, -1, far.astype(np.int64))), far.shape)
    out['serpentine'] = (np.repeat(f[None], 3, 0), np.repeat(g[None], 3, 0), np.array([(0, 0), (c, r), (16, 14)], np.int32), False)
    for name, (w, h) in (('spiral 255 x 85', (255, 85)), ('spiral 256 x 86', (256, 86))):
        f, g = flood_ref.spiral(w, h)
        inner = goal_ref.flood(f, g, (0, 0))
        r, c = np.unravel_index(np.argmax(np.where(inner == U, -1, inner.astype(np.int64))), inner.shape)
        out[name] = (np.stack([f, f]), np.stack([g, g]), np.array([(0, 0), (c, r)], np.int32), False)  # inwards and outwards
    f, g, seed = flood_ref.staircase(350, 200)
    out['staircase'] = (np.stack([f, f]), np.stack([g, g]), np.array([seed, (0, 0)], np.int32), False)  # the way it goes, and against it
    out['staircase towards'] = (np.stack([f, f]), np.stack([g, g]), np.array([(0, 0), seed], np.int32), True)
    rng = np.random.default_rng(11)
    f = np.where(rng.random((3, 131, 257)) < 0.15, 0.3, 0.0).astype(F)  # rooms with pillars and raised cells
    g = np.where(rng.random((3, 131, 257)) < 0.1, 0.2, 1.5).astype(F)
    seeds = np.array([(128, 65), (0, 0), (256, 130)], np.int32)
    f[np.arange(3), seeds[:, 1], seeds[:, 0]], g[np.arange(3), seeds[:, 1], seeds[:, 0]] = 0.0, 1.5
    out['257 x 131'] = (f, g, seeds, False)
    out['257 x 131 towards'] = (f, g, seeds, True)
    return {k: v + (goal_ref.flood_grids(*v),) for k, v in out.items()}


@pytest.mark.parametrize('name', ['serpentine', 'spiral 255 x 85', 'spiral 256 x 86', 'staircase', 'staircase towards', '257 x 131',
                                  '257 x 131 towards'])
def test_grids_that_take_many_passes_and_shapes_flood_maps_cannot_take(name):
    rd.set_device(0)
    floor, ceiling, seeds, towards, want = _long_grids()[name]
    cells, limit = floor[0].size, rd.flood_max_cells()
    if name in ('serpentine', 'spiral 255 x 85'):
        assert cells <= limit and np.where(want[0] == U, 0, want[0]).max() > 400
    if name == 'spiral 255 x 85':
        assert cells == limit
    if name == 'spiral 256 x 86':  # the first size over flood_maps' limit: one more column and one more row
        assert 255 * 85 == limit < cells and np.where(want[0] == U, 0, want[0]).max() > cells // 3
        with pytest.raises(rd.RdoomError):
            rd.flood_maps(_dev(floor), _dev(ceiling))
    if name == 'staircase':
        assert cells == 70000 > limit and want[1].tolist() == [549, 1] and want[0][0, 0, 0] == 548  # against it: the seed alone
    if name == 'staircase towards':  # towards the top left corner every path cell is finite, towards its own seed only the seed is
        path = flood_ref.open_cells(floor[0], ceiling[0], 0.56)
        assert want[1].tolist() == [549, 1] and np.array_equal(want[0][0] != U, path) and want[0][0, 199, 349] == 548
        assert want[0][1, 199, 349] == 0 and (want[0][1] != U).sum() == 1
    if name.startswith('257 x 131'):
        seg = _run_length(257, 131)
        assert 257 % seg and 131 % seg and (want[1] > 1000).all() and (want[0] == U).any()  # neither side is whole runs
        assert not np.array_equal(want[0], _long_grids()['257 x 131 towards' if not towards else '257 x 131'][4][0])
    _same(_run(floor, ceiling, seeds, towards=towards), want, name)
    if cells <= limit and not towards:
        _same(_run(floor, ceiling, seeds), _maps(floor, ceiling, seeds), (name, 'flood_maps'))


@functools.lru_cache(maxsize=None)
def _ragged_grid():
    """257 x 83, the 257 x 131 recipe at a size flood_maps takes: (floor, ceiling, seeds, goal_ref forwards, goal_ref towards,
    flood_ref widened with its counts): computed once, left unchanged"""
    rng = np.random.default_rng(11)
    f = np.where(rng.random((3, 83, 257)) < 0.15, 0.3, 0.0).astype(F)
    g = np.where(rng.random((3, 83, 257)) < 0.1, 0.2, 1.5).astype(F)
    seeds = np.array([(128, 41), (0, 0), (256, 82)], np.int32)
    f[np.arange(3), seeds[:, 1], seeds[:, 0]], g[np.arange(3), seeds[:, 1], seeds[:, 0]] = 0.0, 1.5
    search = goal_ref.widen(np.stack([flood_ref.flood(f[p], g[p], tuple(int(v) for v in seeds[p])) for p in range(3)]))
    search = (search, (search != U).reshape(3, -1).sum(1).astype(np.uint32))
    return f, g, seeds, goal_ref.flood_grids(f, g, seeds), goal_ref.flood_grids(f, g, seeds, True), search


def test_both_floods_on_a_grid_whose_rows_and_columns_are_ragged_runs():
    """one skeleton, two stores (flood.hip): both kernels on the same 257 x 83 planes, where neither side is whole runs"""
    rd.set_device(0)
    floor, ceiling, seeds, fwd, back, search = _ragged_grid()
    seg = _run_length(257, 83)
    assert floor[0].size <= rd.flood_max_cells() and seg == 28 and 257 % seg == 5 and 83 % seg == 27
    for want in (fwd, back):
        assert want[1][0] > 16000 and want[1][1] < 10 and want[1][2] > 16000 and (want[0] == U).any()
    assert not np.array_equal(fwd[0], back[0])  # the directions differ
    _same(search, fwd, 'the two references')
    _same(_run(floor, ceiling, seeds), fwd, 'flood_grids')
    _same(_run(floor, ceiling, seeds, towards=True), back, 'flood_grids towards')
    maps = _maps(floor, ceiling, seeds)
    _same(maps, search, 'flood_maps')
    _same(maps, _run(floor, ceiling, seeds), 'flood_maps and flood_grids')


# ---- the planes ------------------------------------------------------------------------------------------------------------------------

ROWS_OF_PLANES = 8


@functools.lru_cache(maxsize=None)
def _wad():
    return rd.Wad(ensure_wad(), META_PATH)


@functools.lru_cache(maxsize=None)
def _level(index, cell):
    """the host tables, the grid and the sectors at the cell centres of a level: computed once, left unchanged"""
    host = _wad().build_world(index, device=False)
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    return host, tables, g, goal_ref.level_sectors(tables, g, cell)


def _planes_of(call, **kw):
    sector, floor, ceiling = call(sector_out=True, floor=True, ceiling=True, **kw)
    assert sector.dtype == torch.int16 and floor.dtype == ceiling.dtype == torch.float32
    return sector.cpu().numpy().view(np.uint16), floor.cpu().numpy(), ceiling.cpu().numpy()


def _same_planes(got, want, what):
    for k, name in enumerate(('sector', 'floor', 'ceiling')):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name, got[k].shape, want[k].shape)
        a, b = (got[k], want[k]) if k == 0 else (got[k].view(np.uint32), want[k].view(np.uint32))
        bad = a != b
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:3], want[k][bad][:3])


@pytest.mark.parametrize('index,cell', [(1, 0.25), (1, 0.125), (0, 0.25), (0, 0.125)], ids=['E1M2 0.25', 'E1M2 0.125', 'E1M1 0.25', 'E1M1 0.125'])
def test_the_planes_of_a_level_at_rest_with_offsets_and_padded(index, cell):
    rd.set_device(0)
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    n = ROWS_OF_PLANES
    assert world.area_plane_shape(cell) == (g.gh, g.gw)
    rest = goal_ref.planes(tables, g, cell, n, at_centres=[at])
    assert (rest[0] != sector_ref.NONE16).sum() > 100 * n and (rest[0] == sector_ref.NONE16).any()
    _same_planes(_planes_of(world.draw_area_planes, cell=cell, n=n), rest, 'at rest')
    one = world.draw_area_planes(cell)  # the sector plane of one row, by default
    assert tuple(one.shape) == (1, g.gh, g.gw) and np.array_equal(one.cpu().numpy().view(np.uint16)[0], rest[0][0])
    off = sector_ref.random_offsets(np.random.default_rng(3 + index), n, host.game_objects)
    moved = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    if index == 0:
        assert all((moved[k] != rest[k]).any() for k in (1, 2)) and len({moved[1][p].tobytes() for p in range(n)}) > 4  # rows differ
    _same_planes(_planes_of(world.draw_area_planes, cell=cell, offsets=_dev(off)), moved, 'offsets')
    # planes larger than the grid: the padding is none, in the caller's tensors, which are written in full
    h, w = g.gh + 5, g.gw + 3
    padded = goal_ref.planes(tables, g, cell, n, offsets=off, shape=(h, w), at_centres=[at])
    assert (padded[0][:, g.gh:] == sector_ref.NONE16).all() and np.isposinf(padded[1][:, :, g.gw:]).all() and np.isneginf(padded[2][:, g.gh:]).all()
    mine = (torch.full((n, h, w), 7, dtype=torch.int16, device='cuda'), torch.full((n, h, w), 7.0, device='cuda'),
            torch.full((n, h, w), 7.0, device='cuda'))
    got = world.draw_area_planes(cell, offsets=_dev(off), sector_out=mine[0], floor=mine[1], ceiling=mine[2])
    assert all(a is b for a, b in zip(got, mine))
    _same_planes((mine[0].cpu().numpy().view(np.uint16), mine[1].cpu().numpy(), mine[2].cpu().numpy()), padded, 'padded')
    # one caller's tensor sets the extent of the planes allocated beside it, whichever of the three it is
    mixed = world.draw_area_planes(cell, offsets=_dev(off), sector_out=True, floor=mine[1].fill_(7.0), ceiling=True)
    assert mixed[1] is mine[1] and all(tuple(t.shape) == (n, h, w) for t in mixed)
    _same_planes((mixed[0].cpu().numpy().view(np.uint16), mixed[1].cpu().numpy(), mixed[2].cpu().numpy()), padded, 'padded, mixed')
    only = world.draw_area_planes(cell, offsets=_dev(off), ceiling=True)  # one plane alone
    assert np.array_equal(only.cpu().numpy().view(np.uint32), moved[2].view(np.uint32))


def test_the_planes_of_a_three_level_set_with_a_slot_out_of_range():
    rd.set_device(0)
    cell, slots = 0.25, [1, 0, 7]  # E1M2, E1M1, E1M8
    levels = [_level(i, cell) for i in slots]
    tables, grids, at = [l[1] for l in levels], [l[2] for l in levels], [l[3] for l in levels]
    ws = _wad().build_world_set(slots)
    lv = np.array([0, 1, 2, 3, 1, 0xFFFFFFFF, 2, 0], np.uint32)
    shape = ws.area_plane_shape(cell)
    assert shape == (max(g.gh for g in grids), max(g.gw for g in grids)) and len({(g.gh, g.gw) for g in grids}) == 3
    off = sector_ref.random_offsets(np.random.default_rng(9), len(lv), ws.n_objects)
    want = goal_ref.planes(tables, grids, cell, len(lv), levels=lv, offsets=off, at_centres=at)
    assert (want[0][[3, 5]] == sector_ref.NONE16).all() and all((want[0][p] != sector_ref.NONE16).sum() > 100 for p in (0, 1, 2, 4, 6, 7))
    levels_t = _dev(lv.view(np.int32))
    _same_planes(_planes_of(ws.draw_area_planes, levels=levels_t, cell=cell, offsets=_dev(off)), want, 'set')
    # a level of the set is the single world's, on its own grid
    alone = _planes_of(_wad().build_world(0).draw_area_planes, cell=cell, offsets=_dev(off[1:2]))
    g = grids[1]
    assert np.array_equal(alone[0][0], want[0][1, :g.gh, :g.gw]) and np.array_equal(alone[1][0], want[1][1, :g.gh, :g.gw])
    # and the players' cells in the set: each in the grid of its own level, (-1, -1) outside the set
    st = np.concatenate([sector_ref.players(_wad(), slots[min(int(s), 2)], 1, np.random.default_rng(20 + k), outside=0, nan=0)[0] for k, s in enumerate(lv)])
    want_cells = goal_ref.cells(grids, cell, st, levels=lv)
    assert (want_cells[[3, 5]] == -1).all() and (want_cells[[0, 1, 2, 4, 6, 7]] >= 0).all()
    got = ws.area_cells(_states(st), levels_t, cell)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want_cells)


def test_the_planes_through_the_rows_of_the_explored_area():
    rd.set_device(0)
    index, cell = 0, 0.25
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    n = ROWS_OF_PLANES
    # (seed 34: each of its six players on the map stands where it sees something; the last two are off the map and on a NaN)
    st, _ = sector_ref.players(_wad(), index, n, np.random.default_rng(34), outside=1, nan=1)
    states = _states(st)
    fan = torch.from_numpy(rd.map_fan(64, 1.6)).cuda()
    area = world.reveal_area(states, fan, 12.0, cell)
    for _ in range(3):  # a few more looks around
        st['yaw'] += F(1.6)
        world.reveal_area(_states(st), fan, 12.0, cell, area=area)
    rows = area.cpu().numpy().view(np.uint32)
    off = sector_ref.random_offsets(np.random.default_rng(32), n, host.game_objects)
    whole = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    masked = goal_ref.planes(tables, g, cell, n, offsets=off, area=rows, at_centres=[at])
    is_open = lambda p: np.stack([flood_ref.open_cells(p[1][k], p[2][k], 0.56) for k in range(n)])
    seen, everything = is_open(masked).reshape(n, -1).sum(1), is_open(whole).reshape(n, -1).sum(1)
    assert (seen[:n - 2] > 100).all() and (seen < everything).all() and (seen[n - 2:] == 0).all(), (seen, everything)
    assert (rows[:, 0] & rows[:, 1]).any()  # some cell carries both bits: it is hidden
    _same_planes(_planes_of(world.draw_area_planes, cell=cell, offsets=_dev(off), area=area), masked, 'revealed')
    # rows of all ones in the FREE plane: everything shows; in both planes: nothing does; a longer stride is the caller's
    ones = torch.zeros((n, 2, g.words + 3), dtype=torch.int32, device='cuda')
    ones[:, 0] = -1
    _same_planes(_planes_of(world.draw_area_planes, cell=cell, offsets=_dev(off), area=ones), whole, 'all ones')
    ones[:, 1] = -1
    got = _planes_of(world.draw_area_planes, cell=cell, area=ones)
    assert (got[0] == sector_ref.NONE16).all() and np.isposinf(got[1]).all() and np.isneginf(got[2]).all()
    # the frontier: flooded from the player's cell through what it has seen, the reached cells that border an unseen one
    cells = world.area_cells(states, cell)
    got = rd.flood_grids(_dev(masked[1]), _dev(masked[2]), cells, count_out=True)
    want = goal_ref.flood_grids(masked[1], masked[2], goal_ref.cells(g, cell, st))  # (the yaw has turned, the position has not)
    _same((got[0].cpu().numpy().view(np.uint32), got[1].cpu().numpy().view(np.uint32)), want, 'frontier')
    assert (want[1][:n - 2] > 50).all() and (want[1][n - 2:] == 0).all(), want[1]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

E2E_STEP = 0.32  # the synthetic E1M1 joins most of its sectors by steps of 0.32: at the default 0.24, 1371 of its 25 230 open cells at
#                  0.125 can walk to the start; with 0.32, 21 133 can


def test_planes_cells_and_a_flood_towards_the_start_of_e1m1_end_to_end():
    rd.set_device(0)
    index, cell, n = 0, 0.125, 4
    host, tables, g, at = _level(index, cell)
    assert g.gw * g.gh > rd.flood_max_cells()  # more cells than flood_maps takes
    world = _wad().build_world(index)
    pos, yaw = _wad().build_level(index).start()
    st = rd.player_states(np.repeat(np.asarray(pos, F)[None], n, 0), np.full(n, yaw, F))
    off = sector_ref.random_offsets(np.random.default_rng(7), n, host.game_objects)
    off[0] = 0  # row 0: all at rest
    _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    seeds = goal_ref.cells(g, cell, st)
    assert (seeds >= 0).all()
    for step in (E2E_STEP, 0.24):
        want = goal_ref.flood_grids(floor, ceiling, seeds, True, max_step=step)
        if step == E2E_STEP:  # on the reference: a field worth having, not all of the level, and not the forward flood
            is_open = np.stack([flood_ref.open_cells(floor[p], ceiling[p], 0.56) for p in range(n)])
            reached = want[0] != U
            assert (2 * want[1] > is_open.reshape(n, -1).sum(1)).all(), (want[1], is_open.reshape(n, -1).sum(1))
            assert all((is_open[p] & ~reached[p]).any() for p in range(n))
            forward = goal_ref.flood_grids(floor, ceiling, seeds, False, max_step=step)
            assert all((forward[0][p] != want[0][p]).any() for p in range(n))
            assert len({want[0][p].tobytes() for p in range(n)}) > 1  # the rows' doors and lifts count
        states = _states(st)
        f_t, c_t = world.draw_area_planes(cell, offsets=_dev(off), floor=True, ceiling=True)
        cells = world.area_cells(states, cell)
        assert np.array_equal(cells.cpu().numpy(), seeds)
        dist, count = rd.flood_grids(f_t, c_t, cells, towards=True, max_step=step, count_out=True)
        _same((dist.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)), want, ('end to end', step))
        # the tick's gather: the distance at the player's own cell is 0, and (-1, -1) maps to unreached
        at_player = dist[torch.arange(n, device='cuda'), cells[:, 1].long(), cells[:, 0].long()]
        assert (at_player == 0).all()


def test_a_door_shut_in_one_row_and_open_in_the_other():
    """E1M4's manual door of object 12 (the one behind trigger 16; it rises by 1.24), the goal the cell (166, 170) at cell 0.125, next
    to the door's cells (columns 161-165 of rows 170-174) on the side away from the level's start.  The synthetic levels stand their
    doors free in rooms: with it shut the rest of the room still walks round it, so the cells only the open row brings to the goal
    are the door's own 25, and more than a thousand cells get there sooner through it."""
    rd.set_device(0)
    index, cell, door, lift, goal = 3, 0.125, 12, 1.24, (166, 170)
    host, tables, g, at = _level(index, cell)
    t = host.triggers()
    assert t['triggers']['special_type'][16] == 1 and t['effects'][t['triggers']['effect_start'][16]]['object_id'] == door
    assert any(int(e['object_id']) == door and abs(float(e['first_height_offset']) - lift) < 1e-6 for e in t['effects'])
    off = np.zeros((2, host.game_objects, 3), F)
    off[1, door, 1] = lift
    sector, floor, ceiling = goal_ref.planes(tables, g, cell, 2, offsets=off, at_centres=[at])
    in_door = (sector[0] != sector_ref.NONE16) & (tables.sectors['ceiling_id'][np.minimum(sector[0], len(tables.sectors) - 1)] == door)
    seeds = np.array([goal, goal], np.int32)
    want = goal_ref.flood_grids(floor, ceiling, seeds, True)
    shut, opened = want[0]
    assert in_door.sum() == 25 and not in_door[goal[1], goal[0]] and in_door[goal[1], goal[0] - 1]
    assert (shut[in_door] == U).all() and (opened[in_door] != U).all() and want[1][1] == want[1][0] + 25 > 10000
    assert np.array_equal((opened != U) & (shut == U), in_door)  # the cells the open row reaches and the shut row does not
    both = shut != U
    assert (opened[both] <= shut[both]).all() and (opened[both] < shut[both]).sum() > 1000
    world = _wad().build_world(index)
    got = _planes_of(world.draw_area_planes, cell=cell, offsets=_dev(off))
    _same_planes(got, (sector, floor, ceiling), 'E1M4')
    dist, count = rd.flood_grids(_dev(got[1]), _dev(got[2]), _dev(seeds), towards=True, count_out=True)
    _same((dist.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)), want, 'doors')


# ---- the cells -------------------------------------------------------------------------------------------------------------------------

def test_the_cells_of_64_players_and_the_cells_as_seeds():
    rd.set_device(0)
    index, cell, n = 0, 0.25, 64
    host, tables, g, at = _level(index, cell)
    world = _wad().build_world(index)
    st, on_map = sector_ref.players(_wad(), index, n, np.random.default_rng(5))
    want = goal_ref.cells(g, cell, st)
    assert on_map == n - 6 and (want[:on_map] >= 0).all() and (want[on_map:] == -1).all() and len({tuple(c) for c in want.tolist()}) > 30
    for c in (cell, 0.0625):
        gc = host.area_grid(c)
        got = world.area_cells(_states(st), c)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 2)
        assert np.array_equal(got.cpu().numpy(), goal_ref.cells(gc, c, st)), c
    out = torch.full((n, 2), 7, dtype=torch.int32, device='cuda')
    assert world.area_cells(_states(st), cell, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    # the cells as seeds, valid pairs and (-1, -1) alike: the latter give an all-unreached row
    _, floor, ceiling = goal_ref.planes(tables, g, cell, 1, at_centres=[at])
    floor, ceiling = np.repeat(floor, n, 0), np.repeat(ceiling, n, 0)
    ref = goal_ref.flood_grids(floor, ceiling, want, True)
    assert (ref[1][on_map:] == 0).all() and (ref[0][on_map:] == U).all() and (ref[1][:on_map] > 0).sum() > n // 2
    dist, count = rd.flood_grids(_dev(floor), _dev(ceiling), out, towards=True, count_out=True)
    _same((dist.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)), ref, 'cells as seeds')


# ---- streams, tensors, pointers, a graph -----------------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_goal_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_goal_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
