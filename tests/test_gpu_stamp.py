"""The solid things on the grid on the GPU (stamp.hip: stamp_things_kernel and its world-set twin) against tests/stamp_ref.py, the
header's "solid things on the grid" restated in numpy with no cull, no tiles and no list: every word of both planes and every
index, with no tolerance.  The hand cases of tests/stamp_cases.py, many rows a launch; random tables at the word, wave and pass
boundaries on 67 x 35 and 130 x 19 grids with solid and hidden rows, a wider stride, offsets and a finite window; a heap of things
longer than the kernel's list; grids about the tile's size and the smallest a level has; things on a corner four tiles share and
half outside the grid; planes wider than the grid; in place against out of place, each output alone, an overlap refused; a set of
three levels; the argument errors that read a handle; two corridors with the distances written out; E1M1 end to end through
inflate_grids and flood_grids; streams, raw pointers, a collecting walk and a captured graph in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goal_ref
import rust_doom_amd as rd
import stamp_cases as sc
import stamp_ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
X = goal_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
TX, TY = rd.STAMP_TILE
LIST_CAPACITY = 768  # stamp.hip LIST_CAP: the things a workgroup's LDS list holds; it is folded when fewer than 256 slots are free
POISON_F, POISON_I = 7.0, 0x5EEEEEEE


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).cuda()


def _rows(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _words(t):
    return t.cpu().numpy().view(U)


def same(got, want, what):
    got = got.cpu().numpy()
    a, b = (got.view(U), np.ascontiguousarray(want).view(U)) if got.dtype.itemsize == 4 else (got, want)  # words, not values
    bad = a != b
    assert a.shape == b.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], a[bad][:6], b[bad][:6])


def check(stamp, floor, ceiling, want, what, **kw):
    """one launch out of place into poisoned tensors with the index plane, one in place, the planes alone and the index alone,
    each against the reference's (floor, ceiling, index).  stamp(floor, ceiling, **kw) is the bound call"""
    f, c = _dev(floor, F), _dev(ceiling, F)
    fo, co = torch.full_like(f, POISON_F), torch.full_like(c, POISON_F)
    index = torch.full(f.shape, POISON_I, dtype=torch.int32, device='cuda')
    got = stamp(f, c, floor_out=fo, ceiling_out=co, index_out=index, **kw)
    assert got[0] is fo and got[1] is co and got[2] is index
    same(fo, want[0], (what, 'floor')), same(co, want[1], (what, 'ceiling')), same(index, want[2], (what, 'index'))
    same(f, floor, (what, 'the input floor')), same(c, ceiling, (what, 'the input ceiling'))  # out of place: the inputs stand
    got = stamp(f, c, **kw)  # allocated
    assert len(got) == 2 and got[0].dtype == got[1].dtype == torch.float32
    same(got[0], want[0], (what, 'floor alone')), same(got[1], want[1], (what, 'ceiling alone'))
    only = stamp(f, c, floor_out=False, ceiling_out=False, index_out=True, **kw)
    assert only.dtype == torch.int32
    same(only, want[2], (what, 'index alone'))
    got = stamp(f, c, floor_out=f, ceiling_out=c, **kw)
    assert got[0] is f and got[1] is c
    same(f, want[0], (what, 'floor in place')), same(c, want[1], (what, 'ceiling in place'))


def world_of(wad):
    rd.set_device(0)
    return wad.build_world(0)


# ---- the hand cases -------------------------------------------------------------------------------------------------------------------

def test_the_hand_cases_many_rows_a_launch():
    """the cases of one window share a launch: their tables one after the other in one set, row p stamped with case p's things
    alone -- its hidden row hides every other case's -- on its own floors and offsets; an index counts from the case's first thing"""
    world = world_of(sc.room_wad(2, 2))
    assert world.area_grid(sc.HAND_CELL) == sc.HAND_GRID
    cases = [c for c in sc.hand_cases() if c['name'] != 'an object beyond the row']  # the library refuses such offsets (below)
    for window in (sc.WIDE, sc.NARROW, sc.SHORT):
        group = [c for c in cases if c['window'] == window]
        assert group
        firsts = np.cumsum([0] + [len(c['table']) for c in group])
        total = int(firsts[-1])
        table = np.concatenate([c['table'] for c in group])
        stride = (total + 31) // 32 + 1
        solid, hidden = np.ones(total, bool), np.ones((len(group), total), bool)
        for p, c in enumerate(group):
            lo, hi = firsts[p], firsts[p + 1]
            hidden[p, lo:hi] = False
            if c['hidden'] is not None:
                hidden[p, lo + np.array(c['hidden'], np.int64)] = True
            if c['solid'] is not None:
                solid[lo:hi] = False
                solid[lo + np.array(c['solid'], np.int64)] = True
        # a thing that is not solid is so in every row: it must belong to no other case's expectation, which holds as rows hide them
        floor = np.concatenate([sc.hand_planes(c)[0] for c in group])
        ceiling = np.concatenate([sc.hand_planes(c)[1] for c in group])
        offsets = np.concatenate([sc.hand_offsets(c) for c in group])
        index = np.stack([sc.hand_index(c, first=int(firsts[p])) for p, c in enumerate(group)])
        want = sc.planes_of(floor, ceiling, index) + (index,)
        things = rd.DeviceThings(table)
        kw = dict(solid=_rows(rd.pack_things(solid, stride)[None]), hidden=_rows(np.stack([rd.pack_things(h, stride) for h in hidden])),
                  offsets=_dev(offsets), grow=window[0], block_below=window[1], block_above=window[2])
        check(lambda f, c, **k: world.stamp_things(f, c, things, sc.HAND_CELL, **k), floor, ceiling, want, ('hand cases', window), **kw)
        things.close()
    # offsets whose row ends at or below the set's largest object_id are refused, so off() never reads beyond a row on the device
    things = rd.DeviceThings(sc.things_at([sc.at(3, 4)], object_id=9))
    f, c = (_dev(a) for a in sc.flat(1, sc.HAND_GRID))
    with pytest.raises(rd.RdoomError) as e:
        world.stamp_things(f, c, things, sc.HAND_CELL, offsets=_dev(np.zeros((1, 9, 3), F)))
    assert e.value.status == -1 and 'object_id' in str(e.value)
    things.close(), world.close()


# ---- random tables ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('grid', [(67, 35), (130, 19)], ids=['67x35', '130x19'])
@pytest.mark.parametrize('size', sc.SIZES)
def test_random_tables_at_the_word_wave_and_pass_boundaries(grid, size):
    for grow in (0.0, 0.19):
        c = sc.random_case(grid[0], grid[1], size, grow)
        blocked = c['want'][2] >= 0
        assert blocked[0].any() and not blocked.all()
        world = world_of(c['wad'])
        things = rd.DeviceThings(c['table'])
        kw = dict(solid=_rows(c['solid']), hidden=_rows(c['hidden']), offsets=_dev(c['offsets']), **c['window'])
        check(lambda f, g, **k: world.stamp_things(f, g, things, c['cell'], **k), c['floor'], c['ceiling'], c['want'], (grid, size, grow), **kw)
        things.close(), world.close()


def test_a_heap_of_things_longer_than_the_list():
    """1100 solid things within half a unit of one point, their discs over every tile near it: the list is folded and emptied in
    chunks.  The window is evaluated in the fold, not in the cull: the first 800 things stand 5 up and block only floors at 5, so
    where the floor is 0 a cell's lowest index comes from the list's second chunk"""
    wad, host, cell, grid = sc.room_of_grid(130, 19)
    rng = np.random.default_rng(1100)
    x, z = goal_ref.centres(grid, cell)
    size = 1100
    assert size > LIST_CAPACITY
    table = np.zeros(size, rd.THING)
    table['x'] = (x[63] + rng.uniform(-0.5, 0.5, size)).astype(F)
    table['z'] = (z[9] + rng.uniform(-0.5, 0.5, size)).astype(F)
    table['radius'] = rng.uniform(0.0, 2 * cell, size).astype(F)
    table['base'][:800] = 5.0
    floor, ceiling = sc.flat(3, grid)
    floor[0] = 5.0
    floor[2, :, ::2] = 5.0
    ceiling += floor
    window = dict(block_below=0.25, block_above=0.25)
    want = stamp_ref.stamp(table, grid, cell, floor, ceiling, **window)
    assert want[2][0].max() < 800 and (want[2][0] >= 0).sum() > 400
    low = want[2][1][want[2][1] >= 0]
    assert len(low) > 300 and low.min() >= 800 > LIST_CAPACITY  # every blocked cell of row 1 owes it to the second chunk
    world, things = world_of(wad), rd.DeviceThings(table)
    check(lambda f, c, **k: world.stamp_things(f, c, things, cell, **k), floor, ceiling, want, 'a heap', **window)
    things.close(), world.close()


# ---- tiles ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('grid', [(TX - 1, TY), (TX, TY), (TX + 1, TY), (TX, TY - 1), (TX, TY + 1), (3, 3)], ids=lambda g: '%dx%d' % g)
def test_grids_about_the_tile_and_the_smallest_a_level_has(grid):
    """(no level's grid is below 3 x 3: a cell of margin on each side of the cells its lines touch)"""
    wad, host, cell, g = sc.room_of_grid(*grid)
    x, z = goal_ref.centres(g, cell)
    rng = np.random.default_rng(grid[0] * 100 + grid[1])
    corners = [(x[i], z[j]) for i in (0, -1) for j in (0, -1)]  # a thing on every corner cell, then some anywhere
    pts = corners + [(rng.uniform(x[0], x[-1]), rng.uniform(z[0], z[-1])) for _ in range(12)]
    table = sc.things_at(pts, radius=rng.uniform(0, 2.5 * cell, len(pts)).astype(F))
    floor, ceiling = sc.flat(3, g)
    hidden = sc.bit_rows([[], [0, 1, 2, 3], list(range(4, len(pts)))])
    want = stamp_ref.stamp(table, g, cell, floor, ceiling, hidden=hidden)
    assert (want[2][0][[0, 0, -1, -1], [0, -1, 0, -1]] >= 0).all() and (want[2][2] >= 0).sum() >= 4
    world, things = world_of(wad), rd.DeviceThings(table)
    check(lambda f, c, **k: world.stamp_things(f, c, things, cell, **k), floor, ceiling, want, ('tile', grid), hidden=_rows(hidden))
    things.close(), world.close()


def test_a_corner_four_tiles_share_the_grids_edges_and_planes_wider_than_the_grid():
    wad, host, cell, g = sc.room_of_grid(130, 19)
    x, z = goal_ref.centres(g, cell)
    h = 0.5 * cell
    pts = [(x[TX] - h, z[TY] - h),                  # the corner cells (63, 15), (64, 15), (63, 16) and (64, 16) share, in four tiles
           (x[0] - h, z[7]), (x[-1] + h, z[7]),     # on the grid's left and right edge, half outside
           (x[40], z[0] - h), (x[40], z[-1] + h),   # on its upper and lower edge
           (x[TX - 1], z[3]), (x[TX], z[12]),       # in a tile's last column, and in the next tile's first
           (x[100], z[TY - 1]), (x[101], z[TY])]    # in a tile's last row, and in the next tile's first
    table = sc.things_at(pts, radius=[1.6 * cell] * 5 + [0.0] * 4)
    for shape in ((19, 130), (19 + 3, 130 + 5), (TY * 2 + 1, TX * 3)):  # the level's own extent, and two wider ones
        floor, ceiling = sc.flat(2, g, shape, floor=0.25)
        floor[:, g.gh:, :], floor[:, :, g.gw:] = -0.0, np.nan  # the surplus is passed through, whatever it holds
        hidden = sc.bit_rows([[], [0]])
        want = stamp_ref.stamp(table, g, cell, floor, ceiling, hidden=hidden)
        for i, j in ((TX - 1, TY - 1), (TX, TY - 1), (TX - 1, TY), (TX, TY)):
            assert want[2][0, j, i] == 0 and want[2][1, j, i] == -1
        assert (want[2][0, 7, [0, -1 - (shape[1] - g.gw)]] == [1, 2]).all() and want[2][0, 0, 40] == 3 and want[2][0, g.gh - 1, 40] == 4
        assert (want[2][:, g.gh:, :] == -1).all() and (want[2][:, :, g.gw:] == -1).all()
        world, things = world_of(wad), rd.DeviceThings(table)
        check(lambda f, c, **k: world.stamp_things(f, c, things, cell, **k), floor, ceiling, want, ('seams', shape), hidden=_rows(hidden))
        things.close(), world.close()


# ---- the calls --------------------------------------------------------------------------------------------------------------------------

def test_an_overlapping_output_and_the_errors_that_read_a_handle():
    wad, host, cell, g = sc.room_of_grid(67, 35)
    world = world_of(wad)
    table = sc.things_at([sc.centre(g, cell, 5, 5)], object_id=3)
    things, two = rd.DeviceThings(table), rd.DeviceThings([table, table])
    f, c = (_dev(a) for a in sc.flat(2, g))
    before = _words(f).copy()
    rows = torch.zeros((2, 1), dtype=torch.int32, device='cuda')

    def refused(word, floor=f, ceiling=c, handle=world, th=things, cell_=cell, **kw):
        with pytest.raises(rd.RdoomError) as e:
            handle.stamp_things(floor, ceiling, th, cell_, **kw)
        assert e.value.status == -1 and word in str(e.value), e.value

    refused('overlaps an input', floor_out=f, ceiling_out=torch.empty_like(c))  # in place means both planes
    refused('overlaps an input', floor_out=c, ceiling_out=f)
    refused('overlaps an input', index_out=f.view(torch.int32))
    spare = torch.empty_like(f)
    refused('two outputs overlap', floor_out=spare, ceiling_out=spare)
    host_only = wad.build_world(0, device=False)
    refused('HOST_ONLY', handle=host_only)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        refused('cell', cell_=bad)
    refused('over its limits', cell_=1e-12)
    small = (_dev(sc.flat(2, g, (g.gh, g.gw - 1))[0]), _dev(sc.flat(2, g, (g.gh, g.gw - 1))[1]))
    refused('grid at cell', floor=small[0], ceiling=small[1])
    short = (_dev(sc.flat(2, g, (g.gh - 1, g.gw))[0]), _dev(sc.flat(2, g, (g.gh - 1, g.gw))[1]))
    refused('grid at cell', floor=short[0], ceiling=short[1])
    refused('thing set of 2 levels', th=two)
    refused('stride', hidden=rows.data_ptr(), stride=0)
    refused('stride', solid=rows.data_ptr(), stride=0)
    refused('n_objects', offsets=torch.zeros((2, 3, 3), device='cuda'))  # object 3 needs four rows
    if host.game_objects > 1:
        refused('n_objects', th=rd.DeviceThings(sc.things_at([(0.0, 0.0)])), offsets=torch.zeros((2, 1, 3), device='cuda'))
    torch.cuda.synchronize()
    assert np.array_equal(_words(f), before)  # nothing was queued
    # the set form: null levels, and a thing set of another size
    ws = sc.e1m1_wad().build_world_set([1, 6])
    h, w = ws.area_plane_shape(0.5)
    fs, cs = torch.zeros((2, h, w), device='cuda'), torch.ones((2, h, w), device='cuda')
    with pytest.raises(rd.RdoomError) as e:
        ws.stamp_things(None, fs, cs, two, 0.5)
    assert 'null levels' in str(e.value)
    with pytest.raises(rd.RdoomError) as e:
        ws.stamp_things(torch.zeros(2, dtype=torch.int32, device='cuda'), fs, cs, things, 0.5)
    assert 'thing set of 1 levels' in str(e.value)
    # n == 0 queues nothing and needs no plane
    assert world.stamp_things(f, c, things, cell, n=0, floor_out=f, ceiling_out=c)[0] is f
    for t in (things, two, world, ws):
        t.close()


def test_a_set_of_three_levels_with_slots_out_of_range():
    """each row stamped with its own level's things, solid bits and grid; a row whose slot is outside the set passes through"""
    rd.set_device(0)
    wad, cell, indices = sc.e1m1_wad(), 0.25, [1, 6, 2]
    ws = wad.build_world_set(indices)
    hosts = [wad.build_world(i, device=False) for i in indices]
    grids = [h.area_grid(cell) for h in hosts]
    rng = np.random.default_rng(33)
    tables, solid_bits = [], []
    for hst, g in zip(hosts, grids):  # the level's own things, and random ones over its grid
        x, z = goal_ref.centres(g, cell)
        extra = sc.things_at(np.stack([rng.uniform(x[0], x[-1], 40), rng.uniform(z[0], z[-1], 40)], 1), radius=rng.uniform(0, 0.6, 40).astype(F))
        tables.append(np.concatenate([hst.map_things(), extra]))
        solid_bits.append(np.concatenate([hst.thing_obstacles(), rng.random(40) < 0.5]))
    assert hosts[0].thing_obstacles().sum() == 1  # E1M2's one thing is solid
    levels = np.array([0, 1, 2, 3, 1, 0xFFFFFFFF, 2, 0], U)
    n = len(levels)
    h, w = ws.area_plane_shape(cell)
    assert (h, w) == (max(g.gh for g in grids), max(g.gw for g in grids))
    floor = rng.choice(F([0.0, 0.25, 1.0]), (n, h, w))
    ceiling = floor + F(1.28)
    things = rd.DeviceThings(tables)
    stride = things.words() + 1
    solid = rd.pack_things(solid_bits, stride).view(U)
    hidden = (rng.integers(0, 1 << 32, (n, stride), dtype=np.uint64) & rng.integers(0, 1 << 32, (n, stride), dtype=np.uint64)).astype(U)
    hidden[4] = 0
    window = dict(grow=0.1, block_below=0.5, block_above=0.5)
    want = stamp_ref.stamp(tables, grids, cell, floor, ceiling, levels=levels, solid=solid, hidden=hidden, **window)
    for p, lv in enumerate(levels):
        if lv >= 3:
            assert (want[2][p] == -1).all()
        else:
            assert (want[2][p] >= 0).any() and want[2][p].max() < len(tables[lv])
    assert want[2][1].tobytes() != want[2][4].tobytes()  # the hidden rows count
    lv_t = _rows(levels)
    check(lambda f, c, **k: ws.stamp_things(lv_t, f, c, things, cell, **k), floor, ceiling, want, 'a set', solid=_rows(solid), hidden=_rows(hidden),
          **window)
    things.close(), ws.close()


# ---- corridors --------------------------------------------------------------------------------------------------------------------------

def _split_room(gap_rows):
    """9 x 7, flat, a wall down column 4 with the rows of `gap_rows` left open, the outer ring closed"""
    floor, ceiling = sc.flat(1, None, (7, 9))
    ceiling[0, [0, -1], :] = ceiling[0, :, [0, -1]] = 0.5
    for r in range(7):
        if r not in gap_rows:
            ceiling[0, r, 4] = 0.5
    return floor, ceiling


def test_a_barrel_in_a_gap_forces_the_detour_and_one_in_a_narrow_gap_cuts_the_flood_off():
    wad, host, cell, g = sc.room_of_grid(9, 7)
    world = world_of(wad)
    barrel = rd.DeviceThings(sc.things_at([sc.centre(g, cell, 4, 3)], radius=0.25 * cell))  # in the gap's middle cell
    seed = _dev(np.array([[1, 3]], np.int32))

    def flooded(f, c):
        dist, count = rd.flood_grids(f, c, seed, count_out=True)
        return dist.cpu().numpy().view(U)[0].tolist(), int(count.cpu().numpy()[0])

    floor, ceiling = _split_room({2, 3, 4})
    f, c = _dev(floor), _dev(ceiling)
    got, reached = flooded(f, c)
    assert got[3] == [X, 0, 1, 2, 3, 4, 5, 6, X] and reached == 33  # straight through the gap's middle
    _, _, index = world.stamp_things(f, c, barrel, cell, floor_out=f, ceiling_out=c, index_out=True)
    assert np.argwhere(index.cpu().numpy()[0] >= 0).tolist() == [[3, 4]]
    got, reached = flooded(f, c)
    want = [[X] * 9,
            [X, 2, 3, 4, X, 6, 7, 8, X],
            [X, 1, 2, 3, 4, 5, 6, 7, X],  # the detour through the gap's side cells
            [X, 0, 1, 2, X, 6, 7, 8, X],  # the barrel's cell is shut: two moves more to the cell behind it
            [X, 1, 2, 3, 4, 5, 6, 7, X],
            [X, 2, 3, 4, X, 6, 7, 8, X],
            [X] * 9]
    assert got == want and reached == 32

    floor, ceiling = _split_room({3})
    f, c = _dev(floor), _dev(ceiling)
    got, reached = flooded(f, c)
    assert got[3][5] == 4 and reached == 31
    fo, co = world.stamp_things(f, c, barrel, cell)
    got, reached = flooded(fo, co)
    want = [[X] * 9] + [[X, abs(r - 3) + 0, abs(r - 3) + 1, abs(r - 3) + 2, X, X, X, X, X] for r in range(1, 6)] + [[X] * 9]
    assert got == want and reached == 15  # the seed's side alone: the one gap is shut
    barrel.close(), world.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def test_planes_stamp_inflation_and_a_flood_towards_the_start_of_e1m1_end_to_end():
    rd.set_device(0)
    c = sc.e1m1_case()
    cell = sc.E2E_CELL
    world = sc.e1m1_wad().build_world(0)
    things = rd.DeviceThings(c['table'])
    off, seeds = _dev(c['offsets']), _dev(c['seeds'])
    f, g = world.draw_area_planes(cell, offsets=off, floor=True, ceiling=True)
    same(f, c['floor'], 'planes, floor'), same(g, c['ceiling'], 'planes, ceiling')
    plain_i = rd.inflate_grids(f, g, sc.BODY, cell)
    plain, _ = rd.flood_grids(plain_i[0], plain_i[1], seeds, towards=True, max_step=sc.E2E_STEP, count_out=True)
    same(plain, c['plain'][1][0], 'the unstamped flood')
    got = world.stamp_things(f, g, things, cell, solid=_rows(c['solid']), hidden=_rows(c['hidden']), offsets=off, floor_out=f, ceiling_out=g,
                             index_out=True)
    assert got[0] is f and got[1] is g
    same(f, c['stamped'][0], 'stamped floor'), same(g, c['stamped'][1], 'stamped ceiling'), same(got[2], c['stamped'][2], 'index')
    fi, gi = rd.inflate_grids(f, g, sc.BODY, cell)
    same(fi, c['after'][0][0], 'inflated floor'), same(gi, c['after'][0][1], 'inflated ceiling')
    dist, count = rd.flood_grids(fi, gi, seeds, towards=True, max_step=sc.E2E_STEP, count_out=True)
    same(dist, c['after'][1][0], 'flood')
    assert np.array_equal(count.cpu().numpy().view(U), c['after'][1][1])
    # on the device's output
    stamped, unstamped, index = dist.cpu().numpy().view(U), plain.cpu().numpy().view(U), got[2].cpu().numpy()
    assert np.array_equal(stamped[1], unstamped[1]) and np.array_equal(_words(fi)[1], _words(plain_i[0])[1])  # row 1: word for word
    opened = sc.open_cells(c['floor'], c['ceiling'])
    assert (opened[0] & (index[0] >= 0)).sum() == 14 and count.cpu().numpy()[0] == 17550
    for p in range(4):
        reached = stamped[p] != X
        assert not (reached & (index[p] >= 0)).any()
        assert (unstamped[p][reached] != X).all() and (unstamped[p][reached] <= stamped[p][reached]).all()
    things.close(), world.close()


# ---- streams, tensors, pointers, a collecting walk, a graph -----------------------------------------------------------------------------

def test_streams_raw_pointers_a_collecting_walk_and_a_graph_in_one_child():
    """tests/gpu_stamp_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_stamp_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
