"""The wall distance on the GPU (walls.hip: wall_distance_kernel) against tests/walls_ref.py, every element of every output, bit for
bit: grids written out by hand, fifteen rows a launch; the exact disc round one closed cell at every radius on either side of a
power of two; blocking cells on the last column and row of a tile and the first of the next, at the tile's size and one off it;
random grids against the definition at every radius, with both flags, for the distances alone, the planes alone and both; the
longest strips; a grid of many tiles against the two-phase form; the planes as 32-bit words, NaN payloads and the sign of a zero
included; two corridors whose flooded distances are written out by hand; E1M1 end to end through planes, inflation and a flood
towards the start; the sector maps of eight players of E1M2 through flood_maps; streams, the caller's tensors, raw pointers and a
captured graph, in a child process."""
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
import walls_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
X = walls_ref.FAR
U = goal_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 15  # rows a launch
RADII = (1, 2, 3, 4, 7, 8, 9, 31, 32)
TX, TY = rd.WALL_TILE


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _distances(floor, ceiling, radius, edge_open=False, **kw):
    """wall_distances of numpy planes: the distances as numpy uint16"""
    got = rd.wall_distances(_dev(floor, F), _dev(ceiling, F), radius, edge_open=edge_open, **kw)
    assert got.dtype == torch.uint16 and tuple(got.shape) == floor.shape
    return got.cpu().numpy()


def _inflated(floor, ceiling, radius, edge_open=False, dist2=False, **kw):
    """inflate_grids of numpy planes with close_d2 = radius * radius (a body of `radius` cells at cell 1): numpy (floor, ceiling[,
    dist2]), the planes as float32 whose words are the device's"""
    got = rd.inflate_grids(_dev(floor, F), _dev(ceiling, F), float(radius), 1.0, edge_open=edge_open, dist2_out=True if dist2 else None, **kw)
    assert len(got) == (3 if dist2 else 2) and got[0].dtype == got[1].dtype == torch.float32
    return tuple(t.cpu().numpy() for t in got)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == F else (got, want)
    bad = a != b
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], a[bad][:3], b[bad][:3])


def _all_three(floor, ceiling, exact, radius, edge_open, what):
    """the distances alone, the planes alone and both, against the uncapped distances `exact` of the definition"""
    want = walls_ref.report(exact, radius)
    want_planes = walls_ref.inflate(floor, ceiling, want, radius * radius)
    _same(_distances(floor, ceiling, radius, edge_open), want, (what, radius, edge_open, 'distances'))
    got = _inflated(floor, ceiling, radius, edge_open)
    _same(got[0], want_planes[0], (what, radius, edge_open, 'floor'))
    _same(got[1], want_planes[1], (what, radius, edge_open, 'ceiling'))
    got = _inflated(floor, ceiling, radius, edge_open, dist2=True)
    _same(got[0], want_planes[0], (what, radius, edge_open, 'floor, with distances'))
    _same(got[1], want_planes[1], (what, radius, edge_open, 'ceiling, with distances'))
    _same(got[2], want, (what, radius, edge_open, 'distances, with planes'))


# ---- grids written out by hand -------------------------------------------------------------------------------------------------------

def test_hand_made_grids_fifteen_rows_a_launch():
    rd.set_device(0)
    groups = {}
    for c in walls_ref.hand_cases():  # the cases of one shape, one radius and one flag share a launch
        groups.setdefault((c['floor'].shape, c['radius'], c['edge_open']), []).append(c)
    assert len(groups) >= 8
    for (shape, radius, edge), group in groups.items():
        rows = [group[k % len(group)] for k in range(ROWS)]
        floor, ceiling = np.stack([c['floor'] for c in rows]), np.stack([c['ceiling'] for c in rows])
        want = np.stack([c['want'] for c in rows])
        _same(_distances(floor, ceiling, radius, edge), want, (shape, radius, edge, [c['name'] for c in group]))
    # a different grid in every row: the 5 x 5 disc of the 7 x 7 case, written out there, around fifteen different cells of a 9 x 8 grid
    disc = np.array([[X, X, 4, X, X], [X, 2, 1, 2, X], [4, 1, 0, 1, 4], [X, 2, 1, 2, X], [X, X, 4, X, X]], np.uint16)
    assert np.array_equal(disc, {c['name']: c for c in walls_ref.hand_cases()}['7x7 centre closed, edge open, R 2']['want'][1:6, 1:6])
    floor, ceiling = (np.repeat(a[None], ROWS, 0) for a in flood_ref.room(9, 8))
    want = np.full((ROWS, 8, 9), X, np.uint16)
    cells = [(k * 4 % 9, k * 3 % 8) for k in range(ROWS)]
    assert len(set(cells)) == ROWS
    for k, (c, r) in enumerate(cells):
        ceiling[k, r, c] = F(0.5)
        canvas = np.full((8 + 4, 9 + 4), X, np.uint16)  # the grid with a margin of 2: the disc is cut off at the grid's edge
        canvas[r:r + 5, c:c + 5] = disc
        want[k] = canvas[2:-2, 2:-2]
    _same(_distances(floor, ceiling, 2, True), want, 'a disc a row')
    _same(walls_ref.brute(floor, ceiling, 2, edge_open=True), want, 'a disc a row, the reference')


@pytest.mark.parametrize('radius', RADII)
def test_the_exact_disc_round_one_closed_cell(radius):
    rd.set_device(0)
    R = radius
    side, mid = 2 * R + 3, R + 1
    floor, ceiling = flood_ref.room(side, side)
    ceiling[mid, mid] = F(0.5)
    d = (np.arange(side) - mid).astype(np.int64)
    d2 = d[None, :] ** 2 + d[:, None] ** 2
    want = np.where(d2 <= R * R, d2, X).astype(np.uint16)
    assert want[mid, mid] == 0 and want[mid, mid - R] == want[mid, mid + R] == want[mid - R, mid] == want[mid + R, mid] == R * R
    assert want[mid, 0] == want[0, mid] == want[mid, -1] == want[-1, mid] == X and want[mid - R, mid - 1] == X  # R * R + 1
    assert (want[[0, -1]] == X).all() and (want[:, [0, -1]] == X).all()
    got = _distances(floor[None], ceiling[None], R, True)
    _same(got, want[None], ('disc', R))
    planes = _inflated(floor[None], ceiling[None], R, True)
    assert np.array_equal(np.isposinf(planes[0][0]), d2 <= R * R) and np.array_equal(np.isneginf(planes[1][0]), d2 <= R * R)
    assert (planes[0][0][d2 > R * R] == 0).all() and (planes[1][0][d2 > R * R] == 1).all()


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('radius', [1, 2, 32])
def test_blocking_cells_on_either_side_of_a_tile_s_edge(radius):
    """grids of the tile's size and one off it each way, and one of two tiles and a cell each way: closed cells on the last column
    and the last row of the first tile and on the first of the next, so that every distance within R of them crosses into a
    neighbouring tile; the whole output is compared, R cells into the neighbours and beyond"""
    rd.set_device(0)
    shapes = [(w, h) for w in (TX - 1, TX, TX + 1) for h in (TY - 1, TY, TY + 1)] + [(2 * TX + 1, 2 * TY + 1)]
    for w, h in shapes:
        floor, ceiling = flood_ref.room(w, h)
        cells = [(TX - 1, 3), (TX, h - 2), (TX - 1, TY - 1), (TX, TY), (5, TY - 1), (w - 3, TY), (TX - 1, TY), (2 * TX - 1, TY // 2), (TX + 7, 2 * TY),
                 (w - 1, 2), (2, h - 1)]  # and the grid's own last column and row, the tile's at the tile's size
        placed = [(c, r) for c, r in cells if 0 <= c < w and 0 <= r < h]
        assert len(set(placed)) >= (2 if w < TX or h < TY else 5)
        for c, r in placed:
            ceiling[r, c] = F(0.5)
        is_open = flood_ref.open_cells(floor, ceiling, 0.56)
        assert (~is_open).sum() == len(set(placed))
        for edge in (True, False):
            _all_three(floor[None], ceiling[None], walls_ref.exact_d2(is_open, edge)[None], radius, edge, ('tile edges', w, h))


# ---- random grids ----------------------------------------------------------------------------------------------------------------------

def _random_planes(rng, n, h, w, share):
    """planes of every kind of cell: open ones, some with a floor of -0.0; closed ones that are too low, doors (a finite floor with the
    ceiling on it), the void, NaNs with payloads in the floor or the ceiling, infinities"""
    floor = rng.choice(np.array([0.0, -0.0, 0.25, -1.5], F), (n, h, w))
    ceiling = (floor + rng.choice(np.array([0.6, 1.0, 7.0], F), (n, h, w))).astype(F)
    kind = np.where(rng.random((n, h, w)) < share, 0, rng.integers(1, 7, (n, h, w)))
    ceiling[kind == 1] = floor[kind == 1] + F(0.5)
    ceiling[kind == 2] = floor[kind == 2]
    floor[kind == 3], ceiling[kind == 3] = np.inf, -np.inf
    floor.view(np.uint32)[kind == 4] = 0x7FC00000 | rng.integers(1, 1 << 22, (kind == 4).sum()).astype(np.uint32)
    ceiling.view(np.uint32)[kind == 5] = 0xFFC00000 | rng.integers(1, 1 << 22, (kind == 5).sum()).astype(np.uint32)
    floor[kind == 6] = -np.inf
    return floor, ceiling, kind


@functools.lru_cache(maxsize=None)
def _random_grids(w, h):
    """(floor, ceiling, the definition's uncapped distances with the edge closed, with it open): computed once, left unchanged"""
    rng = np.random.default_rng(w * 1000 + h)
    floor, ceiling, kind = _random_planes(rng, ROWS, h, w, 0.93)
    floor[ROWS - 1], ceiling[ROWS - 1] = 0.0, 1.0  # one row with a single closed cell: FAR at every radius but the largest
    ceiling[ROWS - 1, h // 2, w // 3] = 0.5
    is_open = np.stack([flood_ref.open_cells(floor[p], ceiling[p], 0.56) for p in range(ROWS)])
    assert np.array_equal(is_open[:ROWS - 1], kind[:ROWS - 1] == 0) and all((kind == k).any() for k in range(7))
    assert (np.signbit(floor) & (floor == 0) & is_open).any()
    exact = [np.stack([walls_ref.exact_d2(is_open[p], edge) for p in range(ROWS)]) for edge in (False, True)]
    return floor, ceiling, exact[0], exact[1]


@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('shape', [(67, 35), (130, 19)], ids=['67x35', '130x19'])
def test_random_grids_against_the_definition(shape, radius):
    rd.set_device(0)
    floor, ceiling, closed_edge, open_edge = _random_grids(*shape)
    assert (open_edge > radius * radius).any() and (open_edge == radius * radius).any() and (closed_edge != open_edge).any()
    for edge, exact in ((False, closed_edge), (True, open_edge)):
        _all_three(floor, ceiling, exact, radius, edge, shape)


def test_the_longest_strips_and_a_side_too_long():
    rd.set_device(0)
    R = 32
    line = np.abs(np.arange(8192, dtype=np.int64) - 4096) ** 2
    for shape in ((1, 8192), (8192, 1)):
        floor, ceiling = np.zeros(shape, F), np.ones(shape, F)
        ceiling.reshape(-1)[4096] = F(0.5)
        want = np.where(line <= R * R, line, X).astype(np.uint16).reshape((1,) + shape)
        assert (want != X).sum() == 2 * R + 1
        _same(_distances(floor[None], ceiling[None], R, True), want, (shape, 'edge open'))
        want = np.minimum(want, 1).astype(np.uint16)  # the edge is next to every cell of a strip
        _same(_distances(floor[None], ceiling[None], R, False), want, (shape, 'edge closed'))
        got = _inflated(floor[None], ceiling[None], R, True, dist2=True)
        assert np.isposinf(got[0]).sum() == np.isneginf(got[1]).sum() == (line <= R * R).sum() == 2 * R + 1
    for shape in ((1, 1, 70000), (1, 70000, 1)):  # refused by the side limit, not by the number of cells
        assert 70000 < rd.flood_grid_max_cells()
        with pytest.raises(rd.RdoomError) as e:
            rd.wall_distances(torch.zeros(shape, device='cuda'), torch.ones(shape, device='cuda'), 1)
        assert e.value.status == -1 and 'a side' in str(e.value)


def test_a_grid_of_many_tiles_against_the_two_phase_form():
    rd.set_device(0)
    rng = np.random.default_rng(700)
    floor, ceiling, _ = _random_planes(rng, 1, 600, 700, 0.995)
    floor[0, 200:330, 300:450], ceiling[0, 200:330, 300:450] = 0.0, 1.0  # a hall wider than twice the largest radius
    assert (700 + TX - 1) // TX * ((600 + TY - 1) // TY) > 200
    for radius, edge in ((32, False), (32, True), (5, False)):
        want = walls_ref.capped(floor, ceiling, radius, edge_open=edge)
        assert (want == X).any() and (want != X).any() and want[0, 260, 370] == X
        planes = walls_ref.inflate(floor, ceiling, want, radius * radius)
        got = _inflated(floor, ceiling, radius, edge, dist2=True)
        for k, name in enumerate(('floor', 'ceiling')):
            _same(got[k], planes[k], (radius, edge, name))
        _same(got[2], want, (radius, edge))


# ---- the planes ------------------------------------------------------------------------------------------------------------------------

def test_the_planes_keep_their_words_and_an_output_on_an_input_is_refused():
    rd.set_device(0)
    f = np.array([[[0.0, -0.0, np.nan, 1.0, 0.25]]], F)
    g = np.array([[[1.0, 1.0, 1.0, 2.0, 0.25]]], F)  # a NaN floor, and a door: a finite floor with the ceiling on it
    f.view(np.uint32)[0, 0, 2] = 0x7FC12345  # the NaN's payload
    ft, gt = _dev(f), _dev(g)
    got = rd.inflate_grids(ft, gt, 0.19, 0.25, edge_open=True, dist2_out=True)  # close_d2 0: closed cells alone are touched
    assert _words(got[0]).tolist() == [[[0, 0x80000000, 0x7F800000, 0x3F800000, 0x7F800000]]]
    assert _words(got[1]).tolist() == [[[0x3F800000, 0x3F800000, 0xFF800000, 0x40000000, 0xFF800000]]]
    assert got[2].cpu().numpy().tolist() == [[[X, 1, 0, 1, 0]]]
    got = rd.inflate_grids(ft, gt, 1.0, 1.0, edge_open=True)
    assert _words(got[0]).tolist() == [[[0, 0x7F800000, 0x7F800000, 0x7F800000, 0x7F800000]]]
    assert _words(got[1]).tolist() == [[[0x3F800000] + [0xFF800000] * 4]]
    for kw in (dict(floor_out=ft), dict(ceiling_out=gt), dict(floor_out=gt), dict(ceiling_out=ft), dict(floor_out=ft.data_ptr())):
        with pytest.raises(rd.RdoomError) as e:
            rd.inflate_grids(ft, gt, 1.0, 1.0, **kw)
        assert e.value.status == -1 and 'overlaps' in str(e.value)
    assert _words(ft).tolist() == f.view(np.uint32).tolist() and _words(gt).tolist() == g.view(np.uint32).tolist()  # nothing was written
    with pytest.raises(ValueError):
        rd.inflate_grids(ft, gt, 4.1, 0.125)  # a radius of 33 cells
    with pytest.raises(rd.RdoomError):
        rd.wall_distances(ft, gt, 33)


# ---- corridors ---------------------------------------------------------------------------------------------------------------------------

def _split_room(gap_rows):
    """9 x 7, flat, a wall down column 4 with the rows of `gap_rows` left open"""
    floor, ceiling = flood_ref.room(9, 7)
    for r in range(7):
        if r not in gap_rows:
            ceiling[r, 4] = F(0.5)
    return floor[None], ceiling[None]


def _flooded(floor_t, ceiling_t, seed):
    dist, count = rd.flood_grids(floor_t, ceiling_t, _dev(np.array([seed], np.int32)), count_out=True)
    return dist.cpu().numpy().view(np.uint32)[0], int(count.cpu().numpy()[0])


def test_a_gap_one_cell_wide_is_shut_and_one_three_cells_wide_is_walked_down_its_middle():
    """a body of one cell's radius (close_d2 = 1) in a room split by a wall, the seed in the left half"""
    rd.set_device(0)
    seed = (1, 3)
    floor, ceiling = _split_room({3})
    plain, reached = _flooded(_dev(floor), _dev(ceiling), seed)
    assert reached == 9 * 7 - 6 and plain[3, 7] == 6 and plain[0, 8] == 10  # through the gap, to the far corner
    fi, ci = rd.inflate_grids(_dev(floor), _dev(ceiling), 1.0, 1.0)
    got, reached = _flooded(fi, ci, seed)
    want = [[U] * 9,
            [U, 2, 3, U, U, U, U, U, U],
            [U, 1, 2, U, U, U, U, U, U],
            [U, 0, 1, 2, U, U, U, U, U],  # (3, 3), in front of the gap, stays open: the wall's cells are a diagonal away
            [U, 1, 2, U, U, U, U, U, U],
            [U, 2, 3, U, U, U, U, U, U],
            [U] * 9]
    assert got.tolist() == want and reached == 11  # the eroded cells of the seed's side, and not one beyond the gap
    assert np.isposinf(fi.cpu().numpy()[0, 3, 4])  # the gap's own cell is shut: the wall is one cell from it on either side

    floor, ceiling = _split_room({2, 3, 4})
    fi, ci, d2 = rd.inflate_grids(_dev(floor), _dev(ceiling), 1.0, 1.0, dist2_out=True)
    got, reached = _flooded(fi, ci, seed)
    want = [[U] * 9,
            [U, 2, 3, U, U, U, 7, 8, U],
            [U, 1, 2, 3, U, 5, 6, 7, U],
            [U, 0, 1, 2, 3, 4, 5, 6, U],  # the gap's middle cell alone lets the body through
            [U, 1, 2, 3, U, 5, 6, 7, U],
            [U, 2, 3, U, U, U, 7, 8, U],
            [U] * 9]
    assert got.tolist() == want and reached == 27
    assert d2.cpu().numpy()[0].tolist() == [[1] * 4 + [0] + [1] * 4,
                                            [1, X, X, 1, 0, 1, X, X, 1],
                                            [1, X, X, X, 1, X, X, X, 1],
                                            [1, X, X, X, X, X, X, X, 1],
                                            [1, X, X, X, 1, X, X, X, 1],
                                            [1, X, X, 1, 0, 1, X, X, 1],
                                            [1] * 4 + [0] + [1] * 4]
    plain, reached = _flooded(_dev(floor), _dev(ceiling), seed)
    assert reached == 9 * 7 - 4 and plain[2, 4] == 4  # un-inflated, the gap's other cells are walked too


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

E2E_STEP = 0.32  # the synthetic E1M1 joins most of its sectors by steps of 0.32
BODY = 0.19      # World.step's body


@functools.lru_cache(maxsize=None)
def _wad():
    return rd.Wad(ensure_wad(), META_PATH)


def test_planes_inflation_and_a_flood_towards_the_start_of_e1m1_end_to_end():
    rd.set_device(0)
    index, cell, n = 0, 0.125, 4
    host = _wad().build_world(index, device=False)
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    at = goal_ref.level_sectors(tables, g, cell)
    pos, yaw = _wad().build_level(index).start()
    st = rd.player_states(np.repeat(np.asarray(pos, F)[None], n, 0), np.full(n, yaw, F))
    off = sector_ref.random_offsets(np.random.default_rng(25), n, host.game_objects)
    off[[0, 2]] = 0  # rows 0 and 2: all at rest
    _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    seeds = goal_ref.cells(g, cell, st)
    assert rd.wall_close_d2(BODY, cell) == 2
    fi, ci, d2 = walls_ref.inflate_grids(floor, ceiling, BODY, cell)
    want = goal_ref.flood_grids(fi, ci, seeds, True, max_step=E2E_STEP)
    plain = goal_ref.flood_grids(floor, ceiling, seeds, True, max_step=E2E_STEP)
    # on the reference alone: the start's cell stays open, inflation closes open cells in every row, and the inflated flood reaches
    # more than the seed and strictly less than the plain one
    is_open = np.stack([flood_ref.open_cells(floor[p], ceiling[p], 0.56) for p in range(n)])
    still = np.stack([flood_ref.open_cells(fi[p], ci[p], 0.56) for p in range(n)])
    for p in range(n):
        c, r = seeds[p]
        assert still[p, r, c] and d2[p, r, c] > 2, (p, d2[p, r, c])
        assert (is_open[p] & ~still[p]).any() and not (still[p] & ~is_open[p]).any()
        assert 1 < want[1][p] < plain[1][p], (want[1], plain[1])
    assert len({want[0][p].tobytes() for p in range(n)}) > 1  # the rows' doors and lifts count

    world = _wad().build_world(index)
    f_t, c_t = world.draw_area_planes(cell, offsets=_dev(off), floor=True, ceiling=True)
    fi_t, ci_t, d2_t = rd.inflate_grids(f_t, c_t, BODY, cell, dist2_out=True)
    _same(d2_t.cpu().numpy(), d2, 'distances')
    _same(fi_t.cpu().numpy(), fi, 'floor')
    _same(ci_t.cpu().numpy(), ci, 'ceiling')
    dist, count = rd.flood_grids(fi_t, ci_t, _dev(seeds), towards=True, max_step=E2E_STEP, count_out=True)
    got = dist.cpu().numpy().view(np.uint32)
    _same(got, want[0], 'flood')
    assert np.array_equal(count.cpu().numpy().view(np.uint32), want[1])
    # on the device's output: what the body reaches the point reaches, no sooner; and it never stands within its radius of a wall
    dist, _ = rd.flood_grids(f_t, c_t, _dev(seeds), towards=True, max_step=E2E_STEP, count_out=True)
    point = dist.cpu().numpy().view(np.uint32)
    reached = got != U
    assert (point[reached] != U).all() and (point[reached] <= got[reached]).all() and (point[reached] < got[reached]).any()
    assert (d2_t.cpu().numpy()[reached] > 2).all()


def test_the_sector_maps_of_eight_players_with_an_open_edge_through_flood_maps():
    """E1M2 is some five units across: at 0.03 a pixel the 160 x 120 window is smaller than the level, so open floor runs into the
    window's edge, which is unknown and not a wall.  The body's close_d2 is 40 there, the launch's radius 7."""
    rd.set_device(0)
    index, n, w, h, scale = 1, 8, 160, 120, 0.03
    st, on_map = sector_ref.players(_wad(), index, n, np.random.default_rng(8), outside=0, nan=0)
    tables = sector_ref.Tables(_wad().build_world(index, device=False))
    _, floor, ceiling = sector_ref.draw(tables, st, width=w, height=h, scale=scale)
    assert rd.wall_close_d2(BODY, scale) == 40 and w * h <= rd.flood_max_cells()
    fi, ci, d2 = walls_ref.inflate_grids(floor, ceiling, BODY, scale, edge_open=True)
    closed_edge = walls_ref.inflate_grids(floor, ceiling, BODY, scale)
    want, plain = flood_ref.flood_maps(fi, ci), flood_ref.flood_maps(floor, ceiling)
    # on the reference: the flag counts, every player walks, and the body reaches less than the point
    assert (closed_edge[2] != d2).sum() > 1000 and (want[1] > 1000).all() and (want[1] < plain[1]).all(), (want[1], plain[1])
    world = _wad().build_world(index)
    states = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()
    f_t, c_t = world.draw_sector_maps(states, w, h, scale, floor=True, ceiling=True)
    _same(f_t.cpu().numpy(), floor, 'the map\'s floor')
    _same(c_t.cpu().numpy(), ceiling, 'the map\'s ceiling')
    fi_t, ci_t, d2_t = rd.inflate_grids(f_t, c_t, BODY, scale, edge_open=True, dist2_out=True)
    _same(d2_t.cpu().numpy(), d2, 'distances')
    _same(fi_t.cpu().numpy(), fi, 'floor')
    _same(ci_t.cpu().numpy(), ci, 'ceiling')
    dist, count = rd.flood_maps(fi_t, ci_t, count_out=True)
    _same(dist.cpu().numpy(), want[0], 'flood_maps')
    assert np.array_equal(count.cpu().numpy().view(np.uint32), want[1])
    _same(_distances(floor, ceiling, 16, True), walls_ref.capped(floor, ceiling, 16, edge_open=True), 'a map channel of radius 16')


# ---- streams, tensors, pointers, a graph -----------------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_walls_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_walls_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
