"""The goal distance on the host, with no GPU: the surface -- header, exported symbols, the Python names, the library's constant --
every argument error of the three groups of entry points on host-only handles and NULL device pointers, World.area_plane_shape
against the grid calls and a numpy evaluation of the grid formulas, the reference (tests/goal_ref.py) pinned on flood_ref's hand-made
grids with the TOWARDS distances written out by hand, and the planes' reference pinned on E1M2 and E1M1 by a property that
needs no library kernel: a cell whose four corners lie in one sector carries that sector."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import area_ref
import flood_ref
import goal_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ROOT, ensure_wad

F = np.float32
U = goal_ref.UNREACHED
BAD = -1  # RDOOM_BAD_ARG
SYMBOLS = ['rdoom_world_draw_area_planes', 'rdoom_worldset_draw_area_planes', 'rdoom_flood_grid_max_cells', 'rdoom_flood_grids',
           'rdoom_world_area_cells', 'rdoom_worldset_area_cells']
CASES = flood_ref.hand_cases()
BY_NAME = {c['name']: c for c in CASES}


# ---- the surface -------------------------------------------------------------------------------------------------------------------

def test_the_library_and_the_package_export_the_goal_distance():
    L = ctypes.CDLL(rd.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name) and name in rd.API_SYMBOLS and getattr(rd.lib(), name).restype is ctypes.c_int32, name
    assert rd.flood_grid_max_cells() == 1 << 22
    assert rd.FLOOD_GRID_UNREACHED == 0xFFFFFFFF == U and rd.FLOOD_TOWARDS == 1
    assert rd.lib().rdoom_flood_grid_max_cells(None) == BAD and b'null' in rd.lib().rdoom_last_error()
    sig = inspect.signature(rd.flood_grids)
    assert list(sig.parameters) == ['floor', 'ceiling', 'seeds', 'towards', 'max_step', 'max_drop', 'clearance', 'dist_out', 'count_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['max_step'], d['max_drop'], d['clearance'], d['towards'], d['seeds']) == (0.24, float('inf'), 0.56, False, None)
    assert list(inspect.signature(rd.World.draw_area_planes).parameters) == ['self', 'cell', 'n', 'offsets', 'area', 'sector_out', 'floor', 'ceiling',
                                                                             'stream']
    assert list(inspect.signature(rd.WorldSet.draw_area_planes).parameters) == ['self', 'levels', 'cell', 'n', 'offsets', 'area', 'sector_out',
                                                                                'floor', 'ceiling', 'stream']
    assert list(inspect.signature(rd.World.area_cells).parameters) == ['self', 'states', 'cell', 'out', 'stream']
    assert list(inspect.signature(rd.WorldSet.area_cells).parameters) == ['self', 'states', 'levels', 'cell', 'out', 'stream']
    assert callable(rd.World.area_plane_shape) and callable(rd.WorldSet.area_plane_shape)


def test_the_header_declares_the_goal_distance():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- goal distance:' in text and '(DESIGN section 23)' in text
    assert '#define RDOOM_FLOOD_GRID_UNREACHED 0xFFFFFFFFu' in text and '#define RDOOM_FLOOD_TOWARDS 1u' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)

    def arguments(name):
        proto = re.search(r'rdoom_status %s\((.*?)\);' % name, code, flags=re.S).group(1)
        return [' '.join(a.split()) for a in proto.split(',')]

    planes = ['uint32_t n', 'const float *d_object_offsets', 'uint32_t n_objects', 'float cell', 'uint32_t width', 'uint32_t height',
              'const uint32_t *d_area', 'uint32_t area_stride', 'uint16_t *d_sector_out', 'float *d_floor_out', 'float *d_ceiling_out', 'void *stream']
    assert arguments('rdoom_world_draw_area_planes') == ['const rdoom_world *world'] + planes
    assert arguments('rdoom_worldset_draw_area_planes') == ['const rdoom_worldset *set', 'const uint32_t *d_levels'] + planes
    assert arguments('rdoom_flood_grids') == [
        'const float *d_floor', 'const float *d_ceiling', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'const int32_t *d_seeds',
        'const rdoom_flood_params *params', 'uint32_t *d_dist_out', 'uint32_t *d_count_out', 'void *stream']
    assert arguments('rdoom_flood_grid_max_cells') == ['uint32_t *cells_out']
    assert arguments('rdoom_world_area_cells') == ['const rdoom_world *world', 'const rdoom_player_state *d_states', 'uint32_t n', 'float cell',
                                                   'int32_t *d_cells_out', 'void *stream']
    assert arguments('rdoom_worldset_area_cells') == ['const rdoom_worldset *set', 'const rdoom_player_state *d_states', 'const uint32_t *d_levels',
                                                      'uint32_t n', 'float cell', 'int32_t *d_cells_out', 'void *stream']
    # "Open", "Moves" and "Seeds" are the flood's paragraphs, word for word: each stands in the header twice
    flood = text[text.index('/* ---- flood:'):text.index('/* ---- spawn:')]
    for head, following in ((' * Open.', ' * Moves.'), (' * Moves.', ' * Seeds.'), (' * Seeds.', ' * d_dist_out')):
        paragraph = flood[flood.index(head):flood.index(following)]
        assert len(paragraph) > 150 and text.count(paragraph) == 2, head
    for words in ('x = ((float)(ix0 + (int32_t)ix) + 0.5f) * cell', 'with 0xFFFF widened to 0xFFFFFFFF', 'a wall thinner than a cell',
                  'followed backwards from the seed', '2^22 (2048 x 2048)', 'n == 0 queues nothing', 'captured into a graph'):
        assert words in text, words


# ---- the argument checks -----------------------------------------------------------------------------------------------------------

def _fails(call, word, **kw):
    L = rd.lib()
    assert call(**kw) == BAD, kw
    assert word in L.rdoom_last_error().decode(), (word, kw, L.rdoom_last_error())


def test_the_planes_and_the_cells_check_their_arguments_on_host_only_handles():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(1, device=False), wad.build_world_set([1, 0], device=False)  # E1M2, and E1M2 with E1M1
    cell = 0.25
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks, the last of them the device check
    f = ctypes.c_float
    shape = {world: world.area_plane_shape(cell), ws: ws.area_plane_shape(cell)}
    words = {world: world.area_words(cell), ws: ws.area_words(cell)}
    assert shape[ws][0] > shape[world][0] and shape[ws][1] > shape[world][1] and world.game_objects >= 1

    def draw(h=world, n=4, off=None, no=0, cell=cell, w=None, ht=None, area=None, stride=0, sec=fake, flo=None, cei=None, lv=fake):
        hp = h._h if h is not None else None
        w, ht = shape[h][1] if w is None else w, shape[h][0] if ht is None else ht
        if h is ws:
            return L.rdoom_worldset_draw_area_planes(hp, lv, n, off, no, f(cell), w, ht, area, stride, sec, flo, cei, None)
        return L.rdoom_world_draw_area_planes(hp, n, off, no, f(cell), w, ht, area, stride, sec, flo, cei, None)

    def cells(h=world, st=fake, n=4, cell=cell, out=fake, lv=fake):
        hp = h._h if h is not None else None
        if h is ws:
            return L.rdoom_worldset_area_cells(hp, st, lv, n, f(cell), out, None)
        return L.rdoom_world_area_cells(hp, st, n, f(cell), out, None)

    inf, nan = float('inf'), float('nan')
    for h, noun in ((world, 'world'), (ws, 'world set')):
        gh, gw = shape[h]
        _fails(draw, 'no output plane', h=h, sec=None)
        for c in (0.0, -0.25, inf, nan):
            _fails(draw, 'cell', h=h, cell=c)
            _fails(cells, 'cell', h=h, cell=c)
        for c in (1e-4, 1e-30):  # E1M2 is some ten units wide: a hundred thousand cells a side; a bound of 2^30 cells or more
            _fails(draw, 'limits', h=h, cell=c, w=8192, ht=8192)
            _fails(cells, 'limits', h=h, cell=c)
        _fails(draw, 'planes of', h=h, w=gw - 1)
        _fails(draw, 'planes of', h=h, ht=gh - 1)
        _fails(draw, noun + "'s grid", h=h, w=0)  # the handle's noun is in the text
        _fails(draw, 'planes of', h=h, w=8193)
        _fails(draw, 'planes of', h=h, ht=0xFFFFFFFF)
        _fails(draw, 'too many', h=h, n=1 << 13, w=8192, ht=8192)  # 2^13 rows of 2^18 workgroups
        _fails(draw, 'too many', h=h, n=0xFFFFFFFF)
        _fails(draw, 'n_objects', h=h, off=fake, no=0)
        _fails(draw, 'stride', h=h, area=fake, stride=words[h] - 1)
        _fails(draw, 'stride', h=h, area=fake, stride=0)
        _fails(draw, 'HOST_ONLY', h=h)  # all else in order: the handle has no device copy
        _fails(draw, 'HOST_ONLY', h=h, w=8192, ht=8192, area=fake, stride=words[h], off=fake, no=64, sec=None, flo=fake, cei=fake)
        _fails(draw, 'HOST_ONLY', h=h, n=0, sec=None)
        _fails(cells, 'null', h=h, st=None)
        _fails(cells, 'null', h=h, out=None)
        _fails(cells, 'HOST_ONLY', h=h)
        _fails(cells, 'HOST_ONLY', h=h, n=0, st=None, out=None)
    _fails(draw, 'planes of', h=ws, w=shape[world][1], ht=shape[world][0])  # enough for E1M2, not for every level of the set
    _fails(draw, 'stride', h=ws, area=fake, stride=words[world])
    _fails(draw, 'null levels', h=ws, lv=None)
    _fails(cells, 'null levels', h=ws, lv=None)
    assert draw(h=ws, lv=None, n=0) == BAD and b'HOST_ONLY' in L.rdoom_last_error()  # n == 0 needs no levels
    assert L.rdoom_world_draw_area_planes(None, 4, None, 0, f(cell), 64, 64, None, 0, fake, None, None, None) == BAD and b'null' in L.rdoom_last_error()
    assert L.rdoom_worldset_draw_area_planes(None, fake, 4, None, 0, f(cell), 64, 64, None, 0, fake, None, None, None) == BAD
    assert b'null' in L.rdoom_last_error()
    assert L.rdoom_world_area_cells(None, fake, 4, f(cell), fake, None) == BAD and b'null' in L.rdoom_last_error()
    assert L.rdoom_worldset_area_cells(None, fake, fake, 4, f(cell), fake, None) == BAD and b'null' in L.rdoom_last_error()


def test_the_flood_of_grids_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks or queues nothing
    cells = rd.flood_grid_max_cells()
    inf, nan = float('inf'), float('nan')

    def call(floor=fake, ceil=fake, n=4, w=77, h=53, seeds=None, params=(0.24, inf, 0.56, 0), dist=fake, count=None):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_flood_grids(floor, ceil, n, w, h, seeds, p, dist, count, None)

    _fails(call, 'null params', params=None)
    _fails(call, 'null', floor=None)
    _fails(call, 'null', ceil=None)
    _fails(call, 'null', dist=None)
    _fails(call, '0 x 53', w=0)
    _fails(call, '77 x 0', h=0)
    _fails(call, 'a side', w=8193, h=1)
    _fails(call, 'a side', w=1, h=70000)
    _fails(call, 'a side', w=0xFFFFFFFF, h=0xFFFFFFFF)
    _fails(call, 'too many', w=2048, h=2049)
    _fails(call, 'too many', w=8192, h=513)
    _fails(call, 'too many', w=8192, h=8192)
    for flags in (2, 3, 0x80000000, 0x80000001):
        _fails(call, 'flags', params=(0.24, inf, 0.56, flags))
    for k, name in enumerate(('max_step', 'max_drop', 'clearance')):
        for bad in (nan, -1.0, -inf, -1e-30):
            params = [0.24, inf, 0.56, 1]
            params[k] = bad
            _fails(call, name, params=tuple(params))
    # what is allowed: either direction, zeros, an infinite drop or step, the largest grids, and n == 0 with nothing else valid
    assert call(n=0, floor=None, ceil=None, dist=None) == 0
    assert call(n=0, params=(0.0, 0.0, 0.0, 0)) == 0 and call(n=0, params=(inf, inf, inf, rd.FLOOD_TOWARDS)) == 0
    assert call(n=0, w=2048, h=2048) == 0 and call(n=0, w=8192, h=512) == 0 and call(n=0, w=512, h=8192) == 0 and call(n=0, w=1, h=1) == 0
    assert cells == 2048 * 2048
    _fails(call, 'null params', n=0, params=None)  # n == 0 is not a way round the checks
    _fails(call, 'too many', n=0, w=2049, h=2048)
    # rdoom_flood_maps is untouched: its flags stay "must be 0"
    assert L.rdoom_flood_maps(fake, fake, 4, 77, 53, None, ctypes.byref(rd.FloodParams(0.24, inf, 0.56, 1)), fake, None, None) == BAD
    assert b'must be 0' in L.rdoom_last_error()


# ---- the shape of the planes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cell', [0.25, 0.0625])
def test_the_shape_of_the_planes_is_the_grid_of_the_level(cell):
    wad = rd.Wad(ensure_wad(), META_PATH)
    grids = []
    for index in (0, 1, 7):  # E1M1, E1M2, E1M8
        world = wad.build_world(index, device=False)
        g = world.area_grid(cell)
        assert g == area_ref.grid_numpy(world.map_lines(), cell)
        assert world.area_plane_shape(cell) == (g.gh, g.gw)
        grids.append(g)
    ws = wad.build_world_set([0, 1, 7], device=False)
    assert [ws.area_grid(s, cell) for s in range(3)] == grids
    assert ws.area_plane_shape(cell) == (max(g.gh for g in grids), max(g.gw for g in grids))
    assert len({g.gh for g in grids}) > 1 and len({g.gw for g in grids}) > 1  # the largest is not every level's


# ---- the reference of the flood ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_reference_forwards_on_grids_written_out_by_hand(case):
    got = goal_ref.flood(case['floor'], case['ceiling'], case['seed'], **case['kw'])
    assert got.dtype == np.uint32 and got.shape == case['floor'].shape
    assert np.array_equal(got, goal_ref.widen(case['want'])), (case['name'], got.tolist())
    assert np.array_equal(got, goal_ref.widen(flood_ref.flood(case['floor'], case['ceiling'], case['seed'], **case['kw'])))


def test_the_reference_towards_the_seed_on_the_ledge_written_out_by_hand():
    """columns 0-2 are a plateau at 0.48, columns 3-6 lie at 0: the plateau is dropped from and not climbed"""
    ledge, stair = BY_NAME['ledge from the top'], BY_NAME['ledge with a stair from below']
    f, g = ledge['floor'], ledge['ceiling']

    def towards(floor, seed, **kw):
        return goal_ref.flood(floor, g, seed, towards=True, **kw).tolist()

    # towards a seed on the low side: the plateau's cells reach it by dropping, where the forward flood has U
    assert towards(f, (6, 0)) == [[6 - c + r for c in range(7)] for r in range(5)]
    assert (BY_NAME['ledge from below']['want'][:, :3] == flood_ref.UNREACHED).all()
    # towards a seed on the plateau: the low side cannot climb to it, where the forward flood is finite
    assert towards(f, (0, 0)) == [[c + r if c < 3 else U for c in range(7)] for r in range(5)]
    assert (ledge['want'] != flood_ref.UNREACHED).all()
    # the stair at column 3 of the last row (0.24): towards the low side nothing changes -- every drop is still allowed --
    assert towards(stair['floor'], (6, 0)) == [[6 - c + r for c in range(7)] for r in range(5)]
    # and towards the plateau's corner the low side climbs there and there only: to the stair, one move up, then 2 + 4 on the plateau
    want = [[c + r if c < 3 else (c - 3) + (4 - r) + 1 + (2 + 4) for c in range(7)] for r in range(5)]
    assert want[4][3] == 7 and want[0][6] == 14
    assert towards(stair['floor'], (0, 0)) == want
    # the mirror image of the forward case: from the low corner to the plateau's is 14 moves, the other way 6
    assert stair['want'][0, 0] == 14 and towards(stair['floor'], (6, 0))[0][0] == 6
    # a drop limited to 0.3: the ledge is crossed in neither direction, from either side
    assert towards(f, (6, 0), max_drop=0.3) == [[U, U, U] + [6 - c + r for c in range(3, 7)] for r in range(5)]
    assert towards(f, (0, 0), max_drop=0.3) == [[c + r if c < 3 else U for c in range(7)] for r in range(5)]
    assert towards(f, (0, 0), max_drop=0.3) == goal_ref.flood(f, g, (0, 0), max_drop=0.3).tolist()
    # with the stair and that limit the plateau is left over the stair only: 0.48 -> 0.24 -> 0
    want = [[(2 - c) + (4 - r) + 1 + (6 - 3) + 4 if c < 3 else 6 - c + r for c in range(7)] for r in range(5)]
    assert towards(stair['floor'], (6, 0), max_drop=0.3) == want


def test_the_reference_towards_the_seed_equals_forwards_where_every_move_has_its_reverse():
    for name in ('1x1', '1x9 from the left', '9x1 default seed', 'cells that are not numbers', 'a closed seed', 'clearance missed by an ulp',
                 'shared opening too low', 'a seed outside the grid 0'):
        c = BY_NAME[name]
        assert np.array_equal(goal_ref.flood(c['floor'], c['ceiling'], c['seed'], towards=True, **c['kw']), goal_ref.widen(c['want'])), name
    f, g = flood_ref.room(23, 17)
    for seed in ((0, 0), (11, 8), (22, 16)):
        want = np.abs(np.arange(23) - seed[0])[None, :] + np.abs(np.arange(17) - seed[1])[:, None]
        assert np.array_equal(goal_ref.flood(f, g, seed, towards=True), want) and np.array_equal(goal_ref.flood(f, g, seed), want)
    # and where they do not, the two are transposes of one relation: d_towards(seed a, cell b) == d_forwards(seed b, cell a)
    c = BY_NAME['ledge with a stair from below']
    cells = [(col, row) for row in range(5) for col in range(7)]
    fwd = {a: goal_ref.flood(c['floor'], c['ceiling'], a) for a in cells}
    for a in cells:
        back = goal_ref.flood(c['floor'], c['ceiling'], a, towards=True)
        assert all(back[b[1], b[0]] == fwd[b][a[1], a[0]] for b in cells), a
    # the staircase is walked one way only: towards its own seed nothing but the seed arrives, towards the far corner the whole path
    f, g, seed = flood_ref.staircase(40, 30)
    path = flood_ref.open_cells(f, g, 0.56)
    assert (goal_ref.flood(f, g, seed, towards=True) != U).sum() == 1
    assert (goal_ref.flood(f, g, (0, 0), towards=True) != U).sum() == path.sum() == 69
    assert np.array_equal(goal_ref.flood(f, g, (0, 0), towards=True) != U, path)


# ---- the reference of the planes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('index,cell', [(1, 0.25), (1, 0.125), (0, 0.25)], ids=['E1M2 0.25', 'E1M2 0.125', 'E1M1 0.25'])
def test_a_cell_whose_four_corners_lie_in_one_sector_carries_that_sector(index, cell):
    """the planes' reference without the library's kernels: sector_at at the centres against sector_at at the corners.  (The
    synthetic E1M2 is two sectors in some twenty cells a side at 0.25; E1M1 is the same property over more than a hundred sectors.)"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(index, device=False)
    tables, g = sector_ref.Tables(world), world.area_grid(cell)
    sector, floor, ceiling = goal_ref.planes(tables, g, cell, 1)
    assert sector.shape == (1, g.gh, g.gw) and sector.dtype == np.uint16 and floor.dtype == ceiling.dtype == F
    # the corners of cell (ix, iz): the grid lines ix0 + ix and ix0 + ix + 1, by the contract's cell bounds
    x = (np.arange(g.gw + 1, dtype=np.int32) + np.int32(g.ix0)).astype(F) * F(cell)
    z = (np.arange(g.gh + 1, dtype=np.int32) + np.int32(g.iz0)).astype(F) * F(cell)
    pts = np.stack(np.broadcast_arrays(x[None, :], z[:, None]), 2).reshape(-1, 2)
    at = sector_ref.sector_at(tables, pts).reshape(g.gh + 1, g.gw + 1)
    same = (at[:-1, :-1] == at[:-1, 1:]) & (at[:-1, :-1] == at[1:, :-1]) & (at[:-1, :-1] == at[1:, 1:]) & (at[:-1, :-1] != sector_ref.NONE)
    inside = sector[0] != sector_ref.NONE16
    # not vacuous: most cells inside the level are such cells, and most of its sectors are carried by one
    assert 2 * same.sum() > inside.sum() > 100 and 2 * len(np.unique(at[:-1, :-1][same])) > len(tables.sectors)
    assert np.array_equal(sector[0][same], at[:-1, :-1][same].astype(np.uint16))
    # the heights are the table's, at rest; the void and the margin are none
    assert np.array_equal(floor[0][inside], tables.sectors['floor'][sector[0][inside]])
    assert np.array_equal(ceiling[0][inside], tables.sectors['ceiling'][sector[0][inside]])
    assert np.isposinf(floor[0][~inside]).all() and np.isneginf(ceiling[0][~inside]).all() and (~inside).sum() > 100
    assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any()
    # padding and a slot outside a set are none
    padded = goal_ref.planes([tables, tables], [g, g], cell, 2, levels=[1, 2], shape=(g.gh + 3, g.gw + 5))
    assert np.array_equal(padded[0][0, :g.gh, :g.gw], sector[0]) and (padded[0][0, g.gh:] == sector_ref.NONE16).all()
    assert (padded[0][0, :, g.gw:] == sector_ref.NONE16).all() and (padded[0][1] == sector_ref.NONE16).all() and np.isposinf(padded[1][1]).all()
    if index != 0:
        return
    # an offset row moves the sectors of its object, and those alone (E1M1 has doors and lifts)
    ids = tables.sectors['ceiling_id'][sector[0][inside]]
    moved = int(np.bincount(ids[ids != 0]).argmax())
    off = np.zeros((1, world.game_objects, 3), F)
    off[0, moved, 1] = F(0.72)
    _, same_floor, raised = goal_ref.planes(tables, g, cell, 1, offsets=off)
    changed = raised[0] != ceiling[0]
    assert moved != 0 and changed.any() and (tables.sectors['ceiling_id'][sector[0][changed]] == moved).all()
    assert np.array_equal(raised[0][changed], ceiling[0][changed] + F(0.72))
    floor_too = tables.sectors['floor_id'][np.where(inside, sector[0], 0)] == moved
    assert np.array_equal(same_floor[0][~(floor_too & inside)], floor[0][~(floor_too & inside)])
    # a mask of all ones shows everything, a mask of none nothing, and a WALL bit hides a FREE cell
    ones = np.full((1, 2, g.words), 0xFFFFFFFF, np.uint32)
    ones[:, 1] = 0
    assert np.array_equal(goal_ref.planes(tables, g, cell, 1, area=ones)[0], sector)
    assert (goal_ref.planes(tables, g, cell, 1, area=np.zeros_like(ones))[0] == sector_ref.NONE16).all()
    iz, ix = np.argwhere(inside)[len(np.argwhere(inside)) // 2]
    ones[0, 1, iz * g.pitch + ix // 32] = np.uint32(1) << np.uint32(ix % 32)
    hidden = goal_ref.planes(tables, g, cell, 1, area=ones)[0]
    assert hidden[0, iz, ix] == sector_ref.NONE16 and (hidden != sector).sum() == 1


def test_the_reference_of_the_cells_is_the_grid_s_own_arithmetic():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0, device=False)
    for cell in (0.25, 0.0625):
        g = world.area_grid(cell)
        x, z = goal_ref.centres(g, cell)
        st = rd.player_states(np.stack([x[[0, 5, g.gw - 1, 3]], np.zeros(4, F), z[[0, 7, g.gh - 1, 2]]], 1), np.zeros(4, F))
        assert goal_ref.cells(g, cell, st).tolist() == [[0, 0], [5, 7], [g.gw - 1, g.gh - 1], [3, 2]]  # a centre lies in its cell
        st['pos'][0, 0] -= F(cell)
        st['pos'][1, 2] = np.nan
        st['pos'][2, 2] += F(cell)
        st['pos'][3, 0] = np.inf
        assert goal_ref.cells(g, cell, st).tolist() == [[-1, -1]] * 4
        assert goal_ref.cells([g, g], cell, st[:2], levels=[2, 0xFFFFFFFF]).tolist() == [[-1, -1]] * 2
