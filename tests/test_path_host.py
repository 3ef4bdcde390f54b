"""Waypoints and frontiers on the host, with no GPU: the surface -- header, exported symbols, the Python names -- every argument error
of both groups of entry points on host-only handles and device pointers that are never followed, and the reference
(tests/path_ref.py) pinned by hand: walks written out cell by cell on flood_ref's ledge, on a flat room where the neighbour order
shows, and on a grid where the distances alone would lead into the foot of a ledge; the walk's properties on every hand-made grid;
a field paired with planes it was not flooded from; and the frontier of a 9 x 6 area whose bits are written out."""
import ctypes
import inspect
import os
import re

import numpy as np

import flood_ref
import goal_ref
import path_ref
import rust_doom_amd as rd
from util import META_PATH, ROOT, ensure_wad

F = np.float32
U = path_ref.UNREACHED
BAD = -1  # RDOOM_BAD_ARG
SYMBOLS = ['rdoom_flood_descend', 'rdoom_world_area_frontiers', 'rdoom_worldset_area_frontiers']
CASES = flood_ref.hand_cases()
BY_NAME = {c['name']: c for c in CASES}


# ---- the surface -------------------------------------------------------------------------------------------------------------------

def test_the_library_and_the_package_export_waypoints_and_frontiers():
    L = ctypes.CDLL(rd.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name) and name in rd.API_SYMBOLS and getattr(rd.lib(), name).restype is ctypes.c_int32, name
    sig = inspect.signature(rd.descend_grids)
    assert list(sig.parameters) == ['floor', 'ceiling', 'dist', 'starts', 'towards', 'max_moves', 'stop_dist', 'max_step', 'max_drop', 'clearance',
                                    'cells_out', 'moves_out', 'path_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['towards'], d['max_moves'], d['stop_dist'], d['max_step'], d['max_drop'], d['clearance']) == (False, None, 0, 0.24, float('inf'), 0.56)
    flood = {k: p.default for k, p in inspect.signature(rd.flood_grids).parameters.items()}
    assert all(d[k] == flood[k] for k in ('max_step', 'max_drop', 'clearance'))  # the same params give the same moves
    outs = ['cell_out', 'dist_out', 'count_out', 'mask_out', 'stream']
    assert list(inspect.signature(rd.World.area_frontiers).parameters) == ['self', 'area', 'dist', 'cell'] + outs
    assert list(inspect.signature(rd.WorldSet.area_frontiers).parameters) == ['self', 'levels', 'area', 'dist', 'cell'] + outs


def test_the_header_declares_waypoints_and_frontiers():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- waypoints and frontiers:' in text and '(DESIGN section 24)' in text
    assert text.index('/* ---- goal distance:') < text.index('/* ---- waypoints and frontiers:')
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)

    def arguments(name):
        proto = re.search(r'rdoom_status %s\((.*?)\);' % name, code, flags=re.S).group(1)
        return [' '.join(a.split()) for a in proto.split(',')]

    assert arguments('rdoom_flood_descend') == [
        'const float *d_floor', 'const float *d_ceiling', 'const uint32_t *d_dist', 'uint32_t n', 'uint32_t width', 'uint32_t height',
        'const int32_t *d_starts', 'const rdoom_flood_params *params', 'uint32_t max_moves', 'uint32_t stop_dist', 'int32_t *d_cells_out',
        'uint32_t *d_moves_out', 'int32_t *d_path_out', 'uint32_t path_len', 'void *stream']
    front = ['uint32_t n', 'float cell', 'uint32_t width', 'uint32_t height', 'const uint32_t *d_area', 'uint32_t area_stride', 'const uint32_t *d_dist',
             'int32_t *d_cell_out', 'uint32_t *d_dist_out', 'uint32_t *d_count_out', 'uint8_t *d_mask_out', 'void *stream']
    assert arguments('rdoom_world_area_frontiers') == ['const rdoom_world *world'] + front
    assert arguments('rdoom_worldset_area_frontiers') == ['const rdoom_worldset *set', 'const uint32_t *d_levels'] + front
    block = text[text.index('/* ---- waypoints and frontiers:'):]
    for words in ('(column - 1, column + 1, row - 1, row + 1)', 'D(b) == D(a) - 1', 'the move from b to a', 'every entry is written',
                  'ties to the smallest iz, then the smallest ix', 'are not neighbours', 'every byte written', 'above\n * 2^22',
                  'n == 0 queues nothing', 'captured into a graph'):
        assert words in block, words


# ---- the argument checks -----------------------------------------------------------------------------------------------------------

def _fails(call, word, **kw):
    L = rd.lib()
    assert call(**kw) == BAD, kw
    assert word in L.rdoom_last_error().decode(), (word, kw, L.rdoom_last_error())


def test_the_walk_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks or queues nothing
    inf, nan = float('inf'), float('nan')
    u = ctypes.c_uint32

    def call(floor=fake, ceil=fake, dist=fake, n=4, w=77, h=53, starts=fake, params=(0.24, inf, 0.56, 0), max_moves=8, stop=0, cells=fake, moves=fake,
             path=None, path_len=0):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_flood_descend(floor, ceil, dist, n, w, h, starts, p, u(max_moves), u(stop), cells, moves, path, u(path_len), None)

    _fails(call, 'null params', params=None)
    for name in ('floor', 'ceil', 'dist', 'starts', 'cells', 'moves'):
        _fails(call, 'null', **{name: None})
    _fails(call, '0 x 53', w=0)
    _fails(call, '77 x 0', h=0)
    _fails(call, 'a side', w=8193, h=1)
    _fails(call, 'a side', w=0xFFFFFFFF, h=0xFFFFFFFF)
    _fails(call, 'too many', w=2048, h=2049)
    _fails(call, 'too many', w=8192, h=513)
    for flags in (2, 3, 0x80000000, 0x80000001):
        _fails(call, 'flags', params=(0.24, inf, 0.56, flags))
    for k, name in enumerate(('max_step', 'max_drop', 'clearance')):
        for bad in (nan, -1.0, -inf, -1e-30):
            params = [0.24, inf, 0.56, 1]
            params[k] = bad
            _fails(call, name, params=tuple(params))
    _fails(call, 'too many', n=0x80000000)
    _fails(call, 'a path of 0', path=fake, path_len=0)
    _fails(call, 'a path of', path=fake, path_len=(1 << 22) + 1)
    _fails(call, 'a path of', path=fake, path_len=0xFFFFFFFF)
    # what is allowed: n == 0 with nothing else valid, either direction, any limits on the walk, a path of up to 2^22 entries, a
    # path_len that is not read without a path
    assert call(n=0, floor=None, ceil=None, dist=None, starts=None, cells=None, moves=None) == 0
    assert call(n=0, params=(0.0, 0.0, 0.0, 0)) == 0 and call(n=0, params=(inf, inf, inf, rd.FLOOD_TOWARDS)) == 0
    assert call(n=0, max_moves=0xFFFFFFFF, stop=0xFFFFFFFF) == 0 and call(n=0, max_moves=0, stop=0) == 0
    assert call(n=0, path=fake, path_len=1) == 0 and call(n=0, path=fake, path_len=1 << 22) == 0 and call(n=0, path=None, path_len=0xFFFFFFFF) == 0
    assert call(n=0, w=2048, h=2048) == 0 and call(n=0, w=1, h=1) == 0
    _fails(call, 'null params', n=0, params=None)  # n == 0 is not a way round the checks
    _fails(call, 'too many', n=0, w=2049, h=2048)
    _fails(call, 'a path of', n=0, path=fake, path_len=0)


def test_the_frontiers_check_their_arguments_on_host_only_handles():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(1, device=False), wad.build_world_set([1, 0], device=False)  # E1M2, and E1M2 with E1M1
    cell = 0.25
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks, the last of them the device check
    f = ctypes.c_float
    shape = {world: world.area_plane_shape(cell), ws: ws.area_plane_shape(cell)}
    words = {world: world.area_words(cell), ws: ws.area_words(cell)}
    assert shape[ws][0] > shape[world][0] and shape[ws][1] > shape[world][1]

    def front(h=world, n=4, cell=cell, w=None, ht=None, area=fake, stride=None, dist=fake, out=fake, dout=None, count=None, mask=None, lv=fake):
        hp = h._h if h is not None else None
        w, ht = shape[h][1] if w is None else w, shape[h][0] if ht is None else ht
        stride = words[h] if stride is None else stride
        if h is ws:
            return L.rdoom_worldset_area_frontiers(hp, lv, n, f(cell), w, ht, area, stride, dist, out, dout, count, mask, None)
        return L.rdoom_world_area_frontiers(hp, n, f(cell), w, ht, area, stride, dist, out, dout, count, mask, None)

    inf, nan = float('inf'), float('nan')
    for h, noun in ((world, 'world'), (ws, 'world set')):
        gh, gw = shape[h]
        for name in ('area', 'dist', 'out'):
            _fails(front, 'null', h=h, **{name: None})
        for c in (0.0, -0.25, inf, nan):
            _fails(front, 'cell', h=h, cell=c)
        for c in (1e-4, 1e-30):
            _fails(front, 'limits', h=h, cell=c, w=8192, ht=8192, stride=1 << 20)
        _fails(front, 'distances of', h=h, w=gw - 1)
        _fails(front, 'distances of', h=h, ht=gh - 1)
        _fails(front, noun + "'s grid", h=h, w=0)  # the handle's noun is in the text
        _fails(front, 'distances of', h=h, w=8193)
        _fails(front, 'distances of', h=h, ht=0xFFFFFFFF)
        _fails(front, 'too many', h=h, n=0x80000000)
        _fails(front, 'stride', h=h, stride=words[h] - 1)
        _fails(front, 'stride', h=h, stride=0)
        _fails(front, 'HOST_ONLY', h=h)  # all else in order: the handle has no device copy
        _fails(front, 'HOST_ONLY', h=h, w=8192, ht=8192, stride=words[h] + 7, dout=fake, count=fake, mask=fake)
        _fails(front, 'HOST_ONLY', h=h, n=0, area=None, dist=None, out=None)
    _fails(front, 'distances of', h=ws, w=shape[world][1], ht=shape[world][0])  # enough for E1M2, not for every level of the set
    _fails(front, 'stride', h=ws, stride=words[world])
    _fails(front, 'null levels', h=ws, lv=None)
    assert front(h=ws, lv=None, n=0) == BAD and b'HOST_ONLY' in L.rdoom_last_error()  # n == 0 needs no levels
    assert L.rdoom_world_area_frontiers(None, 4, f(cell), 64, 64, fake, 64, fake, fake, None, None, None, None) == BAD and b'null' in L.rdoom_last_error()
    assert L.rdoom_worldset_area_frontiers(None, fake, 4, f(cell), 64, 64, fake, 64, fake, fake, None, None, None, None) == BAD
    assert b'null' in L.rdoom_last_error()


# ---- the walk's reference, by hand -------------------------------------------------------------------------------------------------

def _field(case, seed, towards):
    return goal_ref.flood(case['floor'], case['ceiling'], seed, towards, **case['kw'])


def test_the_walk_on_the_ledge_cell_by_cell():
    c = BY_NAME['ledge from the top']  # columns 0-2 at 0.48, columns 3-6 at 0
    f, g = c['floor'], c['ceiling']
    to_low = goal_ref.flood(f, g, (6, 0), True)  # towards a seed on the low side: the plateau drops off anywhere
    assert to_low[2, 1] == 7
    cell, m, path = path_ref.descend(f, g, to_low, (1, 2), towards=True)
    assert path == [(2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (6, 1), (6, 0)] and m == 7 and cell == (6, 0)
    # the limits: K moves ahead, or the goal if it is nearer; a stop distance; both
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, max_moves=3)[:2] == ((4, 2), 3)
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, max_moves=0) == ((1, 2), 0, [])
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, max_moves=100)[:2] == ((6, 0), 7)
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, stop_dist=2)[:2] == ((6, 2), 5)
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, stop_dist=7) == ((1, 2), 0, [])
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, stop_dist=100) == ((1, 2), 0, [])
    assert path_ref.descend(f, g, to_low, (1, 2), towards=True, max_moves=2, stop_dist=2)[:2] == ((3, 2), 2)
    # no start, no walk
    for start in ((-1, -1), (7, 2), (1, 5), (1, -1), (-2 ** 31, 2 ** 31 - 1)):
        assert path_ref.descend(f, g, to_low, start, towards=True) == ((-1, -1), 0, [])
    towards_plateau = goal_ref.flood(f, g, (0, 0), True)  # the low side cannot get there: unreached
    assert towards_plateau[2, 4] == U and path_ref.descend(f, g, towards_plateau, (4, 2), towards=True) == ((-1, -1), 0, [])


def test_the_walk_in_a_forward_field_never_crosses_the_ledge_upwards():
    c = BY_NAME['ledge with a stair from below']  # as above, and a stair of 0.24 at (3, 4): the only way up
    f, g = c['floor'], c['ceiling']
    forward = goal_ref.flood(f, g, (6, 0))
    assert np.array_equal(forward, goal_ref.widen(c['want']))
    # from the plateau's far corner the way back to the seed is down the plateau, over the stair, along the low side: written out
    cell, m, path = path_ref.descend(f, g, forward, (0, 0))
    assert m == forward[0, 0] == 14 and cell == (6, 0)
    assert path == [(1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (6, 3), (6, 2), (6, 1), (6, 0)]
    # whichever cell of the plateau it starts from, the walk leaves the plateau over the stair: read backwards it is the way the
    # field's moves came, and they climb nowhere else
    for r in range(5):
        for col in range(3):
            _, m, path = path_ref.descend(f, g, forward, (col, r))
            cells = [(col, r)] + path
            off = next(k for k, (x, _) in enumerate(cells) if x >= 3)
            assert m == forward[r, col] and cells[off] == (3, 4) and cells[off - 1] == (2, 4) and all(x >= 3 for x, _ in cells[off:])
    # from a low cell the walk stays low
    _, m, path = path_ref.descend(f, g, forward, (3, 2))
    assert m == 5 and all(x >= 3 and f[z, x] == 0 for x, z in path)


def test_the_distances_alone_would_walk_into_the_foot_of_a_ledge():
    """column 0 low; column 1 a plateau of 0.48 in rows 0-2, a stair of 0.24 in row 3, low in row 4; the seed at (0, 4).  The plateau's
    (1, 2) is 3 moves from the seed over the stair; its left neighbour (0, 2) is 2 moves from the seed and comes first in the
    neighbour order, but the move from it up to the plateau is not allowed"""
    f, g = flood_ref.room(2, 5, 0.0, 2.0)
    f[:3, 1], f[3, 1] = F(0.48), F(0.24)
    forward = goal_ref.flood(f, g, (0, 4))
    assert forward.tolist() == [[4, 5], [3, 4], [2, 3], [1, 2], [0, 1]]
    assert forward[2, 0] == forward[2, 1] - 1  # the trap
    cell, m, path = path_ref.descend(f, g, forward, (1, 2))
    assert path == [(1, 3), (0, 3), (0, 4)] and m == 3 and cell == (0, 4)
    # towards the same seed the plateau drops straight off, and the walk takes the left neighbour at once
    back = goal_ref.flood(f, g, (0, 4), True)
    assert back[2, 1] == 3 and path_ref.descend(f, g, back, (1, 2), towards=True)[2] == [(0, 2), (0, 3), (0, 4)]


def test_the_order_of_the_neighbours_shows_on_a_flat_room():
    f, g = flood_ref.room(6, 4)
    field = goal_ref.flood(f, g, (0, 0), True)
    cell, m, path = path_ref.descend(f, g, field, (5, 3), towards=True)
    assert path == [(4, 3), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1), (0, 0)] and m == 8 and cell == (0, 0)  # all the way left, then up
    field = goal_ref.flood(f, g, (5, 3), True)
    assert path_ref.descend(f, g, field, (0, 0), towards=True)[2] == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (5, 2), (5, 3)]  # right, then down
    field = goal_ref.flood(f, g, (0, 3), True)
    assert path_ref.descend(f, g, field, (5, 0), towards=True)[2][:5] == [(4, 0), (3, 0), (2, 0), (1, 0), (0, 0)]  # left before down


def _allowed(case, a, b):
    """the move from cell a to its 4-neighbour b, by flood_ref.moves' bits at b"""
    _, bits = flood_ref.moves(case['floor'], case['ceiling'], **dict(flood_ref.DEFAULTS, **case['kw']))
    bit = {(1, 0): flood_ref.FROM_LEFT, (-1, 0): flood_ref.FROM_RIGHT, (0, 1): flood_ref.FROM_ABOVE, (0, -1): flood_ref.FROM_BELOW}[(b[0] - a[0], b[1] - a[1])]
    return bool(bits[b[1], b[0]] & bit)


def test_every_walk_on_every_hand_made_grid_is_a_shortest_path_of_allowed_moves():
    walks = 0
    for c in CASES:
        h, w = c['floor'].shape
        seed = c['seed'] if c['seed'] is not None else (w // 2, h // 2)
        for towards in (False, True):
            field = _field(c, seed, towards)
            for r in range(h):
                for col in range(w):
                    cell, m, path = path_ref.descend(c['floor'], c['ceiling'], field, (col, r), towards=towards, **c['kw'])
                    if field[r, col] == U:
                        assert (cell, m, path) == ((-1, -1), 0, []), (c['name'], towards, col, r)
                        continue
                    assert m == field[r, col] == len(path) and cell == tuple(seed), (c['name'], towards, col, r)
                    cells = [(col, r)] + path
                    for a, b in zip(cells, cells[1:]):
                        assert abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 and field[b[1], b[0]] == field[a[1], a[0]] - 1
                        assert _allowed(c, a, b) if towards else _allowed(c, b, a), (c['name'], towards, a, b)
                    walks += 1
    assert walks > 500


def test_a_field_paired_with_other_planes_stops_early():
    rng = np.random.default_rng(5)
    f = np.where(rng.random((24, 31)) < 0.3, 0.3, 0.0).astype(F)  # steps of 0.3: taken at max_step 0.32, refused at 0.24
    g = np.full((24, 31), 1.5, F)
    f[0, 0] = 0
    stopped = 0
    for towards in (False, True):
        field = goal_ref.flood(f, g, (0, 0), towards, max_step=0.32)
        assert (field != U).all()
        for r in range(24):
            for col in range(31):
                cell, m, path = path_ref.descend(f, g, field, (col, r), towards=towards, max_step=0.24)
                assert m <= field[r, col] and field[cell[1], cell[0]] == field[r, col] - m and len(path) == m
                stopped += m < field[r, col]
    assert stopped > 100
    # and a field of nonsense: the walk ends as soon as no neighbour is one less
    junk = rng.integers(0, 5, (24, 31)).astype(np.uint32)
    for col in range(31):
        cell, m, path = path_ref.descend(f, g, junk, (col, 7), max_step=0.32)
        assert m <= junk[7, col] <= 4


# ---- the frontier's reference, by hand -----------------------------------------------------------------------------------------------

AREA_9x6 = ['.........',   # '.': unknown, 'F': free, 'W': wall, 'B': both bits
            '.FFFW....',
            '.FFFW....',
            '.FFFFF...',
            '.WWWB....',
            '.........']


def rows_of(picture, gw, stride=None):
    """(2, stride) uint32 rows of a picture whose lines are grid rows (left-aligned: cells beyond a line are unknown), and the grid"""
    gh, pitch = len(picture), (gw + 31) // 32
    grid = rd.AreaGrid(0, 0, gw, gh, pitch, gh * pitch)
    rows = np.zeros((2, grid.words if stride is None else stride), np.uint32)
    for iz, line in enumerate(picture):
        for ix, ch in enumerate(line):
            for plane, letters in ((0, 'FB'), (1, 'WB')):
                if ch in letters:
                    rows[plane, iz * pitch + ix // 32] |= np.uint32(1 << (ix % 32))
    return rows, grid


def test_the_frontier_of_a_hand_made_area():
    rows, grid = rows_of(AREA_9x6, 9)
    assert rows[0].tolist() == [0, 0b1110, 0b1110, 0b111110, 0b10000, 0] and rows[1].tolist() == [0, 0b10000, 0b10000, 0, 0b11110, 0]
    f, g = flood_ref.room(9, 6, np.inf, -np.inf)
    for iz, line in enumerate(AREA_9x6):
        for ix, ch in enumerate(line):
            if ch == 'F':
                f[iz, ix], g[iz, ix] = 0, 1
    dist = goal_ref.flood(f, g, (2, 2))  # the player in the middle of what it has seen
    assert dist[3, 5] == 4 and (dist != U).sum() == 11
    cell, d, count, mask = path_ref.frontiers(rows, grid, dist)
    want = np.zeros((6, 9), np.uint8)
    for ix, iz in ((1, 1), (2, 1), (3, 1), (1, 2), (1, 3), (5, 3)):  # the free cells next to a '.'; (4, 3) lies between two walls
        want[iz, ix] = 1
    assert np.array_equal(mask, want) and count == 6
    assert dist[1, 2] == dist[2, 1] == 1 and (cell, d) == ((2, 1), 1)  # a tie: the smaller iz
    # a tie within a row: the smaller ix
    tie = dist.copy()
    tie[1, 1] = tie[1, 3] = 0
    assert path_ref.frontiers(rows, grid, tie)[:2] == ((1, 1), 0)
    # a field that reaches every cell: every cell with an unknown neighbour, itself unknown or not
    cell, d, count, mask = path_ref.frontiers(rows, grid, np.full((6, 9), 3, np.uint32))
    assert mask[0].all() and mask[5].all() and mask[:, 0].all() and mask[:, 6:].all() and not mask[2, 2] and not mask[3, 4] and mask[2, 4] and mask[4, 4]
    assert count == 54 - 5 and (cell, d) == ((0, 0), 3)  # (2, 2), (3, 2), (2, 3), (3, 3) and (4, 3) have none
    # nothing reached, and a slot outside the set: no frontier
    assert path_ref.frontiers(rows, grid, np.full((6, 9), U, np.uint32))[:3] == ((-1, -1), U, 0)
    assert path_ref.frontiers(rows, None, dist)[:3] == ((-1, -1), U, 0)


def test_bits_beyond_the_grid_are_not_unknown_cells():
    # every cell of a 9 x 6 grid free, every cell reached: the clear bits 9 .. 31 of a row, and the zero words a longer stride has
    # after the last row, are no cells -- there is no frontier
    rows, grid = rows_of(['F' * 9] * 6, 9, stride=11)
    assert rows[0].tolist() == [0x1FF] * 6 + [0] * 5
    everywhere = np.zeros((6, 9), np.uint32)
    assert path_ref.frontiers(rows, grid, everywhere)[:3] == ((-1, -1), U, 0)
    # distances padded beyond the grid: reached cells out there are no frontier cells either
    padded = np.zeros((8, 40), np.uint32)
    cell, d, count, mask = path_ref.frontiers(rows, grid, padded)
    assert (cell, d, count) == ((-1, -1), U, 0) and mask.shape == (8, 40) and not mask.any()
    # one unknown cell at the edge: its neighbours inside the grid, and only those
    rows, grid = rows_of(['F' * 9] * 2 + ['F' * 8 + '.'] + ['F' * 9] * 3, 9)
    cell, d, count, mask = path_ref.frontiers(rows, grid, padded)
    assert sorted(zip(*np.nonzero(mask))) == [(1, 8), (2, 7), (3, 8)] and count == 3 and cell == (8, 1)
    # the same across a word edge: gw 33, the unknown cell (32, 2) the only one of its word
    rows, grid = rows_of(['F' * 33] * 2 + ['F' * 32 + '.'] + ['F' * 33] * 3, 33)
    assert grid.pitch == 2
    cell, d, count, mask = path_ref.frontiers(rows, grid, padded)
    assert sorted(zip(*np.nonzero(mask))) == [(1, 32), (2, 31), (3, 32)] and count == 3 and cell == (32, 1)
