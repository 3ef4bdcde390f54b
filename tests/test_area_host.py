"""The explored area on the host, with no GPU: the eight entry points and their argument checks on host-only handles, the grid of a
level against a numpy evaluation of the contract's formulas, rd.area_steps and rd.unpack_area, and the restatement
(tests/area_restatement.c) pinned without the library -- its T_r are the seen-lines restatement's bit for bit; every cell it marks
FREE has a witness sample that, recomputed in float64, lies in the cell or a neighbour and is hidden by no blocking line; every cell
it marks WALL has one that lies on a blocking line; calls accumulate and count what is new; a door a player opened widens that
player's area."""
import ctypes

import numpy as np
import pytest

import area_ref
import automap_ref
import reveal_ref
import rust_doom_amd as rd
from util import META_PATH, ensure_big_wad, ensure_wad

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
SYMBOLS = ['rdoom_world_area_grid', 'rdoom_worldset_level_area_grid', 'rdoom_world_area_words', 'rdoom_worldset_area_words',
           'rdoom_world_reveal_area', 'rdoom_worldset_reveal_area', 'rdoom_world_draw_area_maps', 'rdoom_worldset_draw_area_maps']
GRID_LEVELS = {'E1M1': (ensure_wad, 0), 'E1M2': (ensure_wad, 1), 'E1M8': (ensure_wad, 7), 'big': (ensure_big_wad, 0)}


def test_the_symbols_resolve_and_the_constants_are_the_headers():
    L = rd.lib()
    for name in SYMBOLS:
        assert name in rd.API_SYMBOLS and getattr(L, name).restype is ctypes.c_int32
    assert (rd.AREA_UNKNOWN, rd.AREA_FREE, rd.AREA_WALL) == (0, 1, 2) and rd.AREA_MAX_STEPS == 4096
    assert rd.AREA_COLORS.shape == (3, 3) and rd.AREA_COLORS.dtype == np.uint8 and len({tuple(c) for c in rd.AREA_COLORS}) == 3


def test_the_entry_points_check_their_arguments_on_host_only_handles():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(1, device=False), wad.build_world_set([1, 0], device=False)  # E1M2, and E1M2 with E1M1
    cell = 0.25
    words, set_words = world.area_words(cell), ws.area_words(cell)
    assert set_words > words and world.game_objects >= 1
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks, the last of them the device check
    view = rd.MapView(77, 53, 0.12, 0.0, 0.0, 0)
    f = ctypes.c_float

    def reveal(h=world, st=fake, n=4, dirs=fake, rays=8, rng=10.0, off=None, no=0, cell=cell, steps=80, area=fake, stride=None, new=None, lv=fake):
        hp = h._h if h is not None else None
        stride = (set_words if h is ws else words) if stride is None else stride
        if h is ws:
            return L.rdoom_worldset_reveal_area(hp, st, lv, n, dirs, rays, f(rng), off, no, f(cell), steps, area, stride, new, None)
        return L.rdoom_world_reveal_area(hp, st, n, dirs, rays, f(rng), off, no, f(cell), steps, area, stride, new, None)

    def draw(h=world, st=fake, n=4, v=view, area=fake, stride=None, cell=cell, out=fake, lv=fake):
        hp = h._h if h is not None else None
        vp = ctypes.byref(v) if v is not None else None
        stride = (set_words if h is ws else words) if stride is None else stride
        if h is ws:
            return L.rdoom_worldset_draw_area_maps(hp, st, lv, n, vp, area, stride, f(cell), out, None)
        return L.rdoom_world_draw_area_maps(hp, st, n, vp, area, stride, f(cell), out, None)

    def fails(call, word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    inf, nan = float('inf'), float('nan')
    for h, noun in ((world, 'world'), (ws, 'world set')):
        for kw in (dict(st=None), dict(area=None), dict(dirs=None)):
            fails(reveal, 'null', h=h, **kw)
        fails(reveal, 'n_rays', h=h, rays=0)
        for r in (0.0, -1.0, inf, nan):
            fails(reveal, 'max_range', h=h, rng=r)
        for c in (0.0, -0.25, inf, nan):
            fails(reveal, 'cell', h=h, cell=c)
            fails(draw, 'cell', h=h, cell=c)
        for k in (0, 4097, 0xFFFFFFFF):
            fails(reveal, 'n_steps', h=h, steps=k)
        enough = set_words if h is ws else words
        fails(reveal, 'stride', h=h, stride=enough - 1)
        fails(reveal, 'stride', h=h, stride=0)
        fails(reveal, noun + "'s grid", h=h, stride=0)  # the handle's noun is in the text
        fails(reveal, 'limits', h=h, cell=1e-4, stride=1 << 30)  # E1M2 is some ten units wide: a hundred thousand cells a side
        fails(reveal, 'limits', h=h, cell=1e-30, stride=1 << 30)  # a bound of 2^30 cells or more
        fails(reveal, 'n_objects', h=h, off=fake, no=0)
        fails(reveal, 'HOST_ONLY', h=h)  # all else in order: the handle has no device copy
        fails(reveal, 'HOST_ONLY', h=h, stride=enough + 3, new=fake, steps=4096, off=fake, no=64)
        fails(reveal, 'HOST_ONLY', h=h, n=0, st=None, area=None, dirs=None)
        fails(draw, 'null', h=h, v=None)
        for kw in (dict(st=None), dict(area=None), dict(out=None)):
            fails(draw, 'null', h=h, **kw)
        fails(draw, 'pixels', h=h, v=rd.MapView(0, 53, 0.12, 0.0, 0.0, 0))
        fails(draw, 'pixels', h=h, v=rd.MapView(77, 16385, 0.12, 0.0, 0.0, 0))
        for s in (0.0, -1.0, inf, nan):
            fails(draw, 'scale', h=h, v=rd.MapView(77, 53, s, 0.0, 0.0, 0))
        for flags in (rd.MAP_SHOW_FLAT, rd.MAP_SHOW_HIDDEN, 16):
            fails(draw, 'flags', h=h, v=rd.MapView(77, 53, 0.12, 0.0, 0.0, flags))
        fails(draw, 'stride', h=h, stride=enough - 1)
        fails(draw, 'limits', h=h, cell=1e-4, stride=1 << 30)
        fails(draw, 'too many', h=h, n=1 << 31 - 1, v=rd.MapView(64, 64, 0.12, 0.0, 0.0, 0))
        fails(draw, 'HOST_ONLY', h=h)
        fails(draw, 'HOST_ONLY', h=h, v=rd.MapView(77, 53, 0.12, 0.0, 0.0, rd.MAP_ROTATE | rd.MAP_TOP_DOWN))
    fails(reveal, 'stride', h=ws, stride=words)  # enough for E1M2, not for the set's largest level
    fails(draw, 'stride', h=ws, stride=words)
    fails(reveal, 'null', h=ws, lv=None)
    fails(draw, 'null', h=ws, lv=None)
    assert L.rdoom_world_reveal_area(None, fake, 4, fake, 8, f(10.0), None, 0, f(cell), 80, fake, words, None, None) == BAD
    assert L.rdoom_worldset_reveal_area(None, fake, fake, 4, fake, 8, f(10.0), None, 0, f(cell), 80, fake, words, None, None) == BAD
    assert L.rdoom_world_draw_area_maps(None, fake, 4, ctypes.byref(view), fake, words, f(cell), fake, None) == BAD
    assert L.rdoom_worldset_draw_area_maps(None, fake, fake, 4, ctypes.byref(view), fake, words, f(cell), fake, None) == BAD
    # the grid calls
    g, w = rd.AreaGridStruct(), ctypes.c_uint32()
    assert L.rdoom_world_area_grid(None, f(cell), ctypes.byref(g)) == BAD and L.rdoom_world_area_grid(world._h, f(cell), None) == BAD
    assert L.rdoom_worldset_level_area_grid(None, 0, f(cell), ctypes.byref(g)) == BAD
    assert L.rdoom_worldset_level_area_grid(ws._h, 2, f(cell), ctypes.byref(g)) == BAD and b'slot' in L.rdoom_last_error()
    assert L.rdoom_world_area_words(None, f(cell), ctypes.byref(w)) == BAD and L.rdoom_worldset_area_words(ws._h, f(cell), None) == BAD
    for c in (0.0, -1.0, inf, nan):
        assert L.rdoom_world_area_grid(world._h, f(c), ctypes.byref(g)) == BAD and b'cell' in L.rdoom_last_error()
        assert L.rdoom_worldset_area_words(ws._h, f(c), ctypes.byref(w)) == BAD and b'cell' in L.rdoom_last_error()
    for c in (1e-4, 1e-30):
        assert L.rdoom_world_area_grid(world._h, f(c), ctypes.byref(g)) == BAD and b'limits' in L.rdoom_last_error()
        assert L.rdoom_worldset_level_area_grid(ws._h, 1, f(c), ctypes.byref(g)) == BAD and b'limits' in L.rdoom_last_error()
        assert L.rdoom_world_area_words(world._h, f(c), ctypes.byref(w)) == BAD and L.rdoom_worldset_area_words(ws._h, f(c), ctypes.byref(w)) == BAD
    with pytest.raises(rd.RdoomError):
        world.area_grid(-1.0)


@pytest.mark.parametrize('level', list(GRID_LEVELS))
def test_the_grid_is_the_contracts_formulas(level):
    ensure, index = GRID_LEVELS[level]
    wad = rd.Wad(ensure(), META_PATH)
    world = wad.build_world(index, device=False)
    lines = world.map_lines()
    for cell in (0.25, 0.0625):
        g = world.area_grid(cell)
        assert isinstance(g, rd.AreaGrid) and g == area_ref.grid_numpy(lines, cell) == area_ref.grid(lines, cell)
        assert world.area_words(cell) == g.words == g.gh * g.pitch and g.pitch == (g.gw + 31) // 32
        # the level with a cell of margin: the first and last columns and rows hold no end point
        xs, zs = np.concatenate([lines['a'][:, 0], lines['b'][:, 0]]), np.concatenate([lines['a'][:, 1], lines['b'][:, 1]])
        ix, iz = np.floor(xs / F(cell)).astype(int) - g.ix0, np.floor(zs / F(cell)).astype(int) - g.iz0
        assert ix.min() == 1 and ix.max() == g.gw - 2 and iz.min() == 1 and iz.max() == g.gh - 2
        if (level, cell) == ('E1M1', 0.25):
            assert (g.gw, g.gh, g.words) == (123, 118, 472)
        if (level, cell) == ('E1M2', 0.25):
            assert (g.gw, g.gh) == (13, 21)
        if (level, cell) == ('E1M2', 0.0625):
            assert (g.gw, g.gh) == (44, 75)
        if (level, cell) == ('big', 0.0625):
            assert (g.gw, g.gh, g.words) == (1273, 1274, 50960)


def test_a_sets_grids_are_its_levels_and_its_words_the_largest():
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 1, 7]
    ws = wad.build_world_set(slots, device=False)
    for cell in (0.25, 0.0625):
        each = [wad.build_world(i, device=False).area_grid(cell) for i in slots]
        assert [ws.area_grid(s, cell) for s in range(3)] == each and len({g.words for g in each}) == 3
        assert ws.area_words(cell) == max(g.words for g in each)


def test_area_steps():
    assert rd.area_steps(12.0, 0.25) == 96 and rd.area_steps(40.0, 0.0625) == 1280 and rd.area_steps(12.0, 0.0625) == 384
    assert rd.area_steps(1.0, 0.3) == 7 and rd.area_steps(0.01, 1.0) == 1
    for bad in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0)):
        with pytest.raises(ValueError):
            rd.area_steps(*bad)


def test_unpack_area_round_trip():
    g = rd.AreaGrid(-3, 5, 70, 9, 3, 27)
    rs = np.random.RandomState(5)
    cells = rs.rand(2, g.gh, g.gw) < 0.3
    rows = np.zeros((2, g.words + 2), np.uint32)
    for which, iz, ix in np.argwhere(cells):
        rows[which, iz * g.pitch + ix // 32] |= np.uint32(1) << np.uint32(ix % 32)
    rows[:, g.words:] = 0xFFFFFFFF  # padding is not read
    for p in range(2):
        rows[p, 2:g.words:3] |= np.uint32(0xFFFFFFC0)  # nor are the bits beyond gw = 64 + 6 in a row's last word
    got = rd.unpack_area(rows, g)
    assert got.dtype == bool and got.shape == (2, g.gh, g.gw) and np.array_equal(got, cells)
    assert np.array_equal(rd.unpack_area(rows.view(np.int32), g), cells)
    with pytest.raises(ValueError):
        rd.unpack_area(rows[:, :g.words - 1], g)
    with pytest.raises(ValueError):
        rd.unpack_area(rows[0], g)


def _start(wad, index, yaws):
    pos, yaw = wad.build_level(index).start()
    return rd.player_states(np.repeat(pos[None], len(yaws), 0), np.array([yaw + y for y in yaws], F)), pos, yaw


@pytest.mark.parametrize('level', ['E1M1', 'E1M2', 'E1M8'])
def test_what_the_restatement_marks_has_a_witness_in_float64(level):
    """a player at the level's start, 180 rays over 2 pi at range 20 and cell 0.25.  The T_r are the seen-lines restatement's.  Every
    FREE cell has a witness sample (ray, step) which, recomputed in float64 from the yaw and the fan, lies in the cell or one of
    its eight neighbours, and the segment from the player to it crosses no blocking line; every WALL cell has a witness ray whose
    point at T_r lies in the cell or a neighbour and within 1e-4 units of a blocking line.  1e-4 world units of slack against
    grazing (float32 positions of some tens of units carry 4e-6).  The blocking set is worked out in numpy from the table."""
    ensure, index = GRID_LEVELS[level]
    wad = rd.Wad(ensure(), META_PATH)
    lines = wad.build_world(index, device=False).map_lines()
    st, pos, yaw = _start(wad, index, [0.0])
    fan = rd.map_fan(180, 2 * np.pi)
    max_range, cell, slack = 20.0, 0.25, 1e-4
    steps = rd.area_steps(max_range, cell)
    out = area_ref.reveal(lines, st, fan, max_range, cell, detail=True)
    seen = reveal_ref.reveal(lines, st, fan, max_range, detail=True)
    assert np.array_equal(out['limit'].view(np.uint32), seen['limit'].view(np.uint32))
    g = area_ref.grid(lines, cell)
    planes = rd.unpack_area(out['area'][0], g)
    assert np.array_equal(out['new'][0], planes.reshape(2, -1).sum(1)) and np.array_equal(out['new'], area_ref.popcount(out['area']))
    assert planes[0].sum() > 100 and planes[1].sum() > 10 and (planes[0] & planes[1]).any() and (out['limit'] < 1).mean() > 0.9
    block = reveal_ref.blocking(lines)
    a, b = lines['a'].astype(np.float64)[block], lines['b'].astype(np.float64)[block]
    o = np.array([pos[0], pos[2]], np.float64)
    s, c = np.sin(np.float64(yaw)), np.cos(np.float64(yaw))
    vels = np.stack([c * fan[:, 0] - s * fan[:, 1], -s * fan[:, 0] - c * fan[:, 1]], 1).astype(np.float64) * max_range

    def near(q, iz, ix):
        cx, cz = np.floor(q[0] / cell) - g.ix0, np.floor(q[1] / cell) - g.iz0
        return abs(cx - ix) <= 1 and abs(cz - iz) <= 1

    fw = out['free_witness'][0].reshape(g.gh, g.gw, 2) if g.gw * g.gh == out['free_witness'].shape[1] else None
    ww = out['wall_witness'][0].reshape(g.gh, g.gw)
    assert fw is not None and np.array_equal(planes[0], fw[:, :, 0] != area_ref.NONE) and np.array_equal(planes[1], ww != area_ref.NONE)
    for iz, ix in np.argwhere(planes[0]):
        r, k = fw[iz, ix]
        t = np.float64(k) / steps
        assert t <= np.float64(out['limit'][0, r]) + 1e-6
        q = o + t * vels[r]
        assert near(q, iz, ix), (iz, ix, q)
        assert not area_ref.crossed64(o, q, a, b, slack).any(), (iz, ix)
    for iz, ix in np.argwhere(planes[1]):
        r = ww[iz, ix]
        t = np.float64(out['limit'][0, r])
        assert t < 1
        q = o + t * vels[r]
        assert near(q, iz, ix), (iz, ix, q)
        assert area_ref.distance64(q, a, b).min() <= slack, (iz, ix)
        assert not area_ref.crossed64(o, q, a, b, slack).any(), (iz, ix)
    # the player's own cell is free: the sample of step 0
    own_x, own_z = int(np.floor(F(pos[0]) / F(cell))) - g.ix0, int(np.floor(F(pos[2]) / F(cell))) - g.iz0
    assert planes[0, own_z, own_x]
    # and with a single step only the ends of the rays are sampled: the own cell, and the cells at range of the unstopped rays
    ends = area_ref.reveal(lines, st, fan, max_range, cell, n_steps=1)
    assert 1 <= ends['new'][0, 0] <= 1 + (out['limit'] >= 1).sum() and np.array_equal(ends['area'][0, 1], out['area'][0, 1])


def test_rows_accumulate_and_count_what_is_new():
    wad = rd.Wad(ensure_wad(), META_PATH)
    lines = wad.build_world(0, device=False).map_lines()
    st, _, _ = _start(wad, 0, [0.0, 2.0])
    fan = rd.map_fan(64, 1.6)
    words = area_ref.grid(lines, 0.25).words
    first = area_ref.reveal(lines, st, fan, 20.0, 0.25, stride=words + 2)
    assert (first['area'][0] != first['area'][1]).any() and (first['area'][:, :, -2:] == 0).all()
    again = area_ref.reveal(lines, st[::-1].copy(), fan, 20.0, 0.25, area=first['area'])
    assert np.array_equal(again['area'][0], first['area'][0] | first['area'][1])
    assert np.array_equal(again['new'], area_ref.popcount(again['area'] & ~first['area'])) and (again['new'] > 0).all()
    third = area_ref.reveal(lines, st[::-1].copy(), fan, 20.0, 0.25, area=again['area'])
    assert np.array_equal(third['area'], again['area']) and not third['new'].any()
    # a NaN position or yaw marks nothing; a player far outside the grid marks nothing either
    odd = st.copy()
    odd['pos'][0, 0] = np.nan
    odd['yaw'][1] = np.nan
    assert not area_ref.reveal(lines, odd, fan, 20.0, 0.25)['area'].any()
    odd = st.copy()
    odd['pos'][:, 0] += F(500.0)
    assert not area_ref.reveal(lines, odd, fan, 20.0, 0.25)['new'].any()


def test_a_door_its_player_opened_widens_the_area():
    """E1M1's first door (the first MAP_CLOSED line that an object moves), a player half a unit before the middle of its face on
    either side: with the door's ceiling raised through `offsets` the FREE set strictly contains the one with the door shut, and the
    shut door's face is a WALL"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0, device=False)
    lines = world.map_lines()
    closed = np.nonzero(automap_ref.classes(lines) == rd.MAP_CLOSED)[0]
    l = next(int(k) for k in closed if max(lines['front']['ceiling_id'][k], lines['back']['ceiling_id'][k]) != 0)
    door = int(max(lines['front']['ceiling_id'][l], lines['back']['ceiling_id'][l]))
    a, b = lines['a'][l], lines['b'][l]
    d = b - a
    normal = np.array([d[1], -d[0]], F) / F(np.hypot(*d))
    fan = rd.map_fan(360, 2 * np.pi)
    g = area_ref.grid(lines, 0.25)
    for side in (1.0, -1.0):
        at = (a + b) / 2 + normal * F(0.5 * side)
        st = rd.player_states(np.array([[at[0], 0.0, at[1]]] * 2, F), np.zeros(2, F))
        off = np.zeros((2, world.game_objects, 3), F)
        off[1, door, 1] = 1.0
        assert reveal_ref.blocking(lines, off[0])[l] and not reveal_ref.blocking(lines, off[1])[l]
        out = area_ref.reveal(lines, st, fan, 20.0, 0.25, offsets=off)
        shut, opened = (rd.unpack_area(r, g) for r in out['area'])
        assert not (shut[0] & ~opened[0]).any() and (opened[0] & ~shut[0]).sum() > 20, side  # strictly more, and nothing less
        assert shut[1].any() and (shut[1] & ~opened[1]).any(), side  # the shut door's face stops rays that the open one lets by
        rest = area_ref.reveal(lines, st[:1], fan, 20.0, 0.25)  # NULL offsets: every object at rest, the door shut
        assert np.array_equal(rest['area'][0], out['area'][0])
