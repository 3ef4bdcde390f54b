"""The sectors on the host, with no GPU: the sector table against an independent reading of the MAP and BSP lumps on ten levels, the
restatement (tests/sector_restatement.c) on the library's host arrays against mapcheck's float64 ray cast over LINEDEFS, every
argument error of the four entry points on host-only handles, visited_words, and a patched IWAD with a secret sector."""
import ctypes
import struct

import numpy as np
import pytest

import mapcheck
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_big_wad, ensure_wad

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
LEVELS = [(ensure_wad, i) for i in range(9)] + [(ensure_big_wad, 0)]
IDS = ['E1M%d' % (i + 1) for i in range(9)] + ['big']


def _bsp(path, index):
    """SEGS, SSECTORS and NODES of a level, decoded here from the published formats, and the sub-sectors in the order a walk from
    the last node meets them, left child before right"""
    data, lumps = mapcheck.read_directory(path)
    m = mapcheck.level_markers(lumps)[index]
    by_name = {lumps[m + k][0]: lumps[m + k] for k in range(1, 11)}

    def rec(name, fmt):
        _, pos, size = by_name[name]
        st = struct.Struct(fmt)
        return [st.unpack_from(data, pos + i * st.size) for i in range(size // st.size)]
    segs, ssectors, nodes = rec(b'SEGS', '<HHHHHH'), rec(b'SSECTORS', '<HH'), rec(b'NODES', '<hhhh8hHH')
    order, stack = [], [len(nodes) - 1]
    while stack:
        child = stack.pop()
        if child & 0x8000:
            order.append(child & 0x7FFF)
        else:
            stack.extend([nodes[child][12], nodes[child][13]])  # right is pushed first, so left is met first
    return segs, ssectors, order


@pytest.mark.parametrize('ensure,index', LEVELS, ids=IDS)
def test_the_sector_table_against_the_lumps(ensure, index):
    wad = rd.Wad(ensure(), META_PATH)
    world = wad.build_world(index, device=False)
    m = mapcheck.Map(ensure(), index)
    t = world.map_sectors()
    lines = world.map_lines()
    assert len(t.sectors) == len(m.sectors) and world.visited_words() == (len(m.sectors) + 31) // 32
    for s, (floor, ceil, _, _, light, kind, tag) in enumerate(m.sectors):
        r = t.sectors[s]
        assert r['floor'] == F(floor) / F(100) and r['ceiling'] == F(ceil) / F(100), s
        assert (r['light_level'], r['sector_type'], r['tag']) == (light, kind, tag), s
    # the objects of a sector are those the line table gives every side of it
    sides = 0
    for l in lines:
        _, _, _, _, _, right, left = m.linedefs[l['linedef']]
        for side, name in ((right, 'front'), (left, 'back')):
            sec = m.side_sector(side)
            if l[name]['present']:
                sides += 1
                assert (l[name]['floor_id'], l[name]['ceiling_id']) == (t.sectors[sec]['floor_id'], t.sectors[sec]['ceiling_id'])
                assert (l[name]['floor'], l[name]['ceiling']) == (t.sectors[sec]['floor'], t.sectors[sec]['ceiling'])
    assert sides > len(lines) and ((t.sectors['floor_id'] != 0).any() or index == 1)  # (E1M2, one room, has nothing that moves)
    # leaves: the k-th leaf of the walk is the k-th chunk; its sector is its first seg's, its edges are its one-sided segs
    segs, ssectors, order = _bsp(ensure(), index)
    assert len(order) == len(t.leaf_sector) == len(t.leaf_edges) == len(world.arrays()['chunks'])
    assert np.array_equal(t.leaf_edges[:, 0], np.concatenate([[0], np.cumsum(t.leaf_edges[:, 1])[:-1]]))
    assert t.leaf_edges[:, 1].sum() == len(t.edges) > 0
    for k, sub in enumerate(order):
        count, first = ssectors[sub]
        mine = segs[first:first + count]

        def sector_of(seg, other=False):
            ld = m.linedefs[seg[3]]
            return m.side_sector(ld[5 + ((seg[4] == 1) != other)])
        assert t.leaf_sector[k] == sector_of(mine[0]) and t.leaf_sector[k] in {sector_of(g) for g in mine}, k
        solid = [g for g in mine if sector_of(g, other=True) is None]
        e = t.edges[t.leaf_edges[k, 0]:t.leaf_edges[k, 0] + t.leaf_edges[k, 1]]
        assert len(e) == len(solid), k
        for edge, g in zip(e, solid):
            ld = m.linedefs[g[3]]
            assert ld[5] == 0xFFFF or ld[6] == 0xFFFF
            a = mapcheck.world_to_map(edge['a'])[0]
            b = mapcheck.world_to_map(edge['a'].astype(np.float64) + edge['d'])[0]
            assert np.abs(a - m.vertices[g[0]]).max() < 1e-3 and np.abs(b - m.vertices[g[1]]).max() < 1e-3, (k, a, b)
            # a piece of the linedef: both ends on it -- a vertex where the node builder split a linedef is rounded to whole map
            # units, so it lies within half a unit square's diagonal (0.71) of the line
            v1, v2 = m.vertices[ld[0]], m.vertices[ld[1]]
            length = np.hypot(*(v2 - v1))
            for q in (a, b):
                along = np.dot(q - v1, v2 - v1) / length
                assert -0.75 <= along <= length + 0.75 and np.hypot(*(q - (v1 + along / length * (v2 - v1)))) < 0.75


def test_a_world_sets_tables_are_the_single_worlds():
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [7, 0, 2]
    ws = wad.build_world_set(slots, device=False)
    each = []
    for s, index in enumerate(slots):
        world = wad.build_world(index, device=False)
        for a, b in zip(ws.map_sectors(s), world.map_sectors()):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        each.append(world.visited_words())
    assert ws.visited_words() == max(each) and len(set(each)) > 1
    with pytest.raises(rd.RdoomError):
        ws.map_sectors(3)
    assert rd.MAP_SECTOR.itemsize == 28 and rd.MAP_EDGE.itemsize == 16 and rd.SECTOR_NONE == 0xFFFFFFFF and rd.SECTOR_NONE16 == 0xFFFF


@pytest.mark.parametrize('ensure,index', LEVELS, ids=IDS)
def test_the_restatement_agrees_with_a_ray_cast_over_the_linedefs(ensure, index):
    """4 000 seeded uniform points over the vertex box grown by 50 map units.  Among those farther than 2 map units from every
    linedef the restated sector is mapcheck's sector_at (float64, four rays over LINEDEFS, no BSP) on every point."""
    wad = rd.Wad(ensure(), META_PATH)
    tables = sector_ref.Tables(wad.build_world(index, device=False))
    m = mapcheck.Map(ensure(), index)
    rng = np.random.default_rng(1000 + index)
    pts = rng.uniform(m.vertices.min(0) - 50, m.vertices.max(0) + 50, (4000, 2))
    want, dist = m.sector_at(pts)
    got = sector_ref.sector_at(tables, sector_ref.map_to_world(pts)).astype(np.int64)
    got[got == sector_ref.NONE] = -1
    far = dist > 2
    assert far.mean() >= 0.9, far.mean()
    assert (want[far] < 0).mean() >= 0.3 and (want[far] >= 0).mean() >= 0.3, (want[far] < 0).mean()
    bad = far & (got != want)
    assert not bad.any(), (int(bad.sum()), pts[bad][:4], got[bad][:4], want[bad][:4])
    if index == 1 and ensure is ensure_wad:  # E1M2 has two sectors
        assert len(tables.sectors) == 2 and set(got[far]) == {-1, 0, 1}
    nan = sector_ref.sector_at(tables, F([[np.nan, 0], [0, np.nan], [np.nan, np.nan]]))
    assert (nan == sector_ref.NONE).all()


def test_the_entry_points_check_their_arguments_on_host_only_handles():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(0, device=False), wad.build_world_set([0, 7], device=False)
    words = world.visited_words()
    assert ws.visited_words() > words and world.game_objects > 1
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks, the last of them the device check
    view = rd.MapView(77, 53, 0.12, 0.0, 0.0, 0)

    def locate(h=world, st=fake, n=4, off=None, no=0, out=fake, heights=None, vis=fake, stride=words, new=None, lv=fake):
        hp = h._h if h is not None else None
        if h is ws:
            return L.rdoom_worldset_locate_players(hp, st, lv, n, off, no, out, heights, vis, stride, new, None)
        return L.rdoom_world_locate_players(hp, st, n, off, no, out, heights, vis, stride, new, None)

    def draw(h=world, st=fake, n=4, off=None, no=0, v=view, vis=fake, stride=words, sec=fake, floor=None, ceil=None, lv=fake):
        hp = h._h if h is not None else None
        vp = ctypes.byref(v) if v is not None else None
        if h is ws:
            return L.rdoom_worldset_draw_sector_maps(hp, st, lv, n, off, no, vp, vis, stride, sec, floor, ceil, None)
        return L.rdoom_world_draw_sector_maps(hp, st, n, off, no, vp, vis, stride, sec, floor, ceil, None)

    def fails(call, word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    inf, nan = float('inf'), float('nan')
    for h, w in ((world, words), (ws, ws.visited_words())):
        fails(locate, 'null', h=h, stride=w, st=None)
        fails(locate, 'null', h=h, stride=w, out=None)
        fails(locate, 'stride', h=h, stride=w - 1)
        fails(locate, 'stride', h=h, stride=0)
        fails(locate, 'n_objects', h=h, stride=w, off=fake, no=1)
        fails(locate, 'HOST_ONLY', h=h, stride=w)
        fails(locate, 'HOST_ONLY', h=h, vis=None, stride=0)  # without rows the stride is not looked at
        fails(locate, 'HOST_ONLY', h=h, stride=w + 3, heights=fake, new=fake, off=fake, no=64)
        fails(locate, 'HOST_ONLY', h=h, stride=w, n=0, st=None, out=None)
        fails(draw, 'null', h=h, stride=w, v=None)
        fails(draw, 'null', h=h, stride=w, st=None)
        fails(draw, 'no output', h=h, stride=w, sec=None)
        for bad in (rd.MapView(0, 53, 0.1, 0, 0, 0), rd.MapView(77, 0, 0.1, 0, 0, 0), rd.MapView(16385, 53, 0.1, 0, 0, 0)):
            fails(draw, 'pixels', h=h, stride=w, v=bad)
        for scale in (0.0, -1.0, inf, nan):
            fails(draw, 'scale', h=h, stride=w, v=rd.MapView(77, 53, scale, 0, 0, 0))
        for flags in (rd.MAP_SHOW_FLAT, rd.MAP_SHOW_HIDDEN, 16, rd.MAP_ROTATE | 0x100):
            fails(draw, 'flags', h=h, stride=w, v=rd.MapView(77, 53, 0.1, 0, 0, flags))
        fails(draw, 'n_objects', h=h, stride=w, off=fake, no=1)
        fails(draw, 'stride', h=h, stride=w - 1)
        fails(draw, 'too many', h=h, stride=w, n=1 << 20, v=rd.MapView(16384, 16384, 0.1, 0, 0, 0))
        fails(draw, 'HOST_ONLY', h=h, stride=w)
        fails(draw, 'HOST_ONLY', h=h, vis=None, stride=0, sec=None, ceil=fake)
        # half_width and marker are not read: values draw_maps refuses pass
        fails(draw, 'HOST_ONLY', h=h, stride=w, v=rd.MapView(77, 53, 0.1, nan, -1.0, rd.MAP_ROTATE | rd.MAP_TOP_DOWN))
        fails(draw, 'HOST_ONLY', h=h, stride=w, n=0, st=None, sec=None)
    fails(locate, 'stride', h=ws, stride=words)  # enough for E1M1, not for the set's largest level
    fails(draw, 'stride', h=ws, stride=words)
    fails(locate, 'null', h=ws, stride=ws.visited_words(), lv=None)
    fails(draw, 'null', h=ws, stride=ws.visited_words(), lv=None)
    assert L.rdoom_world_locate_players(None, fake, 4, None, 0, fake, None, None, 0, None, None) == BAD
    assert L.rdoom_worldset_locate_players(None, fake, fake, 4, None, 0, fake, None, None, 0, None, None) == BAD
    assert L.rdoom_world_draw_sector_maps(None, fake, 4, None, 0, ctypes.byref(view), None, 0, fake, None, None, None) == BAD
    assert L.rdoom_worldset_draw_sector_maps(None, fake, fake, 4, None, 0, ctypes.byref(view), None, 0, fake, None, None, None) == BAD
    assert L.rdoom_world_map_sectors(None, fake) == BAD and L.rdoom_world_map_sectors(world._h, None) == BAD


def test_a_patched_iwad_shows_its_sector_types(tmp_path):
    types = rd.Wad(ensure_wad(), META_PATH).build_world(0, device=False).map_sectors().sectors['sector_type']
    assert not np.isin(types, (5, 9)).any() and types.max() <= 17
    wad = rd.Wad(sector_ref.patched_wad(tmp_path, secret=3, damaging=11), META_PATH)
    got = wad.build_world(0, device=False).map_sectors().sectors['sector_type']
    assert got[3] == 9 and got[11] == 5
    rest = np.ones(len(types), bool)
    rest[[3, 11]] = False
    assert np.array_equal(got[rest], types[rest])


def test_the_restatement_keeps_rows_and_flags_what_is_new():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0, device=False)
    tables = sector_ref.Tables(world)
    rng = np.random.default_rng(5)
    st, on_map = sector_ref.players(wad, 0, 64, rng)
    off = sector_ref.random_offsets(rng, 64, world.game_objects)
    first = sector_ref.locate(tables, st, off, stride=world.visited_words() + 2)
    inside = first['sector'] != sector_ref.NONE
    # the last ones are outside the map or on a NaN; of the others a few were jittered off their centroid into a wall
    assert on_map < 64 and inside[:on_map].mean() > 0.8 and not inside[on_map:].any()
    assert np.array_equal(first['new'], inside.astype(np.uint32)) and (first['visited'][:, -2:] == 0).all()
    assert np.array_equal(np.isinf(first['heights'][:, 0]), ~inside) and (first['heights'][~inside] == F([np.inf, -np.inf])).all()
    rec = tables.sectors[first['sector'][inside]]
    at_rest = sector_ref.locate(tables, st)['heights'][inside]
    assert np.array_equal(at_rest, np.stack([rec['floor'], rec['ceiling']], 1))
    moved = first['heights'][inside] != at_rest
    assert moved.any() and not moved.all()  # some players stand in a sector their offsets move
    again = sector_ref.locate(tables, st, off, visited=first['visited'])
    assert not again['new'].any() and np.array_equal(again['visited'], first['visited'])
    for p in np.nonzero(inside)[0]:
        assert np.array_equal(np.nonzero(rd.unpack_seen(first['visited'][p], len(tables.sectors)))[0], [first['sector'][p]])
