"""The top-down map on the host, with no GPU: the line table of rdoom_world_map_lines against tests/mapcheck.py's independent
reading of the MAP lumps (count, order, end points, flags, specials, sides, heights), its object ids against the triggers' move
effects, the world set's tables against the single worlds', the census of line classes, and the restatement
(tests/automap_restatement.c) pinned by the image positions of the linedef mid-points, computed from wad coordinates alone."""
import ctypes

import numpy as np
import pytest

import automap_ref
import mapcheck
import rust_doom_amd as rd
from util import META_PATH, ensure_big_wad, ensure_wad

F = np.float32
LEVELS = [(ensure_wad, i) for i in range(9)] + [(ensure_big_wad, 0)]
IDS = ['E1M%d' % (i + 1) for i in range(9)] + ['big']
# one-sided, floor step, ceiling step, flat, closed at rest (generator seed 1993), counted from the MAP lumps
CENSUS = {0: (396, 198, 29, 22, 68), 2: (169, 132, 19, 7, 31), 7: (526, 281, 31, 20, 109), 1: (8, 1, 0, 0, 0)}


def _world(ensure, index):
    path = ensure()
    wad = rd.Wad(path, META_PATH)
    return path, wad, wad.build_world(index, device=False)


@pytest.mark.parametrize('ensure,index', LEVELS, ids=IDS)
def test_the_line_table_is_the_map(ensure, index):
    path, wad, world = _world(ensure, index)
    ml = world.map_lines()
    assert ml.dtype == rd.MAP_LINE and rd.MAP_LINE.itemsize == 68
    m = mapcheck.Map(path, index)
    valid = [k for k, l in enumerate(m.linedefs) if l[0] < len(m.vertices) and l[1] < len(m.vertices)]
    assert len(ml) == len(valid) > 0 and np.array_equal(ml['linedef'], valid)  # count and order
    lines = [m.linedefs[k] for k in valid]
    assert np.allclose(mapcheck.world_to_map(ml['a']), m.vertices[[l[0] for l in lines]], atol=0.01)
    assert np.allclose(mapcheck.world_to_map(ml['b']), m.vertices[[l[1] for l in lines]], atol=0.01)
    assert np.array_equal(ml['flags'], [l[2] for l in lines]) and np.array_equal(ml['special_type'], [l[3] for l in lines])
    for name, col in (('front', 5), ('back', 6)):
        sec = [m.side_sector(l[col]) for l in lines]
        sec = [s if s is not None and s < len(m.sectors) else None for s in sec]
        side = ml[name]
        assert np.array_equal(side['present'], [int(s is not None) for s in sec]), name
        floor = np.array([F(m.sectors[s][0]) / F(100.0) if s is not None else F(0) for s in sec], F)
        ceil = np.array([F(m.sectors[s][1]) / F(100.0) if s is not None else F(0) for s in sec], F)
        assert np.array_equal(side['floor'], floor) and np.array_equal(side['ceiling'], ceil), name
        absent = side['present'] == 0
        assert (side['floor_id'][absent] == 0).all() and (side['ceiling_id'][absent] == 0).all()


@pytest.mark.parametrize('ensure,index', LEVELS, ids=IDS)
def test_object_ids_are_the_games(ensure, index):
    """the ids are the game's: every object a move effect names is some side's floor or ceiling; a sector has one pair of ids on
    all its lines; no two sectors, and no floor and ceiling, share an object; and the lines account for every object the game
    numbers, so an id is 0 exactly on the sectors the game moves nothing of"""
    path, wad, world = _world(ensure, index)
    ml, t = world.map_lines(), world.triggers()
    m = mapcheck.Map(path, index)
    floor_of, ceil_of = {}, {}
    for line, rec in zip(ml, [m.linedefs[k] for k in ml['linedef']]):
        for name, col in (('front', 5), ('back', 6)):
            if line[name]['present']:
                s = m.side_sector(rec[col])
                assert floor_of.setdefault(s, int(line[name]['floor_id'])) == line[name]['floor_id']
                assert ceil_of.setdefault(s, int(line[name]['ceiling_id'])) == line[name]['ceiling_id']
    used = [v for v in list(floor_of.values()) + list(ceil_of.values()) if v]
    assert len(used) == len(set(used)) and all(0 < v < t['n_objects'] for v in used)
    assert set(int(o) for o in t['effects']['object_id']) <= set(used)
    assert set(used) == set(range(1, t['n_objects']))


def test_the_world_sets_tables_are_the_single_worlds():
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [2, 0, 7, 1]
    ws = wad.build_world_set(slots, device=False)
    for s, index in enumerate(slots):
        one = wad.build_world(index, device=False).map_lines()
        assert np.array_equal(ws.map_lines(s).view(np.uint8), one.view(np.uint8)), index
    with pytest.raises(rd.RdoomError):
        ws.map_lines(len(slots))
    a = rd.MapLines()
    assert rd.lib().rdoom_world_map_lines(None, ctypes.byref(a)) == -1
    assert rd.lib().rdoom_worldset_level_map_lines(ws._h, 0, None) == -1


def _census(path, index):
    """(one-sided, floor step, ceiling step, flat, closed) at rest, from mapcheck's MAP lumps alone"""
    m = mapcheck.Map(path, index)
    count = dict.fromkeys(('one', 'floor', 'ceil', 'flat', 'closed'), 0)
    for v1, v2, flags, _, _, right, left in m.linedefs:
        f, b = m.side_sector(right), m.side_sector(left)
        if f is None or b is None or flags & rd.LINE_SECRET:
            count['one'] += 1
            continue
        (ff, fc), (bf, bc) = m.sectors[f][:2], m.sectors[b][:2]
        key = 'closed' if fc <= ff or bc <= bf else ('floor' if ff != bf else ('ceil' if fc != bc else 'flat'))
        count[key] += 1
    return tuple(count[k] for k in ('one', 'floor', 'ceil', 'flat', 'closed'))


@pytest.mark.parametrize('index', range(9), ids=IDS[:9])
def test_the_census_of_line_classes(index):
    """the restatement's classes of the library's table, at rest, counted: equal to the count from the MAP lumps, to the figures
    the feature was specified with, and rich enough that a comparison of maps cannot pass on missing classes"""
    path, wad, world = _world(ensure_wad, index)
    cls = automap_ref.classes(world.map_lines())
    got = tuple(int((cls == c).sum()) for c in (rd.MAP_ONE_SIDED, rd.MAP_FLOOR_STEP, rd.MAP_CEILING_STEP, rd.MAP_FLAT, rd.MAP_CLOSED))
    assert got == _census(path, index)
    if index in CENSUS:
        assert got == CENSUS[index]
    assert (min(got) >= 1) == (index != 1), got  # every class on every level but E1M2, which has 9 linedefs
    assert not (world.map_lines()['flags'] & (rd.LINE_SECRET | rd.LINE_HIDDEN)).any()  # (hence the GPU test's patched copy)
    hidden = automap_ref.classes(world.map_lines(), show_flat=False)
    assert ((hidden == 0) == (cls == rd.MAP_FLAT)).all()


@pytest.mark.parametrize('ensure,index', [LEVELS[0], LEVELS[7], LEVELS[9]], ids=[IDS[0], IDS[7], IDS[9]])
def test_the_restatement_puts_every_linedef_where_the_map_has_it(ensure, index):
    """Without the library's drawing: a map at a scale that contains the level lights the pixel under every linedef's mid-point,
    whose image position is computed here from mapcheck's wad coordinates alone.  North-up: east is right, north is up, row 0 the
    bottom row (the top row with top_down).  Rotated at yaw 0 the forward (-z = +wad_x, east) is up, so south is right."""
    path, wad, world = _world(ensure, index)
    ml = world.map_lines()
    m = mapcheck.Map(path, index)
    ends = np.array([[m.vertices[l[0]], m.vertices[l[1]]] for l in m.linedefs])  # (n, 2, 2) wad x, y
    mid = ends.mean(1)
    lo, hi = ends.reshape(-1, 2).min(0), ends.reshape(-1, 2).max(0)
    centre = (lo + hi) / 2
    w, h = 200, 150
    scale = float(max((hi[0] - lo[0]) / (w - 8), (hi[1] - lo[1]) / (h - 8), (hi[1] - lo[1]) / (w - 8), (hi[0] - lo[0]) / (h - 8))) / 100.0
    st = rd.player_states([[-centre[1] / 100.0, 0.0, -centre[0] / 100.0]], [0.0])  # x = -wad_y / 100, z = -wad_x / 100
    east, north = (mid - centre)[:, 0] / 100.0 / scale, (mid - centre)[:, 1] / 100.0 / scale
    kw = dict(width=w, height=h, scale=scale, half_width=1.0, marker=0.0, show_flat=True, show_hidden=True)
    cases = [(dict(), east, north), (dict(top_down=True), east, -north), (dict(rotate=True), -north, east),
             (dict(rotate=True, top_down=True), -north, -east)]
    base = None
    for extra, right, up in cases:
        img = automap_ref.draw(ml, st, **kw, **extra)[0]
        col, row = np.floor(right + w / 2).astype(int), np.floor(up + h / 2).astype(int)
        assert (col >= 0).all() and (col < w).all() and (row >= 0).all() and (row < h).all()
        assert (img[row, col] != 0).all(), (extra, int((img[row, col] == 0).sum()))
        assert (img != 0).mean() < 0.75  # lines, not a filled image (the big level at this size: 0.51)
        if not extra:
            base = img
        elif extra == dict(top_down=True):
            assert np.array_equal(img, base[::-1])
    # the points themselves: pixel (i, j) of the north-up map lies (i + 0.5 - w / 2) * scale east and (j + 0.5 - h / 2) * scale north
    pts = mapcheck.world_to_map(automap_ref.points(st, **kw).reshape(-1, 2)).reshape(h, w, 2)
    ii, jj = np.meshgrid(np.arange(w), np.arange(h))
    assert np.allclose(pts[..., 0], centre[0] + (ii + 0.5 - w / 2) * scale * 100.0, atol=0.05)
    assert np.allclose(pts[..., 1], centre[1] + (jj + 0.5 - h / 2) * scale * 100.0, atol=0.05)


def test_the_marker_points_where_the_rays_go():
    """the marker's segment runs from the player along ray_fan's forward, (-sin yaw, -cos yaw) in world (x, z)"""
    lines = np.zeros(0, rd.MAP_LINE)
    for yaw in (0.0, 0.7, 2.0, -2.5):
        st = rd.player_states([[3.0, 0.0, -4.0]], [yaw])
        kw = dict(width=41, height=41, scale=0.1, marker=3.0)
        img = automap_ref.draw(lines, st, **kw)[0]
        assert set(np.unique(img)) == {0, rd.MAP_PLAYER}
        pts = automap_ref.points(st, **kw)[img == rd.MAP_PLAYER].astype(np.float64)
        mean = pts.mean(0) - [3.0, -4.0]
        want = np.array([-np.sin(yaw), -np.cos(yaw)]) * 0.3  # the middle of a segment of 2 * marker * scale
        assert np.allclose(mean, want, atol=0.03), (yaw, mean, want)
        turned = automap_ref.draw(lines, st, rotate=True, **kw)[0]
        rows, cols = np.nonzero(turned == rd.MAP_PLAYER)
        assert abs(cols.mean() - 20) < 0.51 and rows.mean() > 21  # straight up from the centre, whatever the yaw
