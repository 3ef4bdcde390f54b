"""The thing maps on the host, with no GPU: tests/thingmap_ref.py (the header's "thing maps" restated in numpy) on hand cases whose
expected pixels are written out here; where a thing lands in the four orientations against mapcheck.world_to_map; the prototype;
every argument error of rdoom_thingset_draw_maps that is found before a thing set is read, on pointers that are never followed; and
the Python wrapper's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import mapcheck
import rust_doom_amd as rd
import thingmap_ref

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = thingmap_ref.view_of(8, 6, 0.5)  # pixel (i, j) is the world point (pos.x - (j - 2.5) / 2, pos.z - (i - 3.5) / 2), row = j
KEY, AMMO, DECOR = rd.MAP_THING + rd.THING_KEY, rd.MAP_THING + rd.THING_AMMO, rd.MAP_THING + rd.THING_DECORATION


def things_at(points, category=0, radius=0.0):
    t = np.zeros(len(points), rd.THING)
    t['x'], t['z'] = np.asarray(points, F).reshape(-1, 2).T
    t['category'], t['radius'] = category, radius
    return t


def player(x=3.0, z=-2.0, yaw=0.0):
    return rd.player_states(F([[x, 0.0, z]]), F([yaw]))


def one(table, state=None, **kw):
    out, index, covers = thingmap_ref.draw(table, player() if state is None else state, VIEW, **kw)
    return out[0], index[0], covers[0][0]


def centre(value):
    """an 8 x 6 plane that holds `value` in the four pixels around the centre and nothing elsewhere"""
    want = np.zeros((6, 8), np.int64)
    want[2:4, 3:5] = value
    return want


def test_ref_a_thing_at_the_players_position_marks_the_centre_pixels():
    # the four pixel centres around the player lie 0.25 * sqrt 2 = 0.354 away, the next ring at least 0.79; min_radius 1 is 0.5 units
    out, index, cover = one(things_at([(3.0, -2.0)], category=rd.THING_KEY), min_radius=1.0)
    assert np.array_equal(out, centre(KEY)) and np.array_equal(index, centre(1) - 1) and np.array_equal(cover, centre(1))
    # the thing's own radius where it is the larger: 0.8 units reach the ring at 0.79 (eight more pixels), not the corners at 1.06
    out, index, _ = one(things_at([(3.0, -2.0)], category=rd.THING_KEY, radius=0.8), min_radius=1.0)
    want = np.zeros((6, 8), np.int64)
    want[2:4, 2:6] = want[1:5, 3:5] = KEY
    assert np.array_equal(out, want) and np.array_equal(index >= 0, want > 0)


def test_ref_the_larger_code_wins_and_among_equal_codes_the_lower_index():
    here = [(3.0, -2.0), (3.0, -2.0)]
    out, index, cover = one(things_at(here, category=[rd.THING_AMMO, rd.THING_KEY]), min_radius=1.0)
    assert np.array_equal(out, centre(KEY)) and np.array_equal(index, centre(2) - 1) and np.array_equal(cover, centre(2))
    out, index, _ = one(things_at(here, category=[rd.THING_KEY, rd.THING_AMMO]), min_radius=1.0)
    assert np.array_equal(out, centre(KEY)) and np.array_equal(index, centre(1) - 1)
    out, index, _ = one(things_at(here, category=rd.THING_AMMO), min_radius=1.0)
    assert np.array_equal(out, centre(AMMO)) and np.array_equal(index, centre(1) - 1)
    # a caller's codes decide, not the categories: ammo above keys, and two categories on one code fall back to the index
    codes = [1, 1, 1, 1, 9, 3, 1, 1]
    out, index, _ = one(things_at(here, category=[rd.THING_KEY, rd.THING_AMMO]), min_radius=1.0, codes=codes)
    assert np.array_equal(out, centre(9)) and np.array_equal(index, centre(2) - 1)
    out, index, _ = one(things_at(here, category=[rd.THING_MONSTER, rd.THING_WEAPON]), min_radius=1.0, codes=codes)
    assert np.array_equal(out, centre(1)) and np.array_equal(index, centre(1) - 1)


def test_ref_what_is_not_drawn():
    table = things_at([(3.0, -2.0), (3.0, -2.0)], category=[rd.THING_AMMO, rd.THING_KEY])
    codes = list(thingmap_ref.DEFAULT_CODES)
    codes[rd.THING_KEY] = 0  # a code of 0 removes the category: the candle below shows
    out, index, _ = one(table, min_radius=1.0, codes=codes)
    assert np.array_equal(out, centre(AMMO)) and np.array_equal(index, centre(1) - 1)
    bit = lambda *i: np.array([[sum(1 << k for k in i)]], np.uint32)
    out, index, _ = one(table, min_radius=1.0, hidden=bit(1))  # hidden
    assert np.array_equal(out, centre(AMMO)) and np.array_equal(index, centre(1) - 1)
    out, index, _ = one(table, min_radius=1.0, known=bit(0))  # not known
    assert np.array_equal(out, centre(AMMO)) and np.array_equal(index, centre(1) - 1)
    out, index, _ = one(table, min_radius=1.0, hidden=bit(1), known=bit(0, 1))  # hidden and known
    assert np.array_equal(out, centre(AMMO)) and np.array_equal(index, centre(1) - 1)
    out, index, cover = one(table, min_radius=1.0, hidden=bit(0, 1), known=bit(0, 1))
    assert not out.any() and (index == -1).all() and not cover.any()
    out, index, _ = one(table, min_radius=1.0, known=bit())
    assert not out.any() and (index == -1).all()
    # with RDOOM_THING_MARKS_OVER the bytes nothing covers are the caller's; the index plane is whole all the same
    before = np.full((1, 6, 8), 0xAA, np.uint8)
    out, index, _ = one(table, min_radius=1.0, over=before)
    assert np.array_equal(out, np.where(centre(1) > 0, KEY, 0xAA)) and np.array_equal(index, centre(2) - 1)


def test_ref_the_radius_at_its_two_ends():
    # no radius at all: ex * ex + ez * ez <= 0 holds for no pixel centre, the thing being between them
    out, index, _ = one(things_at([(3.0, -2.0)]), min_radius=0.0)
    assert not out.any() and (index == -1).all()
    # ... and for the one it is on
    out, index, _ = one(things_at([(3.25, -1.75)]), min_radius=0.0)
    assert np.array_equal(np.argwhere(out), [[2, 3]]) and out[2, 3] == DECOR and index[2, 3] == 0
    # a radius whose square overflows covers every pixel, wherever the thing is
    with np.errstate(over='ignore'):
        assert F(3e19) * F(3e19) == np.inf
    for at in ((3.0, -2.0), (-1e30, 2e30)):
        out, index, _ = one(things_at([at], radius=3e19), min_radius=0.0)
        assert (out == DECOR).all() and (index == 0).all()


def test_ref_a_nan_player_and_a_slot_out_of_range_get_empty_maps():
    table = things_at([(3.0, -2.0)], radius=3e19)
    for x, z in ((np.nan, -2.0), (3.0, np.nan)):
        out, index, _ = one(table, state=player(x, z), min_radius=1.0)
        assert not out.any() and (index == -1).all()
    states = np.concatenate([player(), player()])
    out, index, _ = thingmap_ref.draw([table], states, VIEW, levels=np.array([0, 1], np.uint32), min_radius=1.0)
    assert (out[0] == DECOR).all() and not out[1].any() and (index[1] == -1).all()
    poison = np.full((2, 6, 8), 0xAA, np.uint8)
    out, _, _ = thingmap_ref.draw([table], states, VIEW, levels=np.array([0, 7], np.uint32), min_radius=1.0, over=poison)
    assert (out[0] == DECOR).all() and (out[1] == 0xAA).all()


@pytest.mark.parametrize('rotate', [False, True])
@pytest.mark.parametrize('top_down', [False, True])
def test_ref_where_a_thing_lands_in_the_four_orientations(rotate, top_down):
    """in map units (mapcheck.world_to_map: east = wad x, north = wad y): north-up, east is right and north is up; rotated, the
    player's forward (-sin yaw, -cos yaw) is up and (cos yaw, -sin yaw) is right.  A thing placed, in float64, on the centre of
    pixel (i, j) with a radius of 0.6 pixels marks that pixel and no other"""
    w, h, scale, yaw = 21, 15, 0.25, 0.9
    view = thingmap_ref.view_of(w, h, scale, rotate=rotate, top_down=top_down)
    st = player(7.5, -12.25, yaw)
    here = mapcheck.world_to_map([[7.5, -12.25]])[0]
    if rotate:
        right = mapcheck.world_to_map([[np.cos(yaw), -np.sin(yaw)]])[0] / 100.0
        up = mapcheck.world_to_map([[-np.sin(yaw), -np.cos(yaw)]])[0] / 100.0
    else:
        right, up = np.array([1.0, 0.0]), np.array([0.0, 1.0])
    assert abs(np.dot(right, up)) < 1e-12 and abs(right[0] * up[1] - right[1] * up[0] - 1.0) < 1e-12  # up is right turned left
    for i, j in ((0, 0), (20, 14), (3, 11), (17, 2), (10, 7)):
        at = here + ((i + 0.5 - w / 2) * right + (j + 0.5 - h / 2) * up) * scale * 100.0  # map units
        world = (-at[1] / 100.0, -at[0] / 100.0)
        assert np.allclose(mapcheck.world_to_map([world])[0], at)
        out, index, _ = thingmap_ref.draw(things_at([world], category=rd.THING_KEY), st, view, min_radius=0.6)
        row = h - 1 - j if top_down else j
        assert np.array_equal(np.argwhere(out[0]), [[row, i]]) and out[0, row, i] == KEY and index[0, row, i] == 0, (i, j)


# ---- the interface ----
def test_the_prototype_argument_by_argument():
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    m = re.search(r'^(\w[\w \*]*?)\s*\brdoom_thingset_draw_maps\(([^;]*)\);', header, flags=re.M)
    assert m and m.group(1).strip() == 'rdoom_status'
    assert [' '.join(a.split()) for a in m.group(2).split(',')] == [
        'const rdoom_thingset *things', 'const rdoom_player_state *d_states', 'const uint32_t *d_levels', 'uint32_t n',
        'const rdoom_map_view *view', 'const rdoom_thing_marks *marks', 'const uint32_t *d_hidden', 'const uint32_t *d_known',
        'uint32_t stride', 'uint8_t *d_out', 'int32_t *d_index_out', 'void *stream']
    assert re.search(r'^#define RDOOM_MAP_THING 16u', header, flags=re.M) and rd.MAP_THING == 16
    assert re.search(r'^#define RDOOM_THING_MARKS_OVER 1u', header, flags=re.M) and rd.THING_MARKS_OVER == 1
    assert ctypes.sizeof(rd.ThingMarks) == 16 == rd.THING_MARKS.itemsize
    assert [rd.THING_MARKS.fields[k][1] for k in ('min_radius', 'codes', 'flags')] == [0, 4, 12]
    assert (rd.ThingMarks.min_radius.offset, rd.ThingMarks.codes.offset, rd.ThingMarks.flags.offset) == (0, 4, 12)
    assert 'rdoom_thingset_draw_maps' in rd.API_SYMBOLS and rd.lib().rdoom_thingset_draw_maps.restype is ctypes.c_int32
    assert rd.MAP_THING > max(rd.MAP_ONE_SIDED, rd.MAP_PLAYER)
    colors = rd.THING_MAP_COLORS
    assert colors.shape == (24, 3) and colors.dtype == np.uint8 and np.array_equal(colors[:16], rd.MAP_COLORS[:16])
    assert len({tuple(c) for c in colors[16:]}) == 8 and colors[16:].any(1).all()


def test_the_call_checks_its_arguments_before_it_reads_a_set():
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)
    inf, nan = float('inf'), float('nan')

    def call(things=None, st=fake, lv=fake, n=4, view=(160, 120, 0.12, 0.0, 0.0, 0), marks=(2.0, 0), hidden=None, known=None, stride=0,
             out=fake, index=None):
        v = ctypes.byref(rd.MapView(*view)) if view is not None else None
        m = ctypes.byref(rd.ThingMarks(marks[0], (ctypes.c_uint8 * 8)(*range(16, 24)), marks[1])) if marks is not None else None
        return L.rdoom_thingset_draw_maps(things, st, lv, n, v, m, hidden, known, stride, out, index, None)

    def fails(word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    # every one of them is found with a set that is never read (`things` is a pointer to nothing) ...
    for things in (None, fake):
        fails('null view', things=things, view=None)
        fails('null view or marks', things=things, marks=None)
        fails('null states', things=things, st=None)
        fails('both outputs', things=things, out=None)
        for w, h in ((0, 120), (160, 0), (16385, 120), (160, 16385)):
            fails('pixels', things=things, view=(w, h, 0.12, 0.0, 0.0, 0))
        for s in (0.0, -1.0, inf, nan):
            fails('scale', things=things, view=(160, 120, s, 0.0, 0.0, 0))
        fails('map flags', things=things, view=(160, 120, 0.12, 0.0, 0.0, 16))
        for r in (-0.5, inf, -inf, nan):
            fails('min_radius', things=things, marks=(r, 0))
        fails('mark flags', things=things, marks=(2.0, 2))
        fails('too many', things=things, n=1 << 27, view=(160, 120, 0.12, 0.0, 0.0, 0))  # 2^27 x 20 tiles
    # ... in the order the header gives: each call below has the error named and every later one
    fails('null view', view=None, st=None, out=None, marks=(nan, 2))
    fails('null states', st=None, out=None, view=(0, 0, nan, 0.0, 0.0, 16), marks=(nan, 2))
    fails('both outputs', out=None, view=(0, 0, nan, 0.0, 0.0, 16), marks=(nan, 2))
    fails('pixels', view=(0, 0, nan, 0.0, 0.0, 16), marks=(nan, 2))
    fails('scale', view=(160, 120, nan, 0.0, 0.0, 16), marks=(nan, 2))
    fails('map flags', view=(160, 120, 0.12, 0.0, 0.0, 16), marks=(nan, 2))
    fails('min_radius', marks=(nan, 2), n=1 << 27)
    fails('mark flags', marks=(2.0, 2), n=1 << 27)
    fails('too many', n=1 << 27)
    # with all of that in order the missing set is what is left; what the call does not read of a view may be anything
    fails('null thing set')
    fails('null thing set', view=(77, 53, 0.05, nan, -1.0, 15), marks=(0.0, 1), index=fake, out=None)
    fails('null thing set', n=0, st=None, lv=None)  # n == 0 needs no states; the set is still checked
    fails('null thing set', n=(1 << 31) // 20, view=(160, 120, 0.12, 0.0, 0.0, 0))  # 2^31 - 1 tiles at the most: this many fit


def test_the_python_wrapper_refuses_before_it_calls():
    torch = pytest.importorskip('torch')
    things = rd.DeviceThings.__new__(rd.DeviceThings)  # a set that was never created: the library refuses it, and is reached last
    things._h = ctypes.c_void_p()
    states = torch.zeros((3, 10), dtype=torch.float32)
    rows = torch.zeros((3, 2), dtype=torch.int32)

    def refused(word, *args, **kw):
        with pytest.raises(ValueError) as e:
            things.draw_maps(*args, **kw)
        assert word in str(e.value), e.value

    refused('n is needed', 0x1000, 160, 120, 0.12, out=0x2000)
    refused('1 x 1', states, 0, 120, 0.12)
    refused('eight bytes', states, 160, 120, 0.12, codes=[16, 17, 18])
    refused('eight bytes', states, 160, 120, 0.12, codes=[16, 17, 18, 19, 20, 21, 22, 256])
    refused('stride is needed', 0x1000, 160, 120, 0.12, n=3, out=0x2000, hidden=0x3000)
    refused('stride is needed', 0x1000, 160, 120, 0.12, n=3, out=0x2000, known=0x3000)
    refused('hidden tensor has 2 rows', states, 160, 120, 0.12, hidden=rows[:2])  # as set_hidden_things refuses a short tensor
    refused('known tensor has 2 rows', states, 160, 120, 0.12, known=rows[:2])
    refused('32-bit integer', states, 160, 120, 0.12, hidden=rows.float())
    refused('32-bit integer', states, 160, 120, 0.12, known=rows.reshape(-1))
    refused('words long', states, 160, 120, 0.12, hidden=rows, known=torch.zeros((3, 3), dtype=torch.int32))
    refused('one 32-bit slot', states, 160, 120, 0.12, levels=torch.zeros(2, dtype=torch.int32))
    refused('over=True', states, 160, 120, 0.12, over=True)
    refused('out is needed', 0x1000, 160, 120, 0.12, n=3)
    refused('index_out must be a tensor', 0x1000, 160, 120, 0.12, n=3, out=0x2000, index_out=True)
    refused('bytes', states, 160, 120, 0.12, out=torch.zeros((3, 120, 160), dtype=torch.int32))
    refused('32-bit integers', states, 160, 120, 0.12, out=False, index_out=torch.zeros((3, 120, 160), dtype=torch.float32))
    refused('GPU tensor', states, 160, 120, 0.12, out=torch.zeros((3, 120, 160), dtype=torch.uint8))  # tensors live on the device
    world = rd.World.__new__(rd.World)
    with pytest.raises(ValueError):
        world.draw_thing_maps(states, 'no set', 160, 120, 0.12)
    with pytest.raises(ValueError):
        rd.WorldSet.__new__(rd.WorldSet).draw_thing_maps(states, None, 'no set', 160, 120, 0.12)
    # raw pointers with everything in order reach the library, which has no set to draw
    with pytest.raises(rd.RdoomError) as e:
        things.draw_maps(0x1000, 160, 120, 0.12, n=3, out=0x2000, hidden=0x3000, stride=2, index_out=0x4000, levels=0x5000)
    assert e.value.status == BAD and 'null thing set' in str(e.value)
