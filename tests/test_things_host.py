"""The things on the host, with no GPU: the thing table of every synthetic level against the THINGS lump and the metadata file, both
read here; against the visit_decor events of a walk of the same level; its sectors against the sector restatement; a set's slots;
tests/things_ref.py (the header's "Sensing" restated in numpy) on hand cases that are written out; the prototypes; and every
argument error of the create call and of both sense calls that is found before a thing set is read, on pointers that are never
followed."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import mapcheck
import rust_doom_amd as rd
import sector_ref
import things_ref
from util import META_PATH, ensure_wad

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKERS = (1, 2, 3, 4, 11, 14)
CATEGORY_ARRAYS = ('decorations', 'weapons', 'powerups', 'artifacts', 'ammo', 'keys', 'monsters')


def lump_things(level):
    """the THINGS lump of a level of the synthetic IWAD: (x, y, angle, type, flags) per entry, in lump order"""
    data, lumps = mapcheck.read_directory(ensure_wad())
    marker = mapcheck.level_markers(lumps)[level]
    _, pos, size = next(l for l in lumps[marker + 1:marker + 11] if l[0] == b'THINGS')
    assert size % 10 == 0
    return [struct.unpack_from('<hhhHH', data, pos + 10 * i) for i in range(size // 10)]


def metadata_things():
    """{thing_type: (category, hanging, radius)} of the metadata file's [[things.<array>]] tables, the first match of a type in the
    order the arrays are merged"""
    text = re.sub(r'#[^\n]*', '', open(META_PATH).read())
    found = {}
    for category, name in enumerate(CATEGORY_ARRAYS):
        for block in re.findall(r'\[\[things\.%s\]\]([^\[]*)' % name, text):
            kind = int(re.search(r'thing_type\s*=\s*(\d+)', block).group(1))
            hanging = re.search(r'hanging\s*=\s*(\w+)', block).group(1) == 'true'
            radius = int(re.search(r'radius\s*=\s*(\d+)', block).group(1))
            found.setdefault(kind, (category, hanging, radius))
    return found


class DecorEvents:
    def __init__(self):
        self.events = []

    def visit_decor(self, d):
        self.events.append((int(d.object_id), tuple(F(v) for v in d.low), tuple(F(v) for v in d.high)))


@pytest.fixture(scope='module')
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


@pytest.mark.parametrize('level', range(9))
def test_the_table_is_the_things_lump_and_the_metadata(wad, level):
    world = wad.build_world(level, device=False)
    table = world.map_things()
    assert table.dtype == rd.THING and rd.THING.itemsize == 32
    meta = metadata_things()
    assert meta[34][0] == rd.THING_AMMO == 4 and meta[63][1] and 9999 not in meta
    want = [e for e in lump_things(level) if e[3] not in MARKERS]
    assert len(table) == len(want) > 0  # count: on these levels every thing stands in a sector
    sectors = world.map_sectors().sectors
    for rec, (x, y, angle, kind, flags) in zip(table, want):  # order
        assert (rec['thing_type'], rec['flags'], rec['angle']) == (kind, flags, angle & 0xFFFF)
        assert rec['x'] == -(F(y) / F(100)) and rec['z'] == -(F(x) / F(100))  # from_wad_coords
        category, hanging, radius = meta.get(kind, (rd.THING_UNKNOWN, False, 0))
        assert rec['category'] == category | (rd.THING_HANGING if hanging else 0)
        assert rec['radius'] == F(radius) / F(100)
        sector = sectors[rec['sector']]
        assert rec['base'] == (sector['ceiling'] if hanging else sector['floor'])
        assert rec['object_id'] == (sector['ceiling_id'] if hanging else sector['floor_id'])
    kinds = table['thing_type']
    assert (table['category'][kinds == 34] == 4).all()
    assert (table['category'][kinds == 9999] == 7).all() and (table['radius'][kinds == 9999] == 0).all()
    hanging = table[kinds == 63]
    assert ((hanging['category'] & rd.THING_HANGING) != 0).all()
    assert np.array_equal(hanging['base'], sectors['ceiling'][hanging['sector']])
    # the sector is the one the sector contract finds at the thing's point: the things stand at cell centres
    at = sector_ref.sector_at(sector_ref.Tables(world), np.stack([table['x'], table['z']], 1))
    assert np.array_equal(at, table['sector'])


def test_level_one_holds_every_kind(wad):
    kinds = set(wad.build_world(0, device=False).map_things()['thing_type'].tolist())
    assert {34, 63, 9999, 2035} <= kinds


@pytest.mark.parametrize('level', range(9))
def test_every_decor_event_has_its_record(wad, level):
    table = wad.build_world(level, device=False).map_things()
    rec = DecorEvents()
    wad.walk(level, rec)
    assert rec.events
    at = 0
    for object_id, low, high in rec.events:  # in order: the walk and the table follow the lump
        while at < len(table) and not (table['x'][at] == low[0] and table['z'][at] == low[2] and table['object_id'][at] == object_id):
            at += 1
        assert at < len(table), (object_id, low)
        hanging = bool(table['category'][at] & rd.THING_HANGING)
        assert table['base'][at] == (high[1] if hanging else low[1])
        assert high[0] == low[0] and high[2] == low[2]
        at += 1


def test_a_sets_slot_gives_the_single_worlds_table(wad):
    slots = [0, 2, 7]
    ws = wad.build_world_set(slots, device=False)
    for s, index in enumerate(slots):
        assert ws.map_things(s).tobytes() == wad.build_world(index, device=False).map_things().tobytes()
    with pytest.raises(rd.RdoomError):
        ws.map_things(3)
    L = rd.lib()
    out = rd.MapThings()
    assert L.rdoom_world_map_things(None, ctypes.byref(out)) == BAD
    assert L.rdoom_worldset_level_map_things(ws._h, 0, None) == BAD


# ---- things_ref on hand cases ----
def one_sided(ax, az, bx, bz):
    line = np.zeros(1, rd.MAP_LINE)
    line['a'], line['b'] = (ax, az), (bx, bz)
    line['front']['present'], line['front']['ceiling'] = 1, 1.28
    return line


def things_at(points, category=0, radius=0.0, base=0.0):
    t = np.zeros(len(points), rd.THING)
    t['x'], t['z'] = np.asarray(points, F).T
    t['category'], t['radius'], t['base'] = category, radius, base
    return t


FAR_LINE = one_sided(100, 100, 101, 100)


def test_ref_a_thing_at_the_players_own_position():
    st = rd.player_states(F([[3.0, 0.0, -2.0]]), F([0.7]))
    table = things_at([(3.0, -2.0)], category=rd.THING_KEY)
    out = things_ref.sense(FAR_LINE, table, st, things_ref.params(5.0, fov=1.0))
    assert out['visible'][0, 0] == 1 and out['touched'][0, 0] == 1
    near = out['nearest'][0]
    assert near['index'][rd.THING_KEY] == 0 and near['d2'][rd.THING_KEY] == 0 and near['right'][rd.THING_KEY] == 0
    others = np.delete(near, rd.THING_KEY)
    assert (others['index'] == -1).all() and np.isposinf(others['d2']).all() and not others['right'].any() and not others['forward'].any()
    assert not out['new'].any() and not out['collected'].any()  # nothing is collected without a mask


def test_ref_of_two_equal_things_the_lower_index_wins():
    st = rd.player_states(F([[0.0, 0.0, 0.0]]), F([0.0]))
    table = things_at([(5.0, 5.0), (0.0, -2.0), (0.0, -2.0), (0.0, -1.0)], category=[1, 3, 3, 2])
    out = things_ref.sense(FAR_LINE, table, st, things_ref.params(10.0))
    assert out['visible'][0, 0] == 0b1111
    near = out['nearest'][0]
    assert near['index'][3] == 1 and near['d2'][3] == 4 and near['forward'][3] == 2 and near['right'][3] == 0  # yaw 0: forward is -z
    assert near['index'][2] == 3 and near['index'][1] == 0 and near['index'][0] == -1
    # behind a cone of 90 degrees about -z, thing 0 (at +x, +z) is out of view
    cone = things_ref.sense(FAR_LINE, table, st, things_ref.params(10.0, fov=np.pi / 2))
    assert cone['visible'][0, 0] == 0b1110 and cone['nearest'][0]['index'][1] == -1


def test_ref_a_thing_on_a_blocking_line_is_visible_and_one_a_hair_behind_is_not():
    line = one_sided(2.0, -1.0, 2.0, 1.0)
    st = rd.player_states(F([[0.0, 0.0, 0.0]]), F([0.0]))
    behind = np.nextafter(F(2.0), F(3.0))
    table = things_at([(2.0, 0.0), (behind, 0.0), (1.5, 0.0), (2.0, 1.0), (3.0, 2.0)])
    out = things_ref.sense(line, table, st, things_ref.params(10.0))
    # on the line (t == 1 leaves T at 1): seen; a hair behind: hidden; in front: seen; on the line's end point: seen; past the end: seen
    assert out['visible'][0, 0] == 0b11101
    assert out['nearest'][0]['index'][0] == 2
    # the same line with a back side and an opening does not block; shut (ceiling on the floor) it does
    open_line = line.copy()
    open_line['back']['present'], open_line['back']['ceiling'] = 1, 1.28
    assert things_ref.sense(open_line, table, st, things_ref.params(10.0))['visible'][0, 0] == 0b11111
    open_line['back']['ceiling'] = 0.0
    assert things_ref.sense(open_line, table, st, things_ref.params(10.0))['visible'][0, 0] == 0b11101
    # out of range: d2 <= max_range * max_range is the test, so a range of exactly 2 still holds the thing on the line
    assert things_ref.sense(line, table, st, things_ref.params(2.0))['visible'][0, 0] == 0b00101


def test_ref_the_vertical_window_from_either_side():
    table = things_at([(0.1, 0.0)], category=rd.THING_AMMO, radius=0.08, base=0.5)
    prm = things_ref.params(5.0, touch_below=0.75, touch_above=1.0, collect=(rd.THING_AMMO,))
    got = []
    step = 2.0 ** -10  # every height here is a binary fraction: the differences are exact
    for y in (0.5 - 0.75, 0.5 - 0.75 - step, 0.5 + 1.0, 0.5 + 1.0 + step, 0.5, np.nan):
        st = rd.player_states(F([[0.0, y, 0.0]]), F([0.0]))
        out = things_ref.sense(FAR_LINE, table, st, prm)
        assert out['visible'][0, 0] == 1  # the height plays no part in sight
        assert out['new'][0, rd.THING_AMMO] == out['touched'][0, 0] == out['collected'][0, 0]
        got.append(int(out['touched'][0, 0]))
    assert got == [1, 0, 1, 0, 1, 0]
    # the horizontal reach is touch_radius + radius; a lift that carries the thing carries the window
    st = rd.player_states(F([[0.0, 0.5, 0.0]]), F([0.0]))
    assert things_ref.sense(FAR_LINE, table, st, things_ref.params(5.0, touch_radius=0.01))['touched'][0, 0] == 0
    table['object_id'] = 2
    off = np.zeros((1, 3, 3), F)
    off[0, 2, 1] = 2.0
    assert things_ref.sense(FAR_LINE, table, st, prm, offsets=off)['touched'][0, 0] == 0
    st['pos'][0, 1] += 2.0
    assert things_ref.sense(FAR_LINE, table, st, prm, offsets=off)['touched'][0, 0] == 1
    # a collected thing is neither visible nor touched, and a NaN position sees and touches nothing
    gone = things_ref.sense(FAR_LINE, table, st, prm, offsets=off, collected=np.array([[1]], np.uint32))
    assert not gone['visible'].any() and not gone['touched'].any() and gone['collected'][0, 0] == 1 and gone['nearest'][0]['index'].max() == -1
    st['pos'][0, 0] = np.nan
    lost = things_ref.sense(FAR_LINE, table, st, prm, offsets=off)
    assert not lost['visible'].any() and not lost['touched'].any() and not lost['new'].any()


# ---- the interface ----
def prototype(name):
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, header, flags=re.M)
    assert m, name
    return m.group(1).strip(), [' '.join(a.split()) for a in m.group(2).split(',')]


def test_the_prototypes_argument_by_argument():
    sense = ['const rdoom_thingset *things', 'const rdoom_player_state *d_states', 'uint32_t n', 'const float *d_object_offsets',
             'uint32_t n_objects', 'const rdoom_thing_sense *params', 'uint32_t *d_collected', 'uint32_t *d_visible_out',
             'uint32_t *d_touched_out', 'uint32_t stride', 'rdoom_thing_nearest *d_nearest_out', 'uint32_t *d_new_out', 'void *stream']
    assert prototype('rdoom_world_sense_things') == ('rdoom_status', ['const rdoom_world *world'] + sense)
    assert prototype('rdoom_worldset_sense_things') == \
        ('rdoom_status', ['const rdoom_worldset *set'] + sense[:2] + ['const uint32_t *d_levels'] + sense[2:])
    assert prototype('rdoom_world_map_things') == ('rdoom_status', ['const rdoom_world *world', 'rdoom_map_things *out'])
    assert prototype('rdoom_worldset_level_map_things') == ('rdoom_status', ['const rdoom_worldset *set', 'uint32_t slot', 'rdoom_map_things *out'])
    assert prototype('rdoom_thingset_create') == \
        ('rdoom_status', ['const rdoom_thing *const *things', 'const uint32_t *counts', 'uint32_t n_levels', 'rdoom_thingset **out'])
    assert prototype('rdoom_thingset_destroy') == ('void', ['rdoom_thingset *set'])
    assert prototype('rdoom_thingset_info') == \
        ('rdoom_status', ['const rdoom_thingset *set', 'uint32_t *out_n_levels', 'uint32_t *out_words', 'uint32_t *out_max_object_id'])
    assert ctypes.sizeof(rd.ThingSense) == 28 and ctypes.sizeof(rd.MapThings) == 16
    assert rd.THING_NEAREST.itemsize == 16 and rd.THING.fields['category'][1] == 28 and rd.THING.fields['object_id'][1] == 16
    assert (rd.THING_DECORATION, rd.THING_WEAPON, rd.THING_POWERUP, rd.THING_ARTIFACT, rd.THING_AMMO, rd.THING_KEY, rd.THING_MONSTER,
            rd.THING_UNKNOWN, rd.THING_HANGING) == (0, 1, 2, 3, 4, 5, 6, 7, 0x100)
    row = np.array([0x80000001, 0x2], np.uint32)
    assert np.array_equal(np.nonzero(rd.unpack_things(row, 40))[0], [0, 31, 33])


def test_create_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)

    def create(tables, counts=None, n=None, out=h):
        arrays = [np.ascontiguousarray(t, rd.THING) if t is not None and not isinstance(t, ctypes.c_void_p) else t for t in tables]
        ptrs = (ctypes.c_void_p * max(1, len(arrays)))(*[a if a is None or isinstance(a, ctypes.c_void_p) else a.ctypes.data for a in arrays])
        cnt = (ctypes.c_uint32 * max(1, len(arrays)))(*(counts if counts is not None else [len(a) for a in arrays]))
        status = L.rdoom_thingset_create(ptrs, cnt, len(arrays) if n is None else n, ctypes.byref(out) if out is not None else None)
        assert not h.value
        return status

    good = things_at([(1.0, 2.0), (3.0, 4.0)], category=rd.THING_AMMO | rd.THING_HANGING, radius=0.1)
    assert create([good], n=0) == BAD
    assert create([good], out=None) == BAD
    assert L.rdoom_thingset_create(None, None, 1, ctypes.byref(h)) == BAD
    assert create([None], counts=[3]) == BAD  # a NULL table with a count
    assert create([fake], counts=[(1 << 20) + 1]) == BAD and 'at most' in L.rdoom_last_error().decode()  # (the table is not read)
    for field, value in (('category', 8), ('category', 0x200), ('category', 0x1FF), ('x', np.nan), ('z', np.inf), ('base', -np.inf),
                         ('radius', np.nan), ('radius', np.inf), ('radius', -0.5)):
        bad = good.copy()
        bad[field][1] = value
        assert create([good, bad]) == BAD, (field, value)
        assert 'level 1, thing 1' in L.rdoom_last_error().decode()
    assert L.rdoom_thingset_info(None, None, None, None) == BAD
    L.rdoom_thingset_destroy(None)  # nothing to do


def test_the_sense_calls_check_their_arguments_on_host_only_handles(wad):
    world, ws = wad.build_world(0, device=False), wad.build_world_set([0, 7], device=False)
    L = rd.lib()
    # the pointers are never followed, the thing set's among them: what needs the set is checked behind the device check of the
    # handle, which a host-only handle fails (tests/test_gpu_things.py has those errors)
    fake = ctypes.c_void_p(0x1000)
    inf, nan = float('inf'), float('nan')

    def sense(h=world, things=fake, st=fake, n=4, off=None, no=0, prm=(10.0, -1.0, 0.19, inf, inf, 0, 0), col=None, vis=fake, tch=None,
              stride=2, near=None, new=None, lv=fake):
        hp = h._h if h is not None else None
        p = ctypes.byref(rd.ThingSense(*prm)) if prm is not None else None
        if h is ws or (h is None and lv is not fake):
            return L.rdoom_worldset_sense_things(hp, things, st, lv, n, off, no, p, col, vis, tch, stride, near, new, None)
        return L.rdoom_world_sense_things(hp, things, st, n, off, no, p, col, vis, tch, stride, near, new, None)

    def fails(word, **kw):
        assert sense(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    for h in (world, ws):
        fails('null', h=h, things=None)
        fails('null', h=h, prm=None)
        fails('null', h=h, st=None)
        fails('output', h=h, vis=None)
        for r in (0.0, -1.0, inf, nan):
            fails('max_range', h=h, prm=(r, -1.0, 0.19, inf, inf, 0, 0))
        for c in (inf, -inf, nan):
            fails('cos_half_fov', h=h, prm=(10.0, c, 0.19, inf, inf, 0, 0))
        for t in (-0.1, inf, nan):
            fails('touch_radius', h=h, prm=(10.0, -1.0, t, inf, inf, 0, 0))
        for below, above in ((-1.0, 1.0), (1.0, -1.0), (nan, 1.0), (1.0, nan)):
            fails('window', h=h, prm=(10.0, -1.0, 0.19, below, above, 0, 0))
        fails('flags', h=h, prm=(10.0, -1.0, 0.19, inf, inf, 0, 1))
        fails('HOST_ONLY', h=h)  # all else in order: the handle has no device copy
        fails('HOST_ONLY', h=h, prm=(10.0, -3.0, 0.0, 0.0, 0.0, 0xFF, 0), col=fake, tch=fake, near=fake, new=fake)
        fails('HOST_ONLY', h=h, vis=None, new=fake)  # any one output will do
        fails('HOST_ONLY', h=h, n=0, st=None, lv=None)  # n == 0 needs no states and no levels, and the handle is still checked
    fails('null', h=ws, lv=None)
    assert sense(h=None) == BAD and sense(h=None, lv=None) == BAD
