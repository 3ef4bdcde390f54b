"""The rays that see things on the host, with no GPU: include/rdoom_rays.h against the Python mirror (the record, both prototypes,
the second symbol list); every argument error of rdoom_world_cast_rays_things and rdoom_worldset_cast_rays_things that is found
before a thing set is read, on host-only handles and pointers that are never followed; the Python wrapper's refusals; and
tests/raythings_ref.py (the header's contract restated in numpy) on its own: the hand cases of tests/raythings_cases.py, its rays
against rays_ref.cast's, and the binary32 restatement against the float64 model of the same lines."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import raythings_cases as rc
import raythings_ref as rt
import rays_ref
import rust_doom_amd as rd
import world_ref
from util import META_PATH, ensure_wad

F = np.float32
U = np.uint32
BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rdoom_rays.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'raythings_error.json')
PROTO_TAIL = ['const float *d_dirs', 'uint32_t n_rays', 'float max_range', 'const float *d_object_offsets', 'uint32_t n_objects',
              'const rdoom_ray_things *params', 'const uint32_t *d_select', 'const uint32_t *d_hidden', 'uint32_t stride',
              'const float *d_frac_in', 'float *d_frac_out', 'int32_t *d_thing_out', 'void *stream']


@pytest.fixture(scope='module')
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


def declared(path):
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(rdoom_[a-z0-9_]+)\s*\(', text)))


# ---- the header and its mirror ------------------------------------------------------------------------------------------------------
def test_the_header_the_record_and_both_prototypes():
    header = open(HEADER).read()
    assert re.search(r'^#include "rdoom.h"$', header, flags=re.M)
    for name, head in (('rdoom_world_cast_rays_things', ['const rdoom_world *world', 'const rdoom_thingset *things',
                                                         'const rdoom_player_state *d_states', 'uint32_t n']),
                       ('rdoom_worldset_cast_rays_things', ['const rdoom_worldset *set', 'const rdoom_thingset *things',
                                                            'const rdoom_player_state *d_states', 'const uint32_t *d_levels', 'uint32_t n'])):
        m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, header, flags=re.M)
        assert m and m.group(1).strip() == 'rdoom_status', name
        assert [' '.join(a.split()) for a in m.group(2).split(',')] == head + PROTO_TAIL, name
        assert getattr(rd.lib(), name).restype is ctypes.c_int32
    m = re.search(r'typedef struct rdoom_ray_things \{(.*?)\} rdoom_ray_things;', header, flags=re.S)
    fields = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert [' '.join(f.split()) for f in fields.split(';') if f.strip()] == ['float height[8]', 'float grow', 'uint32_t category_mask',
                                                                             'uint32_t flags']
    assert ctypes.sizeof(rd.RayThings) == 44 == rd.RAY_THINGS.itemsize
    names = ('height', 'grow', 'category_mask', 'flags')
    assert [rd.RAY_THINGS.fields[k][1] for k in names] == [0, 32, 36, 40] == [getattr(rd.RayThings, k).offset for k in names]
    assert rd.RAY_THINGS.fields['height'][0].shape == (8,) and rd.RayThings.height.size == 32


def test_the_second_symbol_list_is_the_new_header_and_the_first_is_untouched():
    assert declared(HEADER) == sorted(rd.RAY_API_SYMBOLS) and len(set(rd.RAY_API_SYMBOLS)) == 2
    assert not set(rd.RAY_API_SYMBOLS) & set(rd.API_SYMBOLS)
    lib = ctypes.CDLL(rd.LIB_PATH)
    assert all(hasattr(lib, n) for n in rd.RAY_API_SYMBOLS + rd.API_SYMBOLS)
    main = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert len(rd.API_SYMBOLS) == len(re.findall(r'^(?:rdoom_status|void|const char \*)\s*rdoom_\w+\(', main, flags=re.M)) == 135
    assert 'cast_rays_things' not in main
    # no new text of the documents quotes another number of entry points
    for doc, pattern in (('INTEGRATION.md', r'all (\d+)\s+entry points'), ('DESIGN.md', r'(\d+) C entry points')):
        assert all(int(x) == 135 for x in re.findall(pattern, open(os.path.join(ROOT, doc)).read())), doc
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    outside = text[:text.index('<!-- BEGIN GENERATED')] + text[text.index('<!-- END GENERATED'):]
    assert 'rdoom_rays.h' in outside
    for name in rd.RAY_API_SYMBOLS:
        assert re.search(r'pub fn %s\(' % name, outside), name


# ---- the errors ----------------------------------------------------------------------------------------------------------------------
def test_the_calls_check_their_arguments_on_host_only_handles(wad):
    world, ws = wad.build_world(0, device=False), wad.build_world_set([0, 7], device=False)
    L = rd.lib()
    fake = lambda k: ctypes.c_void_p(0x10000000 * k)  # pointers 256 MiB apart, never followed: the thing set's among them
    inf, nan = float('inf'), float('nan')
    THINGS, STATES, DIRS, LEVELS, FRAC, OUT, THING = (fake(k) for k in range(1, 8))
    good = ((0.5,) * 8, 0.0, 0xFF, 0)

    def call(h=world, things=THINGS, st=STATES, lv=LEVELS, n=4, dirs=DIRS, rays=64, rng=30.0, off=None, no=0, prm=good, sel=None, hid=None,
             stride=0, frac=FRAC, out=OUT, thing=THING):
        hp = h._h if h is not None else None
        p = ctypes.byref(rd.RayThings((ctypes.c_float * 8)(*prm[0]), *prm[1:])) if prm is not None else None
        tail = (dirs, rays, ctypes.c_float(rng), off, no, p, sel, hid, stride, frac, out, thing, None)
        if h is ws or (h is None and lv is not LEVELS):
            return L.rdoom_worldset_cast_rays_things(hp, things, st, lv, n, *tail)
        return L.rdoom_world_cast_rays_things(hp, things, st, n, *tail)

    def fails(word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    row = 4 * 64 * 4
    for h in (world, ws):
        fails('null thing set', h=h, things=None)
        fails('null thing set, params', h=h, prm=None)
        fails('ray directions', h=h, dirs=None)
        fails('null states', h=h, st=None)
        fails('fraction output', h=h, out=None)
        fails('n_rays is 0', h=h, rays=0)
        for r in (0.0, -1.0, inf, -inf, nan):
            fails('max_range', h=h, rng=r)
        for c in range(8):
            for bad in (nan, -0.5, -inf):
                fails('height[%d]' % c, h=h, prm=(tuple(bad if k == c else 0.5 for k in range(8)), 0.0, 0xFF, 0))
        for bad in (nan, -0.5, inf):
            fails('grow', h=h, prm=((0.5,) * 8, bad, 0xFF, 0))
        fails('flags', h=h, prm=((0.5,) * 8, 0.0, 0xFF, 1))
        for bad in (0x100, 0x80000001):
            fails('category_mask', h=h, prm=((0.5,) * 8, 0.0, bad, 0))
        fails('too many', h=h, n=1 << 16, rays=(1 << 15) + 1)
        fails('too many', h=h, n=0xFFFFFFFF, rays=0xFFFFFFFF)
        for shift in (4, row - 4, -4, 4 - row):
            fails('overlap in part', h=h, out=ctypes.c_void_p(FRAC.value + shift))
        # what is left is the handle, which has no device copy: +inf heights, a zero mask, in place, no input fractions, no indices,
        # fractions that touch end to end, 2^31 rays and n == 0 without states, levels or outputs are all in order
        fails('HOST_ONLY', h=h)
        fails('HOST_ONLY', h=h, prm=((inf,) * 8, 0.0, 0, 0))
        fails('HOST_ONLY', h=h, out=FRAC)
        fails('HOST_ONLY', h=h, frac=None, thing=None)
        fails('HOST_ONLY', h=h, out=ctypes.c_void_p(FRAC.value + row))
        fails('HOST_ONLY', h=h, out=ctypes.c_void_p(FRAC.value - row))
        fails('HOST_ONLY', h=h, n=1 << 16, rays=1 << 15, out=FRAC)
        fails('HOST_ONLY', h=h, n=0, st=None, lv=None, out=None)
        fails('HOST_ONLY', h=h, sel=fake(9), hid=fake(10), stride=0, off=fake(11), no=0)  # what reads the thing set comes behind
    fails('null states, levels', h=ws, lv=None)
    fails('null world set', h=None, lv=None, n=0)
    fails('null world', h=None)
    fails('null thing set', h=None, things=None, prm=None, rays=0)  # the free checks come first, in the header's order
    fails('n_rays', h=None, rays=0, rng=nan, prm=((nan,) * 8, nan, 0x100, 1))
    fails('max_range', h=None, rng=nan, prm=((nan,) * 8, nan, 0x100, 1))
    fails('height[0]', h=None, prm=((nan,) * 8, nan, 0x100, 1))
    fails('grow', h=None, prm=((0.0,) * 8, nan, 0x100, 1))
    fails('flags', h=None, prm=((0.0,) * 8, 0.0, 0x100, 1))
    fails('category_mask', h=None, prm=((0.0,) * 8, 0.0, 0x100, 0), n=0xFFFFFFFF)
    fails('too many', h=None, n=0xFFFFFFFF, out=ctypes.c_void_p(FRAC.value + 4))


def test_the_python_wrapper_refuses_before_it_calls():
    torch = pytest.importorskip('torch')
    things = rd.DeviceThings.__new__(rd.DeviceThings)  # a set that was never created
    things._h, things.n_levels = ctypes.c_void_p(), 1
    world = rd.World.__new__(rd.World)
    world._h = ctypes.c_void_p()
    ws = rd.WorldSet.__new__(rd.WorldSet)
    ws._h = ctypes.c_void_p()
    host = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(ValueError) as e:
        world.cast_rays_things(0x1000, 'no set', host, 10.0, n=2)
    assert 'DeviceThings' in str(e.value)
    for call in (lambda *a, **k: world.cast_rays_things(0x1000, *a, **k), lambda *a, **k: ws.cast_rays_things(0x1000, 0x2000, *a, **k)):
        with pytest.raises(ValueError) as e:
            call(things, host, 10.0, n=2)  # the directions live on the device
        assert 'on the GPU' in str(e.value)
    if not torch.cuda.is_available():
        return
    dirs = torch.zeros((4, 3), dtype=torch.float32, device='cuda')
    states = torch.zeros((3, rd.PLAYER_STATE.itemsize), dtype=torch.uint8, device='cuda')
    rows = torch.zeros((3, 2), dtype=torch.int32, device='cuda')
    frac = torch.zeros((3, 4), dtype=torch.float32, device='cuda')

    def refused(word, st=states, **kw):
        with pytest.raises(ValueError) as e:
            world.cast_rays_things(st, things, dirs, 10.0, **kw)
        assert word in str(e.value), e.value

    refused('n is needed', st=0x1000)
    refused('frac_out is needed', st=0x1000, n=3)
    refused('hidden tensor has 2 rows', hidden=rows[:2])
    refused('select tensor has 0 rows', select=rows[:0])
    refused('32-bit integer', hidden=rows.float())
    refused('words long', hidden=rows, select=torch.zeros((1, 3), dtype=torch.int32, device='cuda'))
    refused('stride is needed', hidden=0x3000)
    refused('n_objects is needed', offsets=0x3000)
    refused('offsets must be', offsets=torch.zeros((2, 4, 3), device='cuda'))
    refused('heights must be', heights=[0.5] * 7)
    refused('categories names', categories=[8])
    refused('frac must be', frac=rows)
    refused('frac_out must be', frac_out=rows)
    refused('thing_out must be', thing_out=frac)
    refused('at least 48 bytes', frac=frac[:2])
    with pytest.raises(rd.RdoomError) as e:  # with everything in order the library is reached, which has no world to read
        world.cast_rays_things(states, things, dirs, 10.0, heights=[0.5] * 8, categories=[rd.THING_KEY], hidden=rows, frac=frac, frac_out=frac,
                               thing_out=True)
    assert e.value.status == BAD and 'null thing set' in str(e.value)


# ---- the reference on its own --------------------------------------------------------------------------------------------------------
def test_ref_the_hand_cases():
    cases = rc.hand_cases()
    a = rc.assemble(cases)
    frac, thing = rt.cast(a['table'], a['states'], a['dirs'], rc.MAX_RANGE, heights=rc.HEIGHTS, categories=rc.CATEGORIES, select=a['select'],
                          hidden=a['hidden'], offsets=a['offsets'], frac=a['frac'])
    rc.check(a['want'], frac, thing)
    # a ray that names no thing keeps the world's word; one that names a thing is strictly nearer than the world
    none = thing < 0
    assert np.array_equal(frac.view(U)[none], a['frac'].view(U)[none])
    assert (frac[~none] < a['frac'][~none]).all()
    # the players stand where the cases say: the identity quaternion, the eye at y = 0
    origin, vel = rt.rays(a['states'], a['dirs'], rc.MAX_RANGE)
    sound = np.isfinite(origin).all(1)
    assert (origin[sound, 1] == 0).all() and np.array_equal(vel[0, :4].view(U), (rc.DIRS[:4] * F(rc.MAX_RANGE)).view(U))
    # without its refinements a case reads differently: the cases are about what they say
    plain, _ = rt.cast(a['table'], a['states'], a['dirs'], rc.MAX_RANGE, heights=rc.HEIGHTS, grow=0.5)
    names = [c['name'] for c in cases]
    for name in ('a thing that is not selected', 'a masked category', 'R == 0'):
        k = names.index(name)
        assert frac[k, rc.WEST] == np.inf and plain[k, rc.WEST] < 1, name


def test_ref_the_rays_are_cast_rays_own(wad):
    """raythings_ref.rays against the origin and vel of the ray-cast restatement on a real level, bit for bit"""
    ref = world_ref.RefWorld(wad, 0)
    states = rays_ref.players(wad.build_level(0), 33, count=40)
    for dirs, rng in ((rd.ray_fan(9, 2.0, pitch=0.1), 30.0), (rays_ref.odd_table(), 5.0)):
        want = rays_ref.cast(ref, states, dirs, rng)
        origin, vel = rt.rays(states, dirs, rng)
        assert np.array_equal(vel.view(U), want['vel'].view(U))
        assert np.array_equal(np.broadcast_to(origin[:, None, :], want['origin'].shape).view(U), want['origin'].view(U))


@pytest.fixture(scope='module')
def field():
    return rt.field_comparison()


def test_ref_binary32_against_the_float64_model(field):
    """the winning index agrees on at least 99 % of the rays (a sketch of these formulas disagreed on 0 of 25 600), and on those
    |t32 - t64| stays within four times what tests/golden/make_raythings_error.py recorded: the margin covers other numpy builds;
    the yardstick is the float64 model, never the kernel"""
    record = json.load(open(GOLDEN))
    assert record['field'] == rt.FIELD and record['rays'] == field['rays'] == 400 * 64
    print('agree %d of %d, hits %d, worst |t32 - t64| %.3g (recorded %.3g)' % (field['agree'], field['rays'], field['hits'], field['worst'],
                                                                              record['worst_abs_t']))
    assert field['agree'] >= 0.99 * field['rays']
    assert field['hits'] > 2000  # the field is dense enough to say something
    assert 0 < record['worst_abs_t'] < 1e-4  # the issue's sketch saw 1.9e-5
    assert field['worst'] <= 4 * record['worst_abs_t']


def test_ref_every_hit_point_lies_on_its_cylinder(field):
    """in float64, to the recorded tolerance times max_range: on the side within the height, or on a cap within the radius; an eye
    inside (t = 0) lies within both"""
    tol = 4 * json.load(open(GOLDEN))['worst_abs_t'] * rt.FIELD['max_range']
    table, heights = field['table'], field['heights'].astype(np.float64)
    p_i, r_i = np.nonzero(field['thing'] >= 0)
    i = field['thing'][p_i, r_i]
    t = field['t'][p_i, r_i]
    point = field['origin'][p_i].astype(np.float64) + t[:, None] * field['vel'][p_i, r_i].astype(np.float64)
    radial = np.hypot(point[:, 0] - table['x'][i].astype(np.float64), point[:, 2] - table['z'][i].astype(np.float64))
    big_r = table['radius'][i].astype(np.float64)
    h = heights[table['category'][i] & 0xFF]
    hanging = (table['category'][i] & rd.THING_HANGING) != 0
    y = table['base'][i].astype(np.float64)
    bottom, top = np.where(hanging, y - h, y), np.where(hanging, y, y + h)
    within_r, within_h = radial <= big_r + tol, (point[:, 1] >= bottom - tol) & (point[:, 1] <= top + tol)
    on_side = (np.abs(radial - big_r) <= tol) & within_h
    on_cap = ((np.abs(point[:, 1] - bottom) <= tol) | (np.abs(point[:, 1] - top) <= tol)) & within_r
    inside = (t == 0) & within_r & within_h
    assert len(i) == field['hits'] and (on_side | on_cap | inside).all(), int((~(on_side | on_cap | inside)).sum())
    assert on_side.sum() > 1000 and on_cap.sum() > 20  # both kinds occur
