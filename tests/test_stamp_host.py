"""The solid things on the grid on the host, with no GPU: tests/stamp_ref.py (the header's "solid things on the grid" restated in
numpy) on hand cases whose expected cells are written out in tests/stamp_cases.py; the parameter record and both prototypes; every
argument error of rdoom_world_stamp_things and rdoom_worldset_stamp_things that is found before a handle is read, in the header's
order, on pointers that are never followed; the Python wrapper's refusals; the one-room levels the GPU tests stamp; and what the
issue measured on the synthetic E1M1, asserted on the restatements."""
import ctypes
import os
import re

import numpy as np
import pytest

import goal_ref
import rust_doom_amd as rd
import stamp_cases as sc
import stamp_ref

F = np.float32
U = np.uint32
BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.hand_cases()


def ref_of(case, **kw):
    """a hand case through the restatement: (floor, ceiling, index) of its one row"""
    floor, ceiling = sc.hand_planes(case)
    t_n = len(case['table'])
    solid = None if case['solid'] is None else sc.bit_rows([case['solid']])
    hidden = None if case['hidden'] is None else sc.bit_rows([case['hidden']])
    offsets = None if case['offsets'] is None else sc.hand_offsets(case)
    grow, below, above = case['window']
    assert t_n <= 32
    return (floor, ceiling) + stamp_ref.stamp(case['table'], sc.HAND_GRID, sc.HAND_CELL, floor, ceiling, solid=solid, hidden=hidden, offsets=offsets,
                                              grow=grow, block_below=below, block_above=above, **kw)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_ref_the_hand_cases(case):
    floor, ceiling, fo, co, index = ref_of(case)
    want = sc.hand_index(case)
    assert np.array_equal(index[0], want), (case['name'], index[0], want)
    wf, wc = sc.planes_of(floor, ceiling, want[None])
    assert np.array_equal(fo.view(U), wf.view(U)) and np.array_equal(co.view(U), wc.view(U))
    # every word nothing blocks is the input's, -0 and NaN payloads included
    free = index < 0
    assert np.array_equal(fo.view(U)[free], floor.view(U)[free]) and np.array_equal(co.view(U)[free], ceiling.view(U)[free])


def test_ref_the_words_that_pass_through():
    case = {c['name']: c for c in CASES}['-0 and a NaN payload pass through']
    floor, _, fo, _, index = ref_of(case)
    assert fo.view(U)[0, 0, 0] == 0x80000000 and fo.view(U)[0, 0, 1] == sc.PAYLOAD and fo.view(U)[0, 7, 7] == 0x80000000
    assert fo.view(U)[0, 6, 6] == 0x7F800000 and index[0, 6, 6] == 0


def test_ref_a_slot_out_of_range_and_the_cells_beyond_the_level_pass_through():
    case = CASES[1]  # the plus
    floor, ceiling = sc.hand_planes(case, shape=(11, 13))  # wider and taller than the level's 8 x 8
    floor, ceiling = np.repeat(floor, 3, 0), np.repeat(ceiling, 3, 0)
    far = sc.things_at([sc.at(9, 4), sc.at(3, 9)], radius=0.25)  # discs that reach beyond the grid's last column and row
    table = np.concatenate([case['table'], far])
    fo, co, index = stamp_ref.stamp([table], [sc.HAND_GRID], sc.HAND_CELL, floor, ceiling, levels=np.array([0, 1, 7], U))
    want = np.full((11, 13), -1, np.int32)
    want[:8, :8] = sc.hand_index(case)
    assert np.array_equal(index[0], want)  # (8, 4) and (3, 8) are outside the level's grid: passed through
    assert (index[1:] == -1).all() and np.array_equal(fo[1:].view(U), floor[1:].view(U)) and np.array_equal(co[1:].view(U), ceiling[1:].view(U))


def test_ref_the_own_cell_rule_is_needed_at_a_quarter():
    """the issue's measurement: at cell 0.25, 4 of E1M1's 7 barrels cover no cell centre with their disc"""
    host = sc.e1m1_wad().build_world(0, device=False)
    g, table = host.area_grid(0.25), host.map_things()
    xc, zc = goal_ref.centres(g, 0.25)
    none = 0
    for i in sc.E1M1_BARRELS:
        ex, ez = xc - F(table['x'][i]), zc - F(table['z'][i])
        r = F(table['radius'][i]) + F(0)
        none += not ((ex * ex)[None, :] + (ez * ez)[:, None] <= r * r).any()
    assert none == 4
    floor, ceiling = sc.flat(1, g)
    _, _, index = stamp_ref.stamp(table, g, 0.25, floor, ceiling, solid=rd.pack_things(host.thing_obstacles()).view(U)[None])
    assert sorted(set(index[index >= 0].tolist())) == list(sc.E1M1_BARRELS)  # each of the seven closes a cell all the same


def test_the_levels_the_gpu_tests_stamp():
    """the one-room levels have the grids asked of them; no level has a grid below 3 x 3 (a cell of margin on each side of the
    cells its lines touch), so that is the smallest the tests stamp"""
    wad = sc.room_wad(2, 2)
    host = wad.build_world(0, device=False)
    assert host.area_grid(sc.HAND_CELL) == sc.HAND_GRID and len(host.map_things()) == 0 and host.game_objects <= sc.HAND_OBJECTS
    tx, ty = rd.STAMP_TILE
    for gw, gh in ((67, 35), (130, 19), (tx - 1, ty), (tx, ty), (tx + 1, ty), (tx, ty - 1), (tx, ty + 1), (3, 3), (9, 7)):
        _, host, cell, grid = sc.room_of_grid(gw, gh)
        assert (grid.gw, grid.gh) == (gw, gh) and host.area_plane_shape(cell) == (gh, gw)


def test_the_e1m1_preconditions_on_the_restatements():
    """what the issue measured on the synthetic E1M1 at cell 0.125 with assets/meta/synth.toml"""
    c = sc.e1m1_case()
    assert tuple(np.nonzero(c['obstacles'])[0]) == sc.E1M1_BARRELS and (c['table']['radius'][list(sc.E1M1_BARRELS)] == F(0.1)).all()
    before, after = sc.open_cells(c['floor'], c['ceiling']), sc.open_cells(c['stamped'][0], c['stamped'][1])
    assert before[0].sum() == 25230 and (before[0] & ~after[0]).sum() == 14 and not (after & ~before).any()
    assert sc.open_cells(*c['plain'][0])[0].sum() == 21076 and sc.open_cells(*c['after'][0])[0].sum() == 20995
    assert c['plain'][1][1][0] == 17622 and c['after'][1][1][0] == 17550
    plain, stamped = c['plain'][1][0], c['after'][1][0]
    reached = stamped[0] != goal_ref.UNREACHED
    assert (stamped[0][reached] > plain[0][reached]).sum() == 98 and not (stamped[0][reached] < plain[0][reached]).any()
    # row 1 hides all seven: the unstamped pipeline word for word; row 2 hides thing 0 alone
    assert np.array_equal(c['stamped'][0][1].view(U), c['floor'][1].view(U)) and np.array_equal(stamped[1], plain[1])
    assert (c['stamped'][2][1] == -1).all() and 0 not in c['stamped'][2][2] and 0 in c['stamped'][2][0]
    assert c['stamped'][0][3].tobytes() != c['stamped'][0][0].tobytes()  # rng 25's offsets count
    for p in range(4):
        got = stamped[p] != goal_ref.UNREACHED
        assert not (got & (c['stamped'][2][p] >= 0)).any()  # no reached cell is a blocked one
        assert (plain[p][got] != goal_ref.UNREACHED).all() and (plain[p][got] <= stamped[p][got]).all()


# ---- the interface ----
PROTO_TAIL = ['uint32_t n', 'const float *d_object_offsets', 'uint32_t n_objects', 'float cell', 'uint32_t width', 'uint32_t height',
              'const uint32_t *d_solid', 'const uint32_t *d_hidden', 'uint32_t stride', 'const rdoom_stamp_params *params',
              'const float *d_floor', 'const float *d_ceiling', 'float *d_floor_out', 'float *d_ceiling_out', 'int32_t *d_index_out',
              'void *stream']


def test_the_record_and_both_prototypes():
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    for name, head in (('rdoom_world_stamp_things', ['const rdoom_world *world', 'const rdoom_thingset *things']),
                       ('rdoom_worldset_stamp_things', ['const rdoom_worldset *set', 'const rdoom_thingset *things', 'const uint32_t *d_levels'])):
        m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, header, flags=re.M)
        assert m and m.group(1).strip() == 'rdoom_status', name
        assert [' '.join(a.split()) for a in m.group(2).split(',')] == head + PROTO_TAIL, name
        assert name in rd.API_SYMBOLS and getattr(rd.lib(), name).restype is ctypes.c_int32
    m = re.search(r'typedef struct rdoom_stamp_params \{(.*?)\} rdoom_stamp_params;', header, flags=re.S)
    fields = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert [' '.join(f.split()) for f in fields.split(';') if f.strip()] == ['float grow', 'float block_below, block_above', 'uint32_t flags']
    assert ctypes.sizeof(rd.StampParams) == 16 == rd.STAMP_PARAMS.itemsize
    assert [rd.STAMP_PARAMS.fields[k][1] for k in ('grow', 'block_below', 'block_above', 'flags')] == [0, 4, 8, 12]
    assert [getattr(rd.StampParams, k).offset for k in ('grow', 'block_below', 'block_above', 'flags')] == [0, 4, 8, 12]
    assert len(rd.API_SYMBOLS) == 135 and len(set(rd.API_SYMBOLS)) == 135
    kernels = open(os.path.join(ROOT, 'rust-doom_amd', 'csrc', 'hip', 'kernels.hpp')).read()
    tile = re.search(r'constexpr uint32_t STAMP_TILE_X = (\d+), STAMP_TILE_Y = (\d+);', kernels)
    assert tile and (int(tile.group(1)), int(tile.group(2))) == tuple(rd.STAMP_TILE)


@pytest.mark.parametrize('form', ['world', 'worldset'])
def test_the_calls_check_their_arguments_before_they_read_a_handle(form):
    L = rd.lib()
    fake = lambda k: ctypes.c_void_p(0x10000000 * k)  # pointers 256 MiB apart, never followed
    inf, nan = float('inf'), float('nan')
    FLOOR, CEILING, FLOOR_OUT, CEILING_OUT, INDEX = (fake(k) for k in range(1, 6))

    def call(handle=None, things=None, lv=fake(9), n=4, cell=0.125, size=(160, 120), params=(0.0, inf, inf, 0), floor=FLOOR, ceiling=CEILING,
             floor_out=FLOOR_OUT, ceiling_out=CEILING_OUT, index=None):
        p = ctypes.byref(rd.StampParams(*params)) if params is not None else None
        tail = (n, None, 0, ctypes.c_float(cell), size[0], size[1], None, None, 0, p, floor, ceiling, floor_out, ceiling_out, index, None)
        if form == 'world':
            return L.rdoom_world_stamp_things(handle, things, *tail)
        return L.rdoom_worldset_stamp_things(handle, things, lv, *tail)

    def fails(word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    null_handle = 'null world set' if form == 'worldset' else 'null world'
    plane = 4 * 160 * 120 * 4
    for things in (None, fake(8)):  # none of them reads the handle (there is none) or the thing set (a pointer to nothing)
        fails('null params', things=things, params=None)
        for bad in ((nan, inf, inf, 0), (-0.5, inf, inf, 0), (inf, inf, inf, 0)):
            fails('grow', things=things, params=bad)
        for bad in ((0.0, nan, inf, 0), (0.0, -1.0, inf, 0), (0.0, inf, nan, 0), (0.0, inf, -0.25, 0), (0.0, -inf, inf, 0)):
            fails('vertical window', things=things, params=bad)
        fails('flags', things=things, params=(0.0, inf, inf, 1))
        fails('every output is null', things=things, floor_out=None, ceiling_out=None)
        fails('without the other', things=things, ceiling_out=None)
        fails('without the other', things=things, floor_out=None, index=INDEX)
        fails('null floor or ceiling', things=things, floor=None)
        fails('null floor or ceiling', things=things, ceiling=None)
        # the overlap rule: in place means both planes; every other meeting of an output with an input or an output is refused
        fails('overlaps an input', things=things, floor_out=FLOOR)
        fails('overlaps an input', things=things, ceiling_out=CEILING)
        fails('overlaps an input', things=things, floor_out=CEILING, ceiling_out=FLOOR)
        fails('overlaps an input', things=things, floor_out=ctypes.c_void_p(FLOOR.value + plane - 4))
        fails('overlaps an input', things=things, floor_out=ctypes.c_void_p(FLOOR.value - plane + 4))
        fails('overlaps an input', things=things, index=FLOOR)
        fails('overlap', things=things, floor_out=FLOOR, ceiling_out=CEILING, index=CEILING)  # an input's bytes and an output's at once
        fails('two outputs overlap', things=things, ceiling_out=FLOOR_OUT)
        fails('two outputs overlap', things=things, index=ctypes.c_void_p(CEILING_OUT.value + 4))
        fails('two outputs overlap', things=things, floor_out=FLOOR, ceiling_out=CEILING, index=ctypes.c_void_p(FLOOR.value + plane - 4))
        for size in ((0, 120), (160, 0)):
            fails('a side is 0', things=things, size=size)
        for size in ((8193, 120), (160, 8193)):
            fails('at most 8192', things=things, size=size)
        # what is left is the handle: planes that touch end to end, in place, the index alone and n == 0 with no plane are all in order
        fails(null_handle, things=things)
        fails(null_handle, things=things, floor_out=ctypes.c_void_p(FLOOR.value + plane), ceiling_out=ctypes.c_void_p(FLOOR.value - plane))
        fails(null_handle, things=things, floor_out=FLOOR, ceiling_out=CEILING, index=INDEX)
        fails(null_handle, things=things, floor_out=None, ceiling_out=None, index=INDEX)
        fails(null_handle, things=things, n=0, floor=None, ceiling=None, lv=None)
        fails(null_handle, things=things, params=(0.19, 0.0, 0.0, 0), cell=nan, size=(8192, 8))
        fails('overlaps an input', things=things, size=(8192, 8192), n=0xFFFFFFFF)  # planes of 2^60 bytes meet: no size overflows the check
    # ... in the order the header gives: each call below has the error named and every later one
    fails('null params', params=None, floor_out=None, ceiling_out=None, floor=None, size=(0, 9000))
    fails('grow', params=(nan, nan, nan, 1), floor_out=None, ceiling_out=None, floor=None, size=(0, 9000))
    fails('vertical window', params=(0.0, nan, nan, 1), floor_out=None, ceiling_out=None, floor=None, size=(0, 9000))
    fails('flags', params=(0.0, inf, inf, 1), floor_out=None, ceiling_out=None, floor=None, size=(0, 9000))
    fails('every output is null', floor_out=None, ceiling_out=None, floor=None, size=(0, 9000))
    fails('without the other', ceiling_out=None, floor=None, size=(0, 9000))
    fails('null floor or ceiling', floor=None, ceiling_out=FLOOR_OUT, size=(0, 9000))
    fails('two outputs overlap', ceiling_out=FLOOR_OUT, size=(8193, 8))
    fails('a side is 0', size=(0, 9000))
    fails('at most 8192', size=(160, 9000))


def test_the_python_wrapper_refuses_before_it_calls():
    torch = pytest.importorskip('torch')
    things = rd.DeviceThings.__new__(rd.DeviceThings)  # a set that was never created
    things._h, things.n_levels = ctypes.c_void_p(), 1
    world = rd.World.__new__(rd.World)
    world._h = ctypes.c_void_p()
    ws = rd.WorldSet.__new__(rd.WorldSet)
    ws._h = ctypes.c_void_p()
    host = torch.zeros((3, 8, 8), dtype=torch.float32)
    with pytest.raises(ValueError) as e:
        world.stamp_things(host, host, 'no set', 0.25)
    assert 'DeviceThings' in str(e.value)
    for call in (lambda *a, **k: world.stamp_things(*a, **k), lambda *a, **k: ws.stamp_things(None, *a, **k)):
        with pytest.raises(ValueError) as e:
            call(host, host, things, 0.25)  # planes live on the device
        assert 'on the GPU' in str(e.value)
        with pytest.raises(ValueError):
            call(0x1000, 0x2000, things, 0.25)  # the input planes are tensors: their shape is the call's
    if not torch.cuda.is_available():
        return
    floor = torch.zeros((3, 8, 8), dtype=torch.float32, device='cuda')
    ceiling = torch.ones_like(floor)
    rows = torch.zeros((3, 2), dtype=torch.int32, device='cuda')

    def refused(word, **kw):
        with pytest.raises(ValueError) as e:
            world.stamp_things(floor, ceiling, things, 0.25, **kw)
        assert word in str(e.value), e.value

    refused('hidden tensor has 2 rows', hidden=rows[:2])  # as set_hidden_things refuses a short tensor
    refused('solid tensor has 0 rows', solid=rows[:0])
    refused('32-bit integer', hidden=rows.float())
    refused('32-bit integer', hidden=rows.reshape(-1))
    refused('words long', hidden=rows, solid=torch.zeros((1, 3), dtype=torch.int32, device='cuda'))
    refused('stride is needed', hidden=0x3000)
    refused('n_objects is needed', offsets=0x3000)
    refused('offsets must be', offsets=torch.zeros((2, 4, 3), device='cuda'))
    refused('go together', floor_out=floor)
    refused('go together', floor_out=False)
    refused('nothing asked for', floor_out=False, ceiling_out=False)
    refused('index_out must be', index_out=torch.zeros((3, 8, 8), device='cuda'))
    refused('float32 tensor', floor_out=rows, ceiling_out=rows)
    refused('planes have 3 rows', n=4)
    with pytest.raises(rd.RdoomError) as e:  # with everything in order the library is reached, which has no world to read
        world.stamp_things(floor, ceiling, things, 0.25, hidden=rows, floor_out=floor, ceiling_out=ceiling, index_out=True)
    assert e.value.status == BAD and 'null world' in str(e.value)
