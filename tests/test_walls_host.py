"""The wall distance on the host, with no GPU: the surface -- header, exported symbol, the Python names and constants -- the two
statements of the reference (tests/walls_ref.py) against each other on random grids and against distances written out by hand,
wall_close_d2 and the radius a launch derives from it, and every argument error of rdoom_wall_distance on pointers that are never
followed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import flood_ref
import rust_doom_amd as rd
import walls_ref
from util import ROOT

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
CASES = walls_ref.hand_cases()


# ---- the surface -------------------------------------------------------------------------------------------------------------------

def test_the_library_and_the_package_export_the_wall_distance():
    L = ctypes.CDLL(rd.LIB_PATH)
    assert hasattr(L, 'rdoom_wall_distance') and 'rdoom_wall_distance' in rd.API_SYMBOLS
    assert rd.lib().rdoom_wall_distance.restype is ctypes.c_int32
    assert rd.WALL_FAR == 0xFFFF == walls_ref.FAR and rd.WALL_MAX_RADIUS == 32 == walls_ref.MAX_RADIUS and rd.WALL_EDGE_OPEN == 1
    assert ctypes.sizeof(rd.WallParams) == 16 and [f[0] for f in rd.WallParams._fields_] == ['clearance', 'radius', 'close_d2', 'flags']
    assert list(inspect.signature(rd.wall_distances).parameters) == ['floor', 'ceiling', 'radius_cells', 'clearance', 'edge_open', 'dist2_out',
                                                                     'stream']
    assert list(inspect.signature(rd.inflate_grids).parameters) == ['floor', 'ceiling', 'radius', 'cell', 'clearance', 'edge_open', 'floor_out',
                                                                    'ceiling_out', 'dist2_out', 'stream']
    for fn in (rd.wall_distances, rd.inflate_grids):
        d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
        assert (d['clearance'], d['edge_open'], d['dist2_out'], d['stream']) == (0.56, False, None, None)


def test_the_header_declares_the_wall_distance_and_the_tile_is_the_kernel_s():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- wall distance:' in text and '(DESIGN section 25)' in text
    for words in ('#define RDOOM_WALL_FAR 0xFFFFu', '#define RDOOM_WALL_MAX_RADIUS 32u', '#define RDOOM_WALL_EDGE_OPEN 1u',
                  'Ledges are not\n * inflated', 'point\n * sample per cell', 'n == 0 queues nothing', 'there is no in-place form'):
        assert words in text, words
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    proto = re.search(r'rdoom_status rdoom_wall_distance\((.*?)\);', code, flags=re.S).group(1)
    assert [' '.join(a.split()) for a in proto.split(',')] == [
        'const float *d_floor', 'const float *d_ceiling', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'const rdoom_wall_params *params',
        'uint16_t *d_dist2_out', 'float *d_floor_out', 'float *d_ceiling_out', 'void *stream']
    struct = re.search(r'typedef struct rdoom_wall_params \{(.*?)\}', code, flags=re.S).group(1)
    assert [' '.join(a.split()) for a in struct.split(';') if a.strip()] == ['float clearance', 'uint32_t radius', 'uint32_t close_d2',
                                                                            'uint32_t flags']
    kernels = open(os.path.join(ROOT, 'rust-doom_amd', 'csrc', 'hip', 'kernels.hpp')).read()
    tile = re.search(r'constexpr uint32_t WALL_TILE_X = (\d+), WALL_TILE_Y = (\d+);', kernels)
    assert tile and (int(tile.group(1)), int(tile.group(2))) == tuple(rd.WALL_TILE)


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def test_the_two_statements_of_the_reference_agree_on_random_grids():
    rng = np.random.default_rng(25)
    radii = (1, 2, 3, 5, 32)
    seen = set()
    for k in range(200):
        w, h = (1, 1) if k == 0 else (int(rng.integers(1, 41)), int(rng.integers(1, 41)))
        share = rng.uniform(0.3, 0.95)
        is_open = rng.random((h, w)) < share
        f, g = flood_ref.room(w, h)
        g[~is_open] = F(0.5)
        assert np.array_equal(flood_ref.open_cells(f, g, 0.56), is_open)
        R, edge = radii[k % 5], bool((k // 5) % 2)
        a, b = walls_ref.brute(f, g, R, edge_open=edge), walls_ref.capped(f, g, R, edge_open=edge)
        assert a.dtype == b.dtype == np.uint16 and a.shape == (h, w)
        assert np.array_equal(a, b), (k, w, h, R, edge)
        assert ((a == 0) == ~is_open).all() and ((a <= R * R) | (a == walls_ref.FAR)).all()
        seen.add((R, edge))
    assert len(seen) == 10


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_reference_on_grids_written_out_by_hand(case):
    for fn in (walls_ref.brute, walls_ref.capped):
        got = fn(case['floor'], case['ceiling'], case['radius'], edge_open=case['edge_open'])
        assert np.array_equal(got, case['want']), (case['name'], fn.__name__, got.tolist())


def test_the_hand_cases_cover_what_they_are_there_for():
    by = {c['name']: c for c in CASES}
    X = walls_ref.FAR
    assert by['1x1 open']['want'].tolist() == [[1]] and by['1x1 open, edge open']['want'].tolist() == [[X]]
    assert by['1x1 closed']['want'].tolist() == [[0]] and by['1x1 closed, edge open']['want'].tolist() == [[0]]
    disc = by['7x7 centre closed, edge open, R 2']['want']
    assert sorted(set(disc.reshape(-1).tolist())) == [0, 1, 2, 4, X] and (disc[[0, -1]] == X).all() and (disc[:, [0, -1]] == X).all()
    assert disc[1, 1] == disc[1, 2] == X  # D2 = 8 and 5: inside the square window, outside the disc
    ring = by['7x7 centre closed, R 2']['want']
    assert (ring[[0, -1]] == 1).all() and (ring[:, [0, -1]] == 1).all() and np.array_equal(ring[2:5, 2:5], disc[2:5, 2:5])
    assert np.isnan(by['7x7 centre NaN, edge open, R 2']['floor'][3, 3])
    assert np.array_equal(by['7x7 centre NaN, edge open, R 2']['want'], disc)


def test_the_plane_rule_keeps_every_word_it_does_not_close():
    f = np.array([[0.0, -0.0, np.nan, 1.0, 0.25]], F)
    g = np.array([[1.0, 1.0, 1.0, 2.0, 0.25]], F)  # a NaN floor, and a door: a finite floor with the ceiling on it
    f.view(np.uint32)[0, 2] = 0x7FC12345  # the NaN's payload
    d2 = walls_ref.brute(f, g, 1, edge_open=True)
    assert d2.tolist() == [[walls_ref.FAR, 1, 0, 1, 0]]
    fo, go = walls_ref.inflate(f, g, d2, 0)
    assert fo.view(np.uint32).tolist() == [[0, 0x80000000, 0x7F800000, 0x3F800000, 0x7F800000]]
    assert go.view(np.uint32).tolist() == [[0x3F800000, 0x3F800000, 0xFF800000, 0x40000000, 0xFF800000]]
    fo, go = walls_ref.inflate(f, g, d2, 1)
    assert fo.view(np.uint32).tolist() == [[0, 0x7F800000, 0x7F800000, 0x7F800000, 0x7F800000]]
    assert go.view(np.uint32).tolist() == [[0x3F800000] + [0xFF800000] * 4]


# ---- the radius of a body ----------------------------------------------------------------------------------------------------------

def test_the_close_d2_of_a_body_and_the_radius_of_its_launch():
    for radius, cell, d2, R in ((0.19, 0.125, 2, 2), (0.19, 0.25, 0, 1), (0.19, 0.0625, 9, 3), (0.25, 0.125, 4, 2)):
        assert rd.wall_close_d2(radius, cell) == d2 == walls_ref.close_d2(radius, cell), (radius, cell)
        assert rd._wall_radius(d2) == R == walls_ref.radius_of(d2), d2
    for d2 in range(0, 1025):
        R = rd._wall_radius(d2)
        assert R >= 1 and R * R >= d2 and (R == 1 or (R - 1) * (R - 1) < d2) and R == walls_ref.radius_of(d2), d2
    assert rd._wall_radius(1024) == 32
    with pytest.raises(ValueError):
        rd._wall_radius(1025)
    assert rd.wall_close_d2(4.0, 0.125) == 1024 and rd.wall_close_d2(4.1, 0.125) > 1024


# ---- the argument checks -----------------------------------------------------------------------------------------------------------

def _fails(call, word, **kw):
    L = rd.lib()
    assert call(**kw) == BAD, kw
    assert word in L.rdoom_last_error().decode(), (word, kw, L.rdoom_last_error())


def test_the_wall_distance_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    v = ctypes.c_void_p
    inf, nan = float('inf'), float('nan')
    # never followed: every call fails its checks or queues nothing.  Four planes of 4 x 53 x 77 floats, 0x10000 bytes, well apart
    FLOOR, CEIL, OUT_F, OUT_C, DIST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    bytes_ = 4 * 53 * 77 * 4

    def call(floor=FLOOR, ceil=CEIL, n=4, w=77, h=53, params=(0.56, 2, 2, 0), dist=DIST, fo=OUT_F, co=OUT_C):
        p = ctypes.byref(rd.WallParams(*params)) if params is not None else None
        return L.rdoom_wall_distance(v(floor), v(ceil), n, w, h, p, v(dist), v(fo), v(co), None)

    _fails(call, 'null params', params=None)
    _fails(call, 'null floor or ceiling', floor=None)
    _fails(call, 'null floor or ceiling', ceil=None)
    _fails(call, 'no output', dist=None, fo=None, co=None)
    _fails(call, 'without the other', fo=None)
    _fails(call, 'without the other', co=None, dist=None)
    _fails(call, '0 x 53', w=0)
    _fails(call, '77 x 0', h=0)
    _fails(call, 'a side', w=8193, h=1)
    _fails(call, 'a side', w=1, h=70000)
    _fails(call, 'too many', w=2048, h=2049)
    _fails(call, 'too many', w=8192, h=513)
    _fails(call, 'radius', params=(0.56, 0, 0, 0))
    _fails(call, 'radius', params=(0.56, 33, 0, 0))
    _fails(call, 'radius', params=(0.56, 0xFFFFFFFF, 0, 0))
    _fails(call, 'close_d2', params=(0.56, 2, 5, 0))
    _fails(call, 'close_d2', params=(0.56, 32, 1025, 0))
    _fails(call, 'close_d2', params=(0.56, 1, 0xFFFFFFFF, 0))
    for flags in (2, 3, 0x80000000, 0x80000001):
        _fails(call, 'flags', params=(0.56, 2, 2, flags))
    for bad in (nan, -1.0, -inf, -1e-30):
        _fails(call, 'clearance', params=(bad, 2, 2, 0))
    _fails(call, 'too many for one launch', n=0x7FFFFFFF, dist=DIST, fo=None, co=None)
    # an output plane on an input plane: the same, by one byte at either end, and either output on either input
    for fo, co in ((FLOOR, OUT_C), (OUT_F, CEIL), (CEIL, OUT_C), (OUT_F, FLOOR), (FLOOR + bytes_ - 4, OUT_C), (OUT_F, CEIL - bytes_ + 4)):
        _fails(call, 'overlaps', fo=fo, co=co)
    # what is allowed: either flag, the limits themselves, any one group of outputs, and n == 0 with nothing else valid -- all with
    # n == 0, so that nothing is queued
    assert call(n=0, floor=None, ceil=None) == 0
    assert call(n=0, dist=None) == 0 and call(n=0, fo=None, co=None) == 0
    assert call(n=0, params=(0.0, 1, 0, 0)) == 0 and call(n=0, params=(inf, 32, 1024, rd.WALL_EDGE_OPEN)) == 0
    assert call(n=0, w=2048, h=2048) == 0 and call(n=0, w=8192, h=512) == 0 and call(n=0, w=1, h=8192) == 0 and call(n=0, w=1, h=1) == 0
    _fails(call, 'null params', n=0, params=None)  # n == 0 is not a way round the checks
    _fails(call, 'too many', n=0, w=2049, h=2048)
    _fails(call, 'no output', n=0, dist=None, fo=None, co=None)
    _fails(call, 'radius', n=0, params=(0.56, 0, 0, 0))
