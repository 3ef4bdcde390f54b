"""The flood on the host, with no GPU: the reference (tests/flood_ref.py, a deque breadth-first search) pinned on grids whose distances
are written out by hand, the properties of the grids the GPU tests converge on, the surface -- header, exported symbols, the Python
names, the struct's size -- and every argument error of rdoom_flood_maps, none of which touches a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import flood_ref
import rust_doom_amd as rd
from util import ROOT

F = np.float32
U = flood_ref.UNREACHED
BAD = -1  # RDOOM_BAD_ARG
CASES = flood_ref.hand_cases()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_reference_on_grids_written_out_by_hand(case):
    got = flood_ref.flood(case['floor'], case['ceiling'], case['seed'], **case['kw'])
    assert got.dtype == np.uint16 and got.shape == case['floor'].shape
    assert np.array_equal(got, case['want']), (case['name'], got.tolist())


def test_the_hand_made_grids_cover_what_they_are_meant_to():
    by_name = {c['name']: c for c in CASES}
    assert {c['floor'].shape for c in CASES} >= {(1, 1), (1, 9), (9, 1), (5, 7)}
    # the ledge: all of the low side from the top, none of the top from the low side, and with the stair a longer way up than down
    down, up = by_name['ledge from the top']['want'], by_name['ledge from below']['want']
    assert (down != U).all() and (up[:, :3] == U).all() and (up[:, 3:] != U).all()
    stair = by_name['ledge with a stair from below']['want']
    assert (stair != U).all() and stair[0, 0] == 14 and down[0, 6] == 6  # corner to corner: 6 moves down the ledge, 14 up the stair
    # moves are directed: some neighbours a, b with a move a -> b and none b -> a
    c = by_name['ledge from the top']
    _, bits = flood_ref.moves(c['floor'], c['ceiling'], **flood_ref.DEFAULTS)
    assert (bits[:, 3] & flood_ref.FROM_LEFT).all() and not (bits[:, 2] & flood_ref.FROM_RIGHT).any()
    # the shared opening: both cells open, the step small enough, the move refused both ways
    c = by_name['shared opening too low']
    is_open, bits = flood_ref.moves(c['floor'], c['ceiling'], **flood_ref.DEFAULTS)
    assert is_open.all() and not (bits[:, 3] & flood_ref.FROM_LEFT).any() and not (bits[:, 2] & flood_ref.FROM_RIGHT).any()
    assert (c['floor'][:, 3] - c['floor'][:, 2] <= F(0.24)).all()
    # not numbers: seven closed cells, the +inf ceiling open
    c = by_name['cells that are not numbers']
    is_open = flood_ref.open_cells(c['floor'], c['ceiling'], 0.56)
    assert (~is_open).sum() == 7 and is_open[2, 3] and np.isposinf(c['ceiling'][2, 3]) and c['want'][2, 3] != U
    # the limits are met exactly, not approximately
    c = by_name['clearance met exactly']
    assert (c['ceiling'] - c['floor'] == F(0.56)).all()
    c = by_name['a rise exactly max_step']
    rises = c['floor'][0, 1:] - c['floor'][0, :-1]
    assert rises.max() == F(c['kw']['max_step']) and len(set(rises.tolist())) > 1


def test_the_grids_that_take_many_passes():
    f, g = flood_ref.serpentine(33, 31)
    dist, count = flood_ref.flood_maps(f[None], g[None], np.array([[0, 0]]))
    corridor = flood_ref.open_cells(f, g, 0.56)
    assert count[0] == corridor.sum() and dist[0][corridor].max() == corridor.sum() - 1 > 400  # one path through every open cell
    r, c = np.unravel_index(np.argmax(np.where(dist[0] == U, -1, dist[0].astype(np.int64))), dist[0].shape)
    back = flood_ref.flood(f, g, (c, r))
    assert back[0, 0] == corridor.sum() - 1

    cells = rd.flood_max_cells()
    w = next(w for w in range(255, 2, -2) if cells % w == 0)
    assert w % 2 == 1 and cells // w > 8
    f, g = flood_ref.spiral(w, cells // w)
    corridor = flood_ref.open_cells(f, g, 0.56)
    dist = flood_ref.flood(f, g, (0, 0))
    assert (dist != U).sum() == corridor.sum() and dist[corridor].max() == corridor.sum() - 1 > cells // 3

    f, g, seed = flood_ref.staircase()
    path = flood_ref.open_cells(f, g, 0.56)
    dist = flood_ref.flood(f, g, seed)
    assert f.size <= cells and dist[0, 0] == path.sum() - 1 == f.shape[0] + f.shape[1] - 2 > 400 and (dist != U).sum() == path.sum()
    assert (flood_ref.flood(f, g, (0, 0)) != U).sum() == 1  # walked the other way: nowhere
    # every move of it goes left or up
    _, bits = flood_ref.moves(f, g, **flood_ref.DEFAULTS)
    assert not (bits & (flood_ref.FROM_LEFT | flood_ref.FROM_ABOVE)).any() and (bits & flood_ref.FROM_RIGHT).any() and (bits & flood_ref.FROM_BELOW).any()


def test_the_header_declares_the_flood():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- flood:' in text and '(DESIGN section 20)' in text
    assert '#define RDOOM_FLOOD_UNREACHED 0xFFFFu' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'typedef struct rdoom_flood_params \{\s*float max_step, max_drop, clearance;\s*uint32_t flags;\s*\} rdoom_flood_params;', code)
    proto = re.search(r'rdoom_status rdoom_flood_maps\((.*?)\);', code, flags=re.S).group(1)
    assert [' '.join(a.split()) for a in proto.split(',')] == [
        'const float *d_floor', 'const float *d_ceiling', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'const int32_t *d_seeds',
        'const rdoom_flood_params *params', 'uint16_t *d_dist_out', 'uint32_t *d_count_out', 'void *stream']
    assert re.search(r'rdoom_status rdoom_flood_max_cells\(uint32_t \*cells_out\);', code)
    for words in ('g - f >= clearance', 'f_b - f_a <= max_step', 'f_a - f_b <= max_drop', 'fminf(g_a, g_b) - fmaxf(f_a, f_b) >= clearance',
                  '(width / 2, height / 2)', 'captured into a graph', 'n == 0 queues nothing'):
        assert words in text, words


def test_the_library_and_the_package_export_the_flood():
    L = ctypes.CDLL(rd.LIB_PATH)
    assert hasattr(L, 'rdoom_flood_maps') and hasattr(L, 'rdoom_flood_max_cells')
    assert {'rdoom_flood_maps', 'rdoom_flood_max_cells'} <= set(rd.API_SYMBOLS)
    assert rd.FLOOD_UNREACHED == 0xFFFF == U
    assert 19200 <= rd.flood_max_cells() < 65535
    assert ctypes.sizeof(rd.FloodParams) == 16 and [f[0] for f in rd.FloodParams._fields_] == ['max_step', 'max_drop', 'clearance', 'flags']
    sig = inspect.signature(rd.flood_maps)
    assert list(sig.parameters) == ['floor', 'ceiling', 'seeds', 'max_step', 'max_drop', 'clearance', 'dist_out', 'count_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['max_step'], d['max_drop'], d['clearance']) == (0.24, float('inf'), 0.56) and d['seeds'] is None and d['count_out'] is None
    assert rd.lib().rdoom_flood_max_cells(None) == BAD and b'null' in rd.lib().rdoom_last_error()


def test_the_flood_checks_its_arguments_before_it_touches_a_device():
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks or queues nothing
    cells = rd.flood_max_cells()
    inf, nan = float('inf'), float('nan')

    def call(floor=fake, ceil=fake, n=4, w=77, h=53, seeds=None, params=(0.24, inf, 0.56, 0), dist=fake, count=None):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_flood_maps(floor, ceil, n, w, h, seeds, p, dist, count, None)

    def fails(word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    fails('null params', params=None)
    fails('null', floor=None)
    fails('null', ceil=None)
    fails('null', dist=None)
    fails('0 x 53', w=0)
    fails('77 x 0', h=0)
    fails('too many', w=cells + 1, h=1)
    fails('too many', w=1, h=cells + 1)
    fails('too many', w=65536, h=65536)  # the product is not taken in 32 bits
    fails('too many', w=0xFFFFFFFF, h=0xFFFFFFFF)
    fails('flags', params=(0.24, inf, 0.56, 1))
    fails('flags', params=(0.24, inf, 0.56, 0x80000000))
    for k, name in enumerate(('max_step', 'max_drop', 'clearance')):
        for bad in (nan, -1.0, -inf, -1e-30):
            params = [0.24, inf, 0.56, 0]
            params[k] = bad
            fails(name, params=tuple(params))
    # what is allowed: zeros, an infinite drop or step, and n == 0 with nothing else valid but the shape and the limits
    assert call(n=0, floor=None, ceil=None, dist=None) == 0
    assert call(n=0, params=(0.0, 0.0, 0.0, 0)) == 0 and call(n=0, params=(inf, inf, inf, 0)) == 0
    assert call(n=0, w=cells, h=1) == 0 and call(n=0, w=1, h=cells) == 0
    fails('null params', n=0, params=None)  # n == 0 is not a way round the checks
    fails('too many', n=0, w=cells + 1, h=1)
