"""The straight walks on the host, with no GPU: the reference (tests/line_ref.py) pinned on chains and grids written out by hand, then
its properties -- a chain reversed is the chain back, a line between neighbours is that move, a free room is all clear, and what a
straightened path is -- the surface -- header, exported symbols, the Python names -- and every argument error of the two entry
points with device pointers that are never followed."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import flood_ref
import line_ref
import octile_ref
import rust_doom_amd as rd
from util import ROOT

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
BY_NAME = {c['name']: c for c in flood_ref.hand_cases()}
CASES_7x5 = [c for c in flood_ref.hand_cases() if c['floor'].shape == (5, 7)]
CELLS_7x5 = [(col, row) for row in range(5) for col in range(7)]


# ---- the reference on chains and grids written out by hand ---------------------------------------------------------------------------

def test_chains_written_out_by_hand():
    assert line_ref.chain((0, 0), (3, 1)) == [(1, 0), (2, 1), (3, 1)]  # column, diagonal, column
    assert line_ref.chain((0, 0), (2, 2)) == [(1, 1), (2, 2)]          # two diagonals
    assert line_ref.chain((4, 4), (4, 4)) == []
    assert line_ref.chain((0, 0), (3, 0)) == [(1, 0), (2, 0), (3, 0)] and line_ref.chain((0, 3), (0, 0)) == [(0, 2), (0, 1), (0, 0)]
    # a slope of 2/5: crossings at 1/10 c, 1/4 r, 3/10 c, 1/2 c, 7/10 c, 3/4 r, 9/10 c
    assert line_ref.chain((0, 0), (5, 2)) == [(1, 0), (1, 1), (2, 1), (3, 1), (4, 1), (4, 2), (5, 2)]
    assert line_ref.chain((5, 2), (0, 0)) == [(4, 2), (4, 1), (3, 1), (2, 1), (1, 1), (1, 0), (0, 0)]
    # the mirror images of the first, all eight octants: the same kinds of move
    for sx in (1, -1):
        for sy in (1, -1):
            assert line_ref.chain((0, 0), (3 * sx, sy)) == [(sx, 0), (2 * sx, sy), (3 * sx, sy)]
            assert line_ref.chain((0, 0), (sx, 3 * sy)) == [(0, sy), (sx, 2 * sy), (sx, 3 * sy)]


def test_no_line_passes_the_corner_of_the_pillar():
    m = line_ref.moves_of(*octile_ref.pillar())
    for rev in (False, True):
        assert line_ref.walk_line(m, (0, 1), (1, 0), rev) == (False, (0, 1), 0)
        assert line_ref.walk_line(m, (0, 0), (2, 2), rev) == (False, (0, 0), 0)
        assert line_ref.walk_line(m, (0, 0), (2, 0), rev) == (True, (2, 0), 2)
        assert line_ref.walk_line(m, (0, 0), (2, 1), rev) == (False, (1, 0), 1)  # column, then the row move into the pillar
        assert line_ref.walk_line(m, (1, 1), (1, 1), rev) == (False, (1, 1), 0)  # a closed start, no move
        assert line_ref.walk_line(m, (0, 0), (0, 0), rev) == (True, (0, 0), 0)
        assert line_ref.walk_line(m, (0, 1), (2, 1), rev) == (False, (0, 1), 0)
        assert line_ref.walk_line(m, (0, 0), (3, 0), rev) == (False, (-1, -1), 0) and line_ref.walk_line(m, (-1, 0), (1, 0), rev) == (False, (-1, -1), 0)


def test_a_line_across_the_ledge_is_clear_one_way():
    c = BY_NAME['ledge from the top']  # columns 0-2 at 0.48, columns 3-6 at 0
    m = line_ref.moves_of(c['floor'], c['ceiling'])
    assert line_ref.walk_line(m, (0, 2), (6, 2)) == (True, (6, 2), 6)
    assert line_ref.walk_line(m, (0, 2), (6, 2), True) == (False, (2, 2), 2)   # (3, 2) -> (2, 2) is a rise of 0.48
    assert line_ref.walk_line(m, (6, 2), (0, 2)) == (False, (3, 2), 3)
    assert line_ref.walk_line(m, (6, 2), (0, 2), True) == (True, (0, 2), 6)    # the walk from (0, 2) to (6, 2), asked from its far end
    # diagonally across it: every one of the four axial moves round a corner is flat or a drop
    assert line_ref.walk_line(m, (0, 0), (4, 4)) == (True, (4, 4), 4) and line_ref.walk_line(m, (0, 0), (4, 4), True) == (False, (2, 2), 2)
    clear, stop, _ = line_ref.walk_lines(c['floor'][None], c['ceiling'][None], [(0, 2)], [[(6, 2), (2, 4), (7, 2)]])
    assert clear.tolist() == [[1, 1, 0]] and stop.tolist() == [[[6, 2], [2, 4], [-1, -1]]] and clear.dtype == np.uint8 and stop.dtype == np.int32


# ---- properties -----------------------------------------------------------------------------------------------------------------------

def test_the_chain_back_is_the_chain_reversed_over_every_pair_of_a_9_x_7_grid():
    cells = [(c, r) for c in range(9) for r in range(7)]
    for a in cells:
        for b in cells:
            there, back = [a] + line_ref.chain(a, b), [b] + line_ref.chain(b, a)
            assert there == back[::-1] and there[-1] == b, (a, b)
            steps = np.abs(np.diff(np.array(there), axis=0)) if len(there) > 1 else np.zeros((0, 2), int)
            assert (steps.max(1, initial=1) == 1).all()  # every move to an 8-neighbour
            diagonals = int((steps.sum(1) == 2).sum())
            assert len(there) - 1 == abs(b[0] - a[0]) + abs(b[1] - a[1]) - diagonals, (a, b)


@pytest.mark.parametrize('k', range(len(CASES_7x5)), ids=[c['name'] for c in CASES_7x5])
def test_a_line_between_neighbours_is_that_move_on_every_7x5_hand_grid(k):
    c = CASES_7x5[k]
    kw = dict(line_ref.LIMITS, **c['kw'])
    m = line_ref.moves_of(c['floor'], c['ceiling'], **kw)
    is_open, axial = flood_ref.moves(c['floor'], c['ceiling'], **kw)
    _, eight = octile_ref.octile_moves(c['floor'], c['ceiling'], False, **kw)
    for (col, row) in CELLS_7x5:
        for dc, dr, bit, is_axial in octile_ref.NEIGHBOURS:
            a = (col + dc, row + dr)  # the bit says: (col, row) may be entered from a
            if not (0 <= a[0] < 7 and 0 <= a[1] < 5):
                continue
            want = bool((axial if is_axial else eight)[row, col] & bit)
            assert line_ref.walk_line(m, a, (col, row))[0] == want, (a, (col, row))
            assert line_ref.walk_line(m, (col, row), a, True)[0] == want, (a, (col, row))  # the same move, asked from its far end


def test_every_line_of_a_free_room_is_clear():
    f, g = flood_ref.room(9, 7)
    m = line_ref.moves_of(f, g)
    cells = [(c, r) for c in range(9) for r in range(7)]
    for rev in (False, True):
        assert all(line_ref.walk_line(m, a, b, rev)[:2] == (True, b) for a in cells for b in cells)


@pytest.mark.parametrize('seed', range(12))
def test_what_a_straightened_octile_descent_is(seed):
    """on sparse rooms: corners are path cells in increasing index, the last the path's end; consecutive corners are clear lines;
    and the length lies between the straight line and the octile estimate.  Costs (2, 3) make the estimate an upper bound -- a
    diagonal move of 1.5 is longer than sqrt 2 -- while (5, 7) prices a diagonal at 1.4 < sqrt 2, so there the bound is
    sqrt 2 / 1.4 times the estimate"""
    rng = np.random.default_rng(500 + seed)
    w, h = int(rng.integers(20, 60)), int(rng.integers(12, 40))
    f, g = line_ref.sparse_room(w, h, seed, 0.02)
    m = line_ref.moves_of(f, g)
    at = np.argwhere(np.array(m[0]) & (f == 0))  # the field's seed: an open cell that is no pedestal, reached either way
    straightened = 0
    for towards in (False, True):
        for costs, slack in (((2, 3), 1.0), ((5, 7), math.sqrt(2) / 1.4)):
            r, c = at[int(rng.integers(len(at)))]
            field = octile_ref.flood(f, g, (c, r), towards, *costs)
            reached = np.argwhere(field != octile_ref.UNREACHED)
            rr, cc = reached[np.argmax(field[field != octile_ref.UNREACHED])]  # the farthest cell
            start = (int(cc), int(rr))
            cell, made, path = octile_ref.descend(f, g, field, start, towards, *costs)
            assert cell == (c, r) and made > 10
            corners, length = line_ref.straighten(m, start, path, towards, max_look=1024, corner_len=made)
            index = [path.index(k) for k in corners]
            assert index == sorted(set(index)) and corners[-1] == path[-1] and len(corners) <= made
            for a, b in zip([start] + corners, corners):
                assert line_ref.walk_line(m, a, b, not towards)[0], (a, b)
            euclid = math.hypot(cell[0] - start[0], cell[1] - start[1])
            estimate = int(field[rr, cc]) / costs[0]
            assert euclid * (1 - 1e-6) <= float(length) <= estimate * slack * (1 + 1e-6), (euclid, float(length), estimate)
            straightened += len(corners) < made
            # a short look-ahead and few corners: a prefix of the same kind, every corner within max_look of the one before
            few, _ = line_ref.straighten(m, start, path, towards, max_look=3, corner_len=4)
            steps = np.diff([-1] + [path.index(k) for k in few])
            assert len(few) == min(4, len(few)) and (steps >= 1).all() and (steps <= 3).all()
    assert straightened >= 3


def test_straighten_stops_where_the_contract_says():
    f, g = octile_ref.pillar()
    m = line_ref.moves_of(f, g)
    path = [(1, 0), (2, 0), (2, 1), (2, 2), (-1, -1), (1, 2)]
    # from (0, 0), of the four cells before the (-1, -1): the lines to (2, 2) and (2, 1) pass the pillar, (2, 0) is clear; then (2, 2)
    corners, length = line_ref.straighten(m, (0, 0), path, True)
    assert corners == [(2, 0), (2, 2)] and length == F(4)
    assert line_ref.straighten(m, (0, 0), path, True, max_look=1) == ([(1, 0), (2, 0), (2, 1), (2, 2)], F(4))
    assert line_ref.straighten(m, (0, 0), path, True, corner_len=1) == ([(2, 0)], F(2))
    assert line_ref.straighten(m, (3, 0), path, True) == ([], F(0)) and line_ref.straighten(m, (1, 1), path, True) == ([], F(0))
    assert line_ref.straighten(m, (0, 0), [(2, 2), (1, 2)], True) == ([], F(0))  # the first cell is not walkable from the start
    got = line_ref.straighten_paths(f[None], g[None], [(0, 0)], [path], True, corner_len=3)
    assert got[0].tolist() == [[[2, 0], [2, 2], [-1, -1]]] and got[1].tolist() == [2] and got[1].dtype == np.uint32 and got[2].dtype == F


def test_the_sparse_rooms_have_what_they_are_for():
    f, g = line_ref.sparse_room(257, 131, 3, 0.02)
    is_open, bits = octile_ref.octile_moves(f, g, False, **line_ref.LIMITS)
    assert 0.97 < is_open.mean() < 0.99 and 0.01 < (f == F(0.96)).mean() < 0.03
    one_way = 0
    for c, r in np.argwhere(f == F(0.96))[:20, ::-1]:
        if 0 < c < 256 and is_open[r, c] and is_open[r, c + 1] and f[r, c + 1] == 0:
            one_way += bool(bits[r, c + 1] & flood_ref.FROM_LEFT) and not bits[r, c] & flood_ref.FROM_RIGHT
    assert one_way >= 5  # pedestals are dropped from, not climbed


# ---- the surface -----------------------------------------------------------------------------------------------------------------------

def test_the_library_and_the_package_export_the_straight_walks():
    L = ctypes.CDLL(rd.LIB_PATH)
    for name in ('rdoom_grid_walk_lines', 'rdoom_path_straighten'):
        assert hasattr(L, name) and name in rd.API_SYMBOLS and getattr(rd.lib(), name).restype is ctypes.c_int32, name
    assert rd.LINE_REVERSED == 1 and rd.STRAIGHTEN_MAX_LOOK == 1024
    sig = inspect.signature(rd.walk_lines)
    assert list(sig.parameters) == ['floor', 'ceiling', 'starts', 'targets', 'reversed', 'max_step', 'max_drop', 'clearance', 'clear_out',
                                    'stop_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['reversed'], d['max_step'], d['max_drop'], d['clearance'], d['clear_out'], d['stop_out'], d['stream']) == \
        (False, 0.24, float('inf'), 0.56, None, None, None)
    sig = inspect.signature(rd.straighten_paths)
    assert list(sig.parameters) == ['floor', 'ceiling', 'starts', 'path', 'towards', 'max_look', 'corners', 'max_step', 'max_drop', 'clearance',
                                    'count_out', 'length_out', 'stream']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['towards'], d['max_look'], d['corners'], d['max_step'], d['max_drop'], d['clearance'], d['count_out'], d['length_out']) == \
        (False, 64, 8, 0.24, float('inf'), 0.56, None, None)


def test_the_header_declares_the_straight_walks():
    text = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert '/* ---- straight walks:' in text and '(DESIGN section 27)' in text
    assert text.index('/* ---- octile distance:') < text.index('/* ---- straight walks:')
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'#define RDOOM_LINE_REVERSED 1u\b', code) and re.search(r'#define RDOOM_STRAIGHTEN_MAX_LOOK 1024u\b', code)

    def arguments(name):
        proto = re.search(r'rdoom_status %s\((.*?)\);' % name, code, flags=re.S).group(1)
        return [' '.join(a.split()) for a in proto.split(',')]

    assert arguments('rdoom_grid_walk_lines') == [
        'const float *d_floor', 'const float *d_ceiling', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'const int32_t *d_from',
        'const int32_t *d_to', 'uint32_t n_to', 'const rdoom_flood_params *params', 'uint8_t *d_clear_out', 'int32_t *d_stop_out', 'void *stream']
    assert arguments('rdoom_path_straighten') == [
        'const float *d_floor', 'const float *d_ceiling', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'const int32_t *d_starts',
        'const int32_t *d_path', 'uint32_t path_len', 'const rdoom_flood_params *params', 'uint32_t max_look', 'int32_t *d_corners_out',
        'uint32_t corner_len', 'uint32_t *d_count_out', 'float *d_length_out', 'void *stream']
    section = ' '.join(re.sub(r'\n \*', '\n', text[text.index('/* ---- straight walks:'):]).split())  # the comment's lines joined
    for words in ('column crossing i (0 <= i < dx) is at parameter (2i + 1) / (2 dx)', 'row crossing j (0 <= j < dy) at (2j + 1) / (2 dy)',
                  'if j == dy, or i < dx and (2i + 1) * dy < (2j + 1) * dx: a column move to (c + sx, r), then i += 1',
                  'else if i == dx, or (2i + 1) * dy > (2j + 1) * dx: a row move to (c, r + sy), then j += 1',
                  'a diagonal move to (c + sx, r + sy), then i += 1 and j += 1', 'Every product is an integer below 2^28',
                  'Nothing is rounded', 'The chain ends at b', 'all four axial moves round both sides must be allowed',
                  'never cuts the corner of a closed cell, a ledge or a door', "a diagonal's four axial moves are reversed likewise",
                  'A zero-move line (a == b) is clear exactly when a is open', 'the cell the first refused move starts from',
                  '(-1, -1) when a or b is outside the grid', 'flags is 0 or RDOOM_LINE_REVERSED', 'every byte written',
                  'n_to == 0', 'n * n_to above 2^31 - 1', 'k* is the largest k in [0, K) whose line from a to path[i + k] is clear',
                  'length += sqrtf((float)(dc * dc + dr * dr))', 'a = corner, i += k* + 1, count += 1', 'every entry is written',
                  'Entry 0 is the any-angle waypoint', '1 <= max_look <= RDOOM_STRAIGHTEN_MAX_LOOK', '1 <= path_len <= 2^22',
                  '1 <= corner_len <= 2^22', 'n == 0 queues nothing', 'captured into a graph'):
        assert words in section, words


# ---- the argument checks -----------------------------------------------------------------------------------------------------------------

def _fails(call, word, **kw):
    L = rd.lib()
    assert call(**kw) == BAD, kw
    assert word in L.rdoom_last_error().decode(), (word, kw, L.rdoom_last_error())


def _calls():
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never followed: every call fails its checks or queues nothing
    inf = float('inf')

    def lines(floor=fake, ceil=fake, n=4, w=77, h=53, starts=fake, to=fake, n_to=3, params=(0.24, inf, 0.56, 0), clear=fake, stop=None):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_grid_walk_lines(floor, ceil, n, w, h, starts, to, n_to, p, clear, stop, None)

    def straighten(floor=fake, ceil=fake, n=4, w=77, h=53, starts=fake, path=fake, path_len=9, params=(0.24, inf, 0.56, 0), max_look=64, corners=fake,
                   corner_len=8, count=fake, length=None):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_path_straighten(floor, ceil, n, w, h, starts, path, path_len, p, max_look, corners, corner_len, count, length, None)

    return fake, lines, straighten


@pytest.mark.parametrize('which', ['lines', 'straighten'])
def test_both_calls_check_the_arguments_they_share_with_the_floods(which):
    fake, lines, straighten = _calls()
    call = lines if which == 'lines' else straighten
    inf, nan = float('inf'), float('nan')
    _fails(call, 'null params', params=None)
    _fails(call, 'null', floor=None)
    _fails(call, 'null', ceil=None)
    _fails(call, 'null', starts=None)
    _fails(call, '0 x 53', w=0)
    _fails(call, '77 x 0', h=0)
    _fails(call, 'a side', w=8193, h=1)
    _fails(call, 'a side', w=1, h=70000)
    _fails(call, 'too many', w=2048, h=2049)
    _fails(call, 'too many', w=8192, h=8192)
    _fails(call, 'too many', n=0x80000000)
    for flags in (2, 3, 0x80000000, 0x80000001):
        _fails(call, 'flags', params=(0.24, inf, 0.56, flags))
    for k, name in enumerate(('max_step', 'max_drop', 'clearance')):
        for bad in (nan, -1.0, -inf, -1e-30):
            params = [0.24, inf, 0.56, 1]
            params[k] = bad
            _fails(call, name, params=tuple(params))
    # what is allowed: either flag, the limits at their ends, the largest grids, and n == 0 with nothing else valid
    assert call(n=0, floor=None, ceil=None, starts=None) == 0
    assert call(n=0, params=(0.0, 0.0, 0.0, 0)) == 0 and call(n=0, params=(inf, inf, inf, 1)) == 0
    assert call(n=0, w=2048, h=2048) == 0 and call(n=0, w=8192, h=512) == 0 and call(n=0, w=1, h=1) == 0
    _fails(call, 'null params', n=0, params=None)  # n == 0 is not a way round the checks
    _fails(call, 'too many', n=0, w=2049, h=2048)
    _fails(call, 'flags', n=0, params=(0.24, inf, 0.56, 2))


def test_walk_lines_checks_its_own_arguments():
    fake, lines, _ = _calls()
    for name in ('to', 'clear'):
        _fails(lines, 'null', **{name: None})
    _fails(lines, 'n_to', n_to=0)
    _fails(lines, 'n_to', n=0, n_to=0)
    for n, n_to in ((65536, 32768), (2, 0x40000000), (0x7FFFFFFF, 2), (3, 0xFFFFFFFF), (0x7FFFFFFF, 0xFFFFFFFF)):
        _fails(lines, 'too many lines', n=n, n_to=n_to)
    assert lines(n=0, to=None, clear=None, stop=None, n_to=1) == 0 and lines(n=0, n_to=0xFFFFFFFF, stop=fake) == 0
    assert rd.LINE_REVERSED == rd.FLOOD_TOWARDS  # the one flag bit of rdoom_flood_params either way


def test_path_straighten_checks_its_own_arguments():
    fake, _, straighten = _calls()
    for name in ('path', 'corners', 'count'):
        _fails(straighten, 'null', **{name: None})
    for look in (0, 1025, 0xFFFFFFFF):
        _fails(straighten, 'max_look', max_look=look)
        _fails(straighten, 'max_look', n=0, max_look=look)
    for length in (0, (1 << 22) + 1, 0xFFFFFFFF):
        _fails(straighten, 'path', path_len=length)
        _fails(straighten, 'corner_len', corner_len=length)
        _fails(straighten, 'corner_len', n=0, corner_len=length)
    assert straighten(n=0, max_look=1, path_len=1, corner_len=1) == 0
    assert straighten(n=0, max_look=1024, path_len=1 << 22, corner_len=1 << 22, path=None, corners=None, count=None, length=fake) == 0
