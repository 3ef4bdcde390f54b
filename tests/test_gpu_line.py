"""The straight walks on the GPU (line.hip: the two walk_lines kernels and the two path_straighten kernels) against tests/line_ref.py,
every element of every output, bit for bit.  Every 7 x 5 hand grid from each of its 35 cells to all 35, fifteen rows a launch, with
both flags and with and without stop_out; 1 x 1; lines longer than a wave in sparse rooms, with targets outside the grid; the longest
lines, 8192 cells either way; the diagonal of a 2048 x 2048 room and the line one row off it; straighten_paths on the descents of the
hand grids, of the sparse rooms and of a band three cells wide, on paths longer than one look-ahead, cut short, cut in the middle and
not walkable at all; E1M1 end to end; streams, the caller's tensors, raw pointers and a captured graph, in a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flood_ref
import goal_ref
import line_ref
import octile_ref
import rust_doom_amd as rd
import sector_ref
import walls_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = octile_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 15  # rows a launch of the hand-made grids
LIMITS = line_ref.LIMITS
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LOOKS = [(1, 4), (3, 2), (64, 8), (1024, 300)]  # (max_look, corner_len)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype, order='C')).cuda()  # (a copy: the shared fixtures are read-only)


def _lines(floor, ceiling, starts, targets, rows=None, stop=True, **kw):
    """walk_lines of device tensors, `rows` rows a launch (None: all in one), into tensors filled with sevens: (clear, stop or None)
    as numpy"""
    n, q = targets.shape[:2]
    rows = n if rows is None else rows
    clear = torch.full((n, q), 7, dtype=torch.uint8, device='cuda')
    stops = torch.full((n, q, 2), 7, dtype=torch.int32, device='cuda') if stop else None
    for a in range(0, n, rows):
        b = a + rows
        got = rd.walk_lines(floor[a:b], ceiling[a:b], starts[a:b], targets[a:b], clear_out=clear[a:b], stop_out=stops[a:b] if stop else None, **kw)
        assert (isinstance(got, tuple) and len(got) == 2) if stop else isinstance(got, torch.Tensor)
    return clear.cpu().numpy(), stops.cpu().numpy() if stop else None


def _same_lines(got, want, what):
    for k, name in enumerate(('clear', 'stop')):
        if got[k] is None:
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name, got[k].shape, want[k].shape, got[k].dtype)
        bad = got[k] != want[k]
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:6], want[k][bad][:6])


def _pulled(floor, ceiling, starts, path, corner_len, rows=None, **kw):
    """straighten_paths of device tensors, `rows` rows a launch, into tensors filled with sevens: (corners, count, length) as numpy"""
    n = len(path)
    rows = n if rows is None else rows
    corners = torch.full((n, corner_len, 2), 7, dtype=torch.int32, device='cuda')
    count = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    length = torch.full((n,), 7.0, dtype=torch.float32, device='cuda')
    for a in range(0, n, rows):
        b = a + rows
        got = rd.straighten_paths(floor[a:b], ceiling[a:b], starts[a:b], path[a:b], corners=corners[a:b], count_out=count[a:b],
                                  length_out=length[a:b], **kw)
        assert len(got) == 3
    return corners.cpu().numpy(), count.cpu().numpy().view(np.uint32), length.cpu().numpy()


def _same_pulled(got, want, what):
    for k, name in enumerate(('corners', 'count', 'length')):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name, got[k].shape, want[k].shape, got[k].dtype)
        bad = got[k].view(np.uint32) != want[k].view(np.uint32)  # the length: its bits
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:6], want[k][bad][:6])


# ---- the 7 x 5 hand grids ----------------------------------------------------------------------------------------------------------------

CELLS_7x5 = np.array([(col, row) for row in range(5) for col in range(7)], np.int32)
CASES_7x5 = [c for c in flood_ref.hand_cases() if c['floor'].shape == (5, 7)]


@functools.lru_cache(maxsize=None)
def _moves_7x5(k):
    c = CASES_7x5[k]
    return line_ref.moves_of(c['floor'], c['ceiling'], **dict(LIMITS, **c['kw']))


@functools.lru_cache(maxsize=None)
def _lines_7x5(k, rev):
    """the reference of case k: from each of the 35 cells to all 35, computed once and left unchanged"""
    targets = np.repeat(CELLS_7x5[None], 35, 0)
    return line_ref.walk_lines(None, None, CELLS_7x5, targets, rev, moves=[_moves_7x5(k)] * 35)


@pytest.mark.parametrize('stop', [True, False], ids=['with stop_out', 'without stop_out'])
@pytest.mark.parametrize('rev', [False, True], ids=['forwards', 'reversed'])
def test_the_7x5_grids_from_each_of_their_35_cells_to_all_35_fifteen_rows_a_launch(rev, stop):
    """all eight octants, every slope up to 6, corners passed exactly, a == b, closed ends and ledges"""
    rd.set_device(0)
    assert len(CASES_7x5) >= 15
    targets = _dev(np.repeat(CELLS_7x5[None], 35, 0))
    clear = blocked = one_way = 0
    for k, c in enumerate(CASES_7x5):
        floor, ceiling = _dev(np.repeat(c['floor'][None], 35, 0)), _dev(np.repeat(c['ceiling'][None], 35, 0))
        want = _lines_7x5(k, rev)
        _same_lines(_lines(floor, ceiling, _dev(CELLS_7x5), targets, rows=ROWS, stop=stop, reversed=rev, **c['kw']), want, (c['name'], rev, stop))
        clear, blocked = clear + int(want[0].sum()), blocked + int((want[0] == 0).sum())
        one_way += int((want[0] != _lines_7x5(k, not rev)[0]).sum())
    assert clear > 5000 and blocked > 3000 and one_way > 300  # the ledges: the two flags are two answers


def test_the_smallest_grid():
    rd.set_device(0)
    for ceiling, is_open in ((1.0, 1), (0.5, 0)):
        f, g = flood_ref.room(1, 1, 0.0, ceiling)
        targets = np.array([[(0, 0), (1, 0), (0, -1)]], np.int32)
        for rev in (False, True):
            got = _lines(_dev(f[None]), _dev(g[None]), _dev(np.zeros((1, 2), np.int32)), _dev(targets), reversed=rev)
            want = line_ref.walk_lines(f[None], g[None], [(0, 0)], targets, rev)
            assert want[0].tolist() == [[is_open, 0, 0]] and want[1].tolist() == [[[0, 0], [-1, -1], [-1, -1]]]
            _same_lines(got, want, ('1 x 1', ceiling, rev))
        path = np.array([[(0, 0), (0, 0), (-1, -1)]], np.int32)
        got = _pulled(_dev(f[None]), _dev(g[None]), _dev(np.zeros((1, 2), np.int32)), _dev(path), 4, towards=True)
        want = line_ref.straighten_paths(f[None], g[None], [(0, 0)], path, True, corner_len=4)
        assert want[1].tolist() == [is_open] and want[2].tolist() == [0.0]  # the farther of the two zero-move lines, then the path is used up
        _same_pulled(got, want, ('1 x 1', ceiling))


# ---- lines longer than a wave, in sparse rooms ---------------------------------------------------------------------------------------------

SPARSE_SEEDS = {(130, 19): 11, (257, 131): 5}  # chosen on the CPU: the conditions test_lines_longer_than_a_wave asserts hold


@functools.lru_cache(maxsize=None)
def _sparse(w, h):
    """two sparse rooms of w x h cycled over eight rows, a start near the left or right edge of each row, 64 targets a row -- six
    outside the grid or extreme, one in the start's column, one in its row, the start itself, the three nearest pedestals, the rest
    anywhere -- and the reference either way: computed once, left unchanged"""
    seed = SPARSE_SEEDS[(w, h)]
    rng = np.random.default_rng(seed)
    rooms = [line_ref.sparse_room(w, h, 100 * seed + p, 0.004) for p in range(2)]
    moves = [line_ref.moves_of(*r) for r in rooms]
    which = np.arange(8) % 2
    starts = np.zeros((8, 2), np.int32)
    for p in range(8):
        while True:
            c, r = int(rng.integers(0, w // 8)), int(rng.integers(0, h))
            c = w - 1 - c if p & 2 else c
            if moves[which[p]][0][r][c] and rooms[which[p]][0][r, c] == 0:
                break
        starts[p] = c, r
    targets = np.stack([rng.integers(0, w, (8, 64)), rng.integers(0, h, (8, 64))], 2).astype(np.int32)
    targets[:, :6] = [(-1, -1), (w, 5), (5, h), (-1, 5), (INT_MIN, INT_MAX), (INT_MAX, 0)]
    targets[:, 6, 0], targets[:, 7, 1], targets[:, 8] = starts[:, 0], starts[:, 1], starts
    for p in range(8):  # three pedestals a row: walked off towards the start, not climbed from it
        tops = np.argwhere(rooms[which[p]][0] == F(0.96))[:, ::-1]
        targets[p, 9:12] = tops[np.argsort(np.abs(tops - starts[p]).sum(1))[:3]]
    floor, ceiling = np.stack([rooms[p][0] for p in which]), np.stack([rooms[p][1] for p in which])
    want = {rev: line_ref.walk_lines(None, None, starts, targets, rev, moves=[moves[p] for p in which]) for rev in (False, True)}
    for a in (floor, ceiling, starts, targets):
        a.setflags(write=False)
    return floor, ceiling, starts, targets, [moves[p] for p in which], want


@pytest.mark.parametrize('grid', [(130, 19), (257, 131)], ids=lambda g: '%dx%d' % g)
def test_lines_longer_than_a_wave_in_sparse_rooms(grid):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, starts, targets, _, want = _sparse(w, h)
    crossings = np.abs(targets.astype(np.int64) - starts[:, None]).sum(2)
    long_clear = late = 0
    for rev in (False, True):
        clear, stop, made = want[rev]
        # on the reference alone: a pass cannot be vacuous
        assert clear.mean() >= 0.15 and (clear == 0).mean() >= 0.15, (grid, rev, clear.mean())
        inside = (stop[:, :, 0] >= 0)
        assert (~inside[:, :6]).all() and inside[:, 6:].all() and clear[:, 8].all() and (made[:, 8] == 0).all()
        long_clear += int(((clear == 1) & (crossings > 64)).sum())
        late += int(((clear == 0) & inside & (made > 64)).sum())  # the first refusal lies beyond crossing 64
        _same_lines(_lines(_dev(floor), _dev(ceiling), _dev(starts), _dev(targets), reversed=rev), want[rev][:2], (grid, rev))
        got = _lines(_dev(floor), _dev(ceiling), _dev(starts), _dev(targets), stop=False, reversed=rev)
        _same_lines(got, want[rev][:2], (grid, rev, 'without stop_out'))
    assert long_clear >= 20 and late >= 20, (grid, long_clear, late)
    assert (want[False][0] != want[True][0]).any()  # the pedestals: dropped from, not climbed


# ---- the longest lines ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(8192, 1), (1, 8192)], ids=['8192x1', '1x8192'])
def test_the_longest_lines_from_either_end(shape):
    """end to end, 8191 moves: clear; with cell 8000 closed the walk stops at 7999 from the near end and at 8001 from the far one;
    reversed, the same cells from the other end"""
    rd.set_device(0)
    w, h = shape
    along = (lambda k: (k, 0)) if h == 1 else (lambda k: (0, k))
    f, g = flood_ref.room(w, h)
    f2, g2 = f.copy(), g.copy()
    f2[along(8000)[::-1]], g2[along(8000)[::-1]] = np.inf, -np.inf
    floor, ceiling = np.stack([f, f, f2, f2]), np.stack([g, g, g2, g2])
    starts = np.array([along(0), along(8191)] * 2, np.int32)
    targets = np.array([[along(8191), along(7999), along(0)], [along(0), along(8001), along(8191)]] * 2, np.int32)
    moves = [octile_ref.octile_moves(f, g, False, **LIMITS)] * 2 + [octile_ref.octile_moves(f2, g2, False, **LIMITS)] * 2
    for rev in (False, True):
        want = line_ref.walk_lines(None, None, starts, targets, rev, moves=moves)
        assert want[0].tolist() == [[1, 1, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1]]
        assert want[1][2, 0].tolist() == list(along(7999)) and want[1][3, 0].tolist() == list(along(8001)) and want[2][2, 0] == 7999
        _same_lines(_lines(_dev(floor), _dev(ceiling), _dev(starts), _dev(targets), reversed=rev), want[:2], (shape, rev))


@functools.lru_cache(maxsize=None)
def _big_room():
    """a flat 2048 x 2048 room, the same with a closed cell on its diagonal, and the same with a closed cell on the line one row off
    the diagonal and beside it"""
    f, g = flood_ref.room(2048, 2048)
    rooms = [(f, g)]
    for c, r in ((1500, 1500), next(c for c in line_ref.chain((0, 0), (2047, 2046))[1000:] if c[0] != c[1])):
        f2, g2 = f.copy(), g.copy()
        f2[r, c], g2[r, c] = np.inf, -np.inf
        rooms.append((f2, g2))
    return rooms, [octile_ref.octile_moves(f, g, False, **LIMITS) for f, g in rooms]


def test_the_diagonal_of_a_2048_x_2048_room_and_the_line_one_row_off_it():
    """corner to corner, 2047 diagonal moves; (0, 0) -> (2047, 2046), 4093 axial moves that pass no corner: both again with a closed
    cell on the way, from either end -- the cell beside the diagonal stops the diagonal too, by the corner rule"""
    rd.set_device(0)
    rooms, moves = _big_room()
    assert len(line_ref.chain((0, 0), (2047, 2047))) == 2047 and len(line_ref.chain((0, 0), (2047, 2046))) == 2047 + 2046
    which = [0, 1, 2, 1, 2]
    starts = np.array([(0, 0), (0, 0), (0, 0), (2047, 2047), (2047, 2046)], np.int32)
    targets = np.array([[(2047, 2047), (2047, 2046)]] * 3 + [[(0, 0), (0, 2047)], [(0, 0), (2047, 0)]], np.int32)
    f_t, g_t = _dev(np.stack([rooms[p][0] for p in which])), _dev(np.stack([rooms[p][1] for p in which]))
    for rev in (False, True):
        want = line_ref.walk_lines(None, None, starts, targets, rev, moves=[moves[p] for p in which])
        assert want[0][0].tolist() == [1, 1] and want[0][2:].tolist() == [[0, 0], [0, 1], [0, 1]] and want[0][1, 0] == 0
        assert want[1][1, 0].tolist() == [1499, 1499] and want[1][3, 0].tolist() == [1501, 1501]
        assert 490 <= want[2][2, 0] <= 510 and 1000 <= want[2][2, 1] <= 1001 and want[2][4, 0] > 3000  # moves made before the refusal
        _same_lines(_lines(f_t, g_t, _dev(starts), _dev(targets), reversed=rev), want[:2], ('2048 x 2048', rev))


# ---- straightened paths --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [(0, 0), (6, 0)], ids=['from the top left', 'from the top right'])
def test_the_descents_of_the_7x5_grids_pulled_straight(seed):
    """from every start, down both fields; a path of 20 takes every walk, one of 3 is shorter than most"""
    rd.set_device(0)
    pulled = cut = none = 0
    for k, c in enumerate(CASES_7x5):
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        f_t, g_t, s_t = _dev(floor), _dev(ceiling), _dev(CELLS_7x5)
        moves = [_moves_7x5(k)] * 35
        for towards in (False, True):
            kw = dict(towards=towards, **c['kw'])
            field = np.repeat(octile_ref.flood(c['floor'], c['ceiling'], seed, **kw)[None], 35, 0)
            for path_len, looks in ((20, LOOKS), (3, LOOKS[2:3])):
                _, made, path = octile_ref.descend_grids(floor, ceiling, field, CELLS_7x5, path_len=path_len, **kw)
                for max_look, corner_len in looks:
                    want = line_ref.straighten_paths(None, None, CELLS_7x5, path, towards, max_look, corner_len, moves=moves)
                    got = _pulled(f_t, g_t, s_t, _dev(path), corner_len, rows=ROWS, max_look=max_look, **kw)
                    _same_pulled(got, want, (c['name'], seed, towards, path_len, max_look, corner_len))
                    if max_look == 64:
                        pulled += int((want[1] < np.minimum(made, path_len)).sum())
                        cut += int((made > path_len).sum())
                        none += int((want[1] == 0).sum())
    assert pulled > 300 and cut > 100 and none > 100


@functools.lru_cache(maxsize=None)
def _sparse_descents(w, h):
    """the octile descents of _sparse's eight rows towards a seed near the middle of each room and down the field from it, the whole
    way: {towards: (field seeds, paths (8, path_len, 2), moves made)}"""
    floor, ceiling, starts, _, moves, _ = _sparse(w, h)
    out = {}
    for towards in (False, True):
        fields = {}
        for p in range(2):  # the two rooms
            rows, cols = np.nonzero((np.array(moves[p][0])) & (floor[p] == 0))
            k = np.argmin((rows - h // 2) ** 2 + (cols - w // 2) ** 2)
            fields[p] = ((int(cols[k]), int(rows[k])), octile_ref.flood(floor[p], ceiling[p], (cols[k], rows[k]), towards))
        field = np.stack([fields[p % 2][1] for p in range(8)])
        _, made, path = octile_ref.descend_grids(floor, ceiling, field, starts, path_len=w + h, towards=towards)
        assert (made > 40).all() and made.max() < w + h
        out[towards] = (path, made)
    return out


@pytest.mark.parametrize('grid', [(130, 19), (257, 131)], ids=lambda g: '%dx%d' % g)
@pytest.mark.parametrize('towards', [False, True], ids=['forwards', 'towards'])
def test_the_descents_of_the_sparse_rooms_pulled_straight(grid, towards):
    rd.set_device(0)
    w, h = grid
    floor, ceiling, starts, _, moves, _ = _sparse(w, h)
    path, made = _sparse_descents(w, h)[towards]
    f_t, g_t = _dev(floor), _dev(ceiling)
    # rows 0 .. 7 as they are; then row 0's path cut by a (-1, -1) in the middle, a start outside the grid, and a start on a
    # closed cell
    closed = np.argwhere(~np.array(moves[0][0]))[0][::-1]
    extra = np.array([0, 0, 0])
    paths = np.concatenate([path, path[extra]])
    paths[8, 20] = -1
    begin = np.concatenate([starts, [starts[0], (w, 3), closed]]).astype(np.int32)
    rows = np.concatenate([np.arange(8), extra])
    f_t, g_t, all_moves = f_t[torch.from_numpy(rows).cuda()].contiguous(), g_t[torch.from_numpy(rows).cuda()].contiguous(), [moves[p] for p in rows]
    for path_len in (w + h, 30):  # longer and shorter than the walks
        for max_look, corner_len in LOOKS:
            want = line_ref.straighten_paths(None, None, begin, paths[:, :path_len], towards, max_look, corner_len, moves=all_moves)
            got = _pulled(f_t, g_t, _dev(begin), _dev(paths[:, :path_len]), corner_len, towards=towards, max_look=max_look)
            _same_pulled(got, want, (grid, towards, path_len, max_look, corner_len))
            if (max_look, path_len) == (1024, w + h):
                assert (want[1][:8] < made).all() and (want[1][:8] >= 1).all() and want[1][9:].tolist() == [0, 0] and want[1][8] >= 1
                assert want[0][8, want[1][8] - 1].tolist() == path[0, 19].tolist()  # the cut path ends before the (-1, -1)
                ends = paths[np.arange(8), made - 1]
                assert (want[0][np.arange(8), want[1][:8] - 1] == ends).all()  # the last corner is the path's end
                euclid = np.sqrt(((ends - starts).astype(np.float64) ** 2).sum(1))
                assert (want[2][:8] >= euclid * (1 - 1e-6)).all() and (want[2][9:] == 0).all()
            if (max_look, corner_len) == (1, 4):
                assert (want[0][:8] == paths[:8, :4]).all()  # a look-ahead of one: the path's own cells


def test_the_band_three_cells_wide_and_paths_longer_than_one_look_ahead():
    """the band's edges force corners; a straight corridor of 2000 cells listed whole is more than one look-ahead of 1024, and a closed
    cell in it ends the pull; a path whose first cell cannot be walked to gives no corner"""
    rd.set_device(0)
    n = 300
    f, g = octile_ref.band(n)
    # along the band's edge the straight line is all diagonal moves past closed corners: refused, and the walk has to bend
    starts = np.array([(n - 1, n - 1), (n - 1, n - 2), (n - 2, n - 1), (n - 1, n - 1)], np.int32)
    seeds = [(0, 0), (1, 0), (0, 1), (1, 0)]
    floor, ceiling = np.repeat(f[None], 4, 0), np.repeat(g[None], 4, 0)
    moves = [line_ref.moves_of(f, g)] * 4
    for towards in (False, True):
        field = np.stack([octile_ref.flood(f, g, s, towards) for s in seeds])
        _, made, path = octile_ref.descend_grids(floor, ceiling, field, starts, path_len=n, towards=towards)
        assert (made >= 297).all()
        for max_look, corner_len in LOOKS:
            want = line_ref.straighten_paths(None, None, starts, path, towards, max_look, corner_len, moves=moves)
            _same_pulled(_pulled(_dev(floor), _dev(ceiling), _dev(starts), _dev(path), corner_len, towards=towards, max_look=max_look), want,
                         ('band', towards, max_look, corner_len))
            if max_look == 1024:
                assert want[1][0] == 1 and (want[1][1:3] > 1).all(), want[1]  # the diagonal itself is one straight walk; along an edge, corners

    w = 2000
    f, g = flood_ref.room(w, 1)
    f2, g2 = f.copy(), g.copy()
    f2[0, 700], g2[0, 700] = np.inf, -np.inf
    floor, ceiling = np.stack([f, f2, f2]), np.stack([g, g2, g2])
    path = np.zeros((3, w - 1, 2), np.int32)
    path[:, :, 0] = np.arange(1, w)
    path[2, 0] = 701, 0  # (0, 0) -> (701, 0) passes the closed cell, and nothing else is listed
    path[2, 1:] = -1
    starts = np.zeros((3, 2), np.int32)
    moves = [line_ref.moves_of(f, g)] + [line_ref.moves_of(f2, g2)] * 2
    for towards in (False, True):
        want = line_ref.straighten_paths(None, None, starts, path, towards, 1024, 8, moves=moves)
        assert want[1].tolist() == [2, 1, 0] and want[0][0, :2].tolist() == [[1024, 0], [1999, 0]] and want[0][1, 0].tolist() == [699, 0]
        assert want[2].tolist() == [1999.0, 699.0, 0.0]
        _same_pulled(_pulled(_dev(floor), _dev(ceiling), _dev(starts), _dev(path), 8, towards=towards, max_look=1024), want, ('corridor', towards))
        want = line_ref.straighten_paths(None, None, starts, path, towards, 100, 300, moves=moves)
        assert want[1].tolist() == [20, 7, 0]
        _same_pulled(_pulled(_dev(floor), _dev(ceiling), _dev(starts), _dev(path), 300, towards=towards, max_look=100), want, ('corridor, 100', towards))


# ---- E1M1 end to end -------------------------------------------------------------------------------------------------------------------------

E2E_STEP = 0.32  # tests/test_gpu_goal.py: the synthetic E1M1 joins most of its sectors by steps of 0.32
BODY = 0.19


@functools.lru_cache(maxsize=None)
def _wad():
    return rd.Wad(ensure_wad(), META_PATH)


def test_e1m1_planes_inflated_flooded_descended_and_pulled_straight_for_64_players():
    """draw_area_planes at cell 0.125, inflate_grids at 0.19, an octile flood towards the start, 64 players and their descent with a
    path of 64 on the device -- each pinned by its own tests -- then straighten_paths and walk_lines to the goal against the
    reference on goal_ref's planes inflated by walls_ref"""
    rd.set_device(0)
    index, cell, n = 0, 0.125, 2
    host = _wad().build_world(index, device=False)
    tables, g = sector_ref.Tables(host), host.area_grid(cell)
    at = goal_ref.level_sectors(tables, g, cell)
    world = _wad().build_world(index)
    pos, yaw = _wad().build_level(index).start()
    st = rd.player_states(np.repeat(np.asarray(pos, F)[None], n, 0), np.full(n, yaw, F))
    off = sector_ref.random_offsets(np.random.default_rng(7), n, host.game_objects)
    off[0] = 0  # row 0: all at rest
    _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=[at])
    floor, ceiling, _ = walls_ref.inflate_grids(floor, ceiling, BODY, cell)
    goal = goal_ref.cells(g, cell, st)
    f_t, c_t = world.draw_area_planes(cell, offsets=_dev(off), floor=True, ceiling=True)
    f_t, c_t = rd.inflate_grids(f_t, c_t, BODY, cell)
    assert np.array_equal(f_t.cpu().numpy().view(np.uint32), floor.view(np.uint32)) and np.array_equal(c_t.cpu().numpy().view(np.uint32), ceiling.view(np.uint32))
    dist = rd.flood_grids_octile(f_t, c_t, world.area_cells(_dev(np.ascontiguousarray(st).view(np.uint8).reshape(-1)), cell), towards=True,
                                 max_step=E2E_STEP)
    field = dist.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(5)
    which = np.arange(64) % n
    starts = np.zeros((64, 2), np.int32)
    for k, p in enumerate(which):
        rows, cols = np.nonzero(field[p] != U)
        at_k = rng.integers(len(rows))
        starts[k] = cols[at_k], rows[at_k]
    starts[:2] = [(-1, -1), (g.gw, 0)]
    big = lambda t: t[torch.from_numpy(which).cuda()].contiguous()
    kw = dict(towards=True, max_step=E2E_STEP)
    _, made_t, path_t = rd.descend_grids_octile(big(f_t), big(c_t), big(dist), _dev(starts), max_moves=64, path_out=64, **kw)
    path, made = path_t.cpu().numpy(), made_t.cpu().numpy()
    moves = [line_ref.moves_of(floor[p], ceiling[p], max_step=E2E_STEP) for p in range(n)]
    moves = [moves[p] for p in which]
    want = line_ref.straighten_paths(None, None, starts, path, True, 64, 8, moves=moves)
    assert (want[1] < made).sum() >= 40 and (want[1][:2] == 0).all() and ((want[1] >= 1) == (made > 0)).all(), (want[1], made)
    _same_pulled(_pulled(big(f_t), big(c_t), _dev(starts), path_t, 8, **kw), want, 'E1M1, pulled straight')
    targets = np.stack([goal[which], want[0][:, 0]], 1).astype(np.int32)  # the goal, and the any-angle waypoint
    for rev in (False, True):
        lines = line_ref.walk_lines(None, None, starts, targets, rev, moves=moves)
        assert rev or lines[0][made > 0, 1].all()  # the waypoint is a straight walk away, in the walk's direction
        _same_lines(_lines(big(f_t), big(c_t), _dev(starts), _dev(targets), reversed=rev, max_step=E2E_STEP), lines[:2], ('E1M1, lines', rev))
    assert 0 < line_ref.walk_lines(None, None, starts, targets, False, moves=moves)[0][:, 0].sum() < 64  # some see the goal, not all


# ---- streams, tensors, pointers, a graph -------------------------------------------------------------------------------------------------

def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_line_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_line_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
