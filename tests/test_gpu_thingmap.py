"""The thing maps on the GPU (thingmap.hip draw_thing_maps_kernel) against tests/thingmap_ref.py, the header's "thing maps" restated
in numpy with no cull, no tiles and no list: every byte of every map and every index, with no tolerance.  E1M1's own table with
players near things, on NaNs and far outside; custom tables at the word, wave and pass boundaries with hidden and known rows, a
codes table and a wider stride; a heap of things longer than the kernel's list; the seams between tiles and the window's edges;
RDOOM_THING_MARKS_OVER on a line map and on poison; a set of three levels; every output alone and the argument errors that read the
set; streams, raw pointers, the collecting walk and a captured graph in a child process."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import automap_ref
import rust_doom_amd as rd
import things_ref
import thingmap_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
POISON = 0xA5A5A5A5
SIZES = (1, 31, 32, 33, 255, 256, 257, 600)
LIST_CAPACITY = 768  # thingmap.hip LIST_CAP: the things a workgroup's LDS list holds; it is folded when fewer than 256 slots are free
SMALL = thingmap_ref.view_of(77, 53, 0.12)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _rows(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


@functools.lru_cache(maxsize=None)
def level(index=0):
    wad = rd.Wad(ensure_wad(), META_PATH)
    host = wad.build_world(index, device=False)
    return dict(wad=wad, index=index, host=host, lines=host.map_lines(), things=host.map_things())


def flags(view):
    return dict(rotate=view['rotate'], top_down=view['top_down'])


def same(got, want, what):
    got = got.cpu().numpy()
    bad = got != want
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:8], want[bad][:8])


def run(things, states, view, want, levels=None, hidden=None, known=None, over=None, what='', **kw):
    """one launch with both outputs, poisoned (or `over`: the bytes the call finds), against the reference's result `want`"""
    n = len(states)
    shape = (n, view['height'], view['width'])
    out = torch.full(shape, 0xEE, dtype=torch.uint8, device='cuda') if over is None else torch.from_numpy(np.ascontiguousarray(over)).cuda()
    index = torch.full(shape, 0x5EEEEEEE, dtype=torch.int32, device='cuda')
    got = things.draw_maps(_dev(states), view['width'], view['height'], view['scale'], levels=None if levels is None else _rows(levels),
                           hidden=None if hidden is None else _rows(hidden), known=None if known is None else _rows(known),
                           over=over is not None, out=out, index_out=index, **flags(view), **kw)
    assert got[0] is out and got[1] is index
    torch.cuda.synchronize()
    same(out, want[0], (what, 'out'))
    same(index, want[1], (what, 'index'))


# ---- 1. the level's own table ------------------------------------------------------------------------------------------------------

OWN_VIEWS = {'160x120 0.12 rotated': (1, 1.5), '160x120 0.30 top_down': (2, 1.5), '77x53 0.05 rotated top_down': (4, 0.5), '77x53 0.12': (5, 1.5)}


@functools.lru_cache(maxsize=None)
def own_case(name):
    """64 players near things of E1M1, two on NaNs, two far outside, in one of automap_ref.VIEWS, with min_radius 0 and 2.5"""
    k, spread = OWN_VIEWS[name]
    view = thingmap_ref.view_of(**automap_ref.VIEWS[k])
    table = level()['things']
    rng = np.random.default_rng(40 + k)
    st = things_ref.players_near(table, 68, rng, spread=spread)
    st['pos'][64, 0], st['pos'][65, 2] = np.nan, np.nan
    st['pos'][66, 0] += 4000.0
    st['pos'][67, 2] -= 90000.0
    return dict(view=view, states=st, table=table, want={r: thingmap_ref.draw(table, st, view, min_radius=r) for r in (0.0, 2.5)})


def check_own_case(name):
    """on the reference alone (runs on the CPU).  With min_radius 2.5 every near player's map holds a mark: the player lies within
    spread * sqrt 2 of a thing, which is inside the window's smaller half extent in each of these views, and a centre inside the
    window with a mark radius above 0.71 pixels covers the centre of the pixel that contains it"""
    c = own_case(name)
    view, spread = c['view'], OWN_VIEWS[name][1]
    assert len(c['table']) == 35
    assert spread * np.sqrt(2.0) < 0.5 * min(view['width'], view['height']) * view['scale']
    out, index, _ = c['want'][2.5]
    assert out[:64].reshape(64, -1).any(1).all()
    assert not out[64:].any() and (index[64:] == -1).all()  # on a NaN and far outside: nothing
    assert (index[:64].reshape(64, -1).max(1) >= 0).all() and index.max() < 35
    thin = c['want'][0.0][0]
    assert thin.any() and (thin != 0).sum() < (out != 0).sum()  # min_radius widens at least the things that have no radius


@pytest.mark.parametrize('name', list(OWN_VIEWS))
def test_the_levels_own_things(name):
    check_own_case(name)
    rd.set_device(0)
    c = own_case(name)
    things = rd.DeviceThings(c['table'])
    for r, want in c['want'].items():
        run(things, c['states'], c['view'], want, min_radius=r, what=(name, r))
    things.close()


# ---- 2. custom tables at the word, wave and pass boundaries -------------------------------------------------------------------------

CODES = [21, 9, 0, 9, 40, 255, 1, 3]  # one zero (powerups are not drawn), two categories on one code


@functools.lru_cache(maxsize=None)
def custom_case(size):
    """a random table of `size` things for 16 players near things of it; from 31 things on, three pairs by hand, each pair at one
    point and drawn for every player: things 0 and 1 of different codes on player 0, things 2 and 3 of one category on player 1,
    things 4 and 5 of the two categories that share a code in CODES on player 2"""
    d = level()
    rng = np.random.default_rng(7000 + size)
    near = np.stack([d['things']['x'], d['things']['z']], 1)
    table = things_ref.make_table(rng, size, things_ref.bounds_of(d['lines']), near)
    st = things_ref.players_near(table, 16, rng)
    words = things_ref.words_of(size)
    stride = words + 2
    hidden = rng.integers(0, 1 << 32, (16, stride), dtype=np.uint64).astype(U) & rng.integers(0, 1 << 32, (16, stride), dtype=np.uint64).astype(U)
    known = rng.integers(0, 1 << 32, (16, stride), dtype=np.uint64).astype(U) | rng.integers(0, 1 << 32, (16, stride), dtype=np.uint64).astype(U)
    hidden[:, words:], known[:, words:] = POISON, ~U(POISON)  # the words beyond the set's are not read
    if size >= 31:
        for pair, p, cats in (((0, 1), 0, (rd.THING_DECORATION, rd.THING_AMMO)), ((2, 3), 1, (rd.THING_WEAPON, rd.THING_WEAPON)),
                              ((4, 5), 2, (rd.THING_WEAPON, rd.THING_ARTIFACT))):
            for i, cat in zip(pair, cats):
                table['x'][i], table['z'][i], table['category'][i] = st['pos'][p, 0], st['pos'][p, 2], cat
        hidden[:, 0] &= ~U(63)
        known[:, 0] |= U(63)
    want = dict(hidden=thingmap_ref.draw(table, st, SMALL, hidden=hidden),
                known=thingmap_ref.draw(table, st, SMALL, known=known),
                both=thingmap_ref.draw(table, st, SMALL, hidden=hidden, known=known, codes=CODES, min_radius=1.25))
    return dict(states=st, table=table, hidden=hidden, known=known, want=want)


def check_custom_case(size):
    c = custom_case(size)
    for name, (out, index, covers) in c['want'].items():
        assert out.any(), (size, name)
        if size < 31:
            continue
        meet = [(cover >= 2, low >> U(20)) for cover, low in covers]
        assert any((two & (low != out[p])).any() for p, (two, low) in enumerate(meet)), (size, name)  # different codes on a pixel
        assert any((two & (low == out[p])).any() for p, (two, low) in enumerate(meet)), (size, name)  # one code, decided by the index
    out = c['want']['both'][0]
    assert set(np.unique(out)) <= set(CODES)
    if size >= 31:
        assert (c['want']['both'][1][2] == 4).any()  # the shared code: the lower index of the pair
    if size == 600:
        assert set(np.unique(out)) == set(CODES)
        assert (c['want']['hidden'][0] != c['want']['known'][0]).any()


@pytest.mark.parametrize('size', SIZES)
def test_custom_tables(size):
    check_custom_case(size)
    rd.set_device(0)
    c = custom_case(size)
    things = rd.DeviceThings(c['table'])
    assert things.words() == things_ref.words_of(size) == c['hidden'].shape[1] - 2
    run(things, c['states'], SMALL, c['want']['hidden'], hidden=c['hidden'], what=(size, 'hidden'))
    run(things, c['states'], SMALL, c['want']['known'], known=c['known'], what=(size, 'known'))
    run(things, c['states'], SMALL, c['want']['both'], hidden=c['hidden'], known=c['known'], codes=CODES, min_radius=1.25, what=(size, 'both'))
    things.close()


# ---- 3. the chunked path -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def heap_case():
    """1100 things within 0.5 units of one point and four players around it, at 0.05 units a pixel: more than any list of 16-byte
    entries in 16 KiB holds, so the tile that holds the heap is folded in chunks"""
    rng = np.random.default_rng(31)
    at = F([12.5, -7.25])
    table = np.zeros(1100, rd.THING)
    angle, dist = rng.uniform(0, 2 * np.pi, 1100), 0.5 * rng.uniform(0, 1, 1100) ** 3  # most of them close to the point
    table['x'], table['z'] = at[0] + dist * np.cos(angle), at[1] + dist * np.sin(angle)
    table['category'] = rng.integers(0, 8, 1100)
    table['radius'] = rng.uniform(0, 0.09, 1100)  # below min_radius 2 at this scale: every mark is 0.1 units
    st = rd.player_states(F([[at[0] + 0.3, 0, at[1]], [at[0], 0, at[1] - 0.4], [at[0] - 0.6, 0, at[1] + 0.6], [at[0] + 1.0, 0, at[1] + 0.9]]),
                          F([0.0, 1.0, 2.5, -2.0]))
    view = thingmap_ref.view_of(77, 53, 0.05, rotate=True)
    return dict(table=table, states=st, view=view, want=thingmap_ref.draw(table, st, view, min_radius=2.0))


def test_a_heap_longer_than_the_list_is_folded_in_chunks():
    c = heap_case()
    out, index, covers = c['want']
    assert len(c['table']) > 16 * 1024 // 16 > LIST_CAPACITY
    assert max(int(cover.max()) for cover, _ in covers) > 256  # whatever the capacity: some pixel folds more than a stride of things
    assert (index >= LIST_CAPACITY).any() and ((index >= 0) & (index < 256)).any() and len(np.unique(index)) > 50  # winners from the first chunk and the last
    rd.set_device(0)
    things = rd.DeviceThings(c['table'])
    run(things, c['states'], c['view'], c['want'], min_radius=2.0, what='heap')
    things.close()


# ---- 4. tile seams and the window's edges --------------------------------------------------------------------------------------------

def seam_table(view, pos):
    """a thing whose centre is the pixel corner (64, 64) (clamped into the window: the corner four tiles share at 160 x 120), and one
    half outside the window on each of its four edges; north-up, so q = (pos.x - v, pos.z - u), exactly in these numbers"""
    w, h, s = view['width'], view['height'], view['scale']
    corners = [(min(64, w - 1), min(64, h - 1)), (0, h / 2), (w, h / 2), (w / 2, 0), (w / 2, h)]
    table = np.zeros(len(corners), rd.THING)
    for k, (i, j) in enumerate(corners):
        u, v = (i - w / 2) * s, (j - h / 2) * s
        table['x'][k], table['z'][k] = pos[0] - v, pos[1] - u
    table['category'] = (rd.THING_KEY, rd.THING_AMMO, rd.THING_WEAPON, rd.THING_MONSTER, rd.THING_DECORATION)
    return table


@pytest.mark.parametrize('size', [(160, 120), (77, 53), (33, 31), (65, 97), (32, 32), (1, 1)])
def test_tile_seams_and_window_edges(size):
    pos = (-20.5, 9.25)
    st = rd.player_states(F([[pos[0], 0, pos[1]]] * 2), F([0.3, 0.3]))
    for top_down in (False, True):
        view = thingmap_ref.view_of(size[0], size[1], 0.125, top_down=top_down)
        table = seam_table(view, pos)
        want = thingmap_ref.draw(table, st, view, min_radius=3.0)
        out, index = want[0][0], want[1][0]
        if size == (160, 120):  # the mark at the shared corner lies in all four tiles, symmetrically
            j = 64 if not top_down else 120 - 64
            assert out[j - 1, 63] == out[j - 1, 64] == out[j, 63] == out[j, 64] == rd.MAP_THING + rd.THING_KEY
            assert (index == 0).sum() % 4 == 0 and (index[:, :64] == 0).sum() == (index[:, 64:] == 0).sum()
            for k, edge in ((1, index[:, 0]), (2, index[:, -1]), (3, index[-1 if top_down else 0]), (4, index[0 if top_down else -1])):
                assert (edge == k).sum() >= 4 and (index == k).sum() < 20  # half a disc of 3 pixels is in the window
        else:
            assert (index == 3).all() if size == (1, 1) else set(np.unique(index)) >= {-1, 0, 1, 2}  # one pixel: the largest code of the five
        rd.set_device(0)
        things = rd.DeviceThings(table)
        run(things, st, view, want, min_radius=3.0, what=(size, top_down))
        things.close()


# ---- 5. RDOOM_THING_MARKS_OVER -------------------------------------------------------------------------------------------------------

def test_marks_over_a_line_map_and_over_poison():
    rd.set_device(0)
    d, c = level(), own_case('160x120 0.12 rotated')
    view, st = c['view'], c['states'][:16]
    world = d['wad'].build_world(d['index'])
    lines = world.draw_maps(_dev(st), view['width'], view['height'], view['scale'], **flags(view)).cpu().numpy()
    assert (lines != 0).mean() > 0.01
    things = rd.DeviceThings(c['table'])
    for before in (lines, np.full(lines.shape, 0xAA, np.uint8)):
        want = thingmap_ref.draw(c['table'], st, view, min_radius=2.5, over=before)
        covered = want[1] >= 0
        assert covered.any() and np.array_equal(want[0][~covered], before[~covered]) and (want[0][covered] >= rd.MAP_THING).all()
        assert (before[covered] != 0).any()  # a mark replaces what it covers
        run(things, st, view, want, over=before, min_radius=2.5, what='over')
    # the colours of an overlaid map: the lines' for the lines, one per category for the marks
    overlaid = things.draw_maps(_dev(st), view['width'], view['height'], view['scale'], min_radius=2.5, over=True,
                                out=torch.from_numpy(lines).cuda(), **flags(view))
    rgb = torch.from_numpy(rd.THING_MAP_COLORS).cuda()[overlaid.long()].cpu().numpy()
    marks = overlaid.cpu().numpy() >= rd.MAP_THING
    assert rgb.shape == lines.shape + (3,) and np.array_equal(rgb[~marks], rd.MAP_COLORS[lines[~marks]]) and rgb[marks].any(1).all()
    things.close()


# ---- 6. a set of three levels --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def set_case():
    wad = level()['wad']
    hosts = [wad.build_world(i, device=False) for i in (0, 2, 7)]
    rng = np.random.default_rng(5)
    tables = [hosts[0].map_things(), things_ref.make_table(rng, 70, things_ref.bounds_of(hosts[1].map_lines()),
                                                           np.stack([hosts[1].map_things()['x'], hosts[1].map_things()['z']], 1)),
              hosts[2].map_things()[:9]]
    lv = np.array([0, 1, 2, 3, 1, 0, 2, 0xFFFFFFFF, 1, 2], U)
    st = np.concatenate([things_ref.players_near(tables[min(int(s), 2)], 1, rng) for s in lv])
    stride = things_ref.set_words(tables) + 2
    hidden = rng.integers(0, 1 << 32, (len(lv), stride), dtype=np.uint64).astype(U) & rng.integers(0, 1 << 32, (len(lv), stride), dtype=np.uint64).astype(U)
    return dict(tables=tables, levels=lv, states=st, hidden=hidden, want=thingmap_ref.draw(tables, st, SMALL, levels=lv, hidden=hidden))


def test_a_set_of_three_levels_with_a_slot_out_of_range():
    c = set_case()
    out, index, _ = c['want']
    outside = c['levels'] >= 3
    assert outside.sum() == 2 and not out[outside].any() and (index[outside] == -1).all()
    assert out[~outside].reshape(8, -1).any(1).all()
    assert [int(index[c['levels'] == s].max()) < len(c['tables'][s]) for s in range(3)] == [True] * 3
    rd.set_device(0)
    things = rd.DeviceThings(c['tables'])
    assert things.info()[:2] == (3, 3)
    run(things, c['states'], SMALL, c['want'], levels=c['levels'], hidden=c['hidden'], what='set')
    poison = np.full(out.shape, 0xAA, np.uint8)
    over = thingmap_ref.draw(c['tables'], c['states'], SMALL, levels=c['levels'], hidden=c['hidden'], over=poison)
    assert (over[0][outside] == 0xAA).all()
    run(things, c['states'], SMALL, over, levels=c['levels'], hidden=c['hidden'], over=poison, what='set, over')
    # without levels every player is in slot 0: a set of one level takes that, a set of three does not
    one = rd.DeviceThings(c['tables'][1])
    run(one, c['states'], SMALL, thingmap_ref.draw(c['tables'][1], c['states'], SMALL), what='no levels')
    with pytest.raises(rd.RdoomError) as e:
        things.draw_maps(_dev(c['states']), 77, 53, 0.12)
    assert e.value.status == -1 and 'levels' in str(e.value)
    things.close(), one.close()


# ---- 7. every output alone, and the errors that read the set ---------------------------------------------------------------------------

def test_every_output_alone():
    rd.set_device(0)
    c = custom_case(257)
    things = rd.DeviceThings(c['table'])
    states, want = _dev(c['states']), c['want']['hidden']
    hidden = _rows(c['hidden'])
    out = things.draw_maps(states, 77, 53, 0.12, hidden=hidden)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8
    same(out, want[0], 'out alone')
    index = things.draw_maps(states, 77, 53, 0.12, hidden=hidden, out=False, index_out=True)
    assert isinstance(index, torch.Tensor) and index.dtype == torch.int32
    same(index, want[1], 'index alone')
    both = things.draw_maps(states, 77, 53, 0.12, hidden=hidden, index_out=True)
    same(both[0], want[0], 'out of both'), same(both[1], want[1], 'index of both')
    with pytest.raises(rd.RdoomError) as e:
        things.draw_maps(states, 77, 53, 0.12, out=False)
    assert e.value.status == -1 and 'both outputs' in str(e.value)
    things.close()


def test_the_argument_errors_that_read_the_thing_set():
    rd.set_device(0)
    table = level()['things']
    one, two = rd.DeviceThings(table), rd.DeviceThings([table, table[:3]])
    assert one.words() == 2
    L = rd.lib()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device='cuda')  # two players at the origin in slot 0, and room for what the good calls write
    ptr, rows_at, out_at = (ctypes.c_void_p(buf.data_ptr() + 4 * k) for k in (0, 1024, 2048))
    view, marks = rd.MapView(77, 53, 0.12, 0.0, 0.0, 0), rd.ThingMarks(2.0, (ctypes.c_uint8 * 8)(*range(16, 24)), 0)

    def call(things, n=2, lv=ptr, hidden=None, known=None, stride=2):
        return L.rdoom_thingset_draw_maps(things._h, ptr, lv, n, ctypes.byref(view), ctypes.byref(marks), hidden, known, stride, out_at, None, None)

    def fails(word, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert word in L.rdoom_last_error().decode(), L.rdoom_last_error()

    fails('levels', two, lv=None)
    fails('levels', two, lv=None, n=0)
    fails('stride', one, hidden=rows_at, stride=1)
    fails('stride', one, known=rows_at, stride=1)
    fails('stride', two, known=rows_at, stride=0)
    assert call(one, stride=0) == 0  # without a row the stride is not looked at
    assert call(one, lv=None) == 0 and call(two) == 0 and call(one, hidden=rows_at, known=rows_at) == 0
    assert call(one, n=0) == 0 and call(two, n=0) == 0  # n == 0 queues nothing
    torch.cuda.synchronize()
    if rd.device_count() > 1:  # a set lives on the device that was current when it was created
        rd.set_device(1)
        fails('device', one)
        rd.set_device(0)
    empty = rd.DeviceThings([np.zeros(0, rd.THING)])  # a level may hold no thing
    out, index = empty.draw_maps(buf[:20].view(torch.uint8), 77, 53, 0.12, index_out=True)
    assert not out.any() and (index == -1).all()
    for t in (one, two, empty):
        t.close()


# ---- 8. streams, tensors, pointers, the walk and a graph ---------------------------------------------------------------------------------

def test_streams_raw_pointers_the_walk_and_a_graph_in_one_child():
    """tests/gpu_thingmap_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_thingmap_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]
