"""The flood on the GPU (flood.hip flood_maps_kernel) against tests/flood_ref.py's breadth-first search: every element of every
output, bit for bit.  Hand-made planes, several players a launch, each with its own grid and seed; grids that take hundreds of
passes -- a serpentine corridor, a spiral on the largest grid the library takes, a staircase that is walked right to left and
bottom to top only; the planes World.draw_sector_maps drew of E1M1 for 64 players in four views; a door open in one player's game
only; streams, the caller's tensors, raw pointers and a captured graph, in a child process; every argument error."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flood_ref
import rust_doom_amd as rd
import sector_ref
import world_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = flood_ref.UNREACHED
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')


def _run(floor, ceiling, seeds=None, **kw):
    """flood_maps of numpy planes on the device: (distances, counts) as numpy"""
    f, g = torch.from_numpy(np.ascontiguousarray(floor, F)).cuda(), torch.from_numpy(np.ascontiguousarray(ceiling, F)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(seeds, np.int32)).cuda() if seeds is not None else None
    dist, count = rd.flood_maps(f, g, s, count_out=True, **kw)
    return dist.cpu().numpy().view(np.uint16), count.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    assert got[0].dtype == np.uint16 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    bad = got[0] != want[0]
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[0][bad][:3], want[0][bad][:3])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def test_hand_made_planes_several_players_a_launch():
    rd.set_device(0)
    cases = flood_ref.hand_cases()
    groups = {}
    for c in cases:  # one launch per shape and set of limits, its players the cases of that shape
        groups.setdefault((c['floor'].shape, tuple(sorted(c['kw'].items()))), []).append(c)
    assert len(groups) >= 6 and max(len(g) for g in groups.values()) >= 10
    for (shape, kw), group in groups.items():
        floor, ceiling = np.stack([c['floor'] for c in group]), np.stack([c['ceiling'] for c in group])
        h, w = shape
        seeds = np.array([c['seed'] if c['seed'] is not None else (w // 2, h // 2) for c in group], np.int64).astype(np.int32)
        want = np.stack([c['want'] for c in group])
        want = (want, (want != U).reshape(len(group), -1).sum(1).astype(np.uint32))
        _same(_run(floor, ceiling, seeds, **dict(kw)), want, (shape, kw, [c['name'] for c in group]))
        if all(c['seed'] is None for c in group):
            _same(_run(floor, ceiling, None, **dict(kw)), want, (shape, kw, 'default seeds'))
    # the 7 x 5 grids again, each from every cell of it: 35 players a grid, against the search
    for c in cases:
        if c['floor'].shape != (5, 7):
            continue
        seeds = np.array([(col, row) for row in range(5) for col in range(7)], np.int32)
        floor, ceiling = np.repeat(c['floor'][None], 35, 0), np.repeat(c['ceiling'][None], 35, 0)
        _same(_run(floor, ceiling, seeds, **c['kw']), flood_ref.flood_maps(floor, ceiling, seeds, **c['kw']), c['name'])


@functools.lru_cache(maxsize=None)
def _long_grids():
    """name -> (floor, ceiling, seeds, the search's result): computed once, left unchanged"""
    out = {}
    f, g = flood_ref.serpentine(33, 31)
    far = flood_ref.flood(f, g, (0, 0))
    r, c = np.unravel_index(np.argmax(np.where(far == U, -1, far.astype(np.int64))), far.shape)
    seeds = np.array([(0, 0), (c, r), (16, 14)], np.int32)  # from either end, and from the middle both ways
    out['serpentine'] = (np.repeat(f[None], 3, 0), np.repeat(g[None], 3, 0), seeds)
    cells = rd.flood_max_cells()
    w = next(w for w in range(255, 2, -2) if cells % w == 0)
    f, g = flood_ref.spiral(w, cells // w)
    inner = flood_ref.flood(f, g, (0, 0))
    r, c = np.unravel_index(np.argmax(np.where(inner == U, -1, inner.astype(np.int64))), inner.shape)
    out['spiral'] = (np.stack([f, f]), np.stack([g, g]), np.array([(0, 0), (c, r)], np.int32))  # inwards and outwards
    f, g, seed = flood_ref.staircase()
    out['staircase'] = (np.stack([f, f]), np.stack([g, g]), np.array([seed, (0, 0)], np.int32))  # the way it goes, and against it
    return {k: v + (flood_ref.flood_maps(*v),) for k, v in out.items()}


@pytest.mark.parametrize('name', ['serpentine', 'spiral', 'staircase'])
def test_grids_that_take_many_passes(name):
    rd.set_device(0)
    floor, ceiling, seeds, want = _long_grids()[name]
    assert np.where(want[0] == U, 0, want[0]).max() > 400
    if name == 'spiral':
        assert floor[0].size == rd.flood_max_cells() and floor.shape[2] % 2 == 1
    if name == 'staircase':
        assert want[1][1] == 1  # against it: the seed alone
    _same(_run(floor, ceiling, seeds), want, name)


VIEWS = [
    dict(width=160, height=120, scale=0.12),
    dict(width=160, height=120, scale=0.12, rotate=True, top_down=True),
    dict(width=77, height=53, scale=0.30, rotate=True),
    dict(width=77, height=53, scale=0.30, top_down=True),
]
PLAYERS = 64
PLAYER_SEED = 2021  # (one with which no player's seed cell of the even-sized views falls into a wall)


@functools.lru_cache(maxsize=None)
def _e1m1():
    """the wad, the sector tables and 64 players at jittered floor centroids of sectors a body fits in"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    tables = sector_ref.Tables(wad.build_world(0, device=False))
    cent = wad.build_level(0).floor_centroids().astype(F)
    at = sector_ref.sector_at(tables, cent[:, [0, 2]])
    fits = np.zeros(len(cent), bool)
    inside = at != sector_ref.NONE
    fits[inside] = tables.sectors['ceiling'][at[inside]] - tables.sectors['floor'][at[inside]] >= F(0.56)
    rng = np.random.default_rng(PLAYER_SEED)
    pick = np.nonzero(fits)[0]
    pos = cent[pick[rng.integers(0, len(pick), PLAYERS)]]
    pos[:, [0, 2]] += rng.uniform(-0.1, 0.1, (PLAYERS, 2)).astype(F)
    return wad, tables, rd.player_states(pos, rng.uniform(-7, 7, PLAYERS).astype(F))


def _states(st):
    return torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize('view', range(len(VIEWS)))
def test_the_planes_of_e1m1_as_the_device_drew_them(view):
    rd.set_device(0)
    wad, tables, st = _e1m1()
    world = wad.build_world(0)
    kw = VIEWS[view]
    flags = {k: v for k, v in kw.items() if k in ('rotate', 'top_down')}
    w, h = kw['width'], kw['height']
    floor_t, ceiling_t = world.draw_sector_maps(_states(st), w, h, kw['scale'], floor=True, ceiling=True, **flags)
    floor, ceiling = floor_t.cpu().numpy(), ceiling_t.cpu().numpy()
    # explicit seeds for a third of the players: anywhere on the map, some of them in the void or closed
    rng = np.random.default_rng(40 + view)
    seeds = np.repeat(np.array([[w // 2, h // 2]], np.int32), PLAYERS, 0)
    explicit = np.arange(PLAYERS) % 3 == 2
    seeds[explicit] = np.stack([rng.integers(0, w, explicit.sum()), rng.integers(0, h, explicit.sum())], 1)
    want = flood_ref.flood_maps(floor, ceiling, seeds)
    # on the reference, from the planes the GPU drew
    is_open = np.stack([flood_ref.open_cells(floor[p], ceiling[p], 0.56) for p in range(PLAYERS)])
    assert (is_open & (want[0] == U))[~explicit].any(), 'no open cell is unreached'
    some = np.nonzero(~explicit)[0][:16]
    any_step = flood_ref.flood_maps(floor[some], ceiling[some], seeds[some], max_step=INF)
    assert (any_step[0] != want[0][some]).any(), 'no step blocks'
    assert (want[1][~explicit] > 1).all(), np.nonzero(want[1] <= 1)[0]
    assert (want[1][explicit] > 1).any()
    _same(_run(floor, ceiling, seeds), want, kw)
    # the default seeds are those seeds; the tensors the draw left, without a trip through the host
    dist = rd.flood_maps(floor_t, ceiling_t)
    assert np.array_equal(dist.cpu().numpy()[~explicit], want[0][~explicit])
    if view == 0:
        _same(_run(floor[some], ceiling[some], seeds[some], max_step=INF), any_step, 'any step')
        low = flood_ref.flood_maps(floor[some], ceiling[some], seeds[some], max_drop=0.24, clearance=0.0)
        _same(_run(floor[some], ceiling[some], seeds[some], max_drop=0.24, clearance=0.0), low, 'a limited drop, no clearance')


def test_a_door_blocks_the_flood_of_the_player_who_has_not_opened_it():
    """pairs of players 0.45 in front of every manual door of E1M4 that opens high enough (the recipe of test_gpu_game's _door),
    the door raised by hand-written offsets in the second player's game only.  The door's own cells are UNREACHED by the first
    and reached by the second, opening it closes no way, and behind some door (the synthetic levels stand most of their doors free
    in a room, where a walk round them leads to the same cells) lie cells only the second player reaches."""
    from test_gpu_game import _floor_y, _front
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ref = wad.build_world(3), world_ref.RefWorld(wad, 3)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    pairs, doors, lifts = [], [], []
    for i in np.nonzero(trig['special_type'] == 1)[0]:
        e = effs[trig['effect_start'][i]:trig['effect_end'][i]]
        if len(e) != 1 or e[0]['first_height_offset'] < 0.9:
            continue
        p, yaw = _front(trig[i:i + 1], 0.45)
        y = _floor_y(ref, p)
        if np.isfinite(y[0]):
            pairs.append(np.repeat(rd.player_states([[p[0, 0], y[0] + 0.25, p[0, 1]]], yaw), 2))
            doors.append(int(e[0]['object_id']))
            lifts.append(e[0]['first_height_offset'])
    assert len(doors) >= 4
    st = np.concatenate(pairs)
    off = np.zeros((len(st), world.game_objects, 3), F)
    for k, (door, lift) in enumerate(zip(doors, lifts)):
        off[2 * k + 1, door, 1] = lift
    w, h, scale = 77, 53, 0.05
    sector, floor, ceiling = world.draw_sector_maps(_states(st), w, h, scale, offsets=torch.from_numpy(off).cuda(), rotate=True,
                                                    sector_out=True, floor=True, ceiling=True)
    dist, count = rd.flood_maps(floor, ceiling, count_out=True)
    got = (dist.cpu().numpy(), count.cpu().numpy().view(np.uint32))
    _same(got, flood_ref.flood_maps(floor.cpu().numpy(), ceiling.cpu().numpy()), 'doors')
    sectors = world.map_sectors().sectors
    sec = sector.cpu().numpy().view(np.uint16)
    beyond = []
    for k, door in enumerate(doors):
        assert np.array_equal(sec[2 * k], sec[2 * k + 1])
        in_door = (sec[2 * k] != sector_ref.NONE16) & (sectors['ceiling_id'][np.minimum(sec[2 * k], len(sectors) - 1)] == door)
        shut, opened = got[0][2 * k], got[0][2 * k + 1]
        assert in_door.sum() > 4 and (shut[in_door] == U).all() and (opened[in_door] != U).any(), k
        assert (opened[shut != U] <= shut[shut != U]).all() and got[1][2 * k + 1] > got[1][2 * k] > 1, k  # opening a door closes no way
        beyond.append(int(((shut == U) & (opened != U) & ~in_door).sum()))
    assert max(beyond) > 20, beyond


def test_streams_tensors_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_flood_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_flood_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]


def test_argument_errors_by_status_and_text():
    rd.set_device(0)
    L = rd.lib()
    n, h, w = 3, 5, 7
    floor, ceiling = torch.zeros((n, h, w), device='cuda'), torch.ones((n, h, w), device='cuda')
    dist = torch.full((n, h, w), 7, dtype=torch.int16, device='cuda')
    count = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    cells = rd.flood_max_cells()
    v = ctypes.c_void_p
    nan = float('nan')

    def call(f=floor.data_ptr(), g=ceiling.data_ptr(), n=n, w=w, h=h, params=(0.24, INF, 0.56, 0), d=dist.data_ptr()):
        p = ctypes.byref(rd.FloodParams(*params)) if params is not None else None
        return L.rdoom_flood_maps(v(f), v(g), n, w, h, None, p, v(d), v(count.data_ptr()), None)

    def fails(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    fails('null params', params=None)
    fails('null', f=None)
    fails('null', g=None)
    fails('null', d=None)
    fails('0 x 5', w=0)
    fails('7 x 0', h=0)
    fails('too many', w=cells + 1, h=1)
    fails('too many', w=65536, h=65536)
    fails('flags', params=(0.24, INF, 0.56, 2))
    for k, name in enumerate(('max_step', 'max_drop', 'clearance')):
        for bad in (nan, -0.5):
            params = [0.24, INF, 0.56, 0]
            params[k] = bad
            fails(name, params=tuple(params))
    with pytest.raises(rd.RdoomError) as e:
        rd.flood_maps(floor, ceiling, max_step=nan)
    assert e.value.status == -1 and 'max_step' in str(e.value)
    with pytest.raises(rd.RdoomError):
        rd.flood_maps(torch.zeros((1, 1, cells + 1), device='cuda'), torch.ones((1, 1, cells + 1), device='cuda'))
    # nothing was queued by any of them, and n == 0 queues nothing either
    assert call(n=0) == 0 and call(n=0, f=None, g=None, d=None) == 0
    torch.cuda.synchronize()
    assert (dist == 7).all() and (count == 7).all()
    assert call() == 0  # the same arguments, valid
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == np.abs(np.arange(w) - 3)[None, None, :] + np.abs(np.arange(h) - 2)[None, :, None]).all() and (count == 35).all()
