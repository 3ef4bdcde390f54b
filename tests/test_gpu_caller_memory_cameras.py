"""GPU: WHERE the camera and light kernels write (frames.hip, lights.hip).  rdoom_poses_from_players_device and its clocked form
with states, offsets, times, poses and modelviews in carvings of a guarded arena (tests/guarded.py) at 4 and 12 mod 16, for 1, 63
and 65 players and for 63 of 65 -- the wave's tail; rdoom_lightset_tables into a carving, its last rows left alone; and
rdoom_batch_render_players with the levels' light tables at 1 mod 16, where frames.hip copies them byte by byte, at 0, where it
copies sixteen uint4, and shared at 3.  Expected values: tests/frames_ref.py, tests/lights_ref.py, the oracle's frames; every
byte outside the outputs must be what it was, with the arena poisoned 0xFF and 0x00."""
import ctypes

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import frames_ref
import lights_ref
import rust_doom_amd as rd
from guarded import GUARD, run_guarded
from util import META_PATH, ensure_wad

pytestmark = pytest.mark.gpu
F = np.float32
N_OBJ = 5
W, H = 77, 31


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def players(n, seed):
    """n states anywhere, turned far (yaw in +-60 pi) and some looking straight up or down, with offsets of which a third are zero"""
    rng = np.random.default_rng(seed)
    lim = F(1.57079637) - F(1e-2)
    st = rd.player_states(rng.uniform(-40.0, 40.0, (n, 3)).astype(F), rng.uniform(-60 * np.pi, 60 * np.pi, n).astype(F))
    st['pitch'] = rng.uniform(-1.5, 1.5, n).astype(F)
    st['pitch'][::5] = lim
    st['vel'] = rng.normal(size=(n, 3)).astype(F)
    offs = rng.uniform(-2.0, 2.0, (n, N_OBJ, 3)).astype(F)
    offs[rng.random((n, N_OBJ)) < 0.33] = 0.0
    offs[:, 0] = 0.0
    return st, offs, rng.uniform(0.0, 100.0, n).astype(F)


@pytest.mark.parametrize('clocked', [False, True], ids=['one_time', 'clocked'])
@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', [(1, 1), (63, 63), (65, 65), (63, 65)])
def test_poses_from_players_device(n, held, residue, clocked):
    """`held` players in every array, n of them asked for: players n .. held keep the poison"""
    rd.set_device(0)
    st, offs, times = players(held, 1000 + held)
    want_p, want_m = frames_ref.cameras(st[:n], W, H, 2.5, offs[:n])
    if clocked:
        want_p['time'] = times[:n]
    assert rd.POSE.itemsize == 136 and (n == 1 or (residue + 136) % 16 != residue)  # pose 1 is aligned differently from pose 0

    def setup(arena):
        d_st = arena.place(st, 16, residue, 'states')
        d_off = arena.place(offs, 16, residue, 'offsets', torch.float32)
        d_t = arena.place(times, 16, residue, 'times', torch.float32)
        poses = arena.carve((held, 34), torch.float32, 16, residue, 'poses_out')
        mvs = arena.carve((held, N_OBJ, 16), torch.float32, 16, residue, 'modelviews_out')
        for t in (d_st, d_off, d_t, poses, mvs):
            assert t.data_ptr() % 16 == residue

        def call():
            if clocked:
                rd._check(rd.lib().rdoom_poses_from_players_device_clocked(ptr(d_st), n, W, H, ptr(d_t), ptr(d_off), N_OBJ, ptr(poses), ptr(mvs), None))
            else:
                rd._check(rd.lib().rdoom_poses_from_players_device(ptr(d_st), n, W, H, ctypes.c_float(2.5), ptr(d_off), N_OBJ, ptr(poses), ptr(mvs),
                                                                   None))
        return call, [('poses', poses[:n], want_p.view(np.uint32).reshape(n, 34)), ('modelviews', mvs[:n], want_m)]
    run_guarded(held * (40 + N_OBJ * 12 + 4 + 136 + N_OBJ * 64) + 8 * (GUARD + 64), setup,
                'poses_from_players_device n=%d of %d at %d clocked=%s' % (n, held, residue, clocked))


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', [(1, 1), (65, 65), (63, 65)])
def test_lightset_tables(n, held, residue):
    """rdoom_lightset_tables has no stride: rows are 256 bytes apart, so what lies behind row n - 1 is rows n .. held of the same
    carving, which must keep the poison, and the guard band.  Two levels, one with 37 lights: a last dword of one byte and zeros"""
    rd.set_device(0)
    infos = [lights_ref.handwritten_infos(15), lights_ref.handwritten_infos(16)[:37]]
    rng = np.random.default_rng(n * 7 + residue)
    times = rng.uniform(0.0, 3600.0, held).astype(F)
    levels = rng.integers(0, 2, held).astype(np.int32)
    levels[0] = 1
    want = np.stack([lights_ref.tables(infos[levels[p]], times[p:p + 1])[0] for p in range(n)])
    assert (want[levels[:n] == 1][:, 37:] == 0).all() and len(np.unique(want)) > 8
    lights = rd.DeviceLights(infos)

    def setup(arena):
        d_t = arena.place(times, 16, residue, 'times', torch.float32)
        d_l = arena.place(levels, 16, residue, 'levels', torch.int32)
        out = arena.carve((held, 256), torch.uint8, 16, residue, 'tables')
        assert out.data_ptr() % 16 == residue

        def call():
            rd._check(rd.lib().rdoom_lightset_tables(lights._h, ptr(d_l), ptr(d_t), n, ptr(out), None))
        return call, [('tables', out[:n], want)]
    run_guarded(held * 264 + 4 * (GUARD + 64), setup, 'lightset_tables n=%d of %d at %d' % (n, held, residue))


_render = {}


def render_scene():
    """two levels of the IWAD as one set, five players at and around their starts, and the oracle's frames of their cameras"""
    if not _render:
        from oracle import raster
        from test_gpu_player_frames import _exact_poses
        wad = rd.Wad(ensure_wad(), META_PATH)
        built = [wad.build_level(i) for i in (0, 1)]
        lop = np.array([0, 1, 1, 0, 1], np.int32)
        rng = np.random.default_rng(5)
        pos = np.array([built[k].start()[0] for k in lop], F)
        yaw = np.array([built[k].start()[1] for k in lop], F) + rng.normal(scale=0.8, size=5).astype(F)
        st = rd.player_states(pos, yaw)
        table = np.stack([b.lights_at(0.75) for b in built])
        assert not np.array_equal(table[0], table[1])
        w, h = 160, 100
        poses, _ = frames_ref.cameras(st, w, h, 0.75)
        exact = _exact_poses(poses, None, 0)  # the poses whose sky angle the host and the device round alike
        assert exact.any()
        oracles = [raster.RasterOracle(b.arrays()) for b in built]
        want = np.stack([oracles[lop[p]].render(poses[p]['modelview'], poses[p]['projection'], 0.75, table[lop[p]], w, h) for p in range(5)])
        lset = rd.DeviceLevelSet(built)
        plain = rd.Batch(lset, w, h, 5)  # the same call with ordinary tensors
        plain.render_players(torch.from_numpy(st.view(np.uint8).copy()).cuda(), torch.from_numpy(table).cuda(),
                             levels=torch.from_numpy(lop).cuda(), time=0.75)
        ordinary = plain.read_framebuffer()
        assert np.array_equal(ordinary[exact], want[exact])
        _render.update(st=st, lop=lop, table=table, size=(w, h), poses=poses, exact=exact, want=want, ordinary=ordinary, lset=lset, built=built)
    return _render


@pytest.mark.parametrize('residue', [4, 12])
def test_render_players_clocked(residue):
    """the clocked render takes no caller's light tables: its states, slots and times in carvings, every clock at 0.75.  The frames
    are the oracle's with tests/lights_ref.py's tables at that time, on the poses whose sky angle the host rounds as the device does"""
    from oracle import raster
    rd.set_device(0)
    s = render_scene()
    w, h = s['size']
    infos = [b.light_infos() for b in s['built']]
    table = np.stack([lights_ref.tables(i, np.array([0.75], F))[0] for i in infos])
    oracles = [raster.RasterOracle(b.arrays()) for b in s['built']]
    want = {p: oracles[s['lop'][p]].render(s['poses'][p]['modelview'], s['poses'][p]['projection'], 0.75, table[s['lop'][p]], w, h)
            for p in np.nonzero(s['exact'])[0]}
    lights = rd.DeviceLights(s['built'])
    times = np.full(5, 0.75, F)
    frames = []

    def setup(arena):
        d_st = arena.place(s['st'], 16, residue, 'states')
        d_lv = arena.place(s['lop'], 16, residue, 'levels', torch.int32)
        d_t = arena.place(times, 16, residue, 'times', torch.float32)
        poses = arena.carve((5, 34), torch.float32, 16, residue, 'poses_out')
        batch = rd.Batch(s['lset'], w, h, 5)

        def call():
            rd._check(rd.lib().rdoom_batch_render_players_clocked(batch._h, ptr(d_st), ptr(d_lv), None, 0, lights._h, ptr(d_t), 5, rd.ALL_KINDS, 0,
                                                                  None, ptr(poses), None))
            batch.last_n = 5
            frames.append(batch.read_framebuffer())
        return call, [('poses', poses, s['poses'].view(np.uint32).reshape(5, 34))]
    run_guarded(5 * (40 + 4 + 4 + 136) + 5 * (GUARD + 64), setup, 'render_players_clocked at %d' % residue)
    assert len(frames) == 2 and np.array_equal(frames[0], frames[1]) and len(want) > 0
    for p, frame in want.items():
        assert np.array_equal(frames[0][p], frame), p


@pytest.mark.parametrize('residue,stride', [(1, 256), (0, 256), (3, 0)], ids=['bytes', 'uint4', 'shared'])
def test_render_players_light_tables(residue, stride):
    """frames.hip's copy of a level's light table both ways: at 1 mod 16 both levels' tables are copied byte by byte, at 0 as sixteen
    uint4 (a stride of 256, the only one the entry point takes beside 0, keeps level 1 aligned when level 0 is)"""
    rd.set_device(0)
    s = render_scene()
    w, h = s['size']
    table = s['table'] if stride else s['table'][:1]
    lop = s['lop'] if stride else np.zeros(5, np.int32)
    want_p = s['poses'].view(np.uint32).reshape(5, 34)
    frames = []

    def setup(arena):
        d_st = arena.place(s['st'], 16, 4, 'states')
        d_lv = arena.place(s['lop'], 16, 4, 'levels', torch.int32)
        d_li = arena.place(table, 16, residue, 'lights')
        poses = arena.carve((5, 34), torch.float32, 16, 12, 'poses_out')
        aligned = [(d_li.data_ptr() + int(k) * stride) % 16 == 0 for k in set(lop.tolist())]
        assert all(aligned) if residue == 0 else not any(aligned)  # frames.hip's condition, for every table this render reads
        batch = rd.Batch(s['lset'], w, h, 5)

        def call():
            rd._check(rd.lib().rdoom_batch_render_players(batch._h, ptr(d_st), ptr(d_lv), None, 0, ptr(d_li), stride, ctypes.c_float(0.75), 5,
                                                          rd.ALL_KINDS, 0, None, ptr(poses), None))
            batch.last_n = 5
            frames.append(batch.read_framebuffer())
        return call, [('poses', poses, want_p)]
    run_guarded(5 * (40 + 4 + 136) + 512 + 5 * (GUARD + 64), setup, 'render_players lights at %d stride %d' % (residue, stride))
    assert len(frames) == 2 and np.array_equal(frames[0], frames[1])
    if stride:
        assert np.array_equal(frames[0], s['ordinary']) and np.array_equal(frames[0][s['exact']], s['want'][s['exact']])
    else:  # every level with level 0's table: the players of level 0 show what they showed
        mine = s['lop'] == 0
        assert np.array_equal(frames[0][mine], s['ordinary'][mine]) and np.array_equal(frames[0][mine & s['exact']], s['want'][mine & s['exact']])


@pytest.mark.parametrize('residue', [1, 2, 3])
def test_light_tables_off_a_dword_boundary_are_refused(residue):
    """rdoom_lightset_tables asks for 4 bytes: less is RDOOM_BAD_ARG, and nothing is queued"""
    from guarded import Arena
    rd.set_device(0)
    lights = rd.DeviceLights([lights_ref.handwritten_infos(15)])
    arena = Arena(3 * 260 + 3 * (GUARD + 64), 0xFF)
    d_t = arena.place(np.array([0.5, 1.5, 2.5], F), 16, 4, 'times', torch.float32)
    out = arena.carve((3, 256), torch.uint8, 16, residue, 'tables')
    assert out.data_ptr() % 4 == residue
    arena.snapshot()
    assert rd.lib().rdoom_lightset_tables(lights._h, None, ptr(d_t), 3, ptr(out), None) == -1
    assert '4-byte aligned' in rd.lib().rdoom_last_error().decode()
    arena.check(written=[], what='light tables at %d' % residue)
