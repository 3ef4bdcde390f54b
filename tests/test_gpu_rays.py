"""Range-sensor rays on the GPU (world.hip cast_rays_kernel / worldset_cast_rays_kernel) against the test-side restatement
(tests/rays_restatement.c), bit for bit; doors moved by the game step; world sets; the relation to the shipped radius-0 sweep;
the central ray against the depth plane of the same players' frames; streams; argument checks."""
import ctypes

import numpy as np
import pytest

import rays_ref
import rust_doom_amd as rd
import world_ref
from test_game_host import patched_variant
from test_rays_host import LEVEL_IDS, check_hits_lie_on_their_triangles, levels, sweep_relation
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _dirs(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


def _cast_all(world, st, dirs, max_range, offsets=None, levels_t=None):
    """every output of a cast as numpy: frac, hit (uint32), origin, vel"""
    n, r = len(st), len(dirs)
    origin = torch.empty((n, r, 3), dtype=torch.float32, device='cuda')
    vel = torch.empty((n, r, 3), dtype=torch.float32, device='cuda')
    args = (_dev(st),) + ((levels_t,) if levels_t is not None else ()) + (_dirs(dirs), max_range)
    frac, hit = world.cast_rays(*args, offsets=offsets, hit_out=True, origin_out=origin, vel_out=vel)
    torch.cuda.synchronize()
    return dict(frac=frac.cpu().numpy(), hit=hit.cpu().numpy().view(np.uint32), origin=origin.cpu().numpy(), vel=vel.cpu().numpy())


def _assert_equal(got, want, what):
    for k in ('frac', 'hit', 'origin', 'vel'):
        bad = _u32(got[k]) != _u32(want[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:3], got[k][bad][:3], want[k][bad][:3])


@pytest.mark.parametrize('path,index', levels(), **LEVEL_IDS)
def test_cast_rays_matches_the_restatement(path, index):
    rd.set_device(0)
    wad = rd.Wad(path, META_PATH)
    built = wad.build_level(index)
    world, ref = wad.build_world(index), world_ref.RefWorld(wad, index)
    st = rays_ref.players(built, 9000 + index, count=4096)
    fan = rd.ray_fan(64, 2.0)
    for max_range in rays_ref.RANGES:
        got, want = _cast_all(world, st, fan, max_range), rays_ref.cast(ref, st, fan, max_range)
        _assert_equal(got, want, 'fan %g' % max_range)
    assert np.isfinite(want['frac']).any()
    # waves that straddle players: 1, 7 and 100 rays (7: the pitched, unnormalised table)
    few = st[:517]
    for dirs in (rd.ray_fan(1, 2.0), rays_ref.odd_table(), rd.ray_fan(100, 3.0, pitch=0.1)):
        _assert_equal(_cast_all(world, few, dirs, 30.0), rays_ref.cast(ref, few, dirs, 30.0), '%d rays' % len(dirs))
    # frac alone, into a preallocated tensor
    out = torch.full((len(few), 64), -1.0, dtype=torch.float32, device='cuda')
    res = world.cast_rays(_dev(few), _dirs(fan), 30.0, frac_out=out)
    assert res is out
    assert np.array_equal(_u32(out.cpu().numpy()), _u32(rays_ref.cast(ref, few, fan, 30.0)['frac']))


def _front(trig, dist):
    mid = trig['origin'] + trig['displace'] * (trig['length'] * F(0.5))
    normal = np.array([-trig['displace'][1], trig['displace'][0]], F)
    p = mid + normal * F(dist)
    face = -normal
    return p, float(np.arctan2(-face[0], -face[1]))


def test_rays_see_a_door_the_game_step_opened(tmp_path):
    """on the patched E1M1: players in front of a manual door push it; with the offsets tensor the step left, the rays that
    ended on the door at rest pass under it or end further away, the rays that still end on it name its object, and every ray
    equals the restatement under the same offsets"""
    rd.set_device(0)
    wad_path, meta_path = patched_variant(str(tmp_path))
    wad = rd.Wad(wad_path, meta_path)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    tri_objects = world.triangle_objects()
    arrays = world.arrays()
    assert np.array_equal(tri_objects[:arrays['n_static_triangles']], np.zeros(arrays['n_static_triangles'], np.uint32))
    assert set(tri_objects[arrays['n_static_triangles']:]) == set(arrays['dynamics'][:, 0])
    fan = np.concatenate([rd.ray_fan(33, 1.2), rd.ray_fan(31, 1.2, pitch=0.6)])  # level rays, and rays that look up at the lintel
    found = None
    for i in np.nonzero(trig['special_type'] == 1)[0]:
        e = effs[trig['effect_start'][i]:trig['effect_end'][i]]
        if len(e) != 1 or e[0]['first_height_offset'] < 0.9:
            continue
        door = int(e[0]['object_id'])
        p, yaw = _front(trig[i], 0.45)
        # the floor under the point: a ray straight down from one unit up (the restatement's)
        probe = rd.player_states([[p[0], 1.0, p[1]]], yaw, pitch=0.0)
        down = rays_ref.cast(ref, probe, np.array([[0, -1, 0]], F), 4.0)
        if not np.isfinite(down['frac'][0, 0]):
            continue
        floor = float(down['origin'][0, 0, 1]) - 4.0 * float(down['frac'][0, 0])
        st = rd.player_states([[p[0], floor + 0.21, p[1]]], yaw)
        rest = rays_ref.cast(ref, st, fan, 30.0)
        on_door = tri_objects[np.where(rest['hit'] == rays_ref.NO_HIT, 0, rest['hit'])] == door
        if on_door[0, :33].sum() >= 8:
            found = (i, door, st)
            break
    assert found is not None, 'no manual door with a floor in front'
    i, door, st = found
    n = 64
    st = np.repeat(st, n)
    st['yaw'] += np.linspace(-0.15, 0.15, n).astype(F)
    states = _dev(st)
    rest = _cast_all(world, st, fan, 30.0)
    _assert_equal(rest, rays_ref.cast(ref, st, fan, 30.0), 'at rest')
    ticks = 90
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    act = np.zeros((ticks, n), np.uint8)
    act[0, ::2] = rd.ACTION_PUSH  # every other player opens its door
    game, offs = world.game_state(n)
    world.step_game(states, _dev(inp), game, offs, actions=_dev(act), n_ticks=ticks)
    torch.cuda.synchronize()
    off_np = offs.cpu().numpy()
    lifted = off_np[:, door, 1]
    assert (lifted[::2] > 0.5).all() and (lifted[1::2] == 0).all(), lifted[:4]
    st2 = states.cpu().numpy().view(rd.PLAYER_STATE).reshape(-1)
    n_obj = int(offs.shape[1])
    origin = torch.empty((n, len(fan), 3), dtype=torch.float32, device='cuda')
    vel = torch.empty_like(origin)
    frac, hit = world.cast_rays(states, _dirs(fan), 30.0, offsets=offs, hit_out=True, origin_out=origin, vel_out=vel)
    torch.cuda.synchronize()
    got = dict(frac=frac.cpu().numpy(), hit=hit.cpu().numpy().view(np.uint32), origin=origin.cpu().numpy(), vel=vel.cpu().numpy())
    want = rays_ref.cast(ref, st2, fan, 30.0, off_np)
    _assert_equal(got, want, 'door open')
    check_hits_lie_on_their_triangles(arrays, want, off_np, tri_objects.astype(np.int64))
    # the same rays before and after (the players stood still: the same origins up to the settling of the first ticks)
    before = rays_ref.cast(ref, st2, fan, 30.0)
    obj = lambda h: np.where(h == rays_ref.NO_HIT, 0, tri_objects[np.where(h == rays_ref.NO_HIT, 0, h)])
    was_door = obj(before['hit']) == door
    opened = np.zeros(n, bool)
    opened[::2] = True
    level_rays = np.zeros(len(fan), bool)
    level_rays[:33] = True
    through = was_door & opened[:, None] & level_rays[None, :]
    assert through.sum() >= 8 * 32
    assert (got['frac'][through] > before['frac'][through]).all()  # (+inf included: nothing else within range)
    assert np.array_equal(_u32(got['frac'][~opened]), _u32(before['frac'][~opened]))  # a closed door is where it was
    still = (obj(got['hit']) == door) & opened[:, None]
    assert still.any(), 'no ray looks up at the lifted door'
    door_tris = arrays['triangles'][tri_objects == door]
    bottom = arrays['verts'][door_tris[:, :3].reshape(-1), 1].min()
    speed = np.linalg.norm(got['vel'].astype(np.float64), axis=2)
    y = got['origin'][..., 1] + got['vel'][..., 1] / speed * (got['frac'].astype(np.float64) * speed)
    rows = np.nonzero(still)[0]
    assert (y[still] >= bottom + lifted[rows] - 1e-3).all()  # ... and ends on the door where the door now is


def test_world_set_rays_equal_each_level_alone():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 4]
    ws = wad.build_world_set(slots)
    worlds = [wad.build_world(i) for i in slots]
    builts = [wad.build_level(i) for i in slots]
    per = 1024
    fan = rd.ray_fan(64, 2.0)
    sts = [rays_ref.players(builts[s], 300 + s, count=per) for s in range(3)]
    single = [_cast_all(worlds[s], sts[s], fan, 30.0) for s in range(3)]
    for s in range(3):  # a slot's arrays are the level's own, so the hit indices mean the same
        assert np.array_equal(ws.arrays(s)['triangles'], worlds[s].arrays()['triangles'])
        assert np.array_equal(ws.triangle_objects(s), worlds[s].triangle_objects())
    st = np.concatenate(sts)
    lv = np.repeat(np.arange(3), per).astype(np.int32)
    want = {k: np.concatenate([single[s][k] for s in range(3)]) for k in single[0]}
    rng = np.random.default_rng(8)
    for name, order in (('grouped', np.arange(3 * per)), ('shuffled', rng.permutation(3 * per))):
        for dirs, w in ((fan, want), (rays_ref.odd_table(), None)):  # 7 rays: mixed waves even when grouped
            if w is None:
                w1 = [_cast_all(worlds[s], sts[s], dirs, 30.0) for s in range(3)]
                w = {k: np.concatenate([w1[s][k] for s in range(3)]) for k in w1[0]}
            got = _cast_all(ws, st[order], dirs, 30.0, levels_t=torch.from_numpy(lv[order]).cuda())
            _assert_equal(got, {k: v[order] for k, v in w.items()}, '%s %d rays' % (name, len(dirs)))
    # moved objects: the set takes the same offsets rows
    off = np.zeros((3 * per, ws.n_objects, 3), F)
    off[:, 1:, 1] = rng.uniform(-1, 1, (3 * per, ws.n_objects - 1)).astype(F)
    order = rng.permutation(3 * per)
    got = _cast_all(ws, st[order], fan, 30.0, offsets=torch.from_numpy(off[order]).cuda(), levels_t=torch.from_numpy(lv[order]).cuda())
    for s in range(3):
        rows = np.nonzero(lv[order] == s)[0]
        alone = _cast_all(worlds[s], st[order][rows], fan, 30.0, offsets=torch.from_numpy(off[order][rows]).cuda())
        _assert_equal({k: v[rows] for k, v in got.items()}, alone, 'offsets, slot %d' % s)
    # a slot outside the set: +inf / no hit, and nothing else of that player's rays is written
    bad = lv.copy()
    bad[[5, 700, 2049]] = [3, 0x7FFFFFFF, -1]
    origin = torch.full((3 * per, 64, 3), -7.0, dtype=torch.float32, device='cuda')
    vel = torch.full((3 * per, 64, 3), -7.0, dtype=torch.float32, device='cuda')
    frac, hit = ws.cast_rays(_dev(st), torch.from_numpy(bad).cuda(), _dirs(fan), 30.0, hit_out=True, origin_out=origin, vel_out=vel)
    torch.cuda.synchronize()
    frac, hit = frac.cpu().numpy(), hit.cpu().numpy().view(np.uint32)
    out = np.zeros(3 * per, bool)
    out[[5, 700, 2049]] = True
    assert np.isposinf(frac[out]).all() and (hit[out] == rd.RAY_NO_HIT).all()
    assert (origin.cpu().numpy()[out] == -7.0).all() and (vel.cpu().numpy()[out] == -7.0).all()
    assert np.array_equal(_u32(frac[~out]), _u32(want['frac'][~out])) and np.array_equal(hit[~out], want['hit'][~out])
    assert np.array_equal(_u32(origin.cpu().numpy()[~out]), _u32(want['origin'][~out]))


@pytest.mark.parametrize('path,index', [levels()[0], levels()[-1]], **LEVEL_IDS)
def test_rays_against_the_shipped_sweep(path, index):
    """both sides the library: the rays' own origin_out / vel_out with radius 0 through World.sweep.  The sweep can only be
    earlier (it takes the minimum over the plane branch and the vertex / edge branches), and is bit-identical on at least 99 % of
    the rays -- the condition of tests/test_rays_host.py, whose docstring has the reasoning and the restatements' own figure.
    max_range 1000, so that the time <= 1 cut removes (nearly) nothing."""
    rd.set_device(0)
    wad = rd.Wad(path, META_PATH)
    world = wad.build_world(index)
    st = rays_ref.players(wad.build_level(index), 9100 + index, count=4096)
    fan = _dirs(rd.ray_fan(64, 2.0))
    n = len(st)
    origin = torch.empty((n, 64, 3), dtype=torch.float32, device='cuda')
    vel = torch.empty_like(origin)
    frac = world.cast_rays(_dev(st), fan, 1000.0, origin_out=origin, vel_out=vel)
    spheres = torch.cat([origin.view(-1, 3), torch.zeros((n * 64, 1), dtype=torch.float32, device='cuda')], 1).contiguous()
    swept = world.sweep(spheres, vel.view(-1, 3))
    torch.cuda.synchronize()
    s, r = swept[:, 0].cpu().numpy(), frac.cpu().numpy().reshape(-1)
    cut = np.isinf(r) & (s > 1.0)  # the ray's range cut, not a difference
    s = np.where(cut, np.inf, s).astype(F)
    violations, same = sweep_relation(s, r)
    print('%d rays: %.4f %% bit-identical to World.sweep at radius 0, %d with sweep > ray' % (s.size, 100 * same, violations))
    assert violations == 0
    assert same >= 0.99, 'only %.4f %% of the rays equal the radius-0 sweep' % (100 * same)


def test_the_central_ray_against_the_depth_plane():
    """A loose check that ties the sensor to the frames: the central ray (-z) times max_range against Batch.read_depth at the
    centre of a 321 x 201 frame (odd, so the ray goes through the centre of the centre pixel) of render_players for the same
    states.  Only pixels that show a flat or a wall of the static level count.  rays_ref.depth_agreement has the tolerance --
    geometric slack for "same surface", not tuned to the library -- and the assertion is one-sided: collision geometry omits
    non-blocking walls, so a ray may see further than the frame, never nearer.  The sampled players are chosen by the
    restatement alone (central ray on a static triangle within range); tests/test_rays_host.py shows on the CPU that at least
    half of them match."""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    st = rays_ref.players(built, 77)
    pick, _ = rays_ref.depth_candidates(ref, st)
    pick = pick[:48]
    states = _dev(st[pick])
    w, h = rays_ref.DEPTH_FRAME
    batch = rd.Batch(rd.DeviceLevel(built), w, h, len(pick))
    batch.render_players(states, torch.from_numpy(built.lights_at(0.0).copy()).cuda())
    depth = batch.read_depth()
    label = batch.read_plane(rd.PLANE_LABEL)
    frac = world.cast_rays(states, _dirs([[0, 0, -1]]), rays_ref.DEPTH_RANGE)
    dist = frac.cpu().numpy()[:, 0].astype(np.float64) * rays_ref.DEPTH_RANGE
    usable, matches, nearer = rays_ref.depth_agreement(dist, depth, label)
    print('%d sampled, %d usable, %d match, %d nearer' % (len(pick), usable.sum(), matches.sum(), nearer.sum()))
    assert not nearer.any(), (np.nonzero(nearer)[0], dist[nearer], depth[nearer, h // 2, w // 2])
    assert 2 * matches.sum() >= len(pick), (usable.sum(), matches.sum())


def test_a_closed_loop_on_a_side_stream_and_a_captured_graph():
    """step_game -> cast_rays, tick after tick on one side stream with preallocated outputs and no host wait in between (the
    pattern of test_gpu_player_frames.py's closed loops); the last tick's rays are the restatement's for the last states and
    offsets.  Then the cast alone captured into a graph: a call that waited or allocated could not be captured."""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    n, ticks = 2048, 30
    st = rays_ref.players(wad.build_level(0), 5, count=n)
    fan = rd.ray_fan(64, 2.0)
    rng = np.random.default_rng(4)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0
    inp['look'][..., 0] = rng.normal(scale=0.02, size=(ticks, n)).astype(F)
    act = (rng.random((ticks, n)) < 0.2).astype(np.uint8) * rd.ACTION_PUSH
    states, dirs, ti, ta = _dev(st), _dirs(fan), _dev(inp), _dev(act)
    game, offs = world.game_state(n)
    frac = torch.empty((n, 64), dtype=torch.float32, device='cuda')
    hit = torch.empty((n, 64), dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(ticks):
        world.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=side)
        res = world.cast_rays(states, dirs, 30.0, offsets=offs, frac_out=frac, hit_out=hit, stream=side)
        assert res[0] is frac and res[1] is hit
    side.synchronize()
    last = states.cpu().numpy().view(rd.PLAYER_STATE).reshape(-1)
    off_np = offs.cpu().numpy()
    assert (off_np[:, :, 1] != 0).any()  # some doors moved
    want = rays_ref.cast(ref, last, fan, 30.0, off_np)
    assert np.array_equal(_u32(frac.cpu().numpy()), _u32(want['frac']))
    assert np.array_equal(hit.cpu().numpy().view(np.uint32), want['hit'])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        world.cast_rays(states, dirs, 30.0, offsets=offs, frac_out=frac, hit_out=hit, stream=torch.cuda.current_stream())
    frac.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_u32(frac.cpu().numpy()), _u32(want['frac']))


def test_argument_checks_queue_nothing():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(0), wad.build_world_set([0, 2])
    host_only, host_set = wad.build_world(0, device=False), wad.build_world_set([0, 2], device=False)
    st = rays_ref.players(wad.build_level(0), 6, count=64)
    states, dirs = _dev(st), _dirs(rd.ray_fan(8, 1.0))
    lv = torch.zeros(64, dtype=torch.int32, device='cuda')
    frac = torch.full((64, 8), -3.0, dtype=torch.float32, device='cuda')
    small = torch.zeros((64, 1, 3), dtype=torch.float32, device='cuda')
    assert world.n_objects > 1
    L = rd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    BAD = -1  # RDOOM_BAD_ARG

    def one(h=world, st_=states, n=64, d=dirs, r=8, rng=30.0, off=None, no=0, fr=frac):
        return L.rdoom_world_cast_rays(h._h if h is not None else None, p(st_), n, p(d), r, ctypes.c_float(rng), p(off), no, p(fr), None,
                                       None, None, None)

    def many(h=ws, st_=states, lv_=lv, n=64, d=dirs, r=8, rng=30.0, off=None, no=0, fr=frac):
        return L.rdoom_worldset_cast_rays(h._h if h is not None else None, p(st_), p(lv_), n, p(d), r, ctypes.c_float(rng), p(off), no,
                                          p(fr), None, None, None, None)

    for call in (one, many):
        for kw in (dict(h=None), dict(st_=None), dict(d=None), dict(fr=None), dict(r=0), dict(rng=0.0), dict(rng=-1.0),
                   dict(rng=float('inf')), dict(rng=float('nan')), dict(off=small, no=1)):
            assert call(**kw) == BAD, (call.__name__, kw)
            assert rd.lib().rdoom_last_error()
    assert many(lv_=None) == BAD
    assert one(h=host_only) == BAD and many(h=host_set) == BAD
    torch.cuda.synchronize()
    assert (frac == -3.0).all().item()  # nothing was queued
    assert one(n=0) == 0 and many(n=0) == 0
    torch.cuda.synchronize()
    assert (frac == -3.0).all().item()
    assert one() == 0 and many() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(frac).any().item() and not (frac == -3.0).any().item()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        world.cast_rays(states, _dirs(np.zeros((0, 3), F)), 30.0)
    with pytest.raises(ValueError):
        world.cast_rays(states.cpu(), dirs, 30.0)
    with pytest.raises(ValueError):
        world.cast_rays(states, dirs, 30.0, frac_out=torch.empty((64, 7), dtype=torch.float32, device='cuda'))
    with pytest.raises(ValueError):
        ws.cast_rays(states, lv[:5], dirs, 30.0)
    with pytest.raises(rd.RdoomError):
        world.cast_rays(states, dirs, -2.0)
