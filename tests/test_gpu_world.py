"""The collision world on the GPU (world.hip: sweep_kernel, player_step_kernel) against the test-side restatement
(tests/world_restatement.c), bit for bit as uint32 views; physics invariants that do not rely on the restatement; the kernels'
resources; and step -> pose_from_player -> Batch.render end to end against the oracle."""
import importlib.util
import os

import numpy as np
import pytest

import rust_doom_amd as rd
import world_ref
from step_cases import players as _players, script as _script  # (moved there; the same bytes)
from util import META_PATH, ROOT, ensure_big_wad, ensure_wad, render_checked

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

_syn = __import__('importlib').import_module('rust-doom_amd.synthetic')


def _u32(a):
    """(n, k) uint32 view: one row per query / player record"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def _queries(arrays, built, n, seed):
    """n seeded sweep queries (spheres (n, 4), velocities (n, 3)): around the floor centroids and the start; touching and
    grazing triangles, edges and vertices; zero velocities; velocities parallel to walls"""
    rng = np.random.default_rng(seed)
    verts, tris = arrays['verts'], arrays['triangles']
    cent = built.floor_centroids()
    sph = np.zeros((n, 4), np.float32)
    vel = np.zeros((n, 3), np.float32)
    kind = rng.integers(0, 7, n)
    radius = rng.choice(np.array([0.19, 0.2, 0.05, 0.5], np.float32), n)
    sph[:, 3] = radius
    t = tris[rng.integers(0, len(tris), n)]
    a, b, c, nrm = verts[t[:, 0]], verts[t[:, 1]], verts[t[:, 2]], verts[t[:, 3]]
    u = rng.random((n, 2)).astype(np.float32)
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    on_tri = a + (b - a) * u[:, :1] + (c - a) * u[:, 1:]
    rand_dir = rng.normal(size=(n, 3)).astype(np.float32)
    rand_dir /= np.linalg.norm(rand_dir, axis=1, keepdims=True)
    speed = rng.choice(np.array([0.0, 0.01, 0.1, 1.0, 5.0], np.float32), n)[:, None]
    centre_pick = cent[rng.integers(0, len(cent), n)] + np.array([0, 0.3, 0], np.float32)
    for k in range(7):
        m = kind == k
        if k == 0:    # free spheres near floor centroids, random velocities (some zero)
            sph[m, :3] = centre_pick[m] + rng.normal(scale=0.5, size=(m.sum(), 3)).astype(np.float32)
            vel[m] = rand_dir[m] * speed[m]
        elif k == 1:  # just touching a triangle's plane (radius along the normal, +-1 ulp-ish), moving in
            sph[m, :3] = on_tri[m] + nrm[m] * radius[m, None] * rng.choice([1.0, 1.0 + 1e-6, 1.0 - 1e-6], m.sum())[:, None].astype(np.float32)
            vel[m] = -nrm[m] * speed[m] + rand_dir[m] * 0.1
        elif k == 2:  # parallel to a wall's plane (the edge direction), touching or a little off it
            edge = b[m] - a[m]
            edge /= np.maximum(np.linalg.norm(edge, axis=1, keepdims=True), 1e-6)
            sph[m, :3] = on_tri[m] + nrm[m] * radius[m, None] * rng.choice([0.5, 1.0, 1.01], m.sum())[:, None].astype(np.float32)
            vel[m] = edge * np.maximum(speed[m], 0.1)
        elif k == 3:  # grazing a vertex: the sphere's surface passes within a hair of it
            side = np.cross(rand_dir[m], nrm[m])
            side /= np.maximum(np.linalg.norm(side, axis=1, keepdims=True), 1e-6)
            sph[m, :3] = a[m] + side * radius[m, None] * np.float32(1.0 - 1e-6) - rand_dir[m] * 1.0
            vel[m] = rand_dir[m] * 2.0
        elif k == 4:  # grazing an edge: centre one radius off the edge's midpoint, moving along the edge
            mid = (a[m] + b[m]) * 0.5
            edge = b[m] - a[m]
            off = np.cross(edge, nrm[m])
            off /= np.maximum(np.linalg.norm(off, axis=1, keepdims=True), 1e-6)
            sph[m, :3] = mid + (off + nrm[m]) / np.float32(np.sqrt(2)) * radius[m, None] - edge * 0.5
            vel[m] = edge
        elif k == 5:  # already overlapping a triangle
            sph[m, :3] = on_tri[m] + nrm[m] * radius[m, None] * 0.3
            vel[m] = rand_dir[m] * speed[m]
        else:         # zero velocity anywhere
            sph[m, :3] = on_tri[m] + rand_dir[m] * 0.2
            vel[m] = 0.0
    return sph, vel


def _levels():
    return [(ensure_wad(), i) for i in range(9)] + [(_syn.ensure_rich_wad(), 0), (ensure_big_wad(), 0)]


@pytest.mark.parametrize('path,index', _levels(), ids=lambda v: str(v).rsplit('/', 1)[-1] if isinstance(v, str) else str(v))
def test_sweep_matches_the_restatement(path, index):
    rd.set_device(0)
    wad = rd.Wad(path, META_PATH)
    world, ref = wad.build_world(index), world_ref.RefWorld(wad, index)
    arrays = world.arrays()
    n = 120000
    sph, vel = _queries(arrays, wad.build_level(index), n, seed=1000 + index)
    # per-object offsets on a third of the queries: doors and lifts lifted / lowered by up to one unit, plus some sideways
    off = None
    if world.n_objects > 1:
        rng = np.random.default_rng(index)
        off = np.zeros((n, world.n_objects, 3), np.float32)
        lift = rng.random(n) < 1 / 3
        off[lift, :, 1] = rng.uniform(-1.0, 1.0, (lift.sum(), world.n_objects)).astype(np.float32)
        off[lift, :, 0] = rng.choice(np.array([0.0, 0.0, 0.25], np.float32), (lift.sum(), world.n_objects))
    got = world.sweep(sph, vel, off)
    want = ref.sweep(sph, vel, off)
    hits = np.isfinite(want[:, 0])
    assert 0.05 < hits.mean() < 0.95, hits.mean()  # (the queries exercise both outcomes)
    bad = np.nonzero((_u32(got) != _u32(want)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    if off is not None:  # the offsets changed some answers
        plain = ref.sweep(sph, vel, None)
        assert (_u32(plain) != _u32(want)).any()
    # device tensors in, device tensor out (asynchronous path)
    t = world.sweep(torch.from_numpy(sph).cuda(), torch.from_numpy(vel).cuda())
    assert np.array_equal(_u32(t.cpu().numpy()), _u32(ref.sweep(sph, vel)))


@pytest.mark.parametrize('index', [0, 4])
def test_step_matches_the_restatement(index):
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(index)
    world, ref = wad.build_world(index), world_ref.RefWorld(wad, index)
    n, ticks = 1024, 300
    st = _players(built, n, seed=index)
    inp = _script(n, ticks, seed=index)
    got = world.step(st, inp)
    want = ref.step(st, inp)
    bad = np.nonzero((_u32(got) != _u32(want)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]], want[bad[:2]])
    moved = np.linalg.norm(got['pos'] - st['pos'], axis=1)
    assert (moved > 1.0).mean() > 0.3  # (they really walked)
    # K = 1 x 300 launches == K = 300 x 1 launch, on one stream, on device tensors
    s_dev = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    i_dev = torch.from_numpy(np.ascontiguousarray(inp).view(np.uint8).reshape(ticks, -1).copy()).cuda()
    for t in range(ticks):
        world.step(s_dev, i_dev[t], n_ticks=1)
    torch.cuda.synchronize()
    assert np.array_equal(s_dev.cpu().numpy(), np.ascontiguousarray(got).view(np.uint8))


def test_step_with_object_offsets_matches_the_restatement():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    n, ticks = 256, 120
    st = _players(built, n, seed=9)
    inp = _script(n, ticks, seed=9)
    off = np.zeros((n, world.n_objects, 3), np.float32)
    off[:, :, 1] = np.random.default_rng(3).uniform(0.0, 1.2, (n, world.n_objects)).astype(np.float32)
    assert np.array_equal(_u32(world.step(st, inp, object_offsets=off)), _u32(ref.step(st, inp, offsets=off)))


def test_two_streams_two_worlds_do_not_interfere():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    worlds, states, inputs, alone = [], [], [], []
    for index in (0, 2):
        built = wad.build_level(index)
        w = wad.build_world(index)
        st, inp = _players(built, 512, seed=20 + index), _script(512, 200, seed=20 + index)
        worlds.append(w)
        states.append(torch.from_numpy(st.view(np.uint8).copy()).cuda())
        inputs.append(torch.from_numpy(np.ascontiguousarray(inp).view(np.uint8).copy()).cuda())
        alone.append(w.step(st, inp))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            worlds[k].step(states[k], inputs[k], n_ticks=200, stream=streams[k])
    torch.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(states[k].cpu().numpy(), np.ascontiguousarray(alone[k]).view(np.uint8))


def _rest_height(cfg):
    """where a standing player comes to rest above the floor: the feet sphere (radius 0.2, player.rs:245-247) probes
    cfg.height down; at rest the spring's force (height_diff * spring_const_p) carries gravity's 17 (player.rs:305-313)"""
    return np.float32(0.2) + cfg['height'] - np.float32(17.0) / cfg['spring_const_p']


def test_standing_players_settle_and_dropped_players_land():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    cfg = rd.player_config_default()
    cent = built.floor_centroids()
    stand = rd.player_states(cent + np.array([0, 0.3, 0], np.float32), 0.0)
    out = world.step(stand, np.zeros((300, len(cent)), rd.PLAYER_INPUT))
    assert np.all(np.abs(out['pos'][:, 1] - cent[:, 1] - _rest_height(cfg)) < 1e-3)
    assert np.all(np.abs(out['pos'][:, [0, 2]] - cent[:, [0, 2]]) < 1e-3)
    drop = rd.player_states(cent + np.array([0, 2.0, 0], np.float32), 0.0)
    out = world.step(drop, np.zeros((300, len(cent)), rd.PLAYER_INPUT))
    landed = np.abs(out['pos'][:, 1] - cent[:, 1] - _rest_height(cfg)) < 1e-2
    # (a centroid under a low ceiling keeps the player from rising 2 units: those start inside the ceiling and are not judged)
    assert landed.mean() > 0.8 and np.all(out['pos'][:, 1] < cent[:, 1] + 2.0)
    assert not (out['flags'] & rd.PLAYER_DIVERGED).any()


def test_walking_into_a_blocker_wall_never_passes_it():
    """Players at the floor centroids walk forward for 300 ticks; those whose forward sweep meets a wall never cross a wall that
    covers their whole height from its front (the side its normal faces) to its back.  (The reference's walls are one-sided --
    sphere.rs:29-31 ignores a triangle the velocity leaves -- and a sphere already overlapping a plane meets only its edges and
    vertices, sphere.rs:40-55: so walls are judged from the front, and only where they are taller than the player.)"""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    a = world.arrays()
    cfg = rd.player_config_default()
    cent = built.floor_centroids()
    n = len(cent)
    st = rd.player_states(cent + np.array([0, 0.3, 0], np.float32), 0.0)
    rng = np.random.default_rng(4)
    yaws = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    st['yaw'] = yaws
    d = np.stack([-np.sin(yaws), np.zeros(n), -np.cos(yaws)], 1).astype(np.float32)  # forward (player.rs:207-221)
    sph = np.concatenate([st['pos'], np.full((n, 1), cfg['radius'], np.float32)], 1)
    hit = world.sweep(sph, d * 50.0)
    walls = np.isfinite(hit[:, 0]) & (hit[:, 2] == 0.0)
    assert walls.mean() > 0.5
    inp = np.zeros((1, n), rd.PLAYER_INPUT)
    inp['movement'][:, :, 1] = -1.0
    traj, s = [st['pos'].copy()], st
    for _ in range(300):
        s = world.step(s, inp)
        traj.append(s['pos'].copy())
    traj = np.array(traj)  # (301, n, 3)
    p0, p1 = traj[:-1], traj[1:]
    tris, verts = a['triangles'][:a['n_static_triangles']], a['verts']
    rest = _rest_height(cfg)
    crossed = np.zeros(n, bool)
    for t in tris[verts[tris[:, 3]][:, 1] == 0.0]:
        A, B, N = verts[t[0]], verts[t[1]], verts[t[3]]
        e = B - A
        if e[0] == 0 and e[2] == 0:
            continue
        lo, hi = min(A[1], verts[t[2]][1]), max(A[1], verts[t[2]][1])
        s0 = (p0[..., 0] - A[0]) * N[0] + (p0[..., 2] - A[2]) * N[2]
        s1 = (p1[..., 0] - A[0]) * N[0] + (p1[..., 2] - A[2]) * N[2]
        u = s0 / np.where(s0 != s1, s0 - s1, 1)
        cx, cz = p0[..., 0] + (p1[..., 0] - p0[..., 0]) * u, p0[..., 2] + (p1[..., 2] - p0[..., 2]) * u
        along = ((cx - A[0]) * e[0] + (cz - A[2]) * e[2]) / (e[0] ** 2 + e[2] ** 2)
        y = p0[..., 1]
        crossed |= ((s0 > 0) & (s1 < 0) & (along > 0) & (along < 1) & (lo < y - rest) & (hi > y + cfg['radius'])).any(0)
    assert not crossed[walls].any(), np.nonzero(crossed & walls)[0][:10]
    assert (np.linalg.norm(traj[-1] - traj[0], axis=1)[walls] > 0.05).mean() > 0.5  # (they walked up to their walls)


def test_world_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('sweep_kernel', 'player_step_kernel'):
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)


def test_step_then_render_matches_the_oracle():
    from oracle import raster
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    n, w, h = 6, 160, 100
    st = _players(built, n, seed=31)
    st['flags'] = rd.PLAYER_CLIP
    states = world.step(st, _script(n, 120, seed=31))
    poses = rd.poses_from_players(states, w, h)
    level = rd.DeviceLevel(built)
    batch = rd.Batch(level, w, h, n)
    lights = built.lights_at(0.0)
    fb, fb_ids, _ = render_checked(batch, poses, lights)
    ro = raster.RasterOracle(built.arrays())
    for i in range(n):
        want = ro.render(poses[i]['modelview'], poses[i]['projection'], 0.0, lights, w, h)
        assert np.array_equal(want, fb[i]) and np.array_equal(want, fb_ids[i]), i
