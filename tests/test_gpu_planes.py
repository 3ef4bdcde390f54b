"""GPU: depth, label and primitive planes of a render (rdoom_batch_resolve_plane / rdoom_batch_read_plane).  The expected planes
are the ORACLE's (tests/planes_ref.py: render_varyings' binary32 v_dist, render's winners, the level's draws), never the
product's own output, and the comparison is bit for bit at every pixel of every frame -- depth as uint32 bit patterns, both row
orders.  Every checked render follows a render of other poses (tests/util.py: dirtying_poses) and is checked on the plain path
and again after rdoom_batch_enable_primitive_ids, as tests/test_gpu_rgb.py does."""
import os
import subprocess
import sys

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:  # (the CPU test of this file does not need it)
    torch = None

import planes_ref
import rust_doom_amd as rd
from oracle import raster
from util import META_PATH, dirtying_poses, ensure_wad

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PLANES = {'depth': rd.PLANE_DEPTH, 'label': rd.PLANE_LABEL, 'primitive': rd.PLANE_PRIMITIVE}

# Depth where objects have moved is checked against depth_f64 below, a float64 restatement, because the oracle's render_varyings
# takes no per-object matrices.  The allowed relative difference is not tuned to the library: F64_VS_ORACLE is the largest relative
# difference between that restatement and the ORACLE's own binary32 v_dist over the static golden poses of levels 0, 3 and 7
# (flat and wall winners, where both exist), measured on the CPU and pinned by test_f64_restatement_against_the_oracle; the
# library may differ from the restatement by four times that (the doors' planes have other slopes than the walls').
F64_VS_ORACLE = 1.25e-5  # measured: 1.243e-05 (the binary32 1/w plane's cancellation at grazing walls, not the division)
DEPTH_MOVED_RTOL = 4 * F64_VS_ORACLE


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_planes(batch, want, what, frames=None, names=PLANES):
    """every plane in `names`, both row orders, every pixel of every frame (of `frames`)"""
    for name in names:
        for td in (False, True):
            got = batch.read_plane(PLANES[name], top_down=td)
            exp = want[name][:, ::-1] if td else want[name]
            assert got.shape == exp.shape and got.dtype == exp.dtype, (what, name, got.shape, got.dtype)
            for i in (range(len(exp)) if frames is None else frames):
                bad = int((bits(got[i]) != bits(exp[i])).sum())
                print('%s: %s top_down=%s frame %d: %d differing pixels' % (what, name, td, i, bad))
                assert bad == 0, (what, name, td, i, bad)


def render_both_paths_and_check(batch, poses, lights, want, what, names=PLANES, **kw):
    other = dirtying_poses(poses)
    olights = np.roll(lights, 1, axis=0)
    dkw = {k: v for k, v in kw.items() if k != 'object_modelviews'}
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_planes(batch, want, what + ' (plain path)', names=names)
    batch.enable_primitive_ids()
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_planes(batch, want, what + ' (id path)', names=names)
    # product against product: the plane makes the id facility unnecessary
    assert np.array_equal(batch.read_plane(rd.PLANE_PRIMITIVE), batch.read_primitive_ids()), what


@gpu
@pytest.mark.parametrize('index', [0, 3, 7])
def test_golden_poses_equal_the_oracle_composition(oracle_levels, index):
    from test_gpu_rgb import golden_case
    lv = oracle_levels(index)
    poses, lights, w, h = golden_case(lv, index)
    want = planes_ref.expected_batch(lv, poses, lights, w, h)
    assert np.isfinite(want['depth']).any()
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, want, 'golden level %d' % index)


@gpu
@pytest.mark.parametrize('size', [(321, 200, 4), (1000, 520, 2), (1920, 1080, 2), (16384, 40, 1)])
def test_sweep_poses_at_odd_and_full_sizes(wad_path, oracle_levels, size):
    """321 x 200: padded row pitch, u16 rows that start on odd halfwords; 1000 x 520: an 8-pixel tail per row; 1920 x 1080: the
    bench size.  Each with a view from outside the level: geometry and the void in one frame."""
    import importlib
    from test_gpu_rgb import outside_pose
    sharding = importlib.import_module('rust-doom_amd.sharding')
    w, h, n = size
    lv = oracle_levels(0)
    if w == 1920:
        built = rd.Wad(wad_path, META_PATH).build_level(0)
        poses = sharding.pose_sweep(rd, built, 1024, w, h)[[0, 682]]
    else:
        from test_gpu_raster_parity import sweep_poses
        poses = sweep_poses(lv, n, w, h, seed=31, time=0.7)
    poses = np.concatenate([poses, outside_pose(lv, w, h, float(poses[0]['time']))])
    lights = np.array([lv.lights.fill_buffer_at(float(p['time'])) for p in poses])
    want = planes_ref.expected_batch(lv, poses, lights, w, h)
    none = want['primitive'] == planes_ref.NO_PRIM
    assert none.any() and (~none).any() and (want['label'][none] == rd.LABEL_NONE).all() and np.isposinf(want['depth'][none]).all()
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, want, '%dx%d' % (w, h))


def run_child(mode):
    """tests/gpu_planes_child.py MODE in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_planes_child.py'), mode], cwd=HERE, capture_output=True, text=True,
                       timeout=1200)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(kv.split('=') for kv in out[-1].split()[1:])


@gpu
def test_every_debug_path_in_one_child():
    """vis32, no_qtab, keep_vis, leak_mod (fixups inside described quadrants), no_bins, entry_cap: planes unchanged"""
    fields = run_child('hooks')
    assert int(fields['bad']) == 0 and int(fields['cases']) == 16 and int(fields['fixups']) > 1000


@gpu
def test_level_set_planes_are_per_level(oracle_levels):
    """poses of three levels in one batch, objects moved: object ids and primitive ids are those of the pose's own level"""
    from test_gpu_levelset import mixed_batch
    levels = [oracle_levels(0), oracle_levels(2), oracle_levels(3)]
    w, h = 640, 400
    poses, lop, lights, om = mixed_batch(levels, 2, w, h, seed=77, moving=True)
    assert len(set(lop.tolist())) == 3
    frames = [planes_ref.expected_planes(raster.RasterOracle(levels[lop[i]]), levels[lop[i]], poses[i], lights[i], w, h,
                                         om[i, :int(levels[lop[i]].num_objects)]) for i in range(len(poses))]
    want = {k: np.array([f[k] for f in frames]) for k in ('label', 'primitive')}
    assert len(set((want['label'][want['label'] != rd.LABEL_NONE] >> 4).tolist())) > 1  # (more than the static level is seen)
    batch = rd.Batch(rd.DeviceLevelSet(levels), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, want, 'level set', names=('label', 'primitive'), level_of_pose=lop,
                                object_modelviews=om)
    # static poses of the same set: depth too, against each level's own oracle
    frames = [planes_ref.expected_planes(raster.RasterOracle(levels[lop[i]]), levels[lop[i]], poses[i], lights[i], w, h) for i in range(len(poses))]
    want = {k: np.array([f[k] for f in frames]) for k in PLANES}
    batch.render(poses, lights, level_of_pose=lop)
    check_planes(batch, want, 'level set, objects at rest')


# ---- moved objects: step_game -> render_players ------------------------------------------------------------------------------
def depth_f64(lv, prim, modelview, projection, w, h, object_modelviews=None):
    """float64 restatement of v_dist for the flat / wall winners of one frame: clip-space w of the winning triangle's vertices under
    its object's modelview, 1/w interpolated (affine in window coordinates) to the pixel centre, inverted.  NaN elsewhere."""
    g = (lambda k: lv[k]) if isinstance(lv, dict) else (lambda k: getattr(lv, k))
    sv, si = g('static_vertices'), np.asarray(g('static_indices'))
    draws = np.asarray(g('draws'), np.uint32).reshape(-1, 4)
    kind, obj, owner = planes_ref.draw_tables(lv)
    first_prim = np.concatenate([[0], np.cumsum(draws[:, 3] // 3)[:-1]]).astype(np.int64)
    P = np.asarray(projection, np.float64).reshape(4, 4).T
    out = np.full((h, w), np.nan)
    py, px = np.mgrid[0:h, 0:w].astype(np.float64) + 0.5
    for pid in np.unique(prim[prim != planes_ref.NO_PRIM]):
        if kind[pid] > 1:
            continue
        d = owner[pid]
        at = int(draws[d, 2]) + 3 * int(pid - first_prim[d])
        pos = np.concatenate([sv[si[at:at + 3]]['a_pos'].astype(np.float64), np.ones((3, 1))], axis=1)
        mv = modelview if object_modelviews is None else object_modelviews[obj[pid]]
        clip = pos @ (P @ np.asarray(mv, np.float64).reshape(4, 4).T).T
        cw = clip[:, 3]
        m = np.stack([(clip[:, 0] + cw) * (w / 2), (clip[:, 1] + cw) * (h / 2), cw], axis=1)
        a, b, c = np.linalg.solve(m, np.ones(3))  # a * xw + b * yw + c * w == 1 at the three vertices: 1/w = a X + b Y + c
        sel = prim == pid
        out[sel] = 1.0 / (a * px[sel] + b * py[sel] + c)
    return out


def rel_diff(depth32, f64):
    ok = np.isfinite(f64)
    assert np.isfinite(depth32[ok]).all()
    return float(np.max(np.abs(depth32[ok].astype(np.float64) - f64[ok]) / f64[ok])) if ok.any() else 0.0


def test_f64_restatement_against_the_oracle(oracle_levels):
    """CPU: pins F64_VS_ORACLE -- the oracle's binary32 v_dist against depth_f64 on the static golden poses of levels 0, 3, 7"""
    from test_gpu_rgb import golden_case
    worst, covered = 0.0, 0.0
    for index in (0, 3, 7):
        lv = oracle_levels(index)
        poses, lights, w, h = golden_case(lv, index)
        ro = raster.RasterOracle(lv)
        for i in range(len(poses)):
            _, prim, var = ro.render_varyings(poses[i]['modelview'], poses[i]['projection'], float(poses[i]['time']), lights[i], w, h)
            f64 = depth_f64(lv, prim, poses[i]['modelview'], poses[i]['projection'], w, h)
            covered += float(np.isfinite(f64).mean())
            worst = max(worst, rel_diff(var[..., 2], f64))
    assert covered > 1.0  # (summed over the frames: the comparison is not empty)
    print('largest relative difference oracle v_dist / float64 restatement: %.3e' % worst)
    assert 0.5 * F64_VS_ORACLE <= worst <= F64_VS_ORACLE, worst


@gpu
def test_render_players_after_a_door_opened():
    """step_game opens a door in front of the players, render_players draws them from device state: label and primitive planes
    equal the oracle's winners under the object modelviews bit for bit (poses whose sky angle agrees with the host's; on the
    others every differing pixel is a sky pixel in either plane), depth the float64 restatement within DEPTH_MOVED_RTOL"""
    import frames_ref
    import world_ref
    from test_game_host import patched_variant
    from test_gpu_game import _door
    import tempfile
    rd.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        wad_path, meta_path = patched_variant(tmp)[:2]
        wad = rd.Wad(wad_path, meta_path)
        built = wad.build_level(0)
        world = wad.build_world(0)
        ref = world_ref.RefWorld(wad, 0)
        _, eff, st = _door(world, world.triggers(), ref)
        n, w, h = 4, 160, 100
        st = np.repeat(st, n)
        st['yaw'] += np.linspace(-0.3, 0.3, n).astype(np.float32)
        ticks = 50
        inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
        act = np.zeros((ticks, n), np.uint8)
        act[0, 1:] = rd.ACTION_PUSH
        game, offs = world.game_state(n)
        states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        world.step_game(states, inp, game, offs, actions=act)
        torch.cuda.synchronize()
        o = offs.cpu().numpy()
        assert o[1:, eff['object_id'], 1].min() > 0 and (o[0] == 0).all()
        host_states = states.cpu().numpy().view(rd.PLAYER_STATE).copy().reshape(-1)
        lv = built.arrays()
        n_obj = int(built.counters()['num_objects'])
        poses, mvs = frames_ref.cameras(host_states, w, h, 0.0, o)
        poses, mvs = poses.reshape(-1), mvs[:, :n_obj]
        lights = built.lights_at(0.0)
        ro = raster.RasterOracle(lv)
        frames = [planes_ref.expected_planes(ro, lv, poses[i], lights, w, h, mvs[i]) for i in range(n)]
        want = {k: np.array([f[k] for f in frames]) for k in ('label', 'primitive')}
        # the precondition, from the oracle: a checked pose shows a primitive of an object whose offset is non-zero
        kind, obj, _ = planes_ref.draw_tables(lv)
        h0, c0 = frames_ref.sky_angles(poses['projection'][0], poses['modelview'])
        h1, c1 = frames_ref.sky_angles(poses['projection'][0], mvs)
        exact = (h0 == c0) & (h1 == c1).all(1)
        shows = [i for i in range(n) if exact[i] and any((o[i, obj[p]] != 0).any() for p in np.unique(want['primitive'][i][want['primitive'][i] != planes_ref.NO_PRIM]))]
        assert shows, 'no checked pose shows a moved object'
        batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
        sky_label = lambda a: (a != rd.LABEL_NONE) & ((a & 0xF) == rd.KIND_SKY)  # noqa: E731
        for ids in (False, True):
            if ids:
                batch.enable_primitive_ids()
            batch.render(dirtying_poses(poses), lights)
            batch.render_players(states=states, lights=lights, offsets=offs, time=0.0)
            got = {k: batch.read_plane(PLANES[k]) for k in PLANES}
            for i in range(n):
                dl, dp = got['label'][i] != want['label'][i], got['primitive'][i] != want['primitive'][i]
                print('render_players ids=%s pose %d exact=%s: label %d primitive %d differing pixels' % (ids, i, exact[i], dl.sum(), dp.sum()))
                if exact[i]:
                    assert not dl.any() and not dp.any(), (ids, i)
                else:
                    sky = sky_label(got['label'][i]) | sky_label(want['label'][i])
                    assert sky[dl | dp].all(), (ids, i)
            for i in shows:
                f64 = depth_f64(lv, want['primitive'][i], poses[i]['modelview'], poses[i]['projection'], w, h, mvs[i])
                moved = np.isin(want['primitive'][i], [p for p in range(len(obj)) if (o[i, obj[p]] != 0).any()]) & np.isfinite(f64)
                assert moved.any()
                r = rel_diff(got['depth'][i], f64)
                print('render_players ids=%s pose %d: depth within %.3e of the float64 restatement (allowed %.1e), %d moved pixels'
                      % (ids, i, r, DEPTH_MOVED_RTOL, int(moved.sum())))
                assert r <= DEPTH_MOVED_RTOL, (ids, i, r)
                solid = (want['primitive'][i] != planes_ref.NO_PRIM) & (kind[np.where(want['primitive'][i] != planes_ref.NO_PRIM, want['primitive'][i], 0)] != rd.KIND_SKY)
                assert np.isfinite(got['depth'][i][solid]).all() and np.isposinf(got['depth'][i][~solid]).all()


@gpu
def test_planes_and_rgb_queued_on_one_stream_behind_render_players():
    """resolve_plane (depth) and resolve_rgb queued on one stream behind one render_players, then the next tick's render on the
    same stream: the tensors equal a synchronous read_plane / read_rgb of an identical render"""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    n, w, h = 8, 320, 200
    pos, yaw = built.start()
    st = rd.player_states([[pos[0], pos[1], pos[2]]] * n, [float(yaw) + 0.2 * i for i in range(n)])
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    inp = np.zeros((4, n), rd.PLAYER_INPUT)
    game, offs = world.game_state(n)
    lights = built.lights_at(0.0)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    s = torch.cuda.Stream()
    depth = torch.full((n, h, w), -1.0, dtype=torch.float32, device='cuda')
    rgb = torch.zeros((n, h, w, 3), dtype=torch.uint8, device='cuda')
    before = states.clone()
    torch.cuda.synchronize()
    batch.render_players(states=states, lights=lights, offsets=offs, time=0.0, stream=s)
    assert batch.resolve_depth(depth, stream=s) is depth
    batch.resolve_rgb(rgb, stream=s)
    world.step_game(states, inp, game, offs, stream=s)
    batch.render_players(states=states, lights=lights, offsets=offs, time=0.0, stream=s)  # the next tick overwrites the sources
    s.synchronize()
    batch.finish()
    offs0 = torch.zeros_like(offs)
    batch.render_players(states=before, lights=lights, offsets=offs0, time=0.0)
    want_depth, want_rgb = batch.read_depth(), batch.read_rgb()
    assert np.isfinite(want_depth).mean() > 0.3
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
    assert np.array_equal(rgb.cpu().numpy(), want_rgb)
    # the other planes into tensors of their own dtype, top-down, a sub-range
    label = torch.zeros((2, h, w), dtype=torch.int16, device='cuda')
    prim = torch.zeros((2, h, w), dtype=torch.int32, device='cuda')
    batch.resolve_plane(label, rd.PLANE_LABEL, first=3, count=2, top_down=True, stream=s)
    batch.resolve_plane(prim, rd.PLANE_PRIMITIVE, first=3, count=2, stream=s)
    s.synchronize()
    assert np.array_equal(label.cpu().numpy().view(np.uint16), batch.read_plane(rd.PLANE_LABEL, top_down=True)[3:5])
    assert np.array_equal(prim.cpu().numpy().view(np.uint32), batch.read_plane(rd.PLANE_PRIMITIVE)[3:5])
    # tensors that do not fit are refused before anything is written
    for bad in (torch.zeros((n, h, w), dtype=torch.float32),                         # host memory
                torch.zeros((n, h, w), dtype=torch.int32, device='cuda'),            # the wrong dtype for depth
                torch.zeros((n, h, w + 1), dtype=torch.float32, device='cuda'),      # the wrong size
                torch.zeros((n, h, w + 1), dtype=torch.float32, device='cuda')[..., :w]):  # not contiguous
        with pytest.raises(ValueError):
            batch.resolve_depth(bad)


@gpu
def test_range_and_argument_errors(oracle_levels):
    import ctypes
    from test_gpu_rgb import small_scene
    lv, poses, lights, w, h = small_scene(oracle_levels)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    with pytest.raises(rd.RdoomError) as e:
        batch.read_depth(count=1)
    assert e.value.status == -1 and 'nothing rendered' in str(e.value)
    batch.render(poses, lights)
    for first, count in ((0, 4), (3, 1), (2, 2), (4, 0)):
        with pytest.raises(rd.RdoomError) as e:
            batch.read_plane(rd.PLANE_LABEL, first=first, count=count)
        assert e.value.status == -1 and 'range' in str(e.value), (first, count)
    assert batch.read_depth(first=3, count=0).shape == (0, h, w)
    host = np.zeros((len(poses), h, w), np.float32)
    with pytest.raises(rd.RdoomError) as e:  # a host pointer is not device memory
        batch.resolve_depth(host.ctypes.data)
    assert e.value.status == -1 and 'device memory' in str(e.value)
    L = rd.lib()
    assert L.rdoom_batch_resolve_plane(batch._h, 0, 1, rd.PLANE_DEPTH, None, None) == -1
    assert L.rdoom_batch_read_plane(batch._h, 0, 1, 0x200 | rd.PLANE_DEPTH, host.ctypes.data_as(ctypes.c_void_p)) == -1
    with pytest.raises(ValueError):
        batch.read_plane(7)
    # nothing of that leaks into the next render
    batch.render(poses, lights)
    want = planes_ref.expected_batch(lv, poses, lights, w, h)
    check_planes(batch, want, 'after the refused calls')


@gpu
def test_a_level_without_a_palette_resolves_planes(oracle_levels):
    from test_gpu_rgb import small_scene
    lv, poses, lights, w, h = small_scene(oracle_levels)
    desc, keep = rd.make_desc(lv)
    desc.playpal = None
    batch = rd.Batch(rd.DeviceLevel(desc), w, h, len(poses))
    batch.render(poses, lights)
    with pytest.raises(rd.RdoomError):
        batch.read_rgb()
    check_planes(batch, planes_ref.expected_batch(lv, poses, lights, w, h), 'no playpal')
    del keep
