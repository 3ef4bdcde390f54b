"""GPU: reduced-size observations (rdoom_batch_resolve_observation / rdoom_batch_read_observation).  The expected observations
are tests/observe_ref.py -- the contract restated in numpy -- applied to FULL-SIZE frames that come from the ORACLE, never from
the product: test_gpu_rgb.compose of the oracle's index frames and primitive ids, and tests/planes_ref.py's depth.  The
comparison is bit for bit at every cell of every frame (depth as uint32 bit patterns), for every format and both row orders.
Every checked render follows a render of other poses (tests/util.py: dirtying_poses) and is checked on the plain path and again
after rdoom_batch_enable_primitive_ids, as tests/test_gpu_rgb.py does."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import observe_ref as oref
import planes_ref
import rust_doom_amd as rd
from oracle import raster
from test_gpu_rgb import compose, outside_pose, small_scene
from util import META_PATH, dirtying_poses, ensure_wad

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = (rd.OBS_RGB8, rd.OBS_RGB8_PLANAR, rd.OBS_GRAY8, rd.OBS_DEPTH_MIN)
COLOUR = (rd.OBS_RGB8, rd.OBS_RGB8_PLANAR, rd.OBS_GRAY8)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def oracle_full_size(lv, poses, lights, w, h, palettes=None, object_modelviews=None):
    """(rgb (n, H, W, 3) uint8, depth (n, H, W) float32 or None with moved objects, clear (n, H, W) bool), all from the oracle"""
    ro = raster.RasterOracle(lv)
    rgb, depth, clear = [], [], []
    for i in range(len(poses)):
        om = None if object_modelviews is None else object_modelviews[i]
        fb = ro.render(poses[i]['modelview'], poses[i]['projection'], float(poses[i]['time']), lights[i], w, h, object_modelviews=om)
        planes = planes_ref.expected_planes(ro, lv, poses[i], lights[i], w, h, om)
        pal = lv.palette if palettes is None else palettes[i]
        rgb.append(compose(fb[None], planes['primitive'][None], pal)[0])
        depth.append(planes['depth'])
        clear.append(planes['primitive'] == planes_ref.NO_PRIM)
    return np.array(rgb), (None if depth[0] is None else np.array(depth)), np.array(clear)


def check_observations(batch, rgb, depth, factors, what, formats=FORMATS):
    for factor in factors:
        for fmt in formats:
            for td in (False, True):
                got = batch.read_observation(fmt, factor, top_down=td)
                want = oref.observation(fmt, factor, rgb, depth, td)
                assert got.shape == want.shape == (len(rgb if rgb is not None else depth),) + rd.observation_shape(fmt, batch.width, batch.height, factor)
                assert got.dtype == want.dtype, (what, fmt, got.dtype)
                bad = int((bits(got) != bits(want)).sum())
                print('%s: format %d factor %r top_down=%s: %d differing elements of %d' % (what, fmt, factor, td, bad, want.size))
                assert bad == 0, (what, fmt, factor, td, bad)


def render_both_paths_and_check(batch, poses, lights, rgb, depth, factors, what, formats=FORMATS, **kw):
    other = dirtying_poses(poses)
    olights = np.roll(lights, 1, axis=0)
    dkw = {k: v for k, v in kw.items() if k != 'object_modelviews'}
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_observations(batch, rgb, depth, factors, what + ' (plain path)', formats)
    batch.enable_primitive_ids()
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_observations(batch, rgb, depth, factors, what + ' (id path)', formats)


def test_factor_one_equals_read_rgb_and_read_depth(oracle_levels):
    lv, poses, lights, w, h = small_scene(oracle_levels)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    batch.render(dirtying_poses(poses), lights)
    batch.render(poses, lights)
    for td in (False, True):
        rgb, depth = batch.read_rgb(top_down=td), batch.read_depth(top_down=td)
        assert np.array_equal(batch.read_observation(rd.OBS_RGB8, 1, top_down=td), rgb)
        assert np.array_equal(batch.read_observation(rd.OBS_RGB8_PLANAR, 1, top_down=td), np.moveaxis(rgb, 3, 1))
        assert np.array_equal(batch.read_observation(rd.OBS_DEPTH_MIN, (1, 1), top_down=td).view(np.uint32), depth.view(np.uint32))
    assert np.isfinite(depth).any() and len(np.unique(rgb)) > 8
    orgb, odepth, _ = oracle_full_size(lv, poses, lights, w, h)
    assert np.array_equal(batch.read_rgb(), orgb) and np.array_equal(batch.read_depth().view(np.uint32), odepth.view(np.uint32))


SWEEPS = {(321, 200): (4, [(2, 2), (4, 4), (8, 8), (4, 8), (8, 2)]),
          (77, 53): (4, [(2, 2), (8, 8), (1, 4)]),
          (1920, 1080): (2, [(4, 4)])}


@pytest.mark.parametrize('size', sorted(SWEEPS))
def test_sweep_poses_at_odd_and_full_sizes(wad_path, oracle_levels, size):
    """321 x 200: padded pitch (324), ow 160 / 80 / 40 and a leftover column, grey and planar rows that are no multiple of 4 at
    factor 8; 77 x 53: a partial last quadrant both ways, leftover rows and columns; 1920 x 1080 (poses of the seeded bench sweep):
    the last quadrant row has 24 rows.  Each with a view from outside the level: cells of geometry, of the void, and of both."""
    import importlib
    w, h = size
    n, factors = SWEEPS[size]
    lv = oracle_levels(0)
    if w == 1920:
        sharding = importlib.import_module('rust-doom_amd.sharding')
        built = rd.Wad(wad_path, META_PATH).build_level(0)
        poses = sharding.pose_sweep(rd, built, 1024, w, h)[[682]]
    else:
        from test_gpu_raster_parity import sweep_poses
        poses = sweep_poses(lv, n - 1, w, h, seed=31, time=0.7)
    poses = np.concatenate([poses, outside_pose(lv, w, h, float(poses[0]['time']))])
    assert len(poses) == n
    lights = np.array([lv.lights.fill_buffer_at(float(p['time'])) for p in poses])
    rgb, depth, clear = oracle_full_size(lv, poses, lights, w, h)
    assert clear.any() and (~clear).any()  # undrawn and drawn pixels ...
    for fx, fy in factors:
        if fx * fy > 1:
            c = oref.cells(clear, fx, fy)
            assert (c.any(-1) & ~c.all(-1)).any(), (fx, fy)  # ... and cells that mix them
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, n)
    render_both_paths_and_check(batch, poses, lights, rgb, depth, factors, '%dx%d' % (w, h))


def test_level_set_observations_use_each_poses_own_palette(oracle_levels):
    """the recipe of test_gpu_rgb.test_level_set_uses_each_poses_own_palette: two levels of one IWAD, the second with its PLAYPAL
    permuted, mixed poses with moving objects.  The colour formats against the oracle; the depth of the same (moving) batch
    against the reference applied to the batch's own read_depth -- the oracle's render_varyings takes no per-object matrices,
    tests/test_gpu_planes.py checks that plane -- and, with the objects at rest, against the oracle's depth bit for bit."""
    from test_gpu_levelset import mixed_batch
    levels = [oracle_levels(0), oracle_levels(2)]
    perm = np.random.RandomState(5).permutation(256)
    fields = ('static_vertices', 'static_indices', 'sky_vertices', 'sky_indices', 'decor_vertices', 'decor_indices', 'draws',
              'flat_atlas', 'wall_atlas', 'decor_atlas', 'sky_texture', 'sky_band', 'colormap')
    second = types.SimpleNamespace(**{f: getattr(levels[1], f) for f in fields if hasattr(levels[1], f)})
    second.palette = np.asarray(levels[1].palette, np.uint8).reshape(256, 3)[perm].reshape(-1)
    palettes_of_level = [np.asarray(levels[0].palette, np.uint8), second.palette]
    w, h, factor = 640, 400, (4, 4)
    poses, lop, lights, om = mixed_batch(levels, 3, w, h, seed=77, moving=True)
    assert len(set(lop.tolist())) == 2 and (poses['time'] > 0).any()
    rgb, rest = [], []
    for i in range(len(poses)):
        lv = levels[lop[i]]
        r, _, _ = oracle_full_size(lv, poses[i:i + 1], lights[i:i + 1], w, h, [palettes_of_level[lop[i]]], om[i:i + 1, :int(lv.num_objects)])
        rgb.append(r[0])
        rest.append(planes_ref.expected_planes(raster.RasterOracle(lv), lv, poses[i], lights[i], w, h)['depth'])
    rgb = np.array(rgb)
    batch = rd.Batch(rd.DeviceLevelSet([levels[0], second]), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, rgb, None, [factor], 'level set', COLOUR, level_of_pose=lop, object_modelviews=om)
    moving = batch.read_depth()
    assert np.isfinite(moving).any()
    check_observations(batch, None, moving, [factor], 'level set, moving objects', (rd.OBS_DEPTH_MIN,))
    batch.render(poses, lights, level_of_pose=lop)
    check_observations(batch, None, np.array(rest), [factor], 'level set, objects at rest', (rd.OBS_DEPTH_MIN,))


def test_observations_after_render_players():
    """render_players draws from device states; the observation of frame p equals the reference applied to read_rgb / read_depth
    of the SAME render.  This is the one place where the product's own full-size output is the input: the frames of a device-path
    render differ from the host path's (and so from the oracle's under host-made poses) on the sky column DESIGN section 12
    names, and tests/test_gpu_planes.py / test_gpu_players.py check those frames themselves."""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    n, w, h = 6, 320, 200
    pos, yaw = built.start()
    st = rd.player_states([[pos[0], pos[1], pos[2]]] * n, [float(yaw) + 0.4 * i for i in range(n)])
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    game, offs = world.game_state(n)
    lights = built.lights_at(0.0)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    s = torch.cuda.Stream()
    grey = torch.zeros((n,) + rd.observation_shape(rd.OBS_GRAY8, w, h, 4), dtype=torch.uint8, device='cuda')
    dmin = torch.zeros((n,) + rd.observation_shape(rd.OBS_DEPTH_MIN, w, h, 4), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    batch.render_players(states=states, lights=lights, offsets=offs, time=0.0, stream=s)
    assert batch.resolve_observation(grey, rd.OBS_GRAY8, 4, top_down=True, stream=s) is grey
    batch.resolve_observation(dmin, rd.OBS_DEPTH_MIN, 4, top_down=True, stream=s)
    s.synchronize()
    batch.finish()
    rgb, depth = batch.read_rgb(), batch.read_depth()
    assert np.isfinite(depth).mean() > 0.3 and len(np.unique(rgb)) > 8
    assert np.array_equal(grey.cpu().numpy(), oref.observation(rd.OBS_GRAY8, 4, rgb, top_down=True))
    assert np.array_equal(dmin.cpu().numpy().view(np.uint32), oref.observation(rd.OBS_DEPTH_MIN, 4, depth=depth, top_down=True).view(np.uint32))
    check_observations(batch, rgb, depth, [(4, 4), (2, 8)], 'render_players')


def run_child(mode, timeout):
    """tests/gpu_observe_child.py MODE in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_observe_child.py'), mode], cwd=HERE, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(kv.split('=') for kv in out[-1].split()[1:])


def test_sub_range_streams_tensors_and_graph_replay_in_one_child():
    """in a child that initialises torch before the library: a sub-range, a side stream, the caller's tensors and a raw pointer,
    tensors that do not fit, and a captured graph of a render and its observations replayed"""
    assert run_child('torch', 300)['ok'] == '1'


def test_every_debug_hook_in_one_child():
    """the sweep of tests/gpu_observe_child.py: every hook of tests/gpu_rgb_child.py at its two sizes; factor (4, 4) RGB8, grey and
    depth and factor (2, 8) RGB8 equal the reference on that process's own id-path frames; leak_mod sends thousands of ordinary
    pixels through the fix list, and on the reference those pixels change output cells"""
    fields = run_child('hooks', 1200)
    assert int(fields['bad']) == 0 and int(fields['cases']) == 28 and int(fields['fixups']) > 3000
    assert int(fields['changed']) > 0


def test_argument_errors_by_status_and_text(oracle_levels):
    lv, poses, lights, w, h = small_scene(oracle_levels)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))

    def refused(text, call, *a, **kw):
        with pytest.raises(rd.RdoomError) as e:
            call(*a, **kw)
        assert e.value.status == -1 and text in str(e.value), (text, str(e.value))

    refused('nothing rendered', batch.read_observation, count=1)
    batch.render(poses, lights)
    for first, count in ((0, 4), (3, 1), (2, 2), (4, 0)):
        refused('range', batch.read_observation, rd.OBS_GRAY8, 4, first=first, count=count)
    assert batch.read_observation(first=3, count=0).shape == (0, h // 4, w // 4, 3)
    L = rd.lib()
    host = np.zeros((len(poses), h, w, 3), np.float32)
    hp = host.ctypes.data_as(ctypes.c_void_p)

    def status(fn, *a):
        st = fn(batch._h, *a)
        return st, L.rdoom_last_error().decode()

    for fx, fy in ((3, 4), (4, 16), (0, 1), (4, 3)):
        st, msg = status(L.rdoom_batch_read_observation, 0, 1, rd.OBS_RGB8, fx, fy, hp)
        assert st == -1 and '1, 2, 4 or 8' in msg, (fx, fy, msg)
    tiny = rd.Batch(rd.DeviceLevel(lv), 6, 40, 1)
    tiny.render(poses[:1], lights[:1])
    st = L.rdoom_batch_read_observation(tiny._h, 0, 1, rd.OBS_GRAY8, 8, 2, hp)
    assert st == -1 and 'no cell' in L.rdoom_last_error().decode()
    st, msg = status(L.rdoom_batch_read_observation, 0, 1, 9, 4, 4, hp)
    assert st == -1 and 'RDOOM_OBS_RGB8' in msg, msg
    st, msg = status(L.rdoom_batch_read_observation, 0, 1, 0, 4, 4, hp)
    assert st == -1 and 'RDOOM_OBS_RGB8' in msg, msg
    st, msg = status(L.rdoom_batch_read_observation, 0, 1, 0x200 | rd.OBS_RGB8, 4, 4, hp)
    assert st == -1 and 'format bits' in msg, msg
    st, msg = status(L.rdoom_batch_resolve_observation, 0, 1, rd.OBS_RGB8, 4, 4, None, None)
    assert st == -1 and 'null' in msg, msg
    st, msg = status(L.rdoom_batch_read_observation, 0, 1, rd.OBS_RGB8, 4, 4, None)
    assert st == -1 and 'null' in msg, msg
    refused('device memory', batch.resolve_observation, host.ctypes.data, rd.OBS_DEPTH_MIN, 4)
    refused('aligned', batch.resolve_observation, host.ctypes.data + 2, rd.OBS_DEPTH_MIN, 4)
    st, msg = status(L.rdoom_batch_read_observation, 0, 1, rd.OBS_DEPTH_MIN, 4, 4, ctypes.c_void_p(host.ctypes.data + 2))
    assert st == -1 and 'aligned' in msg, msg
    with pytest.raises(ValueError):
        batch.read_observation(7)
    with pytest.raises(ValueError):
        batch.read_observation(rd.OBS_RGB8, 3)
    # a level without a playpal: the colour formats are refused, the depth minimum resolves
    desc, keep = rd.make_desc(lv)
    desc.playpal = None
    bare = rd.Batch(rd.DeviceLevel(desc), w, h, len(poses))
    bare.render(poses, lights)
    for fmt in COLOUR:
        refused('playpal', bare.read_observation, fmt, 4)
    rgb, depth, _ = oracle_full_size(lv, poses, lights, w, h)
    check_observations(bare, None, depth, [(4, 4)], 'no playpal', (rd.OBS_DEPTH_MIN,))
    del keep
    # nothing of that leaks into the next render
    batch.render(poses, lights)
    batch.finish()
    check_observations(batch, rgb, depth, [(4, 4), (8, 2)], 'after the refused calls')
