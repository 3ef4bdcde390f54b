"""GPU: RGB frames (rdoom_batch_resolve_rgb / rdoom_batch_read_rgb) -- the colours the reference's window shows.  The expected
frames are composed here from the ORACLE's index frames and primitive ids (never from the product's own output): PLAYPAL 0 of
the pose's level at the index, the GL clear colour (15, 18, 23) where the id is 0xFFFFFFFF, alpha 255 / 0, optional flip to
top-down rows.  Every checked render follows a render of other poses (tests/util.py: dirtying_poses), so that a reader of a
visibility word the checked render did not write meets another frame's record; and each is checked on the plain path and
again after rdoom_batch_enable_primitive_ids."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import rust_doom_amd as rd
from oracle import raster
from util import GOLDEN, META_PATH, dirtying_poses

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = [(a, t) for a in (False, True) for t in (False, True)]  # (alpha, top_down)


def compose(fb, prim, playpal, alpha=False, top_down=False):
    """(n, H, W) indices + ids -> (n, H, W, 3|4), as the reference's window shows them"""
    rgb = np.asarray(playpal, np.uint8).reshape(256, 3)[fb]
    clear = prim == 0xFFFFFFFF
    rgb[clear] = (15, 18, 23)  # window.rs:40-44 (tests/gl_readback.py: CLEAR_RGB)
    if alpha:
        rgb = np.concatenate([rgb, np.where(clear, 0, 255).astype(np.uint8)[..., None]], -1)
    return rgb[:, ::-1] if top_down else rgb


def oracle_frames(lv, poses, lights, w, h, object_modelviews=None):
    ro = raster.RasterOracle(lv)
    fbs, prims = [], []
    for i in range(len(poses)):
        om = None if object_modelviews is None else object_modelviews[i]
        f, p = ro.render(poses[i]['modelview'], poses[i]['projection'], float(poses[i]['time']), lights[i], w, h, want_prim=True,
                         object_modelviews=om)
        fbs.append(f)
        prims.append(p)
    return np.array(fbs), np.array(prims)


def check_all_formats(batch, fb, prim, palettes, what):
    """palettes: one 768-byte PLAYPAL per frame"""
    for alpha, top_down in FORMATS:
        got = batch.read_rgb(alpha=alpha, top_down=top_down)
        assert got.shape == (len(fb), batch.height, batch.width, 4 if alpha else 3)
        for i in range(len(fb)):
            want = compose(fb[i:i + 1], prim[i:i + 1], palettes[i], alpha, top_down)[0]
            bad = int((got[i] != want).any(-1).sum())
            assert bad == 0, (what, i, alpha, top_down, bad)


def render_both_paths_and_check(batch, poses, lights, fb, prim, palettes, what, **kw):
    other = dirtying_poses(poses)
    olights = np.roll(lights, 1, axis=0)
    dkw = {k: v for k, v in kw.items() if k != 'object_modelviews'}
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_all_formats(batch, fb, prim, palettes, what + ' (plain path)')
    batch.enable_primitive_ids()
    batch.render(other, olights, **dkw)
    batch.render(poses, lights, **kw)
    check_all_formats(batch, fb, prim, palettes, what + ' (id path)')


def golden_case(lv, index):
    g = json.load(open(os.path.join(GOLDEN, 'digests.json')))
    rows = np.load(os.path.join(GOLDEN, 'poses.npy'))[index]
    poses = np.zeros(len(rows), rd.POSE)
    for i, p in enumerate(rows):
        poses[i]['modelview'], poses[i]['projection'], poses[i]['time'] = p[:16], p[16:32], p[32]
    lights = np.array([lv.lights.fill_buffer_at(float(p['time'])) for p in poses])
    return poses, lights, g['width'], g['height']


@pytest.mark.parametrize('index', [0, 3, 7])
def test_golden_poses_equal_the_oracle_composition(oracle_levels, index):
    lv = oracle_levels(index)
    poses, lights, w, h = golden_case(lv, index)
    fb, prim = oracle_frames(lv, poses, lights, w, h)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, fb, prim, [lv.palette] * len(poses), 'golden level %d' % index)


def outside_pose(lv, w, h, time):
    """a view from outside the level back at it: geometry and the void around it in one frame (the sweeps see geometry only)"""
    from util import reference_projection, view_matrix
    pos = lv.static_vertices['a_pos']
    lo, hi = pos.min(0), pos.max(0)
    eye = np.array([hi[0] + 0.6 * (hi[0] - lo[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    ro = raster.RasterOracle(lv)
    for yaw in np.linspace(0, 2 * np.pi, 16, endpoint=False):
        p = np.zeros(1, rd.POSE)
        p[0]['modelview'], p[0]['projection'], p[0]['time'] = view_matrix(eye, yaw, 0.0), reference_projection(w, h), time
        _, prim = ro.render(p[0]['modelview'], p[0]['projection'], time, lv.lights.fill_buffer_at(time), w, h, want_prim=True)
        if 0.05 < (prim == 0xFFFFFFFF).mean() < 0.95:
            return p
    raise AssertionError('no view from outside the level shows both geometry and the void')


@pytest.mark.parametrize('size', [(321, 200, 4), (1000, 520, 2), (1920, 1080, 2), (16384, 40, 1)])
def test_sweep_poses_at_odd_and_full_sizes(wad_path, oracle_levels, size):
    """321 x 200: padded row pitch (324), byte stores of RGB8 rows; 1000 x 520: a 8-pixel tail per row; 1920 x 1080: the bench size
    (poses of the seeded sweep bench.py times)"""
    import importlib
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
    fb, prim = oracle_frames(lv, poses, lights, w, h)
    assert (prim == 0xFFFFFFFF).any() and (prim != 0xFFFFFFFF).any()  # both kinds of pixel are checked
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, fb, prim, [lv.palette] * len(poses), '%dx%d' % (w, h))


def test_committed_gl_readbacks_differ_exactly_where_the_census_says(wad_path, oracle_levels):
    """the library's own RGB frame against the reference's shaders' RGB readback: the census's mismatch count, frame by frame"""
    import test_gl_readback as gr
    wad = rd.Wad(wad_path, META_PATH)
    by_level = {}
    for k in gr.KEYS:
        by_level.setdefault((gr.CENSUS['frames'][k]['level'], gr.CENSUS['frames'][k]['width']), []).append(k)
    checked = 0
    for (index, width), keys in sorted(by_level.items()):
        lv = oracle_levels(index)
        built = wad.build_level(index)
        height = gr.CENSUS['frames'][keys[0]]['height']
        batch = rd.Batch(rd.DeviceLevel(built), width, height, 1)
        for key in keys:
            c, mv, pr, t, lights, om = gr.frame_inputs(lv, key)
            pose = np.zeros(1, rd.POSE)
            pose[0]['modelview'], pose[0]['projection'], pose[0]['time'] = mv, pr, t
            batch.render(pose, built.lights_at(t), object_modelviews=None if om is None else om[None])
            rgb = batch.read_rgb()[0]
            assert int((rgb != gr.FRAMES[key + '_rgb']).any(-1).sum()) == c['mismatch'], key
            checked += 1
    assert checked == len(gr.KEYS) >= 46


def test_every_debug_hook_in_one_child():
    """the sweep of tests/gpu_rgb_child.py: every hook of tests/test_gpu_debug_paths.py, RGB == the composition of that process's
    own id-path frames (leak_mod: thousands of ordinary pixels through fixup_kernel and the fix-list pass)"""
    fields = run_child('hooks')
    assert int(fields['bad']) == 0 and int(fields['cases']) == 28 and int(fields['fixups']) > 3000


def test_level_set_uses_each_poses_own_palette(oracle_levels):
    """two levels of one IWAD, the second with its PLAYPAL permuted (same COLORMAP: the set is created); mixed poses with moving
    objects and varying times -- every frame in its own level's colours"""
    from test_gpu_levelset import mixed_batch
    levels = [oracle_levels(0), oracle_levels(2)]
    perm = np.random.RandomState(5).permutation(256)
    fields = ('static_vertices', 'static_indices', 'sky_vertices', 'sky_indices', 'decor_vertices', 'decor_indices', 'draws',
              'flat_atlas', 'wall_atlas', 'decor_atlas', 'sky_texture', 'sky_band', 'colormap')
    second = types.SimpleNamespace(**{f: getattr(levels[1], f) for f in fields if hasattr(levels[1], f)})
    second.palette = np.asarray(levels[1].palette, np.uint8).reshape(256, 3)[perm].reshape(-1)
    palettes_of_level = [np.asarray(levels[0].palette, np.uint8), second.palette]
    w, h = 640, 400
    poses, lop, lights, om = mixed_batch(levels, 3, w, h, seed=77, moving=True)
    assert len(set(lop.tolist())) == 2 and (poses['time'] > 0).any()
    lset = rd.DeviceLevelSet([levels[0], second])
    fbs, prims = [], []
    for i in range(len(poses)):
        lv = levels[lop[i]]
        f, p = oracle_frames(lv, poses[i:i + 1], lights[i:i + 1], w, h, om[i:i + 1, :int(lv.num_objects)])
        fbs.append(f[0])
        prims.append(p[0])
    batch = rd.Batch(lset, w, h, len(poses))
    render_both_paths_and_check(batch, poses, lights, np.array(fbs), np.array(prims), [palettes_of_level[k] for k in lop],
                                'level set', level_of_pose=lop, object_modelviews=om)


def small_scene(oracle_levels, n=3, w=160, h=96, seed=3):
    from test_gpu_raster_parity import sweep_poses
    lv = oracle_levels(1)
    poses = sweep_poses(lv, n, w, h, seed=seed, time=0.2)
    lights = np.array([lv.lights.fill_buffer_at(0.2)] * n)
    return lv, poses, lights, w, h


def run_child(mode):
    """tests/gpu_rgb_child.py MODE in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_rgb_child.py'), mode], cwd=HERE, capture_output=True, text=True,
                       timeout=1200)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(kv.split('=') for kv in out[-1].split()[1:])


def test_resolve_into_a_torch_tensor_equals_read_rgb():
    """in a child that initialises torch before the library (torch and the library then share one HIP runtime, as in bench.py):
    resolve_rgb into uint8 tensors / raw pointers on the render's stream == read_rgb, sub-ranges, tensors that do not fit"""
    assert run_child('torch')['ok'] == '1'


def test_a_resolve_after_another_render_shows_it(oracle_levels):
    lv, poses, lights, w, h = small_scene(oracle_levels)
    _, poses2, _, _, _ = small_scene(oracle_levels, seed=4)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    batch.render(poses, lights)
    first = batch.read_rgb()
    batch.render(poses2, lights)
    fb, prim = oracle_frames(lv, poses2, lights, w, h)
    assert np.array_equal(batch.read_rgb(), compose(fb, prim, lv.palette))
    assert not np.array_equal(first, batch.read_rgb())
    batch.render(poses2[:1], lights[:1])  # fewer frames: the range shrinks with the render
    assert batch.read_rgb().shape == (1, h, w, 3)


def test_range_and_argument_errors(oracle_levels):
    lv, poses, lights, w, h = small_scene(oracle_levels)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, len(poses))
    with pytest.raises(rd.RdoomError) as e:  # nothing rendered yet
        batch.read_rgb(count=1)
    assert e.value.status == -1
    batch.render(poses, lights)
    for first, count in ((0, 4), (3, 1), (2, 2), (4, 0)):
        with pytest.raises(rd.RdoomError) as e:
            batch.read_rgb(first=first, count=count)
        assert e.value.status == -1 and 'range' in str(e.value), (first, count)
    assert batch.read_rgb(first=3, count=0).shape == (0, h, w, 3)
    host = np.zeros((len(poses), h, w, 3), np.uint8)
    with pytest.raises(rd.RdoomError) as e:  # a host pointer is not device memory
        batch.resolve_rgb(host.ctypes.data)
    assert e.value.status == -1
    L = rd.lib()
    import ctypes
    assert L.rdoom_batch_resolve_rgb(batch._h, 0, 1, 3, None, None) == -1
    assert L.rdoom_batch_read_rgb(batch._h, 0, 1, 0x203, host.ctypes.data_as(ctypes.c_void_p)) == -1
    # nothing of that leaks into the next render
    batch.render(poses, lights)
    batch.finish()
    fb, prim = oracle_frames(lv, poses, lights, w, h)
    assert np.array_equal(batch.read_rgb(), compose(fb, prim, lv.palette))
    batch.enable_primitive_ids()  # (captures from the next render on: nothing to resolve until then)
    with pytest.raises(rd.RdoomError):
        batch.read_rgb(count=1)


def test_a_level_without_a_palette_renders_but_cannot_be_resolved(oracle_levels):
    lv, poses, lights, w, h = small_scene(oracle_levels)
    desc, keep = rd.make_desc(lv)
    desc.playpal = None
    level = rd.DeviceLevel(desc)
    batch = rd.Batch(level, w, h, len(poses))
    batch.render(poses, lights)
    fb, _ = oracle_frames(lv, poses, lights, w, h)
    assert np.array_equal(batch.read_framebuffer(), fb)
    with pytest.raises(rd.RdoomError) as e:
        batch.read_rgb()
    assert e.value.status == -1 and 'playpal' in str(e.value)
    del keep
