"""GPU: the fragment kernel's listed quads (rust-doom_amd/csrc/hip/fragment.hip, shade_listed).  A run the packed body cannot
finish -- mixed triangles, decor, 1/w out of range, an uncertified mod, a transparent texel -- is listed quad by quad, and every
list entry carries a bit that says where its pixels' records are: in the rasteriser's quadrant table, or, for a quadrant without
an entry, in the visibility words.  shade_listed trusts the bit and loads only that one.  The frames here are those in which the
two kinds meet: 32 x 16 blocks inside one quadrant (1280 x 720 and up), 64 x 8 blocks over two quadrants of which one has an entry
(frag_bw=3), every pixel listed under a table (leak_mod), no table at all (no_qtab), 32-bit words, lanes outside the frame, per-lane
records along moving doors, background and out-of-range poses.  Framebuffers against the oracle, byte for byte."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rust_doom_amd as rd
from oracle import raster
from test_gpu_raster_parity import sweep_poses
from util import reference_projection, render_checked, view_matrix

pytestmark = pytest.mark.gpu


def check(lv, poses, lights, w, h, hooks=None, om=None):
    """the framebuffers of one render (after a dirtying render of other poses) against the oracle"""
    kw = {} if om is None else {'object_modelviews': om}
    try:
        for name, value in (hooks or {}).items():
            rd.debug_set(name, value)
        new, _, _ = render_checked(rd.Batch(rd.DeviceLevel(lv), w, h, len(poses)), poses, lights, want_prim=False, **kw)
    finally:
        rd.debug_set('reset')
    ro = raster.RasterOracle(lv)

    def oracle(i):
        li = lights[i] if getattr(lights, 'ndim', 1) == 2 else lights
        return ro.render(poses[i]['modelview'], poses[i]['projection'], float(poses[i]['time']), li, w, h,
                         object_modelviews=None if om is None else om[i])

    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        want = list(ex.map(oracle, range(len(poses))))
    bad = [(i, int((want[i] != new[i]).sum())) for i in range(len(poses))]
    assert all(b[1] == 0 for b in bad), bad
    return new


@pytest.mark.parametrize('size', [(1280, 720), (1288, 722)])
def test_smallest_frame_and_partial_blocks(oracle_levels, size):
    """1280 x 720: the smallest frame with 32 x 16 blocks, each inside one quadrant -- a block's quads are all of one kind.
    1288 x 722: the last block column and row hold lanes outside the frame, which list nothing."""
    lv, (w, h) = oracle_levels(0), size
    fb = check(lv, sweep_poses(lv, 3, w, h, seed=11, time=0.4), lv.lights.fill_buffer_at(0.4), w, h)
    assert (fb != 0).mean() > 0.3


def test_eye_in_a_wall_and_far_outside(oracle_levels):
    """poses as tests/test_gpu_stress_slice.py generates its extreme ones: a hair's breadth from a vertex (rw out of range), on a
    floor plane, far outside looking back (long runs of background blocks)"""
    lv, w, h, n = oracle_levels(0), 1280, 720, 4
    rng = np.random.RandomState(907)
    verts = lv.static_vertices['a_pos']
    poses = np.zeros(n, rd.POSE)
    for i in range(n):
        v = verts[rng.randint(len(verts))].astype(np.float64)
        if i % 4 == 0:
            eye = v + rng.uniform(-0.02, 0.02, 3)
        elif i % 4 == 1:
            eye = v + np.array([rng.uniform(-0.3, 0.3), 1e-4, rng.uniform(-0.3, 0.3)])
        elif i % 4 == 2:
            eye = v + np.array([rng.uniform(-40, 40), rng.uniform(5, 60), rng.uniform(-40, 40)])
        else:
            eye = v + rng.uniform(-0.5, 0.5, 3)
        poses[i]['modelview'] = view_matrix(eye, rng.uniform(0, 2 * np.pi), [0.3, 0.0, -1.5707, 1.2][i % 4])
        poses[i]['projection'] = reference_projection(w, h)
    check(lv, poses, lv.lights.fill_buffer_at(0.0), w, h)


def test_per_pose_light_tables(oracle_levels):
    """a time-varying render: every pose has its own time and light table"""
    lv, w, h, n = oracle_levels(0), 1280, 720, 3
    poses = sweep_poses(lv, n, w, h, seed=5)
    lights = np.zeros((n, 256), np.uint8)
    for i, t in enumerate((0.0, 3.7, 21.3)):
        poses[i]['time'] = t
        lights[i] = lv.lights.fill_buffer_at(t)
    check(lv, poses, lights, w, h)


def test_moving_objects(oracle_levels):
    """rdoom_batch_render_objects: displaced doors and lifts -- per-lane records along their edges, decor in the list"""
    lv, w, h, n = oracle_levels(0), 1280, 720, 3
    rng = np.random.RandomState(3)
    poses = sweep_poses(lv, n, w, h, seed=9, time=1.5)
    n_obj = int(lv.num_objects)
    om = np.zeros((n, n_obj, 16), np.float32)
    for i in range(n):
        v64 = np.asarray(poses[i]['modelview'], np.float64).reshape(4, 4).T
        for o in range(n_obj):
            m = np.eye(4)
            m[1, 3] = 0.0 if o == 0 else rng.uniform(-0.8, 0.8)
            om[i, o] = (v64 @ m).T.astype(np.float32).reshape(16)
    check(lv, poses, lv.lights.fill_buffer_at(1.5), w, h, om=om)


@pytest.mark.parametrize('hooks', [{'frag_bw': 3}, {'leak_mod': 7}, {'leak_mod': 5, 'frag_bw': 3}, {'no_qtab': 1}, {'vis32': 1}, {'vis32': 1, 'frag_bw': 3},
                                   {'frag_nq': 1}, {'keep_vis': 1, 'frag_bw': 3}])
def test_both_kinds_of_entry_in_one_call(oracle_levels, hooks):
    """frag_bw=3: a 64 x 8 block lies in two quadrants; where one has an entry and the other has none the same call of shade_listed
    holds both kinds.  leak_mod: every pixel is listed, those of described quadrants without the bit.  no_qtab: every entry carries
    the bit.  32-bit words and one quad per lane: the other instantiations."""
    lv, w, h = oracle_levels(0), 1288, 722
    check(lv, sweep_poses(lv, 2, w, h, seed=13, time=0.4), lv.lights.fill_buffer_at(0.4), w, h, hooks=hooks)
