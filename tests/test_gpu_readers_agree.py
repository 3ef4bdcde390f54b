"""GPU: the five values read back from one render -- RGB, depth, label, primitive id and thing -- agree with each other pixel for
pixel, and the reduced observations at factor 1 are the full-size frames.  The readers (resolve.hip, planes.hip, observe.hip) share
one walk over what a render leaves on the device (rust-doom_amd/csrc/hip/render_walk.hpp); the comparisons with the oracle are in
test_gpu_rgb.py, test_gpu_planes.py, test_gpu_observe.py and test_gpu_framethings.py.  This compares the product with itself, on
the smallest frame that takes every path of that walk at once: 161 x 136 is a second workgroup across whose last three waves
return at once, a row tail of one pixel, u16 rows that start on odd halfwords, and a second row group.  Three frames of level 0
with the hand-made grid of decor quads before its start (test_gpu_hidden_things.hand_made): two from so close that whole quadrants
are one decor triangle's and the table describes them, one of the grid and the room behind it.  Floors and ceilings are left out
of the render (kinds), so that the third frame has pixels nothing was drawn to.

  - observe_fix_kernel: one more s_and_saveexec / s_cbranch_execz pair and two fewer v_cndmask (supposed, not traced: the walk's
    frame test and the kernel's cell test are two branches where the copy had one).
  - The main kernels of the RGB pass and of all three public planes have the parent's opcode histogram exactly: the text differs
    in the order of the prologue, in register names and in the offsets of the kernel-argument loads only.
"""
import numpy as np
import pytest

import rust_doom_amd as rd
from util import dirtying_poses

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
W, H, N = 161, 136, 3
LEAK_MOD = 97
KINDS = rd.ALL_KINDS & ~(1 << rd.KIND_FLAT)


def poses_and_level():
    from test_gpu_hidden_things import hand_made, level
    c = hand_made()
    pos, yaw = c['start']
    fwd = np.array([-np.sin(yaw), -np.cos(yaw)])
    right = np.array([np.cos(yaw), -np.sin(yaw)])
    poses = np.zeros(N, rd.POSE)
    for p, d in enumerate((1.1, 1.16)):  # the grid stands 1.2 ahead; the eye before the middle of column 5, row 3
        eye = (pos[0] + d * fwd[0] + 0.045 * right[0], pos[1] - 0.25 + 0.09 * 3 + 0.035, pos[2] + d * fwd[1] + 0.045 * right[1])
        poses[p] = rd.pose_look(eye, float(yaw), 0.0, W, H, 0.0)
    poses[2] = rd.pose_look((pos[0], pos[1] + 0.12, pos[2]), float(yaw) + 0.08, -0.1, W, H, 0.0)
    return c, poses, level(0)['lights']


def readers_agree(batch):
    """every relation between the five values of the batch's last render, in both row orders; returns the pixels that name a thing"""
    things = 0
    for top_down in (False, True):
        prim = batch.read_plane(rd.PLANE_PRIMITIVE, top_down=top_down)
        label = batch.read_plane(rd.PLANE_LABEL, top_down=top_down)
        depth = batch.read_depth(top_down=top_down)
        thing = batch.read_thing_plane(top_down=top_down)
        rgba = batch.read_rgb(alpha=True, top_down=top_down)
        rgb = batch.read_rgb(top_down=top_down)
        assert prim.shape == label.shape == depth.shape == thing.shape == rgba.shape[:3] == (N, H, W)
        none = prim == rd.NO_PRIMITIVE
        print('top_down=%s: %d of %d pixels show nothing' % (top_down, int(none.sum()), none.size))
        assert none.any() and not none.all()
        assert np.array_equal(none, label == rd.LABEL_NONE)
        assert np.array_equal(none, rgba[..., 3] == 0)
        assert np.array_equal(rgba[..., :3], rgb)
        assert (depth.view(np.uint32)[none] == 0x7F800000).all()  # +inf
        assert ((label[thing >= 0] & 0xF) == rd.KIND_DECOR).all()
        things += int((thing >= 0).sum())
        assert np.array_equal(batch.read_observation(rd.OBS_RGB8, 1, top_down=top_down), rgb)
        assert np.array_equal(batch.read_observation(rd.OBS_DEPTH_MIN, 1, top_down=top_down).view(np.uint32), depth.view(np.uint32))
    return things


def test_the_five_readers_of_one_render_agree():
    rd.set_device(0)
    c, poses, lights = poses_and_level()
    dev = rd.DeviceLevel(c['arrays'])
    dev.set_decor_things(c['table'])
    described, fixups = [], []
    try:
        for leak_mod in (0, LEAK_MOD):
            rd.debug_set('reset')
            if leak_mod:
                rd.debug_set('leak_mod', leak_mod)
            batch = rd.Batch(dev, W, H, N)
            batch.render(dirtying_poses(poses), lights, kinds=KINDS)  # another frame's words, table and lists wherever this render writes none
            timings = batch.render(poses, lights, kinds=KINDS, timed=True)
            stats = batch.path_stats()
            print('leak_mod %d: described quadrants %d of %d, fixup pixels %d'
                  % (leak_mod, stats['described_quadrants'], stats['quadrants'], timings['fixup_pixels']))
            described.append(stats['described_quadrants']), fixups.append(timings['fixup_pixels'])
            assert readers_agree(batch) > 0
            batch.close()
    finally:
        rd.debug_set('reset')
    # not vacuous: the table settled quadrants whose visibility words are the other render's, and the fixup list had pixels
    assert described[0] >= 1
    assert fixups[1] >= 1
