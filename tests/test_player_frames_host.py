"""Player cameras on the device (rdoom_poses_from_players_device, rdoom_batch_render_players) at the C-ABI boundary, without a GPU:
the test-side restatement of the device camera (tests/frames_restatement.c, on world_restatement.c's sincos twin) is within the
header's stated bound of the host helpers rdoom_pose_from_player / rdoom_object_modelviews_from_player, objects at rest get the
pose's modelview bit for bit, and the arguments the library can judge without a device are rejected before it is touched."""
import ctypes
import os
import re

import numpy as np

import frames_ref
import rust_doom_amd as rd
from util import ROOT

F = np.float32
HEADER = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
ROT_BOUND = 2.0 ** -19     # modelview rotation entries (magnitude <= 1): absolute (observed: 2^-20)
TRANS_BOUND = 2.0 ** -19   # translation entries: relative to 1 + |x| + |y| + |z| of the position (plus the object's offset)


def random_states(n, seed):
    """yaw in +-60 pi, pitch at the step's clamp limits (a third each) and inside them, positions in a 40-unit box"""
    rng = np.random.default_rng(seed)
    lim = F(1.57079637) - F(1e-2)
    st = np.zeros(n, rd.PLAYER_STATE)
    st['pos'] = rng.uniform(-40, 40, (n, 3)).astype(F)
    st['yaw'] = rng.uniform(-60 * np.pi, 60 * np.pi, n).astype(F)
    pitch = rng.uniform(-lim, lim, n).astype(F)
    pitch[::3], pitch[1::3] = lim, -lim
    st['pitch'] = pitch
    st['flags'] = rd.PLAYER_CLIP
    return st


def random_offsets(n, n_obj, seed):
    rng = np.random.default_rng(seed)
    offs = rng.uniform(-3, 3, (n, n_obj, 3)).astype(F)
    offs[rng.random((n, n_obj)) < 0.4] = 0.0   # objects at rest
    offs[:, :, 0][rng.random((n, n_obj)) < 0.1] = -0.0
    return offs


def _within(got, want, pos):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    scale = 1.0 + np.abs(pos.astype(np.float64)).sum(-1)
    rot = d[..., [0, 1, 2, 4, 5, 6, 8, 9, 10]].max()
    trans = (d[..., 12:15] / scale[..., None]).max()
    rest = d[..., [3, 7, 11, 15]].max()
    return rot, trans, rest


def test_restatement_is_within_the_stated_bound_of_the_host_helpers():
    n, w, h = 10000, 320, 200
    st = random_states(n, 3)
    poses, _ = frames_ref.cameras(st, w, h, 0.25)
    host = rd.poses_from_players(st, w, h, 0.25)
    assert np.array_equal(poses['projection'].view(np.uint32), host['projection'].view(np.uint32))
    assert np.array_equal(poses['time'], host['time'])
    rot, trans, rest = _within(poses['modelview'], host['modelview'], st['pos'])
    assert rot <= ROT_BOUND and trans <= TRANS_BOUND and rest == 0.0, (rot, trans, rest)
    same = (poses['modelview'].view(np.uint32) == host['modelview'].view(np.uint32)).all(1)
    assert 0.2 < same.mean() < 1.0  # (sincos and libm agree on most arguments, not all)


def test_object_modelviews_are_within_the_bound_and_rest_is_the_pose():
    n, n_obj = 10000, 5
    st = random_states(n, 4)
    offs = random_offsets(n, n_obj, 5)
    poses, mvs = frames_ref.cameras(st, 160, 100, 0.0, offs)
    host = rd.object_modelviews_from_players(st, offs)
    rot, trans, rest = _within(mvs, host, st['pos'][:, None, :] + offs)
    assert rot <= ROT_BOUND and trans <= TRANS_BOUND and rest == 0.0, (rot, trans, rest)
    at_rest = (offs == 0.0).all(-1)
    at_rest[:, 0] = True
    pose_mv = np.broadcast_to(poses['modelview'][:, None, :], mvs.shape)
    assert np.array_equal(mvs[at_rest].view(np.uint32), pose_mv[at_rest].view(np.uint32))
    assert not np.array_equal(mvs[~at_rest], pose_mv[~at_rest])


def test_sky_angle_restatement_sees_the_libm_divergence():
    """the host path's atan2f is not correctly rounded for a sizeable share of camera angles"""
    st = random_states(4000, 6)
    poses, _ = frames_ref.cameras(st, 320, 200)
    host, cr = frames_ref.sky_angles(poses['projection'][0], poses['modelview'])
    diff = host != cr
    assert diff.any() and diff.mean() < 0.5
    ulps = np.abs(host.view(np.int32).astype(np.int64) - cr.view(np.int32).astype(np.int64))
    assert ulps.max() <= 2, ulps.max()


def test_header_declares_the_entry_points():
    code = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
    assert re.search(r'rdoom_status rdoom_poses_from_players_device\(const rdoom_player_state \*d_states, uint32_t n, uint32_t width,'
                     r'\s*uint32_t height,\s*float time, const float \*d_object_offsets, uint32_t n_objects,\s*rdoom_pose \*d_poses_out,'
                     r' float \*d_object_modelviews_out, void \*stream\);', code)
    assert re.search(r'rdoom_status rdoom_batch_render_players\(rdoom_batch \*batch, const rdoom_player_state \*d_states,'
                     r' const uint32_t \*d_levels,', code)
    L = rd.lib()
    for name in ('rdoom_poses_from_players_device', 'rdoom_batch_render_players'):
        assert name in rd.API_SYMBOLS and hasattr(L, name)
    assert hasattr(rd.Batch, 'render_players') and callable(rd.poses_from_players_device)


def test_bad_arguments_are_rejected_without_a_device():
    """checks that need no batch: nothing is queued, and no device is needed to see them (this machine may have none)"""
    L = rd.lib()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its host checks first
    f = ctypes.c_float(0.0)
    # rdoom_batch_render_players: a null batch, states or lights
    for b, s, li in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        if b is not None:
            continue  # (a non-null batch must be a real one: the GPU tests check null states / lights on a batch)
        assert L.rdoom_batch_render_players(b, s, None, None, 0, li, 0, f, 1, rd.ALL_KINDS, 0, None, None, None) == -1
        assert b'null' in L.rdoom_last_error()
    # rdoom_poses_from_players_device
    pf = L.rdoom_poses_from_players_device
    assert pf(None, 4, 64, 64, f, None, 0, fake, None, None) == -1 and b'null' in L.rdoom_last_error()
    assert pf(fake, 4, 64, 64, f, None, 0, None, None, None) == -1 and b'null' in L.rdoom_last_error()
    for n, w, h in ((0, 64, 64), (4, 0, 64), (4, 64, 0)):
        assert pf(fake, n, w, h, f, None, 0, fake, None, None) == -1
    assert pf(fake, 4, 64, 64, f, None, 3, fake, fake, None) == -1 and b'offsets' in L.rdoom_last_error()
    assert pf(fake, 4, 64, 64, f, fake, 0, fake, fake, None) == -1
    assert pf(fake, 4, 64, 64, f, fake, 4097, fake, fake, None) == -1
