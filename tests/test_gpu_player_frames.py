"""Player frames on the GPU (frames.hip player_frames_kernel, rdoom_batch_render_players): cameras bit for bit against the test-side
restatement; render_players against rdoom_batch_render_levels fed the matrices it returns (identical frames except sky columns on
the poses whose host sky angle is not correctly rounded) and against the oracle; a closed step -> render -> resolve loop with no
host wait; an out-of-range level slot; host-side argument checks on a real batch; kernel resources and unchanged world kernels."""
import ctypes
import glob
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import frames_ref
import rust_doom_amd as rd
import worldset_ref
from test_gpu_game import _script
from test_gpu_worldset import SET, _players
from util import ROOT, dirtying_poses, render_checked

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
NO_SKY = rd.ALL_KINDS & ~(1 << rd.KIND_SKY)


@pytest.fixture(scope='module')
def exits(tmp_path_factory):
    return worldset_ref.exit_variant(str(tmp_path_factory.mktemp('exit_levels')))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stepped(exits, n, seed, ticks=600):
    """n players of the E1M1..E1M3 exit set after `ticks` game ticks with pushes: (ws, states tensor, game, offsets, levels)"""
    ws, st, lv, inp, act = _players(exits, n, seed)
    game, offs, levels = ws.game_state(lv)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ws.step_game(states, inp[:ticks], game, offs, levels, actions=act[:ticks])
    torch.cuda.synchronize()
    return ws, states, game, offs, levels


def _host_states(states):
    return states.cpu().numpy().view(rd.PLAYER_STATE).copy()


def _sky_mask(built):
    """per primitive id of the level: True for the triangles of KIND_SKY draws (primitive id = position in draw order)"""
    d = built.arrays()['draws']
    ntri = (d[:, 3] // 3).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(ntri)[:-1]])
    mask = np.zeros(int(ntri.sum()) + 1, bool)
    for k in np.nonzero(d[:, 0] == rd.KIND_SKY)[0]:
        mask[first[k]:first[k] + ntri[k]] = True
    return mask


def _exact_poses(poses, mvs, n_obj):
    """poses whose every sky angle (the pose's and each object's it draws) is the same from glibc atan2f and correctly rounded"""
    proj = poses['projection'][0]
    h0, c0 = frames_ref.sky_angles(proj, poses['modelview'])
    ok = h0 == c0
    if mvs is not None:
        h1, c1 = frames_ref.sky_angles(proj, mvs[:, :n_obj])
        ok &= (h1 == c1).all(1)
    return ok


def _check_sky_rule(fb_dev, fb_host, prim, lop, sky, exact):
    """exact poses: identical; the others: every differing pixel shows a sky triangle"""
    diff = fb_dev != fb_host
    assert not diff[exact].any(), np.nonzero(diff[exact].any((1, 2)))[0][:8]
    for p in np.nonzero(diff.any((1, 2)))[0]:
        ids = prim[p][diff[p]]
        assert (ids != rd.NO_PRIMITIVE).all() and sky[lop[p]][ids].all(), p
    return int(diff.any((1, 2)).sum())


def _render_players_checked(batch, other, other_lights, other_lop, **kw):
    """render_checked's discipline for render_players: after a render of other poses, without and then with primitive ids"""
    batch.render(other, other_lights, level_of_pose=other_lop)
    batch.render_players(**kw)
    fb_plain = batch.read_framebuffer()
    batch.enable_primitive_ids()
    batch.render(other, other_lights, level_of_pose=other_lop)
    batch.render_players(**kw)
    return fb_plain, batch.read_framebuffer(), batch.read_primitive_ids()


def test_device_cameras_equal_the_restatement(exits):
    rd.set_device(0)
    ws, states, _, offs, _ = _stepped(exits, 4096, 81, ticks=300)
    st = _host_states(states)
    rng = np.random.default_rng(82)  # and turned far: yaw in +-60 pi, pitch at the clamp
    lim = F(1.57079637) - F(1e-2)
    st[::2]['yaw'] = rng.uniform(-60 * np.pi, 60 * np.pi, len(st[::2])).astype(F)
    st[1::4]['pitch'], st[3::4]['pitch'] = lim, -lim
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    offs_np = offs.cpu().numpy()
    assert (offs_np != 0).any()
    for w, h, t in ((320, 200, 0.0), (1920, 1080, 2.5), (77, 31, 1.0)):
        poses, mvs = rd.poses_from_players_device(states, w, h, t, offsets=offs)
        torch.cuda.synchronize()
        want_p, want_m = frames_ref.cameras(st, w, h, t, offs_np)
        assert np.array_equal(_u32(poses.cpu().numpy()), _u32(want_p).reshape(len(st), -1))
        assert np.array_equal(_u32(mvs.cpu().numpy()), _u32(want_m))
        only, none = rd.poses_from_players_device(states, w, h, t)
        assert none is None and torch.equal(only, poses)


def test_render_players_matches_render_levels_and_the_oracle(exits):
    from oracle import raster
    rd.set_device(0)
    n, w, h = 1024, 160, 100
    ws, states, game, offs, levels = _stepped(exits, n, 91)
    lop = levels.cpu().numpy().astype(np.uint32)
    assert len(set(lop.tolist())) == 3 and (offs.cpu().numpy() != 0).any()
    wad = rd.Wad(exits[0], exits[1])
    built = [wad.build_level(i) for i in SET]
    lset = rd.DeviceLevelSet(built)
    n_obj = lset.num_objects()
    table = np.stack([b.lights_at(0.75) for b in built])
    lights = torch.from_numpy(table).cuda()
    pose_t = torch.empty((n, rd.POSE.itemsize // 4), dtype=torch.float32, device='cuda')
    mv_t = torch.empty((n, offs.shape[1], 16), dtype=torch.float32, device='cuda')
    other = dirtying_poses(rd.poses_from_players(_host_states(states), w, h, 0.75))
    other_lop = np.roll(lop, 1)
    dev = rd.Batch(lset, w, h, n)
    kw = dict(states=states, lights=lights, levels=levels, offsets=offs, time=0.75, poses_out=pose_t, modelviews_out=mv_t)
    fb, fb_ids, prim = _render_players_checked(dev, other, table[other_lop], other_lop, **kw)
    rgb = dev.read_rgb()
    poses = pose_t.cpu().numpy().view(rd.POSE).reshape(-1)
    mvs = mv_t.cpu().numpy()
    want_p, want_m = frames_ref.cameras(_host_states(states), w, h, 0.75, offs.cpu().numpy())
    assert np.array_equal(_u32(poses), _u32(want_p)) and np.array_equal(_u32(mvs), _u32(want_m))
    host = rd.Batch(lset, w, h, n)
    hfb, hfb_ids, hprim = render_checked(host, poses, table[lop], level_of_pose=lop, object_modelviews=mvs[:, :n_obj])
    hrgb = host.read_rgb()
    assert np.array_equal(fb, fb_ids) and np.array_equal(hfb, hfb_ids)
    assert np.array_equal(prim, hprim)  # (the sky angle moves texels, never coverage)
    sky = [_sky_mask(b) for b in built]
    exact = _exact_poses(poses, mvs, n_obj)
    assert 0.5 < exact.mean() < 1.0, exact.mean()
    differing = _check_sky_rule(fb, hfb, prim, lop, sky, exact)
    assert np.array_equal(rgb[exact], hrgb[exact])
    assert not (rgb != hrgb).any(-1)[fb == hfb].any()  # (colours differ only where palette indices do)
    print('poses with a sky angle off by libm: %d, with differing pixels: %d' % (int((~exact).sum()), differing))
    # without sky: every pose identical
    fb2, fb2_ids, prim2 = _render_players_checked(dev, other, table[other_lop], other_lop, kinds=NO_SKY, **kw)
    hfb2, _, hprim2 = render_checked(host, poses, table[lop], kinds=NO_SKY, level_of_pose=lop, object_modelviews=mvs[:, :n_obj])
    assert np.array_equal(fb2, hfb2) and np.array_equal(fb2_ids, hfb2) and np.array_equal(prim2, hprim2)
    # the oracle, on exact poses of every level
    oracles = [raster.RasterOracle(b.arrays()) for b in built]
    picked = [p for lvl in range(3) for p in np.nonzero(exact & (lop == lvl))[0][:6]]
    for p in picked:
        b = built[lop[p]]
        want = oracles[lop[p]].render(poses[p]['modelview'], poses[p]['projection'], 0.75, table[lop[p]], w, h,
                                      object_modelviews=mvs[p, :int(b.counters()['num_objects'])])
        assert np.array_equal(want, fb[p]) and np.array_equal(want, fb_ids[p]), p


def _host_path_rgb(level, states, offs, lights_table, lop, w, h, n_obj):
    """the host path's render of final states (poses from rdoom_poses_from_players_device): (RGB, framebuffers, primitive ids)"""
    poses, mvs = rd.poses_from_players_device(states, w, h, 0.0, offsets=offs)
    poses = poses.cpu().numpy().view(rd.POSE).reshape(-1)
    mvs = mvs.cpu().numpy()
    b = rd.Batch(level, w, h, len(poses))
    b.enable_primitive_ids()
    b.render(poses, lights_table[lop], level_of_pose=lop, object_modelviews=mvs[:, :n_obj])
    return b.read_rgb(), b.read_framebuffer(), b.read_primitive_ids(), poses, mvs


def _closed_loop(step, level, states, offs, levels, lights, ticks, n, w, h):
    """`ticks` x (step 1 tick -> render_players -> resolve_rgb) queued on one stream, no host wait; returns the last RGB frames"""
    stream = torch.cuda.Stream()
    batch = rd.Batch(level, w, h, n)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    for k in range(ticks):
        step(k, stream)
        batch.render_players(states, lights, levels=levels, offsets=offs, stream=stream)
        batch.resolve_rgb(rgb, stream=stream)
    stream.synchronize()
    batch.finish()
    return rgb.cpu().numpy()


def test_closed_loop_on_a_world_set(exits):
    rd.set_device(0)
    n, w, h, ticks = 256, 160, 100, 120
    ws, st, lv, inp, act = _players(exits, n, 101)
    game, offs, levels = ws.game_state(lv)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti = torch.from_numpy(inp[:ticks].view(np.uint8).reshape(-1).copy()).cuda()
    ta = torch.from_numpy(act[:ticks].reshape(-1).copy()).cuda()
    wad = rd.Wad(exits[0], exits[1])
    built = [wad.build_level(i) for i in SET]
    lset = rd.DeviceLevelSet(built)
    table = np.stack([b.lights_at(0.0) for b in built])
    lights = torch.from_numpy(table).cuda()

    def step(k, stream):
        ws.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, levels, actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=stream)
    got = _closed_loop(step, lset, states, offs, levels, lights, ticks, n, w, h)
    lop = levels.cpu().numpy().astype(np.uint32)
    assert (lop != lv).any()  # (some players changed level on the way)
    fresh = rd.Batch(lset, w, h, n)
    fresh.render_players(states, lights, levels=levels, offsets=offs)
    assert np.array_equal(got, fresh.read_rgb())
    fresh.enable_primitive_ids()
    fresh.render_players(states, lights, levels=levels, offsets=offs)
    dfb = fresh.read_framebuffer()
    hrgb, hfb, hprim, poses, mvs = _host_path_rgb(lset, states, offs, table, lop, w, h, lset.num_objects())
    exact = _exact_poses(poses, mvs, lset.num_objects())
    _check_sky_rule(dfb, hfb, hprim, lop, [_sky_mask(b) for b in built], exact)
    assert np.array_equal(got[exact], hrgb[exact])


def test_closed_loop_on_a_single_level_world(exits):
    rd.set_device(0)
    n, w, h, ticks = 128, 160, 100, 120
    wad = rd.Wad(exits[0], exits[1])
    world = wad.build_world(0)
    built = wad.build_level(0)
    level = rd.DeviceLevel(built)
    pos, yaw = built.start()
    rng = np.random.default_rng(111)
    st = rd.player_states(np.repeat(np.asarray(pos, F)[None], n, 0), F(yaw) + rng.normal(scale=1.0, size=n).astype(F))
    inp, act = _script(n, ticks, 112, push=0.1)
    game, offs = world.game_state(n)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda()
    ta = torch.from_numpy(act.reshape(-1).copy()).cuda()
    table = built.lights_at(0.0)[None]
    lights = torch.from_numpy(table[0].copy()).cuda()

    def step(k, stream):
        world.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=stream)
    got = _closed_loop(step, level, states, offs, None, lights, ticks, n, w, h)
    fresh = rd.Batch(level, w, h, n)
    fresh.enable_primitive_ids()
    fresh.render_players(states, lights, offsets=offs)
    assert np.array_equal(got, fresh.read_rgb())
    dfb = fresh.read_framebuffer()
    lop = np.zeros(n, np.uint32)
    hrgb, hfb, hprim, poses, mvs = _host_path_rgb(level, states, offs, table, lop, w, h, level.num_objects())
    exact = _exact_poses(poses, mvs, level.num_objects())
    _check_sky_rule(dfb, hfb, hprim, lop, [_sky_mask(built)], exact)
    assert np.array_equal(got[exact], hrgb[exact])


def test_a_level_outside_the_set_is_reported_and_the_rest_is_rendered(exits):
    rd.set_device(0)
    n, w, h = 64, 128, 80
    ws, states, game, offs, levels = _stepped(exits, n, 121, ticks=120)
    wad = rd.Wad(exits[0], exits[1])
    built = [wad.build_level(i) for i in SET]
    lset = rd.DeviceLevelSet(built)
    table = np.stack([b.lights_at(0.0) for b in built])
    lights = torch.from_numpy(table).cuda()
    bad = levels.clone()
    bad[9], bad[5], bad[40] = 3, 7, -1
    batch = rd.Batch(lset, w, h, n)
    pose_t = torch.empty((n, rd.POSE.itemsize // 4), dtype=torch.float32, device='cuda')
    batch.render_players(states, lights, levels=bad, offsets=offs, kinds=NO_SKY, poses_out=pose_t)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda')
    batch.resolve_rgb(rgb)
    with pytest.raises(rd.RdoomError) as e:
        batch.finish()
    assert e.value.status == -1 and 'pose 5 ' in str(e.value)
    with pytest.raises(rd.RdoomError):
        batch.read_framebuffer()
    with pytest.raises(rd.RdoomError):
        batch.read_rgb()
    # every pose rendered: the bad ones as level 0, the others as named
    lop = levels.cpu().numpy().astype(np.uint32)
    lop[[5, 9, 40]] = 0
    poses = pose_t.cpu().numpy().view(rd.POSE).reshape(-1)
    mvs = rd.poses_from_players_device(states, w, h, 0.0, offsets=offs)[1].cpu().numpy()
    host = rd.Batch(lset, w, h, n)
    host.render(poses, table[lop], kinds=NO_SKY, level_of_pose=lop, object_modelviews=mvs[:, :lset.num_objects()])
    assert np.array_equal(rgb.cpu().numpy(), host.read_rgb())
    batch.render_players(states, lights, levels=levels, offsets=offs)  # the next valid render is clean
    batch.finish()
    assert batch.read_framebuffer().shape[0] == n


def test_host_checks_on_a_batch_queue_nothing(exits):
    rd.set_device(0)
    n, w, h = 16, 64, 40
    ws, states, game, offs, levels = _stepped(exits, n, 131, ticks=30)
    wad = rd.Wad(exits[0], exits[1])
    built = [wad.build_level(i) for i in SET]
    lset = rd.DeviceLevelSet(built)
    lights = torch.from_numpy(np.stack([b.lights_at(0.0) for b in built])).cuda()
    batch = rd.Batch(lset, w, h, n)
    batch.render_players(states, lights, levels=levels, offsets=offs)
    before = batch.read_framebuffer()
    L = rd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    n_obj = int(offs.shape[1])
    f = ctypes.c_float(0.0)

    def call(st=states, lv=levels, of=offs, no=n_obj, li=lights, stride=256, count=n, flags=0):
        return L.rdoom_batch_render_players(batch._h, p(st), p(lv), p(of), no, p(li), stride, f, count, rd.ALL_KINDS, flags, None, None, None)
    cases = [dict(st=None), dict(li=None), dict(count=0), dict(count=n + 1), dict(no=lset.num_objects() - 1), dict(lv=None),
             dict(stride=128), dict(stride=255), dict(flags=2)]
    for c in cases:
        assert call(**c) == -1, c
    assert L.rdoom_batch_render_players(None, p(states), p(levels), p(offs), n_obj, p(lights), 256, f, n, rd.ALL_KINDS, 0, None, None, None) == -1
    batch.finish()
    assert np.array_equal(batch.read_framebuffer(), before)  # nothing was queued
    assert call() == 0
    batch.finish()


# ---- kernel resources; the world kernels' code ----
# sha256 of each world kernel's instructions (llvm-objdump text without addresses), pinned with the compiler that made them.
# The four hot kernels are unchanged since sincos_rd moved to a shared header; player_step_kernel (step_players with the NoGame
# policy) and game_reset_kernel (the shared fresh_word) were re-pinned when their copies of that code were removed.
WORLD_KERNELS_LLVM = 'roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5'
WORLD_KERNELS = {
    '_ZN12_GLOBAL__N_112sweep_kernelENS_9WorldViewEPKfS2_jS2_jPf': '493af72086e0ea257410b4fc3fb242312fb7cd71358a103fff0182baf82eda40',
    '_ZN12_GLOBAL__N_116game_step_kernelENS_9WorldViewENS_9GameLevelEPKNS_10DevTriggerEPKNS_9DevEffectEP18rdoom_player_statePK18rdoom_player_inputj19rdoom_player_config':
        '0d071ad07ec7aa5b803d49c051b3415360f2a637d55fe73068b8883d69d9c767',
    '_ZN12_GLOBAL__N_117game_reset_kernelENS_8GameViewEPjPfjPKh': '833d57333a4745052de32e753496da6d0a392ba3d94780cc28279cfd871fd635',
    '_ZN12_GLOBAL__N_118player_step_kernelENS_9WorldViewEP18rdoom_player_statePK18rdoom_player_inputjj19rdoom_player_configfPKfj':
        '69948695548050607a008e06e5c53e4866b3af4113dc6c4638e078264a16478b',
    '_ZN12_GLOBAL__N_125worldset_game_step_kernelENS_9WorldViewENS_7SetGameEPKNS_10DevTriggerEPKNS_9DevEffectEPKNS_11DevSetLevelEP18rdoom_player_statePK18rdoom_player_inputj19rdoom_player_config':
        'cbcd23b349071a304f9bdff7d0c413da7f365d7795a9aae3ab265cdd05c033ee',
    '_ZN12_GLOBAL__N_126worldset_game_reset_kernelEPKNS_11DevSetLevelEjjPjPfjPKjPKh': '6e7c5ccb3bcdf1993354b0504bc1babb8e2e73e6b323c055d10ca70c7a488e0a',
    # the two ray kernels, pinned since they take the player's orientation and eye from player_quat.hpp
    '_ZN12_GLOBAL__N_116cast_rays_kernelENS_9WorldViewENS_7RayArgsE': '02d6b5c3a74911bd018371c6218ce5a4fbc87d7dffed5471ad3ed589fb3ce0d6',
    '_ZN12_GLOBAL__N_125worldset_cast_rays_kernelENS_9WorldViewENS_7RayArgsEPKNS_11DevSetLevelEPKjS6_j':
        '5fc964c776fc63a7414ef8d5755010de3a92a0b70854366e154661a452ffd77f',
}


def _kernel_text(lib):
    llvm = '/opt/rocm/lib/llvm/bin'
    tmp = tempfile.mkdtemp(prefix='rdoom_isa_')
    try:
        so = os.path.join(tmp, 'lib.so')
        shutil.copy(lib, so)
        subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', so], capture_output=True, check=True, cwd=tmp)
        out = {}
        for co in sorted(glob.glob(so + '.*gfx950*')):
            txt = subprocess.run([os.path.join(llvm, 'llvm-objdump'), '-d', co], capture_output=True, text=True, check=True).stdout
            for part in re.split(r'\n(?=[0-9a-f]+ <[^>]+>:)', txt):
                m = re.match(r'[0-9a-f]+ <([^>]+)>:', part)
                if m:
                    out[m.group(1)] = re.sub(r'// [0-9A-F]{12}:', '//', part.split('\n', 1)[1])
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_kernel_resources_and_pinned_world_kernels():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    r = res['player_frames_kernel']
    assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    version = subprocess.run(['/opt/rocm/lib/llvm/bin/clang', '--version'], capture_output=True, text=True).stdout  # (the pin's compiler)
    if WORLD_KERNELS_LLVM not in version:
        return  # (another compiler makes other code: the pin below is for the one the hashes were taken with)
    # player_step_kernel through step_players: the register allocation of its former copy of the body (144 VGPRs), no more SGPR spills
    r = res['player_step_kernel']
    assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, r
    assert r['vgpr_count'] <= 144 and r['sgpr_spill_count'] <= 10, r
    text = _kernel_text(os.path.join(ROOT, 'rust-doom_amd', 'librdoom_hip.so'))
    for mangled, want in WORLD_KERNELS.items():
        assert hashlib.sha256(text[mangled].encode()).hexdigest() == want, mangled
