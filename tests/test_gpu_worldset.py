"""World sets on the GPU (world.hip worldset_game_step_kernel): bit for bit against the test-side restatement of the level change
(tests/worldset_ref.py over tests/game_restatement.c) on a three-level set with walk-over exits; launch splitting and batch
independence; the two-tick timing of a change; a slot without a destination is rdoom_world_step_game; step -> render through a
level set against the oracle; resources."""
import importlib.util
import os

import numpy as np
import pytest

import rust_doom_amd as rd
import world_ref
import worldset_ref
from test_game_host import patched_variant
from step_cases import set_players as _set_players
from test_gpu_game import _script, _seed
from util import ROOT, render_checked

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
SET = [0, 1, 2]


@pytest.fixture(scope='module')
def exits(tmp_path_factory):
    return worldset_ref.exit_variant(str(tmp_path_factory.mktemp('exit_levels')))


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def _players(exits, n, seed, slots=SET):
    return _set_players(exits, n, seed, slots)  # (moved to step_cases; the same bytes)


def test_set_step_matches_the_restatement(exits):
    rd.set_device(0)
    ws, st, lv, inp, act = _players(exits, 1024, 31)
    n = len(st)
    game, offs, levels = ws.game_state(lv)
    got = ws.step_game(st, inp, game, offs, levels, actions=act)
    ref = worldset_ref.RefWorldSet(exits[0], exits[1], SET, lv)
    want = ref.step(st, inp, act)
    bad = (_u32(got) != _u32(want)).any(1)
    assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:8])
    assert levels.cpu().numpy().tolist() == ref.levels.tolist()
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), ref.offsets().view(np.uint32))
    assert ws.n_objects == ref.n_objects
    changed = ref.levels != lv
    assert changed.sum() > 50 and (ref.levels == 2).sum() > (lv == 2).sum()  # many players moved on, some twice
    assert ((lv == 0) & (ref.levels == 2)).any()
    assert (got['flags'][changed] & rd.PLAYER_EXITED).all()


def test_launch_splitting_and_batch_independence(exits):
    rd.set_device(0)
    ws, st, lv, inp, act = _players(exits, 256, 41)
    n = len(st)
    g1, o1, l1 = ws.game_state(lv)
    a = ws.step_game(st, inp, g1, o1, l1, actions=act)
    g2, o2, l2 = ws.game_state(lv)
    s2 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti, ta = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda(), torch.from_numpy(act.reshape(-1).copy()).cuda()
    for k in range(600):
        ws.step_game(s2, ti[k * n * 20:(k + 1) * n * 20], g2, o2, l2, actions=ta[k * n:(k + 1) * n], n_ticks=1)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(a), _u32(s2.cpu().numpy().view(rd.PLAYER_STATE)))
    assert torch.equal(o1, o2) and torch.equal(g1, g2) and torch.equal(l1, l2)
    assert (l1.cpu().numpy() != lv).sum() > 10
    sub = np.arange(3, n, 7)
    g3, o3, l3 = ws.game_state(lv[sub])
    b = ws.step_game(st[sub], inp[:, sub], g3, o3, l3, actions=act[:, sub])
    idx = torch.from_numpy(sub).cuda()
    assert np.array_equal(_u32(b), _u32(a[sub]))
    assert torch.equal(o3, o1[idx]) and torch.equal(l3, l1[idx])
    assert torch.equal(g3.view(len(sub), -1), g1.view(n, -1)[idx])


def test_the_change_takes_two_ticks(exits):
    """an exit crossed in tick t: tick t + 1 is still the old level's, tick t + 2 is the reset plus one tick in the next"""
    rd.set_device(0)
    wad_path, meta_path, lines = exits
    wad = rd.Wad(wad_path, meta_path)
    ws = wad.build_world_set(SET)
    _, xz, yaw, y = lines[0]
    flags = rd.PLAYER_CLIP | rd.PLAYER_FLY
    st = rd.player_states([[xz[0], y + 0.25, xz[1]]], yaw, flags=flags)
    ticks = 60
    inp = np.zeros((ticks, 1), rd.PLAYER_INPUT)
    inp['movement'][:, 0, 1] = -1.0
    inp['look'][:, 0, 0] = 0.003  # (turning: the reset's yaw shows)
    game, offs, levels = ws.game_state([0])
    world0, world1 = wad.build_world(0), wad.build_world(1)
    wg, wo = world0.game_state(1)
    s_set, s_one = st, st
    t_exit = None
    for k in range(ticks):
        s_set = ws.step_game(s_set, inp[k:k + 1], game, offs, levels)
        s_one = world0.step_game(s_one, inp[k:k + 1], wg, wo)
        lvl = int(levels[0])
        if t_exit is None:
            assert lvl == 0 and np.array_equal(_u32(s_set), _u32(s_one))
            if s_set['flags'][0] & rd.PLAYER_EXITED:
                t_exit = k
        elif k == t_exit + 1:  # still in E1M1, stepped as rdoom_world_step_game steps it
            assert lvl == 0 and np.array_equal(_u32(s_set), _u32(s_one))
            assert torch.equal(offs[0, :world0.game_objects], wo[0])
        elif k == t_exit + 2:  # E1M2: Player::reset at its start, then this tick there
            assert lvl == 1
            start = ws.start_states([1], flags=s_one['flags'][0])
            g1, o1 = world1.game_state(1)
            want = world1.step_game(start, inp[k:k + 1], g1, o1)
            assert np.array_equal(_u32(s_set), _u32(want))
            assert s_set['flags'][0] == flags | rd.PLAYER_EXITED
            fresh, fresh_o = world1.game_state(1)
            assert torch.equal(g1, fresh) and (o1 == 0).all()  # (nothing fired in that one tick)
            words = g1.numel()
            assert torch.equal(game[:words], g1) and (game[words:] == 0).all()
            assert (offs == 0).all()
            break
    assert t_exit is not None and t_exit < 30, t_exit
    assert k == t_exit + 2


def _compare_with_world(ws, world, st, inp, act, slot):
    """players stepped in slot `slot` of ws and in world (the same level): states, offsets, game words and slots agree"""
    n = len(st)
    lv = np.full(n, slot)
    game, offs, levels = ws.game_state(lv)
    got = ws.step_game(st, inp, game, offs, levels, actions=act)
    wg, wo = world.game_state(n)
    want = world.step_game(st, inp, wg, wo, actions=act)
    assert np.array_equal(_u32(got), _u32(want))
    no = world.game_objects
    assert torch.equal(offs[:, :no], wo) and (offs[:, no:] == 0).all()
    words = wg.numel() // n
    g = game.view(n, -1)
    assert torch.equal(g[:, :words], wg.view(n, -1)) and (g[:, words:] == 0).all()
    assert (levels.cpu().numpy() == slot).all()
    return got, wo


def test_a_set_of_one_is_the_world(tmp_path):
    """the patched E1M1 (an exit switch, no next level in the set): rdoom_world_step_game, bit for bit"""
    rd.set_device(0)
    wad_path, meta_path = patched_variant(str(tmp_path))
    wad = rd.Wad(wad_path, meta_path)
    ws, world = wad.build_world_set([0]), wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    st, _ = _seed(ref, world.triggers()['triggers'], 512, 51)
    inp, act = _script(len(st), 400, 52, push=0.1)
    got, wo = _compare_with_world(ws, world, st, inp, act, 0)
    assert (got['flags'] & rd.PLAYER_EXITED).any() and (wo[:, :, 1] != 0).any(1).sum() > 20


def test_a_slot_without_a_destination_keeps_its_players(exits):
    """[0, 2]: E1M3 has no E1M4 in the set, so its exit only sets EXITED, as rdoom_world_step_game does"""
    rd.set_device(0)
    wad_path, meta_path, lines = exits
    wad = rd.Wad(wad_path, meta_path)
    ws, world = wad.build_world_set([0, 2]), wad.build_world(2)
    assert ws.levels()['destination'].tolist() == [rd.WORLDSET_NO_DESTINATION] * 2
    _, xz, yaw, y = lines[2]
    n = 128
    rng = np.random.default_rng(61)
    st = rd.player_states(np.repeat([[xz[0], y + 0.25, xz[1]]], n, 0).astype(F), yaw + rng.normal(scale=0.2, size=n).astype(F))
    inp, act = _script(n, 300, 62)
    inp['movement'][:30, :, 0], inp['movement'][:30, :, 1] = 0.0, -1.0
    got, _ = _compare_with_world(ws, world, st, inp, act, 1)
    assert (got['flags'] & rd.PLAYER_EXITED).sum() > n // 2


def test_step_then_render_matches_the_oracle(exits):
    """players left on different levels, rendered in one batch of a level set of the same list, level_of_pose = their slots"""
    from oracle import raster
    rd.set_device(0)
    wad_path, meta_path, lines = exits
    wad = rd.Wad(wad_path, meta_path)
    ws = wad.build_world_set(SET)
    n, w, h = 9, 160, 100
    lv = np.repeat(np.arange(3), 3)
    st = ws.start_states(lv)
    for p in range(0, n, 3):  # one of each level's three walks out through its exit
        _, xz, yaw, y = lines[SET[lv[p]]]
        st[p]['pos'], st[p]['yaw'] = (xz[0], y + F(0.25), xz[1]), yaw
    inp, act = _script(n, 90, 71, push=0.1)
    inp['movement'][:40, ::3, 0], inp['movement'][:40, ::3, 1] = 0.0, -1.0
    game, offs, levels = ws.game_state(lv)
    states = ws.step_game(st, inp, game, offs, levels, actions=act)
    lop = levels.cpu().numpy().astype(np.uint32)
    assert (lop != lv).sum() >= 2 and len(set(lop.tolist())) >= 2
    built = [wad.build_level(i) for i in SET]
    lset = rd.DeviceLevelSet(built)
    n_obj = lset.num_objects()
    assert ws.n_objects >= n_obj
    poses = rd.poses_from_players(states, w, h)
    mvs = rd.object_modelviews_from_players(states, offs)[:, :n_obj]
    lights = np.stack([built[k].lights_at(0.0) for k in lop])
    batch = rd.Batch(lset, w, h, n)
    fb, fb_ids, _ = render_checked(batch, poses, lights, level_of_pose=lop, object_modelviews=mvs)
    oracles = [raster.RasterOracle(b.arrays()) for b in built]
    for k in range(n):
        b = built[lop[k]]
        want = oracles[lop[k]].render(poses[k]['modelview'], poses[k]['projection'], 0.0, lights[k], w, h,
                                      object_modelviews=mvs[k, :int(b.counters()['num_objects'])])
        assert np.array_equal(want, fb[k]) and np.array_equal(want, fb_ids[k]), k


def test_worldset_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('worldset_game_step_kernel', 'worldset_game_reset_kernel'):
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
