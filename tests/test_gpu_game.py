"""Doors, lifts and exits on the GPU (world.hip game_step_kernel): bit for bit against the test-side restatement
(tests/game_restatement.c) on E1M1 and on the patched variant with an exit switch, an only_once line and a Gun door; launch
splitting and batch independence; invariants that do not rely on the restatement; step -> render against the oracle; resources."""
import importlib.util
import os

import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
import world_ref
from step_cases import floor_y as _floor_y, front as _front, game_script as _script, seed_players as _seed  # (moved there)
from test_game_host import ORDER_A, ORDER_B, ordering_run, ordering_variant, patched_variant
from util import META_PATH, ROOT, ensure_wad, render_checked

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def patched(tmp_path_factory):
    return patched_variant(str(tmp_path_factory.mktemp('patched_level_gpu')))


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def _setup(wad_path, meta_path, n, seed):
    rd.set_device(0)
    wad = rd.Wad(wad_path, meta_path)
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    st, pick = _seed(ref, t['triggers'], n, seed)
    return wad, world, ref, t, st, pick


def _bit_exact(wad_path, meta_path, seed):
    wad, world, ref, t, st, _ = _setup(wad_path, meta_path, 1024, seed)
    n = len(st)
    inp, act = _script(n, 600, seed + 1)
    game, offs = world.game_state(n)
    got = world.step_game(st, inp, game, offs, actions=act)
    rg = game_ref.RefGame(ref, t['triggers'], t['effects'], n, world.game_objects)
    want = rg.step(st, inp, act)
    assert np.array_equal(_u32(got), _u32(want)), int((_u32(got) != _u32(want)).any(1).sum())
    got_off = offs.cpu().numpy()
    assert np.array_equal(got_off.view(np.uint32), rg.offsets.view(np.uint32))
    moved = (rg.offsets[:, :, 1] != 0).any(1).sum()
    return got, rg, moved


def test_game_step_matches_the_restatement_on_e1m1():
    got, rg, moved = _bit_exact(ensure_wad(), META_PATH, 11)
    assert moved > 20  # doors opened and lifts lowered in many games
    assert (rg.counts == rg.counts.max()).all()  # (E1M1 has no only_once trigger)


def test_game_step_matches_the_restatement_on_the_patched_variant(patched):
    got, rg, moved = _bit_exact(patched[0], patched[1], 12)
    assert moved > 20
    assert (got['flags'] & rd.PLAYER_EXITED).any()
    assert (rg.counts < len(rg.trig)).any()  # the only_once line was removed in some games


def test_launch_splitting_and_batch_independence(patched):
    wad, world, ref, t, st, _ = _setup(patched[0], patched[1], 256, 21)
    n = len(st)
    inp, act = _script(n, 600, 22)
    g1, o1 = world.game_state(n)
    a = world.step_game(st, inp, g1, o1, actions=act)
    g2, o2 = world.game_state(n)
    s2 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti, ta = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda(), torch.from_numpy(act.reshape(-1).copy()).cuda()
    for k in range(600):
        world.step_game(s2, ti[k * n * 20:(k + 1) * n * 20], g2, o2, actions=ta[k * n:(k + 1) * n], n_ticks=1)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(a), _u32(s2.cpu().numpy().view(rd.PLAYER_STATE)))
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    sub = np.arange(3, n, 7)
    g3, o3 = world.game_state(len(sub))
    b = world.step_game(st[sub], inp[:, sub], g3, o3, actions=act[:, sub])
    assert np.array_equal(_u32(b), _u32(a[sub]))
    assert torch.equal(o3, o1[torch.from_numpy(sub).cuda()])


def _door(world, t, ref):
    """index of a manual door line that opens high enough to walk through and has a floor in front, and its ceiling effect"""
    trig, effs = t['triggers'], t['effects']
    for i in np.nonzero(trig['special_type'] == 1)[0]:
        e = effs[trig['effect_start'][i]:trig['effect_end'][i]]
        if len(e) != 1 or e[0]['first_height_offset'] < 0.9:
            continue
        p, yaw = _front(trig[i:i + 1], 0.45)
        y = _floor_y(ref, p)
        if not np.isfinite(y[0]):
            continue
        st = rd.player_states([[p[0, 0], y[0] + 0.25, p[0, 1]]], yaw)
        # open, the doorway lets the player's sphere through: no step or ledge within a unit beyond the line
        offs = np.zeros((1, world.game_objects, 3), F)
        offs[0, e[0]['object_id'], 1] = e[0]['first_height_offset']
        fwd = np.array([[-np.sin(yaw[0]), 0.0, -np.cos(yaw[0])]], F)
        hit = ref.sweep(np.array([[*st['pos'][0], 0.19]], F), fwd * F(1.5), offs)
        if hit[0, 0] > 1.0:
            return int(i), e[0], st
    raise AssertionError('no door')


def _side(trig, pos):
    """signed distance of each position from the trigger's line (> 0: the front)"""
    d = trig['displace']
    rel = np.stack([pos[:, 0] - trig['origin'][0], pos[:, 2] - trig['origin'][1]], 1)
    return rel[:, 0] * -d[1] + rel[:, 1] * d[0]


def test_door_invariants():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ref = wad.build_world(0), None
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    i, eff, st = _door(world, t, ref)
    st = np.repeat(st, 2)
    ticks = 600
    inp = np.zeros((ticks, 2), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0  # walk into the door, both players
    act = np.zeros((ticks, 2), np.uint8)
    act[0, 1] = rd.ACTION_PUSH  # player 1 pushes once, on the first tick
    game, offs = world.game_state(2)
    sides = []
    heights = []
    s = st
    for k in range(ticks):
        s = world.step_game(s, inp[k:k + 1], game, offs, actions=act[k:k + 1])
        sides.append(_side(t['triggers'][i], s['pos']))
        heights.append(offs[:, eff['object_id'], 1].cpu().numpy().copy())
    sides, heights = np.array(sides), np.array(heights)
    assert (sides[:, 0] > 0).all(), 'walked through a closed door'
    assert (heights[:, 0] == 0).all()
    assert (sides[:, 1] < 0).any(), 'did not pass the opened door'
    h = heights[:, 1].astype(np.float64)
    step = float(F(eff['speed']) * F(1.0 / 60.0))
    rising = np.nonzero(np.diff(h) > 0)[0]
    assert len(rising) > 0 and np.allclose(np.diff(h)[rising[:-1]], step, rtol=1e-3)
    top = float(eff['first_height_offset'])
    held = np.nonzero(h == np.float64(F(top)))[0]
    assert len(held) > 0
    assert abs(len(held) - float(eff["wait"]) * 60) <= 1, len(held)
    assert h[-1] == 0.0  # closed again, and the effect has ended
    g = game.cpu().numpy().view(np.uint32).reshape(2, -1)
    ow_start = 4 + 2 * ((len(t['triggers']) + 31) // 32)
    assert (g[:, ow_start:ow_start + (world.game_objects + 31) // 32] == 0).all()


def test_lift_exit_only_once_and_masked_reset(patched):
    rd.set_device(0)
    wad = rd.Wad(patched[0], patched[1])
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    index = {int(np.nonzero(trig['special_type'] == s)[0][0]): s for s in (11, 22)}
    exit_i = [i for i, s in index.items() if s == 11][0]
    once_i = [i for i, s in index.items() if s == 22][0]
    lift_i = int(np.nonzero((trig['special_type'] == 88) & (trig['effect_end'] > trig['effect_start']))[0][0])
    pts, yaws = _front(trig[[exit_i, once_i, lift_i]], np.array([0.35, -0.35, -0.35], F)[:, None])
    y = _floor_y(ref, pts)
    assert np.isfinite(y).all(), y
    st = rd.player_states(np.stack([pts[:, 0], y + F(0.25), pts[:, 1]], 1), yaws)
    n = 3
    ticks = 240
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    inp['movement'][:60, 1:, 1] = -1.0  # the walkers cross their lines forwards, then back, then forwards again
    inp['movement'][60:120, 1:, 1] = 1.0
    inp['movement'][120:180, 1:, 1] = -1.0
    act = np.zeros((ticks, n), np.uint8)
    act[5, 0] = rd.ACTION_PUSH  # the switch
    game, offs = world.game_state(n)
    lift_obj = int(effs[trig['effect_start'][lift_i]]['object_id'])
    out = world.step_game(st, inp[:60], game, offs, actions=act[:60])
    assert offs[2, lift_obj, 1].item() < 0  # the lift lowers once its line is crossed
    out = world.step_game(out, inp[60:], game, offs, actions=act[60:])
    assert out['flags'][0] & rd.PLAYER_EXITED and not (out['flags'][1:] & rd.PLAYER_EXITED).any()
    g = game.cpu().numpy().view(np.uint32).reshape(n, -1)
    nt = len(trig)
    assert g[1, 0] == nt - 1 and g[0, 0] == nt and g[2, 0] == nt  # only player 1 removed its only_once line ...
    live = g[1, 4:4 + (nt + 31) // 32]
    assert not (live[once_i >> 5] >> (once_i & 31)) & 1  # ... and it is that line
    # a masked reset touches only the masked players
    before_g, before_o = game.clone(), offs.clone()
    mask = np.array([0, 0, 1], bool)
    world.reset_game(game, offs, mask=mask)
    assert torch.equal(game.view(n, -1)[:2], before_g.view(n, -1)[:2]) and torch.equal(offs[:2], before_o[:2])
    fresh, fresh_o = world.game_state(1)
    assert torch.equal(game.view(n, -1)[2], fresh.view(-1)) and (offs[2] == 0).all()


def test_a_player_on_the_lift_follows_its_floor(patched):
    rd.set_device(0)
    wad = rd.Wad(patched[0], patched[1])
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    lift_i = int(np.nonzero((trig['special_type'] == 88) & (trig['effect_end'] > trig['effect_start']))[0][0])
    eff = effs[trig['effect_start'][lift_i]]
    assert eff['first_height_offset'] < -0.5
    # at the lift's height, just in front of its line, facing away from the lift; then 40 ticks backwards onto it, across the line
    behind, yaw = _front(trig[[lift_i]], np.array([[-0.35]], F))
    y = _floor_y(ref, behind)
    normal = np.array([-trig['displace'][lift_i, 1], trig['displace'][lift_i, 0]], F)
    at = behind + normal * F(0.45)
    st = rd.player_states([[at[0, 0], y[0] + 0.25, at[0, 1]]], yaw)
    ticks = 300
    inp = np.zeros((ticks, 1), rd.PLAYER_INPUT)
    inp['movement'][:40, 0, 1] = 1.0
    game, offs = world.game_state(1)
    ys, lift = [], []
    for k in range(ticks):
        st = world.step_game(st, inp[k:k + 1], game, offs)
        ys.append(float(st['pos'][0, 1]))
        lift.append(float(offs[0, eff['object_id'], 1]))
    ys, lift = np.array(ys), np.array(lift)
    assert lift.min() == np.float32(eff['first_height_offset'])  # lowered all the way ...
    down = np.nonzero(lift == lift.min())[0]
    rest = ys[down[-1]] - lift[down[-1]]
    riding = np.arange(50, down[-1] + 30)  # ... and back up part of the way, the player standing on it
    assert lift[riding[-1]] > lift.min() + 0.3
    # (the height above the floor moves by the spring's transient, a few hundredths, when the lift starts and stops)
    assert np.abs(ys[riding] - lift[riding] - rest).max() < 0.04, np.abs(ys[riding] - lift[riding] - rest).max()
    assert ys[down[-1]] < ys[0] - 0.5


def test_two_triggers_on_one_object_follow_the_players_list(tmp_path):
    rd.set_device(0)
    wad_path, meta_path = ordering_variant(str(tmp_path))
    wad = rd.Wad(wad_path, meta_path)
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    game, offs = world.game_state(2)
    got = ordering_run(lambda st, inp, act: world.step_game(st, inp, game, offs, actions=act), trig, ref)
    rg = game_ref.RefGame(ref, trig, effs, 2, world.game_objects)
    want = ordering_run(lambda st, inp, act: rg.step(st, inp, act), trig, ref)
    assert np.array_equal(_u32(got), _u32(want))
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), rg.offsets.view(np.uint32))
    # the active effect on the door: the layout of include/rdoom.h (rdoom_world_game_bytes)
    nt, no = len(trig), world.game_objects
    lw, ow = (nt + 31) // 32, (no + 31) // 32
    effect = (4 + 2 * lw + 2 * ow + nt + 3) // 4 * 4
    g = game.cpu().numpy().view(np.uint32).reshape(2, -1)
    ea, eb = effs[trig['effect_start'][ORDER_A]], effs[trig['effect_start'][ORDER_B]]
    obj = int(ea['object_id'])
    assert g[0, 0] == nt and g[1, 0] == nt - 1
    records = g[:, effect + 4 * obj:effect + 4 * obj + 4].view(np.float32)
    assert records[:, 3].tolist() == [eb['speed'], ea['speed']]  # linedef order in game 0, the swapped list in game 1
    assert records.view(np.uint32).tolist() == rg.act[:, obj].view(np.uint32).tolist()


def test_players_at_different_doors_do_not_affect_each_other():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    st, pick = _seed(ref, t['triggers'], 64, 41)
    n = len(st)
    inp, act = _script(n, 300, 42, push=0.1)
    game, offs = world.game_state(n)
    full = world.step_game(st, inp, game, offs, actions=act)
    for k in (0, n // 2, n - 1):
        g1, o1 = world.game_state(1)
        one = world.step_game(st[k:k + 1], inp[:, k:k + 1], g1, o1, actions=act[:, k:k + 1])
        assert np.array_equal(_u32(one), _u32(full[k:k + 1])) and torch.equal(o1[0], offs[k])


def test_step_then_render_matches_the_oracle():
    from oracle import raster
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    world = wad.build_world(0)
    ref = world_ref.RefWorld(wad, 0)
    t = world.triggers()
    i, eff, st = _door(world, t, ref)
    n, w, h = 4, 160, 100
    st = np.repeat(st, n)
    ticks = 50
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    act = np.zeros((ticks, n), np.uint8)
    act[0, 1:] = rd.ACTION_PUSH
    game, offs = world.game_state(n)
    states = world.step_game(st, inp, game, offs, actions=act)
    o = offs.cpu().numpy()
    assert o[1:, eff['object_id'], 1].min() > 0 and (o[0] == 0).all()
    poses = rd.poses_from_players(states, w, h)
    mvs = rd.object_modelviews_from_players(states, o)
    level = rd.DeviceLevel(built)
    batch = rd.Batch(level, w, h, n)
    lights = built.lights_at(0.0)
    fb, fb_ids, _ = render_checked(batch, poses, lights, object_modelviews=mvs)
    ro = raster.RasterOracle(built.arrays())
    moved = 0
    for k in range(n):
        want = ro.render(poses[k]['modelview'], poses[k]['projection'], 0.0, lights, w, h, object_modelviews=mvs[k])
        assert np.array_equal(want, fb[k]) and np.array_equal(want, fb_ids[k]), k
        still = ro.render(poses[k]['modelview'], poses[k]['projection'], 0.0, lights, w, h)
        moved += not np.array_equal(still, want)
    assert moved >= 1, 'no frame shows the door moved'


def test_game_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    for name in ('game_step_kernel', 'game_reset_kernel'):
        r = res[name]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)
