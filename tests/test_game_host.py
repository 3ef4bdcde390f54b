"""Doors, lifts and exits on the host: the trigger list and move effects of rdoom_world_triggers against the test-side list built
from oracle.wad_oracle (tests/game_ref.py) on every synthetic level and on a variant with the specials they lack; the game's
object count; rdoom_object_modelviews_from_player against rdoom_pose_from_player and the restated concat; bad arguments."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
from util import META_PATH, ensure_big_wad, ensure_wad

_syn = __import__('importlib').import_module('rust-doom_amd.synthetic')


def _levels():
    out = [(ensure_wad, i) for i in range(9)] + [(ensure_big_wad, 0)]
    return out + [(_syn.ensure_rich_wad, 0)]


# the specials the synthetic levels lack, patched into E1M1's LINEDEFS: the one-sided unknown special 999 -> an exit switch, a
# two-sided walk-over lift line (88, tag 19) -> the only_once raise (22, same tag), a manual door line (1) -> a Gun door
EXIT_LINE, ONCE_LINE, GUN_LINE = 5, 10, 12
PATCHES = {EXIT_LINE: (11, 0), ONCE_LINE: (22, 19), GUN_LINE: (game_ref.GUN_SPECIAL, 0)}
GUN_META = '''
[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 4.0, speed = 8, ceiling = { first = { to = "LowestCeiling", off = -4 }, second = { to = "Floor" } } }
''' % game_ref.GUN_SPECIAL


def patched_variant(directory):
    """(wad path, metadata path) of the patched E1M1 variant, written into `directory`"""
    from oracle import wad_oracle as wo
    src = ensure_wad()
    with open(src, 'rb') as f:
        data = f.read()
    marker = wo.Archive(src, META_PATH).levels[0]
    wad = os.path.join(directory, 'patched.wad')
    with open(wad, 'wb') as f:
        f.write(game_ref.patch_linedefs(data, marker, PATCHES))
    meta = os.path.join(directory, 'patched.toml')
    shutil.copy(META_PATH, meta)
    with open(meta, 'a') as f:
        f.write(GUN_META)
    return wad, meta


# The list-order quirk.  Door object 2 of E1M1 has corner lines, triggers 120 and 122, that one push can cross together.
# Trigger 122 becomes a faster Push special (31) and, with the specials after it cleared, the last trigger.  So when the
# only_once line (trigger 2) is swap_removed, trigger 122 moves ahead of trigger 120 in that player's list.  A push across the
# corner then leaves trigger 120's effect in that game, and trigger 122's in a game whose list is still in linedef order.
ORDER_A, ORDER_B, ORDER_SPECIAL = 120, 122, 31
ORDER_META = GUN_META + '''
[[linedef]]
special_type = %d
trigger = "Push"
move = { wait = 1.0, speed = 16, ceiling = { first = { to = "LowestCeiling", off = -4 }, second = { to = "Floor" } } }
''' % ORDER_SPECIAL


def ordering_variant(directory):
    """(wad path, metadata path) of the patched variant with the list-order case above"""
    from oracle import wad_oracle as wo
    src = ensure_wad()
    with open(src, 'rb') as f:
        data = f.read()
    archive = wo.Archive(src, META_PATH)
    specials = [i for i, ld in enumerate(wo.Level(archive, 0).linedefs) if ld[3] != 0]
    patches = dict(PATCHES)
    patches[specials[ORDER_B]] = (ORDER_SPECIAL, 0)
    patches.update({i: (0, 0) for i in specials[ORDER_B + 1:]})
    wad = os.path.join(directory, 'ordering.wad')
    with open(wad, 'wb') as f:
        f.write(game_ref.patch_linedefs(data, archive.levels[0], patches))
    meta = os.path.join(directory, 'ordering.toml')
    shutil.copy(META_PATH, meta)
    with open(meta, 'a') as f:
        f.write(ORDER_META)
    return wad, meta


def ordering_run(step, trig, ref):
    """Two games on the ordering variant.  Player 1 first walks across the only_once line; player 0 stands.  Then both stand
    outside door object 2's corner and push once, across triggers ORDER_A and ORDER_B.  step(states, inputs, actions) -> states
    advances both games.  Returns the final states."""
    F = np.float32
    once = int(np.nonzero(trig['special_type'] == 22)[0][0])
    a0 = trig['origin'][ORDER_A]
    a1 = a0 + trig['displace'][ORDER_A] * trig['length'][ORDER_A]
    b0 = trig['origin'][ORDER_B]
    corner = a0 if min(np.abs(a0 - b0).max(), np.abs(a0 - b0 - trig['displace'][ORDER_B] * trig['length'][ORDER_B]).max()) < 1e-4 else a1
    at = (corner + np.array([0.314, -0.339], F)).astype(F)  # outside the door, 0.34 and 0.31 from the two lines
    ang = 2.3015  # a 0.5 push from there enters the door through line A and leaves it through line B
    yaw = F(np.arctan2(-np.cos(ang), -np.sin(ang)))
    normal = np.array([-trig['displace'][once, 1], trig['displace'][once, 0]], F)
    walk_from = trig['origin'][once] + trig['displace'][once] * (trig['length'][once] * F(0.5)) - normal * F(0.35)
    xz = np.stack([at, walk_from])
    y = floor_below(ref, xz)
    assert np.isfinite(y).all(), y
    st = rd.player_states(np.stack([xz[:, 0], y + F(0.25), xz[:, 1]], 1), np.array([yaw, np.arctan2(-normal[0], -normal[1])], F))
    inp = np.zeros((60, 2), rd.PLAYER_INPUT)
    inp['movement'][:, 1, 1] = -1.0
    st = step(st, inp, np.zeros((60, 2), np.uint8))
    st[1] = rd.player_states(np.array([[at[0], y[0] + 0.25, at[1]]], F), yaw)[0]
    st[0] = st[1]
    push = np.full((1, 2), rd.ACTION_PUSH, np.uint8)
    return step(st, np.zeros((1, 2), rd.PLAYER_INPUT), push)


def floor_below(ref, xz):
    """the floor under each (x, z) of a world_ref.RefWorld: the first upward-facing contact of a sweep down from a few heights"""
    F = np.float32
    best = np.full(len(xz), np.nan, F)
    for y0 in (-2.0, -1.0, 0.0, 1.0, 2.0, 3.0):
        sph = np.zeros((len(xz), 4), F)
        sph[:, 0], sph[:, 1], sph[:, 2], sph[:, 3] = xz[:, 0], y0, xz[:, 1], 0.2
        vel = np.zeros((len(xz), 3), F)
        vel[:, 1] = -3.0
        hit = ref.sweep(sph, vel)
        ok = np.isfinite(hit[:, 0]) & (hit[:, 2] > 0.5) & np.isnan(best)
        best[ok] = (F(y0) - F(3.0) * hit[:, 0])[ok]
    return best


def test_the_restatement_keeps_the_list_order_quirk(tmp_path):
    import world_ref
    wad_path, meta_path = ordering_variant(str(tmp_path))
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
    assert trig['special_type'][-1] == ORDER_SPECIAL and len(trig) == ORDER_B + 1
    ea = effs[trig['effect_start'][ORDER_A]:trig['effect_end'][ORDER_A]]
    eb = effs[trig['effect_start'][ORDER_B]:trig['effect_end'][ORDER_B]]
    assert len(ea) == len(eb) == 1 and ea[0]['object_id'] == eb[0]['object_id'] and ea[0]['speed'] != eb[0]['speed']
    wad = rd.Wad(wad_path, meta_path)
    ref = world_ref.RefWorld(wad, 0)
    rg = game_ref.RefGame(ref, trig, effs, 2, n_obj)
    ordering_run(lambda st, inp, act: rg.step(st, inp, act), trig, ref)
    obj = ea[0]['object_id']
    assert rg.counts.tolist() == [len(trig), len(trig) - 1]
    assert rg.order[1, 2] == ORDER_B  # the last trigger took the only_once line's place ...
    assert rg.act[0, obj, 3] == eb[0]['speed'] and rg.act[1, obj, 3] == ea[0]['speed']  # ... so the other effect won there


@pytest.fixture(scope='module')
def patched(tmp_path_factory):
    return patched_variant(str(tmp_path_factory.mktemp('patched_level')))


def _check_level(wad_path, meta_path, index):
    wad = rd.Wad(wad_path, meta_path)
    world = wad.build_world(index, device=False)
    got = world.triggers()
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, index)
    assert got['triggers'].tobytes() == trig.tobytes()
    assert got['effects'].tobytes() == effs.tobytes()
    assert got['n_objects'] == n_obj == world.game_objects
    assert world.game_objects >= world.n_objects
    assert world.game_objects >= wad.build_level(index).counters()['num_objects']
    return got


@pytest.mark.parametrize('ensure,index', _levels())
def test_triggers_match_the_test_side_list(ensure, index):
    got = _check_level(ensure(), META_PATH, index)
    if ensure is ensure_wad and index != 1:  # the generator's manual doors, lifts and unknown special are all there
        kinds = set(got['triggers']['special_type'].tolist())
        assert {1, 88, 999} <= kinds, kinds
        unimpl = got['triggers'][got['triggers']['special_type'] == 999]
        assert (unimpl['trigger_type'] == rd.TRIGGER_ANY).all() and (unimpl['flags'] == rd.TRIGGER_UNIMPLEMENTED).all()
        assert (unimpl['effect_end'] == unimpl['effect_start']).all()


def test_triggers_of_the_patched_variant(patched):
    got = _check_level(patched[0], patched[1], 0)
    t = got['triggers']
    by_special = {int(s): t[t['special_type'] == s] for s in (11, 22, game_ref.GUN_SPECIAL)}
    assert len(by_special[11]) == 1 and by_special[11]['flags'][0] == rd.TRIGGER_EXIT and by_special[11]['trigger_type'][0] == rd.TRIGGER_SWITCH
    assert len(by_special[22]) == 1 and by_special[22]['flags'][0] == rd.TRIGGER_ONLY_ONCE
    gun = by_special[game_ref.GUN_SPECIAL]
    assert len(gun) == 1 and gun['trigger_type'][0] == rd.TRIGGER_GUN and gun['effect_end'][0] == gun['effect_start'][0] + 1


def test_game_object_count_covers_the_world_and_the_level():
    wad = rd.Wad(ensure_wad(), META_PATH)
    for index in range(9):
        world = wad.build_world(index, device=False)
        assert world.game_objects >= world.n_objects
        assert world.game_objects >= wad.build_level(index).counters()['num_objects']
        assert world.game_bytes() % 16 == 0 and world.game_bytes() >= 16 * (world.game_objects + 1)


def _states(n, seed):
    rng = np.random.default_rng(seed)
    st = rd.player_states(rng.uniform(-20, 20, (n, 3)).astype(np.float32), rng.uniform(-7, 7, n).astype(np.float32),
                          rng.uniform(-1.5, 1.5, n).astype(np.float32))
    return st


def test_object_modelviews_at_zero_offset_are_the_pose():
    n_obj = 7
    for s in _states(64, 3):
        mv = rd.object_modelviews_from_players(s.reshape(1), np.zeros((1, n_obj, 3), np.float32))[0]
        pose = rd.pose_from_player(s['pos'], float(s['yaw']), float(s['pitch']), 64, 48, 0.0)
        want = np.ascontiguousarray(pose['modelview'], np.float32).reshape(16)
        for o in range(n_obj):
            assert mv[o].view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_object_modelviews_at_offsets_are_the_concat():
    rng = np.random.default_rng(5)
    st = _states(64, 4)
    offs = np.zeros((64, 5, 3), np.float32)
    offs[:, 1:, 1] = rng.uniform(-1.3, 1.3, (64, 4)).astype(np.float32)
    offs[:, 4, :] = rng.uniform(-2, 2, (64, 3)).astype(np.float32)
    mv = rd.object_modelviews_from_players(st, offs)
    for i, s in enumerate(st):
        for o in range(1, 5):
            want = game_ref.object_modelview(s['pos'], s['yaw'], s['pitch'], offs[i, o])
            assert mv[i, o].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (i, o)
    # a door raised by h draws like the static world seen from h lower
    s = st[0]
    lifted = rd.object_modelviews_from_players(st[:1], np.array([[[0, 0, 0], [0, 0.5, 0]]], np.float32))[0, 1]
    low = s.copy()
    low['pos'][1] -= np.float32(0.5)
    base = rd.object_modelviews_from_players(low.reshape(1), np.zeros((1, 1, 3), np.float32))[0, 0]
    np.testing.assert_allclose(lifted, base, atol=2e-5)


def test_bad_arguments():
    lib = rd.lib()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0, device=False)
    v = ctypes.c_void_p
    assert lib.rdoom_world_triggers(None, v(1)) == -1  # RDOOM_BAD_ARG
    assert lib.rdoom_world_triggers(world._h, None) == -1
    assert lib.rdoom_world_game_bytes(world._h, None) == -1
    assert lib.rdoom_world_game_bytes(None, v(0)) == -1
    pos = np.zeros(3, np.float32)
    out = np.zeros(16 * 4, np.float32)
    assert lib.rdoom_object_modelviews_from_player(None, ctypes.c_float(0), ctypes.c_float(0), v(out.ctypes.data), 1, v(out.ctypes.data)) == -1
    assert lib.rdoom_object_modelviews_from_player(v(pos.ctypes.data), ctypes.c_float(0), ctypes.c_float(0), None, 2,
                                                   v(out.ctypes.data)) == -1
    assert lib.rdoom_object_modelviews_from_player(v(pos.ctypes.data), ctypes.c_float(0), ctypes.c_float(0), v(out.ctypes.data), 2,
                                                   None) == -1
    # a fake, aligned device pointer: every check below fails before anything reaches the device
    fake = v(1 << 20)
    n_obj = world.game_objects
    f = ctypes.c_float(1.0 / 60.0)
    assert lib.rdoom_world_game_reset(None, fake, fake, n_obj, 4, None, None) == -1
    assert lib.rdoom_world_game_reset(world._h, None, fake, n_obj, 4, None, None) == -1
    assert lib.rdoom_world_game_reset(world._h, fake, None, n_obj, 4, None, None) == -1
    assert lib.rdoom_world_game_reset(world._h, v((1 << 20) + 4), fake, n_obj, 4, None, None) == -1  # misaligned
    assert lib.rdoom_world_game_reset(world._h, fake, fake, n_obj - 1, 4, None, None) == -1            # n_objects too small
    assert lib.rdoom_world_game_reset(world._h, fake, fake, n_obj, 4, None, None) == -1                # host-only world
    args = lambda game, offs, n_objects: (world._h, fake, fake, None, game, offs, n_objects, 4, 10, None, f, None)
    assert lib.rdoom_world_step_game(*args(fake, fake, n_obj - 1)) == -1
    assert lib.rdoom_world_step_game(*args(None, fake, n_obj)) == -1
    assert lib.rdoom_world_step_game(*args(fake, None, n_obj)) == -1
    assert lib.rdoom_world_step_game(*args(fake, fake, n_obj)) == -1
    assert lib.rdoom_world_step_game(world._h, None, fake, None, fake, fake, n_obj, 4, 10, None, f, None) == -1
    assert lib.rdoom_world_step_game(world._h, fake, fake, None, fake, fake, n_obj, 4, 10, None, ctypes.c_float(-1.0), None) == -1
    # an action above ACTION_SHOOT is refused before any device work
    with pytest.raises(rd.RdoomError) as e:
        world.step_game(rd.player_states(np.zeros((2, 3), np.float32), 0.0), np.zeros((1, 2), rd.PLAYER_INPUT), None, None,
                        actions=np.array([[1, 3]], np.uint8))
    assert e.value.status == -1
