"""Solid things on the host, with no GPU (include/rdoom.h "solid things"): the obstacle bits of every synthetic
level against a lookup in the TOML itself, under both metadata files and under one without the key; pack_things; the prototypes.
And the yardstick of the step that is specified in DESIGN section 31 and not shipped yet: the restatement
(tests/solid_restatement.c) pinned to rs_step / rs_game_step where nothing blocks, the contract on the restatement, each case with
its expected numbers written out, and the condition that keeps the contract honest on a scripted walk over E1M1's own obstacles."""
import ctypes
import os
import re

import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
import solid_ref
import step_cases
import world_ref
from util import GOLDEN, META_PATH, ensure_wad

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
INF, NAN = float('inf'), float('nan')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOOM_META = os.path.join(GOLDEN, 'doom.toml')


@pytest.fixture(scope='module')
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


# ---- which things are solid ----
@pytest.mark.parametrize('meta', [META_PATH, DOOM_META], ids=['synth.toml', 'doom.toml'])
def test_the_obstacle_bits_are_the_metadatas(meta):
    w = rd.Wad(ensure_wad(), meta)
    worlds = [w.build_world(level, device=False) for level in range(9)]
    assert any(world.thing_obstacles().any() for world in worlds)  # first: the key is read at all
    types = solid_ref.obstacle_types(meta)
    assert any(types.values()) and not all(types.values())
    L = rd.lib()
    for level, world in enumerate(worlds):
        table = world.map_things()
        want = solid_ref.expected_obstacles(table, meta)
        got = world.thing_obstacles()
        assert got.dtype == bool and np.array_equal(got, want), level
        # the row itself: max(1, ceil(T / 32)) words, nothing at or above T
        p, n = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_uint32(0)
        assert L.rdoom_world_thing_obstacles(world._h, ctypes.byref(p), ctypes.byref(n)) == 0
        assert n.value == max(1, (len(table) + 31) // 32)
        words = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
        assert np.array_equal(rd.unpack_things(words, 32 * n.value), np.concatenate([want, np.zeros(32 * n.value - len(want), bool)]))
        assert np.array_equal(rd.pack_things(want).view(np.uint32), words)
    ws = w.build_world_set([0, 2, 7], device=False)
    for slot, level in enumerate((0, 2, 7)):
        assert np.array_equal(ws.thing_obstacles(slot), worlds[level].thing_obstacles())
    with pytest.raises(rd.RdoomError):
        ws.thing_obstacles(3)
    assert L.rdoom_world_thing_obstacles(None, ctypes.byref(p), ctypes.byref(n)) == BAD
    assert L.rdoom_world_thing_obstacles(worlds[0]._h, None, ctypes.byref(n)) == BAD
    assert L.rdoom_worldset_level_thing_obstacles(ws._h, 0, ctypes.byref(p), None) == BAD


def test_a_metadata_file_without_the_key_has_no_obstacle(tmp_path):
    text = open(META_PATH).read()
    assert len(re.findall(r'^obstacle\s*=.*$', text, flags=re.M)) >= 1
    plain = tmp_path / 'plain.toml'
    plain.write_text(re.sub(r'^obstacle\s*=.*$', '', text, flags=re.M))
    w = rd.Wad(ensure_wad(), str(plain))
    for level in range(9):
        world = w.build_world(level, device=False)
        assert len(world.map_things()) and not world.thing_obstacles().any()
        assert world.map_things().tobytes() == rd.Wad(ensure_wad(), META_PATH).build_world(level, device=False).map_things().tobytes()


def test_pack_things_is_the_inverse_of_unpack_things():
    rng = np.random.default_rng(3)
    for n in (0, 1, 31, 32, 33, 64, 65):
        bits = rng.random(n) < 0.5
        row = rd.pack_things(bits)
        assert row.dtype == np.int32 and row.shape == (max(1, (n + 31) // 32),)
        assert np.array_equal(rd.unpack_things(row, n), bits)
        wide = rd.pack_things(bits, 5)
        assert wide.shape == (5,) and np.array_equal(rd.unpack_things(wide, 160), np.concatenate([bits, np.zeros(160 - n, bool)]))
    rows = rd.pack_things([np.ones(33, bool), np.zeros(2, bool), np.array([False, True])])
    assert rows.shape == (3, 2) and rows.view(np.uint32).tolist() == [[0xFFFFFFFF, 1], [0, 0], [2, 0]]
    with pytest.raises(ValueError):
        rd.pack_things(np.ones(33, bool), 1)


# ---- the restatement is rs_step / rs_game_step where nothing blocks ----
def _no_triggers():
    return np.zeros(0, rd.TRIGGER), np.zeros(0, rd.MOVE_EFFECT)


@pytest.mark.parametrize('index', step_cases.LEVELS)
def test_with_no_blocking_thing_the_restatement_is_rs_step(wad, index):
    st, inp = step_cases.shared(wad.build_level(index), index)
    ref = world_ref.RefWorld(wad, index)
    want = ref.step(st, inp)
    assert step_cases.differing(want, st) > 0.5
    trig, effs = _no_triggers()
    far = solid_ref.make_things([(1e4, 1e4), (-1e4, 3.0)], radius=0.3)  # out of every sweep's reach
    near = wad.build_world(index, device=False).map_things()           # in reach, and not solid / hidden / outside the window
    for things, kw, solid in ((np.zeros(0, rd.THING), {}, None), (far, {}, None), (near, {}, np.zeros(2, np.uint32)),
                              (near, dict(hidden=np.full((len(st), 2), 0xFFFFFFFF, np.uint32)), None),
                              (near, dict(below=0.0, above=0.0), None)):
        if kw.get('below') == 0.0:  # dy == 0 is inside a window of 0, 0: lift the things out of it
            things = things.copy()
            things['base'] += 50.0
        g = solid_ref.SolidGame(ref, trig, effs, len(st), max(1, ref.n_objects), things, solid)
        got = g.step(st, inp, **kw)
        assert step_cases.differing(got, want) == 0.0 and (g.bumped == -1).all()


def test_with_no_blocking_thing_the_restatement_is_rs_game_step(tmp_path):
    wad, ref, trig, effs, n_obj, st, inp, act = step_cases.game_setup(str(tmp_path), 48, seed=7)
    plain = game_ref.RefGame(ref, trig, effs, len(st), n_obj)
    want = plain.step(st, inp, act)
    assert (plain.offsets != 0).any()  # doors moved: the effect and trigger code ran
    g = solid_ref.SolidGame(ref, trig, effs, len(st), n_obj, wad.build_world(0, device=False).map_things(), np.zeros(2, np.uint32))
    got = g.step(st, inp, act)
    assert step_cases.differing(got, want) == 0.0 and (g.bumped == -1).all()
    for a, b in ((g.offsets, plain.offsets), (g.order, plain.order), (g.counts, plain.counts), (g.act, plain.act), (g.aflags, plain.aflags)):
        assert a.tobytes() == b.tobytes()


def test_in_a_set_the_things_are_those_of_the_players_slot(tmp_path):
    """solid_ref.SolidWorldSet: with nothing solid it is worldset_ref.RefWorldSet bit for bit, through a level change; with a thing
    in front of every level's start, a player who comes through an exit meets the next level's thing, and only after the change"""
    import worldset_ref
    exits = worldset_ref.exit_variant(str(tmp_path))
    wad_path, meta_path, lines = exits
    slots = [0, 1, 2]
    host = rd.Wad(wad_path, meta_path).build_world_set(slots, device=False)
    info = host.levels()
    tables = []
    for slot in range(3):
        yaw = float(info['start_yaw'][slot])
        ahead = np.asarray(info['start_pos'][slot], np.float64)[[0, 2]] + 0.9 * np.array([-np.sin(yaw), -np.cos(yaw)])
        block = solid_ref.make_things([ahead], radius=0.3, base=float(info['start_pos'][slot][1]) - 0.5)
        tables.append(np.concatenate([host.map_things(slot), block]))
    n, ticks = 12, 70
    lv = np.arange(n) % 3
    st = host.start_states(lv)
    walkers = (np.arange(n) // 3 % 2 == 0) & (lv < 2)  # slot 2 has no destination in the set
    for p in np.nonzero(walkers)[0]:
        _, xz, yaw, y = lines[slots[lv[p]]]
        st[p]['pos'], st[p]['yaw'] = (xz[0], y + F(0.25), xz[1]), yaw
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0
    plain = worldset_ref.RefWorldSet(wad_path, meta_path, slots, lv)
    want = plain.step(st, inp)
    none = solid_ref.SolidWorldSet(wad_path, meta_path, slots, lv, tables, np.zeros((3, 2), np.uint32))
    got = none.step(st, inp)
    assert got.tobytes() == want.tobytes() and none.levels.tolist() == plain.levels.tolist() and (none.bumped == -1).all()
    assert none.offsets().tobytes() == plain.offsets().tobytes() and (plain.levels != lv)[walkers].all() and walkers.sum() == 4
    ref = solid_ref.SolidWorldSet(wad_path, meta_path, slots, lv, tables)
    s, changed_at, bumped_at = st, np.full(n, -1), np.full(n, -1)
    for k in range(ticks):
        s = ref.step(s, inp[k:k + 1])
        changed_at[(ref.levels != lv) & (changed_at < 0)] = k
        bumped_at[(ref.bumped >= 0) & (bumped_at < 0)] = k
    last = np.array([len(t) - 1 for t in tables])
    assert (ref.levels[walkers] == lv[walkers] + 1).all() and (ref.bumped[walkers] == last[ref.levels[walkers]]).all()
    assert (bumped_at[walkers] > changed_at[walkers]).all() and (changed_at[walkers] > 0).all()
    # the others walk from their start into the thing in front of it, and stay in their level
    assert (ref.bumped[~walkers] == last[lv[~walkers]]).all() and (ref.levels[~walkers] == lv[~walkers]).all()


# ---- the contract, a sweep at a time: numbers that binary32 holds exactly ----
THING = solid_ref.make_things([(0.0, 0.0)], radius=0.25)  # with a body of 0.25: R = 0.5


def contact(pos, D, things=THING, **kw):
    return solid_ref.thing_contact(things, pos, D, body=0.25, **kw)


def test_the_contact_of_one_sweep():
    # head on from x = 1 along -x: a = 1, b = -1, cc = 0.75, disc = 0.25, t = (1 - 0.5) / 1
    which, t, n = contact((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0))
    assert (which, t, n.tolist()) == (0, 0.5, [1.0, 0.0, 0.0])
    # oblique: from (1, 0.3) along -x: cc = 1.09 - 0.25, disc = 1 - 0.84 = 0.16 -> t = 0.6, the contact point (0.4, 0.3) / 0.5
    which, t, n = contact((1.0, 0.0, 0.3), (-1.0, 0.0, 0.0))
    want_t = (F(1.0) - np.sqrt(F(1.0) - (F(F(1.0) + F(0.3) * F(0.3)) - F(0.25)))) / F(1.0)
    assert which == 0 and t == want_t and abs(float(t) - 0.6) < 1e-6
    m = np.sqrt(F(F(1.0) + F(-1.0) * t) ** 2 + F(0.3) ** 2, dtype=F)
    assert n.tolist() == [F(F(1.0) - t) / m, 0.0, F(0.3) / m] and abs(float(n[0]) - 0.8) < 1e-6 and abs(float(n[2]) - 0.6) < 1e-6
    # a miss: |z| above R
    assert contact((1.0, 0.0, 0.6), (-1.0, 0.0, 0.0))[0] == -1
    # walking away, or along the tangent, is free (b >= 0): from touching, from overlapping and from afar
    for pos in ((0.5, 0.0, 0.0), (0.2, 0.0, 0.0), (3.0, 0.0, 0.0)):
        for D in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.0, -2.0)):
            which, t, n = contact(pos, D)
            assert which == -1 and t == INF
    # overlapping and moving in: stopped where it stands, pushed out along the line of centres
    which, t, n = contact((0.3, 0.0, 0.4), (-1.0, 0.0, 0.0))
    assert (which, t) == (0, 0.0) and n.tolist() == [F(0.3) / F(0.5), 0.0, F(0.4) / F(0.5)]
    # at distance 0 there is no direction to be blocked in
    assert contact((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0))[0] == -1
    # no horizontal displacement: no thing contact
    assert contact((0.3, 5.0, 0.0), (0.0, -9.0, 0.0))[0] == -1
    # the vertical part of D does not enter: the same t
    assert contact((1.0, 0.0, 0.0), (-1.0, 7.0, 0.0))[1] == 0.5


def test_ties_bits_and_the_window():
    two = solid_ref.make_things([(0.0, 0.0), (0.0, 0.0)], radius=0.25)
    pos, D = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)
    assert contact(pos, D, two)[0] == 0                                                # equal things: the lower index
    assert contact(pos, D, two, solid=np.array([2], np.uint32))[0] == 1                # thing 0 not solid
    assert contact(pos, D, two, hidden=np.array([1], np.uint32))[0] == 1               # thing 0 hidden
    assert contact(pos, D, two, solid=np.array([0], np.uint32))[0] == -1
    assert contact(pos, D, two, hidden=np.array([3], np.uint32))[0] == -1
    assert contact(pos, D, two, solid=None)[0] == 0                                    # NULL: every thing is solid
    nearer = solid_ref.make_things([(0.0, 0.0), (0.25, 0.0)], radius=0.25)
    which, t, _ = contact(pos, D, nearer)
    assert (which, t) == (1, 0.25)                                                     # a strictly earlier thing wins
    # the world: a wall at the same time wins, an earlier one too, a later one loses
    wall = (0.0, 1.0, 0.0)
    for time, want in ((0.5, -1), (0.25, -1), (0.75, 0)):
        which, t, n = contact(pos, D, world=(time,) + wall)
        assert which == want and t == min(time, 0.5) and n.tolist() == ([1.0, 0.0, 0.0] if want == 0 else list(wall))
    # the window, on a lift: the thing stands on object 2, which the player's offsets carry 2 up
    lifted = solid_ref.make_things([(0.0, 0.0)], radius=0.25, base=1.0, object_id=2)
    off = np.zeros((3, 3), F)
    at = lambda y: (1.0, y, 0.0)
    assert contact(at(1.5), D, lifted, below=0.25, above=1.0)[0] == 0                  # dy = 0.5
    assert contact(at(1.5), D, lifted, below=0.25, above=1.0, offsets=off)[0] == 0
    off[2, 1] = 2.0                                                                    # the thing is at 3 now
    assert contact(at(1.5), D, lifted, below=0.25, above=1.0, offsets=off)[0] == -1    # dy = -1.5: the thing is above
    assert contact(at(3.5), D, lifted, below=0.25, above=1.0, offsets=off)[0] == 0     # dy = 0.5: it rode the lift
    assert contact(at(2.75), D, lifted, below=0.25, above=1.0, offsets=off)[0] == 0    # dy = -0.25: the bounds are inside
    assert contact(at(4.0), D, lifted, below=0.25, above=1.0, offsets=off)[0] == 0     # dy = 1
    assert contact(at(4.5), D, lifted, below=0.25, above=1.0, offsets=off)[0] == -1    # dy = 1.5: the thing is below
    assert contact(at(1e6), D, lifted, offsets=off)[0] == 0                            # both +inf: infinitely tall
    assert contact(at(3.5), D, lifted, below=0.25, above=1.0, offsets=off[:2])[0] == -1  # an object beyond the row: off() = 0
    # a NaN anywhere in the position: every comparison is false
    for pos in ((NAN, 0.0, 0.0), (1.0, NAN, 0.0), (1.0, 0.0, NAN)):
        assert contact(pos, D)[0] == -1
    assert contact((1.0, 0.0, 0.0), (NAN, 0.0, 0.0))[0] == -1


# ---- the contract, through the tick: room A of the analytic level (floor 0, 2.56 square) ----
C = F(step_cases.ROOM_CENTRE)
REST = 0.2 + 0.21 - 17.0 / 200.0  # step_cases.rest_height of the default config
BODY = F(0.19)


def room(wad, things, starts, yaws, ticks, flags=rd.PLAYER_CLIP, solid=None, move=(0.0, -1.0), **kw):
    """players at the (x, z) `starts` of room A at rest height walking with `move`: (states per tick, bumped at the end)"""
    ref = world_ref.RefWorld(wad, step_cases.MODEL_LEVEL)
    starts = np.asarray(starts, F).reshape(-1, 2)
    st = rd.player_states(np.stack([starts[:, 0], np.full(len(starts), REST, F), starts[:, 1]], 1), np.asarray(yaws, F), flags=flags)
    st['last_height_diff'] = 17.0 / 200.0
    inp = np.zeros((ticks, len(st)), rd.PLAYER_INPUT)
    inp['movement'][..., 0], inp['movement'][..., 1] = move
    trig, effs = _no_triggers()
    g = solid_ref.SolidGame(ref, trig, effs, len(st), 2, things, solid)
    out, s = [], st
    for k in range(ticks):
        s = g.step(s, inp[k:k + 1], **kw)
        out.append(s)
    return out, g.bumped.copy()


def test_a_head_on_walk_ends_at_the_stand_off(wad):
    thing = solid_ref.make_things([(3.0, 3.0), (C, C)], radius=0.2)  # thing 1 is in the way, thing 0 far off
    start = (C + F(0.9), C)
    run, bumped = room(wad, thing, [start], solid_ref.facing(start, (C, C))[None], 60)
    free, _ = room(wad, thing, [start], solid_ref.facing(start, (C, C))[None], 60, solid=np.array([1], np.uint32))
    R = float(BODY + F(0.2))
    d = [solid_ref.distances(s, thing)[0, 1] for s in run]
    # it arrives (the free walk is past the thing by then) and from then on stands 0.001 outside R.  The rounding: the centre is at
    # |x| < 4, so the position's own rounding is at most half an ulp of 4, 2.4e-7, in each of the sweep's sum and the difference
    # the next contact reads; t carries a relative 1e-6 of a displacement of 0.1, and 0.001 / |D| less still: 1e-6 covers them
    assert solid_ref.distances(free[-1], thing)[0, 1] > 1.0 and free[-1]['pos'][0, 0] < C - 0.5
    assert bumped.tolist() == [1] and d[5] > R + 0.1
    assert all(abs(x - (R + 0.001)) <= 1e-6 for x in d[20:]), d[20:]
    # the velocity towards it is what the last tick's force added and no more: a tick's force is at most move_force, 60 / 60 = 1 a
    # tick, where the free walk runs at over 3; and with the input let go it is none at all
    towards = [-float(s['vel'][0, 0]) for s in run]
    assert max(towards[20:]) <= 1.0 and -free[10]['vel'][0, 0] > 3.0
    assert not (run[-1]['flags'][0] & rd.PLAYER_DIVERGED)
    ref = world_ref.RefWorld(wad, step_cases.MODEL_LEVEL)
    trig, effs = _no_triggers()
    g = solid_ref.SolidGame(ref, trig, effs, 1, 2, thing)
    rest = g.step(run[-1], np.zeros((1, 1), rd.PLAYER_INPUT))
    assert -float(rest['vel'][0, 0]) <= 0.0 and abs(solid_ref.distances(rest, thing)[0, 1] - (R + 0.001)) <= 1e-6


def test_an_oblique_walk_slides_past_and_walking_away_is_free(wad):
    thing = solid_ref.make_things([(C, C)], radius=0.2)
    R = float(BODY + F(0.2))
    start = (C + F(0.9), C + F(0.25))  # walking along -x, 0.25 off the line of centres: inside R = 0.39
    yaw = solid_ref.facing((1.0, 0.0), (0.0, 0.0))[None]
    run, bumped = room(wad, thing, [start], yaw, 45)
    d = np.array([solid_ref.distances(s, thing)[0, 0] for s in run])
    assert bumped.tolist() == [0] and d.min() >= R - 1e-6  # (0.001 along D is less than 0.001 from the thing: never inside)
    assert run[-1]['pos'][0, 0] < C - R and run[-1]['pos'][0, 2] > C + 0.25  # past it, and pushed aside on the way
    # away from it, from touching distance: bit for bit the walk with no thing at all
    start = (C + F(0.4), C)
    away = solid_ref.facing((C, C), start)[None]
    with_thing, bumped = room(wad, thing, [start], away, 20)
    without, _ = room(wad, np.zeros(0, rd.THING), [start], away, 20)
    assert bumped.tolist() == [-1] and with_thing[-1].tobytes() == without[-1].tobytes()
    assert with_thing[-1]['pos'][0, 0] > start[0] + 0.3


def test_an_overlapping_body_is_stopped_walking_in_and_free_walking_out(wad):
    thing = solid_ref.make_things([(C, C)], radius=0.2)
    R = float(BODY + F(0.2))
    start = (C + F(0.2), C)
    run, bumped = room(wad, thing, [start], solid_ref.facing(start, (C, C))[None], 30)
    d = np.array([0.2] + [solid_ref.distances(s, thing)[0, 0] for s in run])
    # t = 0: every contact moves it 0.001 back along D (adjusted_time = -0.001 / |D|) and takes the velocity towards the thing
    # away, so it never gets nearer, and it is still inside R after 30 ticks where the free walk has crossed the room
    assert bumped.tolist() == [0] and (np.diff(d) >= -1e-6).all() and d[-1] < R and d[-1] - d[0] <= 30 * 100 * 0.001
    assert not (run[-1]['flags'][0] & rd.PLAYER_DIVERGED)
    out, bumped = room(wad, thing, [start], solid_ref.facing((C, C), start)[None], 20)
    free, _ = room(wad, np.zeros(0, rd.THING), [start], solid_ref.facing((C, C), start)[None], 20)
    assert bumped.tolist() == [-1] and out[-1].tobytes() == free[-1].tobytes() and solid_ref.distances(out[-1], thing)[0, 0] > R
    # at distance 0: not blocked, in any direction
    run, bumped = room(wad, thing, [(C, C)], F([0.3]), 20)
    free, _ = room(wad, np.zeros(0, rd.THING), [(C, C)], F([0.3]), 20)
    assert bumped.tolist() == [-1] and run[-1].tobytes() == free[-1].tobytes()


def test_rows_window_and_flags_through_the_tick(wad):
    thing = solid_ref.make_things([(C, C), (C, C)], radius=0.2)
    start = (C + F(0.9), C)
    yaw = solid_ref.facing(start, (C, C))[None]
    free, _ = room(wad, np.zeros(0, rd.THING), [start], yaw, 40)
    one = lambda **kw: room(wad, kw.pop('things', thing), [start], yaw, 40, **kw)
    assert one()[1].tolist() == [0]                                                     # two equal things: the lower index
    assert one(solid=np.array([2], np.uint32))[1].tolist() == [1]
    assert one(hidden=np.array([[1]], np.uint32))[1].tolist() == [1]
    for kw in (dict(solid=np.array([0], np.uint32)), dict(hidden=np.array([[3]], np.uint32))):  # through, as if nothing stood there
        run, bumped = one(**kw)
        assert bumped.tolist() == [-1] and run[-1].tobytes() == free[-1].tobytes()
    run, bumped = one(flags=0)                                                          # CLIP off: noclip() does not see things
    off, _ = room(wad, np.zeros(0, rd.THING), [start], yaw, 40, flags=0)
    assert bumped.tolist() == [-1] and run[-1].tobytes() == off[-1].tobytes() and run[-1]['pos'][0, 0] < C
    # a flyer with CLIP is blocked: the same loop.  It sinks as it goes, and the 0.001 is taken along D, so in xz it stands off by
    # 0.001 |D.xz| / |D|: less than 0.001, never less than nothing
    run, bumped = one(flags=rd.PLAYER_CLIP | rd.PLAYER_FLY)
    d = solid_ref.distances(run[-1], thing)[0, 0] - float(BODY + F(0.2))
    assert bumped.tolist() == [0] and -1e-6 <= d <= 0.001 + 1e-6
    # the window: the player's centre is at REST = 0.325 above the floor the things stand on
    assert one(below=0.0, above=0.5)[1].tolist() == [0]
    high = solid_ref.make_things([(C, C)], radius=0.2, base=1.0)   # dy = -0.675: above the player
    low = solid_ref.make_things([(C, C)], radius=0.2, base=-1.0)   # dy = 1.325: below it
    for things, kw, want in ((high, dict(below=0.5, above=0.5), -1), (high, dict(below=0.7, above=0.0), 0),
                             (low, dict(below=0.5, above=0.5), -1), (low, dict(below=0.0, above=1.4), 0)):
        assert one(things=things, **kw)[1].tolist() == [want], kw
    # a NaN player is blocked by nothing and moved by nothing
    ref = world_ref.RefWorld(wad, step_cases.MODEL_LEVEL)
    trig, effs = _no_triggers()
    st = rd.player_states(F([[NAN, REST, C]]), yaw)
    g = solid_ref.SolidGame(ref, trig, effs, 1, 2, thing)
    inp = np.zeros((3, 1), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0
    plain = game_ref.RefGame(ref, trig, effs, 1, 2)
    assert g.step(st, inp).tobytes() == plain.step(st, inp).tobytes() and g.bumped.tolist() == [-1]


def test_a_thing_on_a_lift_rides_the_offset(wad):
    thing = solid_ref.make_things([(C, C)], radius=0.2, object_id=1)
    start = (C + F(0.9), C)
    yaw = solid_ref.facing(start, (C, C))[None]
    ref = world_ref.RefWorld(wad, step_cases.MODEL_LEVEL)
    trig, effs = _no_triggers()
    st = rd.player_states(F([[start[0], REST, start[1]]]), yaw)
    st['last_height_diff'] = 17.0 / 200.0
    inp = np.zeros((40, 1), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0
    for lift, want in ((0.0, 0), (2.0, -1), (-2.0, -1)):  # the thing at 0, 2 above and 2 below a window of 0.5 either way
        g = solid_ref.SolidGame(ref, trig, effs, 1, 2, thing)
        g.offsets[0, 1, 1] = lift
        g.step(st, inp, below=0.5, above=0.5)
        assert g.bumped.tolist() == [want], lift


# ---- the condition that keeps the contract honest, on a scripted walk over E1M1's own obstacles ----
def test_the_scripted_walk_keeps_its_distance():
    case = solid_ref.e1m1_case(ensure_wad(), META_PATH)
    things, ob, st = case['things'], case['obstacles'], case['states']
    assert ob.sum() >= 4 and len(st) >= 48
    R = (BODY + things['radius']).astype(np.float64)
    began = ((solid_ref.distances(st, things) < R[None]) & ob[None]).any(1)
    g = solid_ref.e1m1_game(case)
    s, ever, worst = st, np.zeros(len(st), bool), np.inf
    for k in range(solid_ref.E1M1_TICKS):
        s = g.step(s, case['inputs'][k:k + 1])
        margin = (solid_ref.distances(s, things) - (R[None] - 0.001))[:, ob][~began]
        worst = min(worst, float(margin.min()))
        ever |= g.bumped >= 0
    print('worst distance less (R - 0.001): %.6g; bumped %.2f of %d players' % (worst, ever.mean(), len(st)))
    assert worst >= 0.0
    assert not (s['flags'] & rd.PLAYER_DIVERGED).any()
    assert ever.mean() >= 1.0 / 3.0
    # one call of K ticks is K calls of one tick, bumped included
    whole = solid_ref.e1m1_game(case)
    assert whole.step(st, case['inputs']).tobytes() == s.tobytes() and np.array_equal(whole.bumped, g.bumped)


# ---- the interface ----
def prototype(name):
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, header, flags=re.M)
    assert m, name
    return m.group(1).strip(), [' '.join(a.split()) for a in m.group(2).split(',')]


def test_the_prototypes_argument_by_argument():
    assert prototype('rdoom_world_thing_obstacles') == \
        ('rdoom_status', ['const rdoom_world *world', 'const uint32_t **out_words', 'uint32_t *out_n_words'])
    assert prototype('rdoom_worldset_level_thing_obstacles') == \
        ('rdoom_status', ['const rdoom_worldset *set', 'uint32_t slot', 'const uint32_t **out_words', 'uint32_t *out_n_words'])
    assert rd.THING.itemsize == 32  # the record stays as it is
    L = rd.lib()
    for name in ('rdoom_world_thing_obstacles', 'rdoom_worldset_level_thing_obstacles'):
        assert name in rd.API_SYMBOLS and getattr(L, name).restype is ctypes.c_int32
