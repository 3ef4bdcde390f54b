"""The volley family of tests/game_cases.py on the GPU: the branch outcomes of the game tick (world.hip GameLevel::tick, advance,
start_effects, SetGame) that the other game tests' inputs never take -- several triggers fired by one shot, removals that reorder a
player's list, effects restarted, a whole cycle inside one tick, an exit fired in a volley and during a level change -- through
World.step_game and WorldSet.step_game, bit for bit against the restatement: the states, the offsets, the slots, and the whole
game memory decoded by the layout of include/rdoom.h (rdoom_world_game_bytes).  Each case as one launch, as one launch per tick,
and with wave neighbours that stay on the tick's fast path."""
import numpy as np
import pytest

import game_cases as gc
import game_ref
import rust_doom_amd as rd
import step_cases as sc
import world_ref
import worldset_ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in gc.cases()}
AROUND = (0, 1, 63)
u32 = sc.u32


def _same(got, want, what):
    bad = np.nonzero((u32(got) != u32(want)).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[bad[:2]], want[bad[:2]])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def layout(n_triggers, n_objects):
    """the word offsets of one game (include/rdoom.h rdoom_world_game_bytes)"""
    lw, ow = (n_triggers + 31) // 32, (n_objects + 31) // 32
    live = 4
    fired = live + lw
    active = fired + lw
    second = active + ow
    order = second + ow
    effect = (order + n_triggers + 3) // 4 * 4
    return dict(live=live, fired=fired, active=active, second=second, order=order, effect=effect, words=effect + 4 * n_objects,
                n_triggers=n_triggers, n_objects=n_objects)


def _bits(words, n):
    return ((words[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


def check_game(row, lay, rg, p, what):
    """one player's game memory `row` (uint32 words) against row p of the game_ref.RefGame `rg`"""
    t, o = lay['n_triggers'], lay['n_objects']
    count = int(row[0])
    assert count == int(rg.counts[p]), (what, count, int(rg.counts[p]))
    order = row[lay['order']:lay['order'] + t]
    assert order[:count].tolist() == rg.order[p, :count].tolist(), what
    live = _bits(row[lay['live']:lay['fired']], t)
    assert set(np.nonzero(live)[0].tolist()) == set(order[:count].tolist()) and live.sum() == count, what
    assert row[lay['live']:lay['fired']].tolist() == _pack(live).tolist(), what  # (no bit past the last trigger)
    assert (row[lay['fired']:lay['active']] == 0).all(), (what, 'a fired bit is left')
    active, second = _bits(row[lay['active']:lay['second']], o), _bits(row[lay['second']:lay['order']], o)
    assert active.tolist() == ((rg.aflags[p] & 1) != 0).tolist(), what
    assert second.tolist() == ((rg.aflags[p] & 2) != 0).tolist(), what
    assert row[lay['active']:lay['second']].tolist() == _pack(active).tolist(), what
    assert row[lay['second']:lay['order']].tolist() == _pack(second).tolist(), what
    records = row[lay['effect']:lay['effect'] + 4 * o].reshape(o, 4)
    assert records[active].tolist() == rg.act[p].view(np.uint32)[active].tolist(), what
    assert (row[lay['words']:] == 0).all(), (what, 'a word past the level\'s own')


def _pack(bits):
    out = np.zeros((len(bits) + 31) // 32, np.uint32)
    for i in np.nonzero(bits)[0]:
        out[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return out


@pytest.fixture(scope='module')
def variants(tmp_path_factory):
    """{variant: (World, RefWorld, triggers, effects, n_objects)}"""
    rd.set_device(0)
    tmp = str(tmp_path_factory.mktemp('volley_levels'))
    out = {}
    for name in gc.VARIANTS:
        wad_path, meta_path = gc.volley_variant(tmp, name)
        wad = rd.Wad(wad_path, meta_path)
        out[name] = (wad.build_world(0), world_ref.RefWorld(wad, 0)) + game_ref.triggers(wad_path, meta_path, 0)
    return out


def _with_neighbours(c, around):
    """the case's players with `around` fast-path players after them"""
    st, inp, act = gc.neighbours(around, len(c.inputs))
    return np.concatenate([c.states, st]), np.concatenate([c.inputs, inp], 1), np.concatenate([c.actions, act], 1)


@pytest.fixture(scope='module')
def want(variants):
    """{(case, around): (RefGame after the case's ticks, its states)}: computed once, left unchanged"""
    out = {}
    for name, c in CASES.items():
        _, ref, trig, effs, n_obj = variants[c.variant]
        for around in AROUND:
            st, inp, act = _with_neighbours(c, around)
            rg = game_ref.RefGame(ref, trig, effs, len(st), n_obj)
            out[name, around] = rg, rg.step(st, inp, act, threads=1)
    return out


def _check_world(world, game, offs, got, rg, want_states, what):
    n = len(want_states)
    _same(got, want_states, what)
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), rg.offsets.view(np.uint32)), what
    assert world.game_objects == rg.n_objects
    lay = layout(len(rg.trig), rg.n_objects)
    assert lay['words'] * 4 == world.game_bytes()
    rows = game.cpu().numpy().view(np.uint32).reshape(n, -1)
    for p in range(n):
        check_game(rows[p], lay, rg, p, (what, p))


@pytest.mark.parametrize('around', AROUND)
@pytest.mark.parametrize('name', list(CASES))
def test_one_launch_matches_the_restatement(variants, want, name, around):
    """the case's players, alone and with 1 and 63 players after them who fire one plain trigger at a time: a wave mixes the
    tick's two paths"""
    c = CASES[name]
    world = variants[c.variant][0]
    st, inp, act = _with_neighbours(c, around)
    game, offs = world.game_state(len(st))
    got = world.step_game(st, inp, game, offs, actions=_dev(act))
    _check_world(world, game, offs, got, *want[name, around], name)


@pytest.mark.parametrize('name', list(CASES))
def test_one_launch_per_tick_matches_the_restatement(variants, want, name):
    """... and no fired bit is left after any launch; the list's length never grows"""
    c = CASES[name]
    world = variants[c.variant][0]
    n, ticks = len(c.states), len(c.inputs)
    s_dev, i_dev, a_dev = _dev(c.states), _dev(c.inputs), _dev(c.actions)
    game, offs = world.game_state(n)
    lay = layout(len(variants[c.variant][2]), world.game_objects)
    step = n * rd.PLAYER_INPUT.itemsize
    counts = np.full(n, lay['n_triggers'])
    for t in range(ticks):
        world.step_game(s_dev, i_dev[t * step:(t + 1) * step], game, offs, actions=a_dev[t * n:(t + 1) * n], n_ticks=1)
        rows = game.cpu().numpy().view(np.uint32).reshape(n, -1)
        assert (rows[:, lay['fired']:lay['active']] == 0).all(), (name, t)
        assert (rows[:, 0] <= counts).all(), (name, t)
        counts = rows[:, 0].copy()
    torch.cuda.synchronize()
    _check_world(world, game, offs, s_dev.cpu().numpy().view(rd.PLAYER_STATE), *want[name, 0], name)


def test_the_volleys_do_what_they_are_named_for(variants, want):
    """by the product's own memory: the lists shrink by the only_once lines, the exit flag is set, the whole cycle leaves no
    effect behind, and the speed-0 effect stays active where it started"""
    c = CASES['once_volley_short_once']
    world = variants[c.variant][0]
    game, offs = world.game_state(len(c.states))
    got = world.step_game(c.states, c.inputs, game, offs, actions=_dev(c.actions))
    rows = game.cpu().numpy().view(np.uint32).reshape(len(c.states), -1)
    assert rows[:, 0].tolist() == [107 - 4, 107 - 3]
    assert (got['flags'] & rd.PLAYER_EXITED).astype(bool).tolist() == [True, False]
    effs = variants[c.variant][3]
    stuck = int(effs[variants[c.variant][2]['effect_start'][85]]['object_id'])
    assert effs[variants[c.variant][2]['effect_start'][85]]['speed'] == 0
    lay = layout(107, world.game_objects)
    assert _bits(rows[0, lay['active']:lay['second']], world.game_objects)[stuck] and offs[0, stuck, 1].item() == 0.0
    c = CASES['cycle']
    world = variants[c.variant][0]
    game, offs = world.game_state(len(c.states))
    world.step_game(c.states, c.inputs, game, offs, actions=_dev(c.actions))
    rows = game.cpu().numpy().view(np.uint32).reshape(len(c.states), -1)
    lay = layout(128, world.game_objects)
    assert (rows[:, lay['active']:lay['order']] == 0).all() and (offs == 0).all()


# ---- the set --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def volley_set(tmp_path_factory):
    rd.set_device(0)
    exits = gc.volley_variant(str(tmp_path_factory.mktemp('volley_set')), 'full', exits=True)
    return exits, rd.Wad(exits[0], exits[1]).build_world_set(gc.SET)


def _set_with_neighbours(c, around):
    st, inp, act = _with_neighbours(c, around)
    return st, np.concatenate([c.levels, np.zeros(around, np.int64)]), inp, act


def _check_set(ws, game, offs, levels, got, ref, want_states, what):
    n = len(want_states)
    _same(got, want_states, what)
    assert levels.cpu().numpy().tolist() == ref.levels.tolist(), what
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), ref.offsets().view(np.uint32)), what
    table = ws.levels()
    rows = game.cpu().numpy().view(np.uint32).reshape(n, -1)
    assert rows.shape[1] * 4 == ws.game_bytes()
    for p in range(n):
        slot = int(ref.levels[p])
        if slot >= len(gc.SET):
            assert (rows[p] == 0).all(), (what, p)  # in no slot: never reset, never stepped
            continue
        rg = ref.games[slot]
        assert (int(table['n_triggers'][slot]), int(table['n_objects'][slot])) == (len(rg.trig), rg.n_objects)
        check_game(rows[p], layout(len(rg.trig), rg.n_objects), rg, p, (what, p))
        assert int(rows[p, 1]) == int(ref.stage[p]), (what, p, 'stage')


@pytest.mark.parametrize('around', AROUND)
@pytest.mark.parametrize('index', range(len(gc.SET_CASE_NAMES)))
def test_the_set_in_one_launch_matches_the_restatement(volley_set, index, around):
    exits, ws = volley_set
    c = gc.set_cases(exits)[index]
    st, lv, inp, act = _set_with_neighbours(c, around)
    game, offs, levels = ws.game_state(lv)
    got = ws.step_game(st, inp, game, offs, levels, actions=_dev(act))
    ref = worldset_ref.RefWorldSet(exits[0], exits[1], gc.SET, lv)
    want_states = ref.step(st, inp, act, threads=1)
    _check_set(ws, game, offs, levels, got, ref, want_states, c.name)
    if around == 0:  # what the case is named for, by the product's own memory
        assert levels.cpu().numpy().tolist() == [1, 1, gc.OUT_OF_RANGE, 2, 0]
        assert (got['flags'] & rd.PLAYER_EXITED).astype(bool).tolist() == [True, True, False, True, False]
        _same(got[2:3], c.states[2:3], 'the player in no slot')


@pytest.mark.parametrize('index', range(len(gc.SET_CASE_NAMES)))
def test_the_set_in_one_launch_per_tick_matches_the_restatement(volley_set, index):
    """after every tick: the states, the slots, the stage word and the whole game memory"""
    exits, ws = volley_set
    c = gc.set_cases(exits)[index]
    n, ticks = len(c.states), len(c.inputs)
    s_dev, i_dev, a_dev = _dev(c.states), _dev(c.inputs), _dev(c.actions)
    game, offs, levels = ws.game_state(c.levels)
    ref = worldset_ref.RefWorldSet(exits[0], exits[1], gc.SET, c.levels)
    want_states = c.states
    step = n * rd.PLAYER_INPUT.itemsize
    stages = set()
    for t in range(ticks):
        ws.step_game(s_dev, i_dev[t * step:(t + 1) * step], game, offs, levels, actions=a_dev[t * n:(t + 1) * n], n_ticks=1)
        want_states = ref.step(want_states, c.inputs[t:t + 1], c.actions[t:t + 1], threads=1)
        _check_set(ws, game, offs, levels, s_dev.cpu().numpy().view(rd.PLAYER_STATE), ref, want_states, (c.name, t))
        stages |= set(ref.stage.tolist())
    assert stages == {0, 1, 2}
