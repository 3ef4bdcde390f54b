"""The rare family of tests/step_cases.py on the GPU: the branch outcomes of step_players (world.hip) that the other step tests'
inputs never or hardly take -- clip()'s 100 sweeps run out (RDOOM_PLAYER_DIVERGED), the pitch held at its lower limit, no slowdown
at all -- through World.step, World.step_game and WorldSet.step_game (a set of one, and the three-level set), bit for bit against
the restatement as uint32 rows, flags included.  One launch of K ticks is K launches of one; DIVERGED, once set, stays; and the
lanes that share a wave with a diverging one come out as they do without it."""
import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
import step_cases as sc
import world_ref
import worldset_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in sc.rare()}
u32 = sc.u32


def _same(got, want, what):
    bad = np.nonzero((u32(got) != u32(want)).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[bad[:2]], want[bad[:2]])


def _diverged(s):
    return (s['flags'] & rd.PLAYER_DIVERGED) != 0


@pytest.fixture(scope='module')
def wad():
    rd.set_device(0)
    return rd.Wad(ensure_wad(), META_PATH)


@pytest.fixture(scope='module')
def worlds(wad):
    """{level: (World, RefWorld, (triggers, effects, n_objects))} of the levels the family stands on"""
    return {i: (wad.build_world(i), world_ref.RefWorld(wad, i), game_ref.triggers(ensure_wad(), META_PATH, i))
            for i in sorted({c.level for c in CASES.values()})}


@pytest.fixture(scope='module')
def want(worlds):
    """{case: the restatement's states after the case's ticks}: computed once, left unchanged"""
    return {name: worlds[c.level][1].step(c.states, c.inputs, config=c.config, dt=c.dt) for name, c in CASES.items()}


@pytest.fixture(scope='module')
def exits(tmp_path_factory):
    return worldset_ref.exit_variant(str(tmp_path_factory.mktemp('rare_exit_levels')))


def _ref_game(worlds, c, st=None, inp=None):
    _, ref, (trig, effs, n_obj) = worlds[c.level]
    st = c.states if st is None else st
    return game_ref.RefGame(ref, trig, effs, len(st), n_obj).step(st, c.inputs if inp is None else inp, config=c.config, dt=c.dt)


@pytest.mark.parametrize('name', list(CASES))
def test_step_matches_the_restatement(worlds, want, name):
    c = CASES[name]
    world = worlds[c.level][0]
    got = world.step(c.states, c.inputs, config=c.config, dt=c.dt)
    _same(got, want[name], name)
    if name == 'diverged':
        assert _diverged(got).all() and np.isfinite(got['pos']).all() and np.isfinite(got['vel']).all()


@pytest.mark.parametrize('name', list(CASES))
def test_step_game_matches_the_restatement(worlds, name):
    c = CASES[name]
    world = worlds[c.level][0]
    game, offs = world.game_state(len(c.states))
    _same(world.step_game(c.states, c.inputs, game, offs, config=c.config, dt=c.dt), _ref_game(worlds, c), name)


@pytest.mark.parametrize('name', list(CASES))
def test_a_set_of_one_matches_the_restatement(wad, worlds, name):
    c = CASES[name]
    ws = wad.build_world_set([c.level])
    game, offs, levels = ws.game_state(np.zeros(len(c.states), np.int64))
    _same(ws.step_game(c.states, c.inputs, game, offs, levels, config=c.config, dt=c.dt), _ref_game(worlds, c), name)
    assert (levels.cpu().numpy() == 0).all()


@pytest.mark.parametrize('name', list(CASES))
def test_the_three_level_set_matches_the_restatement(exits, name):
    """the exit variant of the test IWAD (tests/test_gpu_worldset.py): the same geometry, a walk-over exit in each level"""
    c = CASES[name]
    ws = rd.Wad(exits[0], exits[1]).build_world_set(sc.SET)
    lv = np.full(len(c.states), sc.SET.index(c.level))
    game, offs, levels = ws.game_state(lv)
    got = ws.step_game(c.states, c.inputs, game, offs, levels, config=c.config, dt=c.dt)
    ref = worldset_ref.RefWorldSet(exits[0], exits[1], sc.SET, lv)
    _same(got, ref.step(c.states, c.inputs, config=c.config, dt=c.dt, threads=1), name)
    assert levels.cpu().numpy().tolist() == ref.levels.tolist()
    if name == 'diverged':
        assert _diverged(got).all()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize('name', list(CASES))
def test_one_launch_of_k_ticks_is_k_launches_of_one(worlds, want, name):
    c = CASES[name]
    world = worlds[c.level][0]
    n, ticks = len(c.states), len(c.inputs)
    s_dev, i_dev = _dev(c.states), _dev(c.inputs)
    g_dev, i2 = _dev(c.states), _dev(c.inputs)
    game, offs = world.game_state(n)
    step = n * rd.PLAYER_INPUT.itemsize
    for t in range(ticks):
        world.step(s_dev, i_dev[t * step:(t + 1) * step], n_ticks=1, config=c.config, dt=c.dt)
        world.step_game(g_dev, i2[t * step:(t + 1) * step], game, offs, n_ticks=1, config=c.config, dt=c.dt)
    torch.cuda.synchronize()
    _same(s_dev.cpu().numpy().view(rd.PLAYER_STATE), want[name], name)
    _same(g_dev.cpu().numpy().view(rd.PLAYER_STATE), _ref_game(worlds, c), name + ' (game)')


def test_the_flag_is_set_in_the_tick_that_runs_out_and_not_before(worlds):
    """after one tick the players of DIVERGING have it and those of DIVERGING_LATE do not; after three all have"""
    c = CASES['diverged']
    world, ref, _ = worlds[0]
    first = len(sc.DIVERGING)
    one = world.step(c.states, c.inputs[:1], dt=c.dt)
    _same(one, ref.step(c.states, c.inputs[:1], dt=c.dt), 'one tick')
    assert _diverged(one)[:first].all() and not _diverged(one)[first:].any()
    assert _diverged(world.step(one, c.inputs[1:3], dt=c.dt)).all()


def _ordinary(wad, n, ticks, seed=7):
    """n ordinary players of E1M1 and their script (tests/step_cases.py): walkers, flyers and players with clipping off"""
    return sc.players(wad.build_level(0), max(n, 1), seed=seed)[:n], sc.script(max(n, 1), ticks, seed=seed)[:, :n]


def test_diverged_stays_set(wad, worlds, want):
    """the library never clears it: a further launch of ordinary ticks keeps it, and inputs that carry it come out with it, the
    rest of their rows as without"""
    c = CASES['diverged']
    world, ref, _ = worlds[0]
    _, script = _ordinary(wad, len(c.states), 40)
    on = world.step(want['diverged'], script, dt=c.dt)
    _same(on, ref.step(want['diverged'], script, dt=c.dt), 'ordinary ticks after diverging')
    assert _diverged(on).all()
    st, inp = _ordinary(wad, 65, 40)
    marked = st.copy()
    marked['flags'] |= rd.PLAYER_DIVERGED
    plain, kept = world.step(st, inp, dt=c.dt), world.step(marked, inp, dt=c.dt)
    assert not _diverged(plain).any() and _diverged(kept).all()
    kept['flags'] &= ~np.uint32(rd.PLAYER_DIVERGED)
    _same(kept, plain, 'rows but for the flag')
    game, offs = world.game_state(65)
    assert _diverged(world.step_game(marked, inp, game, offs, dt=c.dt)).all()


@pytest.mark.parametrize('around', [0, 62, 63, 64])
def test_the_wave_neighbours_of_a_diverging_lane(wad, worlds, around):
    """one lane runs clip()'s 100 sweeps while the others of its wave leave the loop after one or two: the ordinary players' rows
    are what they are when stepped without it, and the diverging player's what it is alone.  With 63 around it the batch fills one
    wave; with 64 the diverging lane or an ordinary one is alone in a second block."""
    c = CASES['diverged']
    world, ref, _ = worlds[0]
    ticks = len(c.inputs)
    st, inp = _ordinary(wad, around, ticks)
    lone, lone_inp = c.states[:1], c.inputs[:, :1]
    alone = world.step(lone, lone_inp, dt=c.dt)
    assert _diverged(alone).all()
    without = world.step(st, inp, dt=c.dt) if around else None
    for at in sorted({0, around // 2, around}):  # the first lane, one in the middle, the last
        both = np.concatenate([st[:at], lone, st[at:]])
        both_inp = np.concatenate([inp[:, :at], lone_inp, inp[:, at:]], 1)
        got = world.step(both, both_inp, dt=c.dt)
        if around:
            _same(np.delete(got, at), without, 'the %d around lane %d' % (around, at))
        _same(got[at:at + 1], alone, 'the diverging lane %d of %d' % (at, around + 1))
        game, offs = world.game_state(around + 1)
        _same(world.step_game(both, both_inp, game, offs, dt=c.dt), got, 'step_game, lane %d' % at)
    _same(got, ref.step(both, both_inp, dt=c.dt), 'the restatement')


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_batch_sizes(wad, worlds, n):
    """the diverging players first, ordinary ones after them, cut to n players: one lane, a wave less one, a full wave, a second
    block of one"""
    c = CASES['diverged']
    world, ref, _ = worlds[0]
    ticks = len(c.inputs)
    st, inp = _ordinary(wad, 65 - len(c.states), ticks)
    st, inp = np.concatenate([c.states, st])[:n], np.concatenate([c.inputs, inp], 1)[:, :n]
    got = world.step(st, inp, dt=c.dt)
    _same(got, ref.step(st, inp, dt=c.dt), n)
    assert _diverged(got)[:len(c.states)].all() and not _diverged(got)[len(c.states):].any()
