"""Which branch outcomes of the player step the suite's inputs take: the step inputs of the four GPU step test files and the rare
family of tests/step_cases.py, replayed on the restatement alone in its census build (tests/world_restatement.c under -DRS_CENSUS,
tests/step_census.py).  Every named outcome is taken by their union, but for the few that no finite input reaches; each rare case
takes what it is named for; and the old inputs go on taking what they take today.  The census build computes what the default build
computes.  No device."""
import numpy as np
import pytest

import rust_doom_amd as rd
import step_cases as sc
import step_census as cs
import world_ref
from util import META_PATH, ensure_wad

RARE = ('diverged', 'pitch_low', 'no_drag')  # the family by name: a case that leaves it fails here
# what the old inputs alone never take, of what can be taken (tools/restatement_coverage.py, profiles/step_branch_census.txt);
# derived again once the game and set replays stepped at 1/60 and not at a tick length of 0: the same one name
OLD_MISS = ('pitch_clamped_low',)


@pytest.fixture(scope='module')
def old():
    """{run: census} of the old inputs, thinned (an eighth of the large runs' players, four of the step case's config pairs)"""
    return cs.take(cs.old_runs(scale=8, thin=True))


@pytest.fixture(scope='module')
def rare():
    return cs.take(cs.rare_runs())


def test_the_unreachable_list_is_short_and_argued():
    assert len(cs.UNREACHABLE) <= 4 and set(cs.UNREACHABLE) <= set(cs.names())
    assert not set(cs.UNREACHABLE) & set(cs.MAY_NOT_BE_UNREACHABLE)
    assert all(len(reason) > 40 for reason in cs.UNREACHABLE.values())


def test_every_outcome_is_taken(old, rare):
    total = cs.add(cs.union(old), cs.union(rare))
    missed = [k for k in cs.names() if total[k] == 0 and k not in cs.UNREACHABLE]
    assert not missed, missed
    assert all(total[k] == 0 for k in cs.UNREACHABLE), {k: total[k] for k in cs.UNREACHABLE}  # (or the proof is wrong)


def test_the_family_is_whole():
    assert tuple(c.name for c in sc.rare()) == RARE
    for c in sc.rare():
        assert set(c.outcomes) <= set(cs.names()), c.name
        assert np.isfinite(c.states['pos']).all() and np.isfinite(c.states['vel']).all(), c.name
    assert {o for c in sc.rare() for o in c.outcomes} >= set(OLD_MISS) | {'clip_diverged'}


@pytest.mark.parametrize('name', RARE)
def test_a_rare_case_takes_its_outcomes(rare, name):
    case = {c.name: c for c in sc.rare()}[name]
    assert all(rare[name][o] > 0 for o in case.outcomes), {o: rare[name][o] for o in case.outcomes}


def test_the_old_inputs_keep_what_they_take(old):
    total = cs.union(old)
    lost = [k for k in cs.names() if total[k] == 0 and k not in OLD_MISS and k not in cs.UNREACHABLE]
    assert not lost, lost
    assert all(total[k] == 0 for k in OLD_MISS)  # (a rare case whose outcome the old inputs take by now is no longer needed)


def test_the_diverging_players_diverge_when_and_as_told():
    """DIVERGING set the flag in their first tick, DIVERGING_LATE in their second or third; an ordinary tick keeps it; and the
    ordinary players of the scripts never have it"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    ref = world_ref.RefWorld(wad, 0)
    case = sc.rare()[0]
    n_first = len(sc.DIVERGING)
    one = ref.step(case.states, case.inputs[:1], dt=case.dt)
    flag = lambda s: (s['flags'] & rd.PLAYER_DIVERGED) != 0
    assert flag(one)[:n_first].all() and not flag(one)[n_first:].any()
    three = ref.step(one, case.inputs[1:3], dt=case.dt)
    assert flag(three).all()
    assert flag(ref.step(three, case.inputs[3:], dt=case.dt)).all()
    assert np.isfinite(three['pos']).all() and np.isfinite(three['vel']).all()
    st, inp = sc.players(wad.build_level(0), 64, seed=7), sc.script(64, 30, seed=7)
    assert not flag(ref.step(st, inp, dt=case.dt)).any()


def test_the_census_build_computes_what_the_default_build_computes():
    wad = rd.Wad(ensure_wad(), META_PATH)
    assert not hasattr(world_ref.lib(), 'rs_census_count')  # the default library carries no counter
    for case in sc.rare():
        plain = world_ref.RefWorld(wad, case.level).step(case.states, case.inputs, config=case.config, dt=case.dt)
        counted = world_ref.RefWorld(wad, case.level, census=True).step(case.states, case.inputs, config=case.config, dt=case.dt)
        assert np.array_equal(sc.u32(plain), sc.u32(counted)), case.name
    world_ref.census(reset=True)


def test_sweeps_asked_for_directly_stay_out_of_the_census():
    wad = rd.Wad(ensure_wad(), META_PATH)
    ref = world_ref.RefWorld(wad, 0, census=True)
    world_ref.census(reset=True)
    st = sc.diverging_states()
    ref.sweep(np.concatenate([st['pos'], np.full((len(st), 1), 0.19, np.float32)], 1), st['vel'] / 30)
    assert not any(world_ref.census(reset=True).values())
