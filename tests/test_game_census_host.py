"""Which branch outcomes of the game tick the suite's inputs take: the game and world-set inputs of the GPU step tests and the volley
family of tests/game_cases.py, replayed on the restatement alone in its census build (tests/game_restatement.c under -DRS_CENSUS,
tests/game_census.py).  Every named outcome is taken by their union; each case of the family takes what it is named for; the old
inputs go on taking what they take today, and their replays are not inert; the census build computes what the default build
computes.  No device."""
import os
import tempfile

import numpy as np
import pytest

import game_cases as gc
import game_census as gcs
import game_ref
import rust_doom_amd as rd
import step_census as cs
import world_ref
import worldset_ref
from util import ROOT

FAMILY = ('plain_volley', 'once_volley_full', 'once_volley_short_plain', 'once_volley_short_once', 'restarts', 'cycle', 'set_volley')
# what the old inputs alone never take (tests/game_census.py, profiles/game_branch_census.txt)
OLD_MISS = ('action_clamped', 'fired_three_plus', 'fired_many_with_once', 'exit_with_others', 'trigger_two_effects', 'removed_two_plus',
            'removed_last', 'swapped_in_fired', 'adv_second_arrives_same_tick', 'adv_speed_zero', 'change_with_effect_active',
            'change_with_trigger_removed', 'change_with_nonzero_offset')


@pytest.fixture(scope='module')
def old():
    """{run: census} of the old game and set inputs, thinned as tests/test_step_census_host.py thins them"""
    return gcs.take(gcs.old_runs(scale=8))


@pytest.fixture(scope='module')
def family():
    return gcs.take(gcs.family_runs())


def _cases():
    with tempfile.TemporaryDirectory() as tmp:
        return gc.cases() + gc.set_cases(gc.volley_variant(tmp, 'full', exits=True))


def test_the_unreachable_list_is_short_and_argued():
    assert len(gcs.UNREACHABLE) <= 3 and set(gcs.UNREACHABLE) <= set(gcs.names())
    assert all(len(reason) > 40 for reason in gcs.UNREACHABLE.values())


def test_every_outcome_is_taken(old, family):
    total = cs.add(cs.union(old), cs.union(family))
    missed = [k for k in gcs.names() if total[k] == 0 and k not in gcs.UNREACHABLE]
    assert not missed, missed
    assert all(total[k] == 0 for k in gcs.UNREACHABLE), {k: total[k] for k in gcs.UNREACHABLE}  # (or the proof is wrong)


def test_the_family_is_whole():
    cases = _cases()
    assert tuple(c.name for c in cases) == FAMILY and gc.SET_CASE_NAMES == FAMILY[len(gc.cases()):]
    for c in cases:
        assert set(c.outcomes) <= set(gcs.names()), c.name
        assert len(c.states) <= 64 and len(c.inputs) <= 240, c.name
    assert {o for c in cases for o in c.outcomes} >= set(OLD_MISS)


@pytest.mark.parametrize('name', FAMILY)
def test_a_case_takes_its_outcomes(family, name):
    case = {c.name: c for c in _cases()}[name]
    assert all(family[name][o] > 0 for o in case.outcomes), {o: family[name][o] for o in case.outcomes}


def test_the_old_inputs_keep_what_they_take(old):
    total = cs.union(old)
    lost = [k for k in gcs.names() if total[k] == 0 and k not in OLD_MISS and k not in gcs.UNREACHABLE]
    assert not lost, lost
    assert all(total[k] == 0 for k in OLD_MISS)  # (a case whose outcome the old inputs take by now is no longer needed)


def test_the_old_replays_are_not_inert(old):
    """every game and set replay steps at a tick length above zero: its players walk lines of non-zero length, far more often
    than not, and its effects move and arrive (a tick length of 0 walks none and moves nothing)"""
    assert len(old) >= 6
    for name, c in old.items():
        assert c['walked_nonzero'] > 0, name
        if name != 'game ordering':  # (one of its two players stands throughout)
            assert c['walked_nonzero'] > 10 * c['walked_zero'], (name, c['walked_nonzero'], c['walked_zero'])
    total = cs.union(old)
    assert total['adv_arrived'] > 0 and total['adv_up'] > 0 and total['adv_down'] > 0


def _game(tmp, case, census):
    wad_path, meta_path = gc.volley_variant(tmp, case.variant)
    ref = world_ref.RefWorld(rd.Wad(wad_path, meta_path), 0, census=census)
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
    rg = game_ref.RefGame(ref, trig, effs, len(case.states), n_obj, census=census)
    return rg, rg.step(case.states, case.inputs, case.actions, threads=1)


def test_the_census_build_computes_what_the_default_build_computes(tmp_path):
    assert not hasattr(game_ref.lib(), 'rs_census_count')  # the default library carries no counter
    for case in gc.cases():
        (a, sa), (b, sb) = _game(str(tmp_path), case, False), _game(str(tmp_path), case, True)
        assert np.array_equal(cs.sc.u32(sa), cs.sc.u32(sb)), case.name
        for field in ('order', 'counts', 'act', 'aflags', 'offsets'):
            assert getattr(a, field).tobytes() == getattr(b, field).tobytes(), (case.name, field)
    exits = gc.volley_variant(str(tmp_path), 'full', exits=True)
    for case in gc.set_cases(exits):
        refs = [worldset_ref.RefWorldSet(exits[0], exits[1], gc.SET, case.levels, census=c) for c in (False, True)]
        sa, sb = [r.step(case.states, case.inputs, case.actions, threads=1) for r in refs]
        assert np.array_equal(cs.sc.u32(sa), cs.sc.u32(sb)) and refs[0].levels.tolist() == refs[1].levels.tolist(), case.name
        assert refs[0].offsets().tobytes() == refs[1].offsets().tobytes()
    game_ref.census(reset=True), world_ref.census(reset=True)


def test_two_lines_on_one_object_follow_the_list_in_both_orders(tmp_path):
    """triggers 61 and 106 move one lift at different speeds.  In linedef order 106 is the later and wins; where the list ends with
    106, the volley's removals carry it ahead of 61, and the same shot a tick later leaves 61's speed"""
    speeds = {}
    for variant in ('full', 'short_plain'):
        case = {c.name: c for c in gc.cases()}['once_volley_' + variant]
        rg, _ = _game(str(tmp_path), case, False)
        e61, e106 = (rg.effs[rg.trig['effect_start'][t]] for t in (61, 106))
        assert e61['object_id'] == e106['object_id'] and e61['speed'] != e106['speed']
        first = game_ref.RefGame(rg.w, rg.trig, rg.effs, len(case.states), rg.n_objects)
        first.step(case.states, case.inputs[:1], case.actions[:1], threads=1)
        assert first.act[0, e61['object_id'], 3] == e106['speed']  # the first shot: linedef order in both
        speeds[variant] = rg.act[0, e61['object_id'], 3], e61['speed'], e106['speed']
        where = {int(t): k for k, t in enumerate(rg.order[0, :rg.counts[0]])}
        assert (where[106] < where[61]) == (variant == 'short_plain')
    assert speeds['full'][0] == speeds['full'][2] and speeds['short_plain'][0] == speeds['short_plain'][1]


def test_the_table_names_every_outcome():
    with open(os.path.join(ROOT, 'profiles', 'game_branch_census.txt')) as f:
        rows = [line.split() for line in f if line.strip() and not line.startswith('#')]
    listed = {r[0]: r for r in rows[1:]}
    assert list(listed) == gcs.names()
    for k, r in listed.items():
        assert (int(r[1]) + int(r[2]) > 0) != (k in gcs.UNREACHABLE), r
        assert (int(r[1]) == 0) == (k in OLD_MISS or k in gcs.UNREACHABLE), r
