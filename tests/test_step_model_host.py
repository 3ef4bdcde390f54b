"""The float64 model of the player step (tests/step_model.py) on the CPU: every case stays inside its box by the model's own
trajectory; the binary32 restatement agrees with the model within 8 times tests/golden/step_model_error.json, which is recomputed
and compared; the closed forms hold of the model; and a config field 1 % off moves the model by more than ten times what the
bound allows, so the bound cannot hide a wrong constant."""
import importlib.util
import json
import os

import numpy as np
import pytest

import step_cases as sc
import step_model
from util import ROOT

QUANTITIES = sc.QUANTITIES


@pytest.fixture(scope='module')
def runs():
    """{(config, dt key): (names, states, inputs, ticks, final)} of the model"""
    return {(name, key): sc.model_run(values, dt) for name, values in sc.CONFIGS.items() for key, dt in sc.DTS.items()}


def test_every_case_stays_in_the_box(runs):
    landings = 0
    for (name, key), (names, st, inp, ticks, final) in runs.items():
        c = dict(zip(sc.FIELDS, sc.CONFIGS[name]))
        # the ticks come from the model's own trajectory (Trace.valid_ticks); here the end points are checked against the box again
        reach = c['radius'] + sc.WALL_MARGIN
        for axis in (0, 2):
            assert (final['pos'][:, axis] - sc.ROOM_LO > reach).all() and (sc.ROOM_HI - final['pos'][:, axis] > reach).all(), (name, key)
        assert (final['pos'][:, 1] + c['radius'] < sc.ROOM_CEILING).all(), (name, key)
        # (1e-9: noclip()'s landing height is a float64 sum about 1000 in the model)
        assert (final['pos'][:, 1] - sc.ROOM_FLOOR >= min(c['radius'], step_model.FEET_RADIUS) - 1e-9).all(), (name, key)
        # a case is cut short of its 60 ticks by the box, by a landing with clipping off -- and where the spring is unstable
        # (step_cases.tick_cap; the record lists each cell's cap: 52 ticks for the default at 1/30, 9 for all_a there)
        cap = sc.tick_cap(c, sc.DTS[key])
        assert cap == sc.MODEL_TICKS or (sc.spring_root(c, sc.DTS[key]) > 1 and cap >= 8), (name, key, cap)
        assert ticks[names.index('stand_rest')] == cap, (name, key, cap)
        short = [n for n, t in zip(names, ticks) if t < sc.MIN_MODEL_TICKS]
        # only the drops may end at once: with a head sphere no wider than the feet's, the feet sphere reaches the floor first
        assert all(n in ('drop', 'noclip_drop') for n in short), (name, key, short)
        assert ticks[names.index('drop')] == cap or c['radius'] <= step_model.FEET_RADIUS, (name, key)
        assert ticks.sum() >= 6 * len(names), (name, key, int(ticks.sum()))
        # noclip()'s landing (player.rs:183-187) is live: a head sphere wider than the feet's lands at every tick length, inside the
        # box, and the case goes on for AFTER_LANDING ticks on the height the 2000-unit probe gave it
        i = names.index('noclip_drop')
        if c['radius'] > step_model.FEET_RADIUS:
            assert final['landings'][i] >= 1 and ticks[i] > sc.AFTER_LANDING, (name, key, final['landings'][i], ticks[i])
        landings += int(final['landings'].sum())
    assert landings >= 24, landings


def test_the_restatement_agrees_with_the_model_and_the_record_is_current(runs):
    spec = importlib.util.spec_from_file_location('make_step_model_error', os.path.join(ROOT, 'tests', 'golden', 'make_step_model_error.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(sc.RECORD) as f:
        committed = json.load(f)
    fresh = gen.record()
    assert committed['factor'] == fresh['factor'] == 8.0
    assert [(r['config'], r['dt']) for r in committed['records']] == list(runs)
    bounds = sc.bounds()
    for old, new in zip(committed['records'], fresh['records']):
        print('%-22s dt %-4s %2d cases %4d ticks (at most %2d a case), %d landings   clipping on: pos %.2e  vel %.2e  last_height_diff %.2e'
              '   off: pos %.2e  vel %.2e  last_height_diff %.2e' % (
                  new['config'], new['dt'], new['cases'], new['ticks'], new['tick_cap'], new['landings'],
                  *[new[cls][q] for cls in sc.CLASSES for q in QUANTITIES]))
        keys = ('config', 'dt', 'cases', 'ticks', 'tick_cap', 'landings')
        assert [old[k] for k in keys] == [new[k] for k in keys]
        b = bounds[new['config'], new['dt']]
        for cls in sc.CLASSES:
            for q in QUANTITIES:
                assert new[cls][q] <= b[cls][q], (new['config'], new['dt'], cls, q)  # within the bound the GPU is held to, and
                assert new[cls][q] == pytest.approx(old[cls][q], rel=1e-6, abs=1e-12), (new['config'], new['dt'], cls, q)  # the record
            assert b[cls]['pos'] <= sc.POS_CAP


def test_closed_forms_hold_of_the_model(runs):
    seen = set()
    for (name, key), (names, st, inp, ticks, final) in runs.items():
        for case, i, closed, at_end, gap in sc.closed_forms(sc.CONFIGS[name], sc.DTS[key], names, st, inp, ticks, final):
            # (closed_forms asserts the model run ten times longer against the formula to 1e-6; the case is `gap` short of it)
            assert abs(at_end - closed) <= gap + 1e-6 * closed, (name, key, case, at_end, closed, gap)
            if case == 'stand_rest':
                assert gap <= 1e-6 * closed, (name, key, case, gap)  # a player at rest stays there
            seen.add((name, key, case))
    # every closed form is held at every config, at two tick lengths or more
    for name in sc.CONFIGS:
        for case in ('stand_rest', 'stand_high', 'diagonal_walk', 'diagonal_fly'):
            assert sum((name, key, case) in seen for key in sc.DTS) >= 2, (name, case)


def _perturbed(values, field):
    """the config with `field` 1 % off (a field that is zero: by 1 % of its default)"""
    v = list(values)
    k = sc.FIELDS.index(field)
    v[k] = v[k] * 1.01 if v[k] != 0 else 0.01 * sc.DEFAULT[k]
    return tuple(v)


def test_one_percent_of_any_field_shows_far_above_the_bound(runs):
    bounds = sc.bounds()
    seen = {f: 0 for f in sc.FIELDS}
    for (name, key), (names, st, inp, ticks, final) in runs.items():
        b = bounds[name, key]
        for f in sc.FIELDS:
            c = dict(zip(sc.FIELDS, _perturbed(sc.CONFIGS[name], f)))
            off = step_model.step(st, inp, c, sc.resolve_dt(sc.DTS[key]), floor=sc.ROOM_FLOOR, n_ticks=ticks)
            ratio = max(np.abs(off[q] - final[q])[mask].max() / (10 * b[cls][q])
                        for cls, mask in sc.classes(st).items() for q in ('pos', 'vel'))
            seen[f] += ratio > 1
            if f != 'radius':
                assert ratio > 1, (name, key, f, ratio)
    print({f: '%d of %d' % (k, len(runs)) for f, k in seen.items()})
    # radius shows over a floor alone only where the head sphere is wider than the feet's 0.2 and is dropped onto it
    wide = [k for k in runs if dict(zip(sc.FIELDS, sc.CONFIGS[k[0]]))['radius'] > step_model.FEET_RADIUS]
    assert seen['radius'] >= len(wide) > 0, (seen['radius'], len(wide))
