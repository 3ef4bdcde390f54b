"""The conditions that keep tests/test_gpu_step_configs.py from passing vacuously, on the restatements alone (no GPU): every
config field and every tick length of tests/step_cases.py changes the shared run's result, dt = 0 is 1/60, doors and lifts
move differently at two tick lengths on the patched E1M1, and the pushes of the door check leave 16 doors or more rising at its
end (step_cases.game_setup and door_setup: the set-ups tests/gpu_step_child.py runs on the GPU)."""
import numpy as np
import pytest

import game_ref
import rust_doom_amd as rd
import step_cases as sc
import world_ref
from util import META_PATH, ensure_wad


@pytest.fixture(scope='module')
def runs():
    """{level: run(config name, dt) -> final states of the shared run}, each result computed once"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    out = {}
    for index in sc.LEVELS:
        ref = world_ref.RefWorld(wad, index)
        st, inp = sc.shared(wad.build_level(index), index)
        cache = {}

        def run(name, dt, ref=ref, st=st, inp=inp, cache=cache):
            if (name, dt) not in cache:
                cache[name, dt] = ref.step(st, inp, config=sc.config(sc.CONFIGS[name]), dt=dt)
            return cache[name, dt]
        out[index] = run
    return out


def test_the_configs_stay_in_the_domain():
    sc.check_domain()
    got = rd.player_config_default()
    assert [float(got[f]) for f in sc.FIELDS] == [float(np.float32(v)) for v in sc.DEFAULT]


def test_the_moved_helpers_make_the_bytes_they_made():
    """sha256 of script(60, 200, 7), of players(E1M1, 70, 7) and of game_script(50, 80, 12, push=0.1), recorded from the copies
    tests/test_gpu_world.py and tests/test_gpu_game.py had before the move"""
    import hashlib
    inp, act = sc.game_script(50, 80, 12, push=0.1)
    assert hashlib.sha256(inp.tobytes() + act.tobytes()).hexdigest() == '51f55df84b950408f723bb2c4b6c4adaa68c675c715b516113942934cf75bba7'
    inp = sc.script(60, 200, 7)
    assert hashlib.sha256(inp.tobytes()).hexdigest() == 'db3130f7c50e9149e7b60fac23a7ea58dfd13a23bdf23f221c75c71907df9f83'
    s = np.arange(60) % 6
    assert (inp['movement'][:, s == 4] == 0).all() and (inp['movement'][151:, s == 0, 0] == 1).all()
    assert inp['jump'][:, s == 2].sum() == 10 * 25 and (inp['look'][:, s == 3, 1] == np.float32(-0.015)).all()
    st = sc.players(rd.Wad(ensure_wad(), META_PATH).build_level(0), 70, 7)
    assert hashlib.sha256(st.tobytes()).hexdigest() == '0ca20589cf595ade349962426ea456eb4a25d337b32c3161a535fee5ad7deeb6'
    assert (st['flags'][3::7] & rd.PLAYER_FLY).all() and not (st['flags'][4::5] & rd.PLAYER_CLIP).any()


@pytest.mark.parametrize('index', sc.LEVELS)
def test_every_single_field_changes_the_run(runs, index):
    base = runs[index]('default', sc.DT_DEFAULT)
    for name in sc.SINGLE_NAMES:
        share = sc.differing(runs[index](name, sc.DT_DEFAULT), base)
        print('level %d  %-22s differs from the default in %5.1f %% of the players' % (index, name, 100 * share))
        assert share >= 0.10, (index, name, share)


@pytest.mark.parametrize('index', sc.LEVELS)
def test_every_tick_length_changes_the_run(runs, index):
    for name in ('default', 'all_a', 'all_b'):
        base = runs[index](name, sc.DT_DEFAULT)
        for key, dt in sc.DTS.items():
            share = sc.differing(runs[index](name, dt), base)
            print('level %d  %-8s dt %-4s differs from 1/60 in %5.1f %% of the players' % (index, name, key, 100 * share))
            if dt == 0:
                assert share == 0.0, (index, name, share)  # zero is 1/60 in every bit
            else:
                assert share >= 0.90, (index, name, key, share)


def test_doors_and_lifts_move_and_depend_on_the_tick_length(tmp_path):
    wad, ref, trig, effs, n_obj, st, inp, act = sc.game_setup(str(tmp_path), sc.N_PLAYERS, 61)
    offsets = {}
    for key in ('35', '120'):
        rg = game_ref.RefGame(ref, trig, effs, len(st), n_obj)
        rg.step(st, inp, act, config=sc.config(sc.CONFIGS['all_a']), dt=sc.DTS[key])
        offsets[key] = rg.offsets.copy()
        moved = int((rg.offsets[:, :, 1] != 0).any(1).sum())
        print('dt 1/%s: %d of %d games end with a door or lift off its rest' % (key, moved, len(st)))
        assert moved >= 1
    assert not np.array_equal(offsets['35'].view(np.uint32), offsets['120'].view(np.uint32))


@pytest.mark.parametrize('key', ['35', '120'])
def test_pushed_doors_are_rising_at_the_end(tmp_path, key):
    d = sc.door_setup(str(tmp_path), key)
    n, dt = len(d['states']), sc.DTS[key]
    print('dt 1/%s: %d ticks, %d players, %d with their door rising at the end' % (key, len(d['inputs']), n, int(d['moving'].sum())))
    assert d['moving'].sum() >= 16
    # the restatement's own doors keep the rule the GPU is held to: within speed * dt of speed * (T - T_fired)
    height = d['offsets'][np.arange(n), d['obj'], 1].astype(np.float64)
    want = np.minimum(d['speed'] * (len(d['inputs']) - d['fired'] - 1) * dt, d['first'])
    assert (np.abs(height - want)[d['moving']] <= (d['speed'] * dt)[d['moving']]).all()
