"""The census of the player step's branch outcomes: the step inputs of the four GPU step test files (tests/test_gpu_world.py,
test_gpu_step_configs.py through gpu_step_child.py, test_gpu_game.py, test_gpu_worldset.py) and the rare family of
tests/step_cases.py replayed on the restatement alone, in its census build (tests/world_restatement.c under -DRS_CENSUS), and what
each run took.  Used by tests/test_step_census_host.py and tools/restatement_coverage.py.  No device.

`world`, `game` and `set` name the restatement's three entry points; `libs` lets the coverage tool put its own builds in their
place (objects with RefWorld / RefGame / RefWorldSet of the same signatures)."""
import tempfile

import numpy as np

import game_ref
import rust_doom_amd as rd
import step_cases as sc
import world_ref
import worldset_ref
from util import META_PATH, ensure_wad

# Outcomes that no finite input reaches, each with its one-line proof from the arithmetic
UNREACHABLE = {
    'clip_time_clamped_low': 'c.time = best / speed with speed > 0, and every candidate for best is accepted only when >= 0: the '
                             'plane\'s -(spd - radius) / ndn has spd >= radius and ndn < 0, a vertex needs d >= 0, an edge tt >= 0',
    'root_first_lower': 'i1 = (-b + i) / 2a and i2 = (-b - i) / 2a with i = sqrtf(.) >= 0 and a = |p2 - p1|^2 = |-nvel|^2 > 0 (sweep_tri '
                        'returns before it when speed == 0), so i1 >= i2 and the comparison i1 < i2 is never true',
    'node_stack_full': 'a depth-first walk that pushes at most two children holds at most depth + 1 pending nodes, and wb_node '
                       'refuses a 1 025th nested node: a built world\'s walk never holds more than 1 025 of the 4 096',
}
MAY_NOT_BE_UNREACHABLE = ('clip_diverged', 'tri_vertex_wins', 'sweep_vertex_wins', 'tri_edge_wins', 'sweep_edge_wins', 'tri_overlap',
                          'pitch_clamped_low', 'pitch_clamped_high', 'noclip_land_falling', 'noclip_land_rising')


class Libs:
    """the census builds of the restatements"""
    RefWorld = staticmethod(lambda wad, index: world_ref.RefWorld(wad, index, census=True))
    RefGame = staticmethod(lambda ref, trig, effs, n, n_obj: game_ref.RefGame(ref, trig, effs, n, n_obj, census=True))
    RefWorldSet = staticmethod(lambda wad, meta, indices, lv: worldset_ref.RefWorldSet(wad, meta, indices, lv, census=True))

    @staticmethod
    def read(reset=True):
        """{outcome: count} over both libraries since the last read"""
        a, b = world_ref.census(reset), game_ref.census(reset)
        return {k: a[k] + b[k] for k in a}


def names():
    return list(world_ref.census())


def add(total, part):
    for k, v in part.items():
        total[k] = total.get(k, 0) + v
    return total


# the (config, tick length) pairs of test_gpu_step_configs.py's step case that the thinned replay keeps: the default, the one
# single-field config and the all-field config whose players run clip()'s loop out on E1M1, and the all-field pair of 1/120
THIN_PAIRS = [('default', sc.DT_DEFAULT), ('radius=0.26', sc.DTS['35']), ('all_a', sc.DTS['120']), ('all_b', sc.DTS['30'])]


def old_runs(scale=4, thin=False, libs=Libs):
    """(name, run) of the old step inputs, each run() stepping them on the restatement alone.  scale: the divisor of the player
    counts of the large runs (test_gpu_world's, test_gpu_game's and test_gpu_worldset's 512 and 1 024 players) and of the set's
    600 ticks; the runs of 256 players stay whole.  thin: of the step case's 26 (config, tick length) pairs only THIN_PAIRS"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    runs = []

    def world_step(index, n, ticks, seed, off_seed=None, cfg=None, dt=sc.DT_DEFAULT):
        def run():
            ref = libs.RefWorld(wad, index)
            st, inp = sc.players(wad.build_level(index), n, seed=seed), sc.script(n, ticks, seed=seed)
            off = None
            if off_seed is not None:
                off = np.zeros((n, ref.n_objects, 3), np.float32)
                off[:, :, 1] = np.random.default_rng(off_seed).uniform(0.0, 1.2, (n, ref.n_objects)).astype(np.float32)
            ref.step(st, inp, config=cfg, dt=dt, offsets=off)
        return run

    for index in (0, 4):  # test_gpu_world.py::test_step_matches_the_restatement
        runs.append(('world level %d' % index, world_step(index, 1024 // scale, 300, index)))
    runs.append(('world offsets', world_step(0, 256, 120, 9, off_seed=3)))  # ::test_step_with_object_offsets_matches_...
    for index in (0, 2):  # ::test_two_streams_two_worlds_do_not_interfere
        runs.append(('world streams %d' % index, world_step(index, 512 // scale, 200, 20 + index)))

    def shared(index, name, dt, off=False):  # gpu_step_child.py: case_step
        def run():
            ref = libs.RefWorld(wad, index)
            st, inp = sc.shared(wad.build_level(index), index)
            o = None
            if off:
                o = np.zeros((len(st), ref.n_objects, 3), np.float32)
                o[:, :, 1] = np.random.default_rng(3).uniform(0.0, 1.2, (len(st), ref.n_objects)).astype(np.float32)
            ref.step(st, inp, config=sc.config(sc.CONFIGS[name]), dt=dt, offsets=o)
        return run

    for index in sc.LEVELS:
        pairs = [(name, dt) for name in sc.CONFIGS for dt in (sc.DT_DEFAULT, sc.DTS['35'])]
        pairs += [(name, dt) for name in sc.ALL_FIELDS for dt in (sc.DTS['120'], sc.DTS['30'])]
        pairs = THIN_PAIRS if thin else pairs
        for name, dt in pairs:
            runs.append(('configs level %d %s dt %.4f' % (index, name, dt), shared(index, name, dt)))
        runs.append(('configs level %d offsets' % index, shared(index, 'all_a', sc.DTS['35'], off=True)))

    def model(name, key):  # gpu_step_child.py: case_model
        def run():
            ref = libs.RefWorld(wad, sc.MODEL_LEVEL)
            names_, st, inp, ticks, final = sc.model_run(sc.CONFIGS[name], sc.DTS[key])
            sc.snapshots(lambda s, i: ref.step(s, i, config=sc.config(sc.CONFIGS[name]), dt=sc.DTS[key]), st, inp, ticks)
        return run

    for name in ('default', 'all_a', 'all_b'):
        for key in ('0', '30'):
            runs.append(('model %s dt %s' % (name, key), model(name, key)))

    # (key '0' is a tick length of 0, which the device and RefGame.step / RefWorldSet.step read as 1/60)
    def game(patched, n, seed, ticks, name='default', key='0', push=0.05):  # test_gpu_game.py: _bit_exact; gpu_step_child: case_game
        def run():
            from test_game_host import patched_variant
            with tempfile.TemporaryDirectory() as tmp:
                wad_path, meta_path = patched_variant(tmp) if patched else (ensure_wad(), META_PATH)
                w = rd.Wad(wad_path, meta_path)
                ref = libs.RefWorld(w, 0)
                trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
                st, _ = sc.seed_players(ref, trig, n, seed)
                inp, act = sc.game_script(len(st), ticks, seed + 1, push=push)
                libs.RefGame(ref, trig, effs, len(st), n_obj).step(st, inp, act, config=sc.config(sc.CONFIGS[name]), dt=sc.DTS[key])
        return run

    runs.append(('game e1m1', game(False, 1024 // scale, 11, 600)))
    runs.append(('game patched', game(True, 1024 // scale, 12, 600)))
    runs.append(('game all_a dt 35', game(True, sc.N_PLAYERS, 61, sc.GAME_TICKS, 'all_a', '35', push=0.1)))

    def worldset(n, seed, ticks, name='default', key='0'):  # test_gpu_worldset.py; gpu_step_child: case_worldset
        def run():
            with tempfile.TemporaryDirectory() as tmp:
                exits = worldset_ref.exit_variant(tmp)
                _, st, lv, inp, act = sc.set_players(exits, n, seed, device=False)
                ref = libs.RefWorldSet(exits[0], exits[1], sc.SET, lv)
                ref.step(st, inp[:ticks], act[:ticks], config=sc.config(sc.CONFIGS[name]), dt=sc.DTS[key])
        return run

    runs.append(('worldset', worldset(1024 // scale, 31, 600 // scale)))
    runs.append(('worldset all_b dt 120', worldset(sc.N_PLAYERS // scale, 31, 160, 'all_b', '120')))
    return runs


def rare_runs(libs=Libs):
    """(name, run) of the rare family through the plain step"""
    wad = rd.Wad(ensure_wad(), META_PATH)

    def one(case):
        return lambda: libs.RefWorld(wad, case.level).step(case.states, case.inputs, config=case.config, dt=case.dt)
    return [(case.name, one(case)) for case in sc.rare()]


def take(runs, libs=Libs, verbose=False):
    """{run name: {outcome: count}} of the runs, in order"""
    import time
    libs.read()
    out = {}
    for name, run in runs:
        t = time.time()
        run()
        out[name] = libs.read()
        if verbose:
            print('%-40s %6.1f s' % (name, time.time() - t), flush=True)
    return out


def union(per_run):
    total = {}
    for c in per_run.values():
        add(total, c)
    return total
