"""The census of the game tick's branch outcomes: the game and world-set inputs of the GPU step tests (tests/step_census.py:
old_runs, and test_game_host.ordering_run) and the volley family of tests/game_cases.py replayed on the restatement alone, in its
census build (tests/game_restatement.c under -DRS_CENSUS: seg_offset, the poll, the removals, advance) and through
worldset_ref.RefWorldSet's own counters of the level change, and what each run took.  Used by tests/test_game_census_host.py.
No device.

  python tests/game_census.py > profiles/game_branch_census.txt

writes the table: every outcome, how often the old inputs take it and how often the family does."""
import os
import sys
import tempfile

if __name__ == '__main__':  # (run as a script: the package and the oracle are in the repository's root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import game_cases as gc
import game_ref
import rust_doom_amd as rd
import step_census as cs
import world_ref
import worldset_ref

# Outcomes that no input reaches, each with its one-line proof from the arithmetic (at most 3)
UNREACHABLE = {}


def names():
    """the game tick's outcomes: the names tests/game_restatement.c appends to the step's table, and the level change's"""
    step = set(world_ref.census())
    return [k for k in game_ref.census() if k not in step] + list(worldset_ref.SET_CENSUS_NAMES)


class Libs(cs.Libs):
    """the census builds, every RefWorldSet remembered so that its counters can be read"""
    sets = []

    @staticmethod
    def RefWorldSet(wad, meta, indices, lv):
        ref = worldset_ref.RefWorldSet(wad, meta, indices, lv, census=True)
        Libs.sets.append(ref)
        return ref

    @staticmethod
    def read(reset=True):
        """{outcome: count} since the last read"""
        world_ref.census(reset)
        c = game_ref.census(reset)
        out = {k: c.get(k, 0) for k in names()}
        for ref in Libs.sets:
            for k, v in ref.set_census.items():
                out[k] += v
        if reset:
            for ref in Libs.sets:
                ref.set_census = dict.fromkeys(ref.set_census, 0)
            del Libs.sets[:]
        return out


def old_runs(scale=8):
    """(name, run) of the old game and set inputs: step_census.old_runs' game and worldset replays, and the list-order run"""
    runs = [(name, run) for name, run in cs.old_runs(scale=scale, thin=True, libs=Libs) if name.startswith(('game', 'worldset'))]

    def ordering():
        from test_game_host import ordering_run, ordering_variant
        with tempfile.TemporaryDirectory() as tmp:
            wad_path, meta_path = ordering_variant(tmp)
            ref = Libs.RefWorld(rd.Wad(wad_path, meta_path), 0)
            trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
            rg = Libs.RefGame(ref, trig, effs, 2, n_obj)
            ordering_run(lambda st, inp, act: rg.step(st, inp, act), trig, ref)
    return runs + [('game ordering', ordering)]


def family_runs():
    """(name, run) of the volley family, the set's cases after the single level's"""
    def one(case):
        def run():
            with tempfile.TemporaryDirectory() as tmp:
                wad_path, meta_path = gc.volley_variant(tmp, case.variant)
                ref = Libs.RefWorld(rd.Wad(wad_path, meta_path), 0)
                trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
                Libs.RefGame(ref, trig, effs, len(case.states), n_obj).step(case.states, case.inputs, case.actions, threads=1)
        return run

    def set_one(index):
        def run():
            with tempfile.TemporaryDirectory() as tmp:
                exits = gc.volley_variant(tmp, 'full', exits=True)
                case = gc.set_cases(exits)[index]
                Libs.RefWorldSet(exits[0], exits[1], gc.SET, case.levels).step(case.states, case.inputs, case.actions, threads=1)
        return run
    return [(c.name, one(c)) for c in gc.cases()] + [(name, set_one(i)) for i, name in enumerate(gc.SET_CASE_NAMES)]


def take(runs):
    return cs.take(runs, libs=Libs)


def main():
    old, family = cs.union(take(old_runs())), cs.union(take(family_runs()))
    print('# The game tick\'s branch outcomes (tests/game_restatement.c under -DRS_CENSUS, worldset_ref.RefWorldSet): how often the')
    print('# old game and set inputs take each (an eighth of the large runs\' players) and how often the volley family of')
    print('# tests/game_cases.py does.  Written by tests/game_census.py; a count says `zero or not` and no more.')
    print('%-32s %12s %12s' % ('outcome', 'old inputs', 'family'))
    for k in names():
        note = '   UNREACHABLE' if k in UNREACHABLE else '   <-- never taken' if old[k] + family[k] == 0 else \
            '   (the family alone)' if old[k] == 0 else ''
        print('%-32s %12d %12d%s' % (k, old[k], family[k], note))
    return 0


if __name__ == '__main__':
    sys.exit(main())
