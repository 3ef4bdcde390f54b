#!/usr/bin/env python3
"""Which branches of the restated player step the suite's inputs take, by gcov: a check of the hand-placed census of
tests/world_restatement.c (-DRS_CENSUS) against the compiler's own list.  CPU only; a tool, not a test.

Builds copies of tests/world_restatement.c and tests/game_restatement.c with gcc --coverage -O1 -fprofile-update=atomic into a
temporary directory, replays the step inputs of the four GPU step test files (tests/step_census.py: old_runs) through them on the
restatement alone -- once alone, once with the rare family of tests/step_cases.py after them -- and prints, for each of the two
replays, the census table (the same replay through the census build) and every branch outcome of tick(), sweep_tri(),
sweep_sphere() and their helpers that was never taken.  Only `zero or not` is to be read from a count.

  python tools/restatement_coverage.py [--scale 8] [--all-pairs] > profiles/step_branch_census.txt

--scale: the divisor of the large runs' player counts (8: an eighth of the players; 1: all of them).  --all-pairs: every (config,
tick length) pair of test_gpu_step_configs.py's step case and not the four of step_census.THIN_PAIRS.  The threads of a replay
share gcov's counters, so the coverage builds run many times slower than the plain ones."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, 'tests')
FUNCTIONS = ('tick', 'sweep_sphere', 'sweep_range', 'sweep_tri', 'sphere_line', 'lowest_root', 'line_line',
             'point_in_triangle', 'in_range01', 'clampf_', 'vnorm0')
SOURCES = ('world_restatement', 'game_restatement')


def _paths():
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)


def child(phase, scale, thin, directory):
    """replay `phase` ('old' or 'old+rare') through coverage builds in `directory`; gcov's counts are written as the process ends"""
    _paths()
    import game_ref
    import step_census as cs
    import world_ref
    import worldset_ref

    def coverage_lib(src, deps=(), flags=(), tag=''):
        name = os.path.splitext(os.path.basename(src))[0]
        obj, out = os.path.join(directory, name + '.o'), os.path.join(directory, 'lib%s.so' % name)
        if not os.path.exists(out):
            common = ['gcc', '--coverage', '-fprofile-update=atomic', '-fPIC', '-O1', '-ffp-contract=off', '-fno-fast-math']
            subprocess.check_call(common + ['-I', TESTS, '-c', '-o', obj, src], cwd=directory)
            subprocess.check_call(common + ['-shared', '-o', out, obj, '-lm'], cwd=directory)
        return ctypes.CDLL(out)

    world_ref.restatement_lib = game_ref.restatement_lib = coverage_lib

    class Plain:
        RefWorld, RefGame, RefWorldSet = world_ref.RefWorld, game_ref.RefGame, worldset_ref.RefWorldSet
        read = staticmethod(lambda reset=True: {})

    runs = cs.old_runs(scale=scale, thin=thin, libs=Plain) + (cs.rare_runs(libs=Plain) if phase == 'old+rare' else [])
    for name, run in runs:
        run()
        print('.', end='', file=sys.stderr, flush=True)
    print(file=sys.stderr)


def untaken(directory):
    """[(line, function, source text, [indices of the branch outcomes never taken], outcomes)] over both builds' counts added"""
    counts, text = {}, {}
    for name in SOURCES:
        out = subprocess.check_output(['gcov', '-b', '-c', '--json-format', '--stdout', name + '.o'], cwd=directory)
        for f in json.loads(out)['files']:
            if os.path.basename(f['file']) != 'world_restatement.c':
                continue
            for ln in f['lines']:
                if ln.get('function_name') in FUNCTIONS and ln['branches']:
                    got = [b['count'] for b in ln['branches']]
                    have = counts.setdefault((ln['line_number'], ln['function_name']), [0] * len(got))
                    assert len(have) == len(got), ln
                    counts[ln['line_number'], ln['function_name']] = [a + b for a, b in zip(have, got)]
    with open(os.path.join(TESTS, 'world_restatement.c')) as f:
        source = f.read().split('\n')
    rows, total, taken = [], 0, 0
    for (line, fn), c in sorted(counts.items()):
        total, taken = total + len(c), taken + sum(1 for v in c if v)
        miss = [i for i, v in enumerate(c) if not v]
        if miss:
            rows.append((line, fn, source[line - 1].strip(), miss, len(c)))
    return rows, total, taken


def census(phase, scale, thin):
    _paths()
    import step_census as cs
    runs = cs.old_runs(scale=scale, thin=thin) + (cs.rare_runs() if phase == 'old+rare' else [])
    return cs.union(cs.take(runs)), cs.UNREACHABLE


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--scale', type=int, default=8)
    ap.add_argument('--all-pairs', action='store_true')
    ap.add_argument('--child', nargs=2, metavar=('PHASE', 'DIRECTORY'), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.scale, not args.all_pairs, args.child[1])
        return 0
    print('# The player step\'s branch outcomes: which of them the suite\'s step inputs take.  Written by')
    print('# tools/restatement_coverage.py --scale %d%s; a count says `zero or not` and no more.' % (args.scale, ' --all-pairs' * args.all_pairs))
    for phase, title in (('old', 'the step inputs of the four GPU step test files alone'),
                         ('old+rare', 'the same inputs and the rare family of tests/step_cases.py')):
        print('\n== %s ==' % title)
        total, unreachable = census(phase, args.scale, not args.all_pairs)
        print('\nthe census (tests/world_restatement.c, -DRS_CENSUS): outcome, times taken')
        for k, v in total.items():
            note = '   UNREACHABLE' if k in unreachable else '   <-- never taken' if v == 0 else ''
            print('  %-28s %12d%s' % (k, v, note))
        sys.stdout.flush()
        with tempfile.TemporaryDirectory(prefix='restatement_coverage_') as tmp:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--scale', str(args.scale), '--child', phase, tmp] +
                                  ['--all-pairs'] * args.all_pairs)
            rows, n, taken = untaken(tmp)
        print('\ngcov -b (gcc --coverage -O1): %d of %d branch outcomes of %s taken; never taken:' % (taken, n, ', '.join(FUNCTIONS)))
        for line, fn, text, miss, k in rows:
            print('  world_restatement.c:%d %s(): outcome%s %s of %d' % (line, fn, 's' if len(miss) > 1 else '',
                                                                         ', '.join(map(str, miss)), k))
            print('      %s' % text[:150])
    return 0


if __name__ == '__main__':
    sys.exit(main())
