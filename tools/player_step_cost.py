#!/usr/bin/env python3
"""What stepping players costs (rdoom_world_step_players, DESIGN section "Collision world and player physics"): 4 096 and 65 536
players x 60 ticks (one second of the reference's 60 Hz tick) on E1M1 (synthetic IWAD) and on the 10x level, from the floor
centroids with the scripted inputs of tests/test_gpu_world.py (walk, strafe, jump, look up, stand, turn).  The GPU time is one
launch of all the ticks, bracketed by torch.cuda.synchronize (the median of --steps launches after --warmup); next to it, the
test-side C restatement (tests/world_restatement.c, gcc -O2) on 16 host threads, timed once.  Prints a table and one JSON
line per row: microseconds per player-tick.  Needs the GPU and torch.
--game also times rdoom_world_step_game (doors, lifts and exits, DESIGN section "Doors, lifts and exits") on the same players and
inputs with about 5 % push actions, each launch from a freshly reset level, next to the test-side restatement
(tests/game_restatement.c) on the same host threads.
--set times rdoom_worldset_step_game (world sets, DESIGN section "World sets and the level change") on the set E1M1..E1M3 of the
synthetic IWAD: every player on E1M1, against --game's step on E1M1 alone with the same players and inputs; then players mixed over
the three levels (a third each, from each level's floor centroids), grouped by level and shuffled.  Next to each, the test-side
restatement of the set (tests/worldset_ref.py) on the same host threads.

    python tools/player_step_cost.py [--steps K] [--warmup W] [--ticks T] [--game] [--set]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--ticks', type=int, default=60)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--game', action='store_true')
    ap.add_argument('--set', action='store_true')
    a = ap.parse_args()
    if a.set:
        return _set_main(a)
    import numpy as np
    import torch

    import rust_doom_amd as rd
    import world_ref
    from test_gpu_world import _players, _script
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    rows = []
    for label, path in (('E1M1', ensure_wad()), ('10x', ensure_big_wad())):
        wad = rd.Wad(path, META_PATH)
        built = wad.build_level(0)
        world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
        for n in (4096, 65536):
            st = _players(built, n, seed=n)
            inp = _script(n, a.ticks, seed=n)
            s0 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
            i_dev = torch.from_numpy(np.ascontiguousarray(inp).view(np.uint8).copy()).cuda()
            times = []
            for k in range(a.warmup + a.steps):
                s_dev = s0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                world.step(s_dev, i_dev, n_ticks=a.ticks)
                torch.cuda.synchronize()
                if k >= a.warmup:
                    times.append(time.perf_counter() - t0)
            gpu = float(np.median(times))
            t0 = time.perf_counter()
            want = ref.step(st, inp, threads=a.threads)
            cpu = time.perf_counter() - t0
            same = bool(np.array_equal(s_dev.cpu().numpy(), np.ascontiguousarray(want).view(np.uint8)))
            pt = n * a.ticks
            row = dict(level=label, players=n, ticks=a.ticks, gpu_us_per_player_tick=gpu * 1e6 / pt,
                       cpu_us_per_player_tick=cpu * 1e6 / pt, cpu_threads=a.threads, gpu_ms=gpu * 1e3, cpu_ms=cpu * 1e3, bit_exact=same)
            if a.game:
                row.update(_game(a, world, ref, st, inp, s0, i_dev, n))
            rows.append(row)
    print('%-6s %8s %6s %14s %14s %8s %6s' % ('level', 'players', 'ticks', 'GPU us/p-tick', 'CPU us/p-tick', 'speedup', 'exact'))
    for r in rows:
        print('%-6s %8d %6d %14.4f %14.4f %8.1f %6s' % (r['level'], r['players'], r['ticks'], r['gpu_us_per_player_tick'],
                                                       r['cpu_us_per_player_tick'], r['cpu_us_per_player_tick'] / r['gpu_us_per_player_tick'],
                                                       r['bit_exact']))
    if a.game:
        print('%-6s %8s %6s %14s %14s %10s %6s' % ('level', 'players', 'ticks', 'game us/p-t', 'CPU us/p-t', 'game/plain', 'exact'))
        for r in rows:
            print('%-6s %8d %6d %14.4f %14.4f %10.2f %6s' % (r['level'], r['players'], r['ticks'], r['game_gpu_us_per_player_tick'],
                                                            r['game_cpu_us_per_player_tick'],
                                                            r['game_gpu_us_per_player_tick'] / r['gpu_us_per_player_tick'], r['game_bit_exact']))
    for r in rows:
        print(json.dumps(r))


def _game(a, world, ref, st, inp, s0, i_dev, n):
    import numpy as np
    import torch

    import game_ref
    act = (np.random.default_rng(n + 1).random((a.ticks, n)) < 0.05).astype(np.uint8)  # ACTION_PUSH on ~5 % of the ticks
    a_dev = torch.from_numpy(act.reshape(-1).copy()).cuda()
    game, offs = world.game_state(n)
    times = []
    for k in range(a.warmup + a.steps):
        s_dev = s0.clone()
        world.reset_game(game, offs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        world.step_game(s_dev, i_dev, game, offs, actions=a_dev, n_ticks=a.ticks)
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
    gpu = float(np.median(times))
    t = world.triggers()
    rg = game_ref.RefGame(ref, t['triggers'], t['effects'], n, world.game_objects)
    t0 = time.perf_counter()
    want = rg.step(st, inp, act, threads=a.threads)
    cpu = time.perf_counter() - t0
    same = bool(np.array_equal(s_dev.cpu().numpy(), np.ascontiguousarray(want).view(np.uint8))) and \
        bool(np.array_equal(offs.cpu().numpy(), rg.offsets))
    pt = n * a.ticks
    return dict(game_gpu_us_per_player_tick=gpu * 1e6 / pt, game_cpu_us_per_player_tick=cpu * 1e6 / pt, game_gpu_ms=gpu * 1e3,
                game_cpu_ms=cpu * 1e3, game_bit_exact=same, triggers=len(t['triggers']))


def _timed(a, launch, reset):
    import numpy as np
    import torch
    times = []
    for k in range(a.warmup + a.steps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
    return float(np.median(times))


def _set_main(a):
    import numpy as np
    import torch

    import rust_doom_amd as rd
    import worldset_ref
    from test_gpu_world import _players, _script
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    slots = [0, 1, 2]
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = [wad.build_level(i) for i in slots]
    ws, world = wad.build_world_set(slots), wad.build_world(0)
    rows = []
    for n in (4096, 65536):
        inp = _script(n, a.ticks, seed=n)
        act = (np.random.default_rng(n + 1).random((a.ticks, n)) < 0.05).astype(np.uint8)
        i_dev = torch.from_numpy(np.ascontiguousarray(inp).view(np.uint8).copy()).cuda()
        a_dev = torch.from_numpy(act.reshape(-1).copy()).cuda()
        rng = np.random.default_rng(n + 2)
        mixed_lv = rng.integers(0, 3, n)
        mixed_st = np.zeros(n, rd.PLAYER_STATE)
        for k in range(3):
            sel = np.nonzero(mixed_lv == k)[0]
            mixed_st[sel] = _players(built[k], len(sel), seed=n + k)
        grouped = np.argsort(mixed_lv, kind='stable')
        cases = [('one level', _players(built[0], n, seed=n), np.zeros(n, np.int64)),
                 ('mixed, grouped', mixed_st[grouped], mixed_lv[grouped]), ('mixed, shuffled', mixed_st, mixed_lv)]
        for label, st, lv in cases:
            s0 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
            game, offs, levels = ws.game_state(lv)
            l0 = levels.clone()
            box = {}

            def reset():
                box['s'] = s0.clone()
                levels.copy_(l0)
                ws.reset_game(game, offs, levels)

            gpu = _timed(a, lambda: ws.step_game(box['s'], i_dev, game, offs, levels, actions=a_dev, n_ticks=a.ticks), reset)
            ref = worldset_ref.RefWorldSet(ensure_wad(), META_PATH, slots, lv)
            t0 = time.perf_counter()
            want = ref.step(st, inp, act, threads=a.threads)
            cpu = time.perf_counter() - t0
            same = bool(np.array_equal(box['s'].cpu().numpy(), np.ascontiguousarray(want).view(np.uint8))) and \
                bool(np.array_equal(offs.cpu().numpy(), ref.offsets())) and levels.cpu().numpy().tolist() == ref.levels.tolist()
            pt = n * a.ticks
            row = dict(case=label, players=n, ticks=a.ticks, set_gpu_us_per_player_tick=gpu * 1e6 / pt, set_gpu_ms=gpu * 1e3,
                       cpu_us_per_player_tick=cpu * 1e6 / pt, cpu_threads=a.threads, bit_exact=same)
            if label == 'one level':
                wg, wo = world.game_state(n)
                box2 = {}

                def reset_world():
                    box2['s'] = s0.clone()
                    world.reset_game(wg, wo)

                one = _timed(a, lambda: world.step_game(box2['s'], i_dev, wg, wo, actions=a_dev, n_ticks=a.ticks), reset_world)
                row.update(game_gpu_us_per_player_tick=one * 1e6 / pt, game_gpu_ms=one * 1e3, set_over_game=gpu / one)
            rows.append(row)
    print('%-16s %8s %6s %14s %14s %10s %6s' % ('case', 'players', 'ticks', 'set us/p-t', 'CPU us/p-t', 'set/game', 'exact'))
    for r in rows:
        print('%-16s %8d %6d %14.4f %14.4f %10s %6s' % (r['case'], r['players'], r['ticks'], r['set_gpu_us_per_player_tick'],
                                                       r['cpu_us_per_player_tick'],
                                                       '%.3f' % r['set_over_game'] if 'set_over_game' in r else '-', r['bit_exact']))
    for r in rows:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
