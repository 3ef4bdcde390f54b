#!/usr/bin/env python3
"""What resetting players on the device costs (rdoom_world_spawn_players): spawn_players for 1024 players of E1M1
and of the nine-level world set (players spread evenly over the slots), every player masked, default parameters, timed with a pair of
events around each launch on one stream -- the median of --steps launches after --warmup.  Next to it, in the same run, a
locate_players launch on the states the spawn left: one descent a player, where a spawn makes up to nine a try.  Prints a table and
one JSON line per row, and appends the rows to --out (default profiles/spawn_cost.jsonl).  Needs the GPU and torch.

    python tools/spawn_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spawn_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    n = a.players
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    states = torch.zeros(n * rd.PLAYER_STATE.itemsize, dtype=torch.uint8, device='cuda')
    tries = torch.zeros(n, dtype=torch.int32, device='cuda')
    sector = torch.zeros(n, dtype=torch.int32, device='cuda')
    rows = []
    world = wad.build_world(0)
    ws = wad.build_world_set(list(range(wad.num_levels())))
    slots = torch.from_numpy((np.arange(n) % ws.n_levels).astype(np.int32)).cuda()
    cases = (('E1M1', 1, lambda: world.spawn_players(states, 1993, tries_out=tries, stream=stream),
              lambda: world.locate_players(states, out=sector, stream=stream)),
             ('set of %d' % ws.n_levels, ws.n_levels, lambda: ws.spawn_players(states, slots, 1993, tries_out=tries, stream=stream),
              lambda: ws.locate_players(states, slots, out=sector, stream=stream)))
    for name, levels, spawn, locate in cases:
        spawn_ms = _event_ms(spawn, stream, a.warmup, a.steps)
        locate_ms = _event_ms(locate, stream, a.warmup, a.steps)
        torch.cuda.synchronize()
        t = tries.cpu().numpy()
        if (sector.cpu().numpy()[t > 0] == -1).any():
            raise SystemExit('a spawned player stands in no sector')
        rows.append(dict(level=name, levels=levels, players=n, spawn_ms=spawn_ms[0], spawn_ms_min=spawn_ms[1], spawn_ms_max=spawn_ms[2],
                         locate_players_ms=locate_ms[0], spawn_over_locate=spawn_ms[0] / locate_ms[0],
                         fallback_share=float((t == 0).mean()), tries_mean=float(t[t > 0].mean())))
    print('%-10s %8s %10s %10s %8s %9s %6s' % ('level', 'players', 'spawn ms', 'locate ms', 'ratio', 'fallback', 'tries'))
    for r in rows:
        print('%-10s %8d %10.4f %10.4f %8.2f %9.4f %6.2f' % (r['level'], r['players'], r['spawn_ms'], r['locate_players_ms'],
                                                            r['spawn_over_locate'], r['fallback_share'], r['tries_mean']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
