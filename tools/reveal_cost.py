#!/usr/bin/env python3
"""What revealing the map costs (rdoom_world_reveal_lines): reveal_lines alone for 1024 players on E1M1
(World), on the E1M1..E1M3 world set and on the big level, with 64 rays over 1.6 rad and 256 rays over 2 pi, at ranges 10 and 40,
timed with events on one stream -- the median of --steps launches after --warmup, each launch between its own pair of events.
Two sets of players: closed_loop_cost's (everyone at the level's start, random yaws) and players spread over the level's floor.
Each launch is timed twice: onto zeroed rows (every line in view is new: the first tick of an episode) and onto the rows it left
(nothing is new: a player who stands still).  Next to each time: draw_maps of the same players at 160 x 120 pixels and 0.12 units
per pixel, drawn through the set, and the wall time tools/closed_loop_cost.py reports for one device-path tick (step_game ->
render_players -> resolve_rgb) of the same number of players at 320x200 with the reveal's share of it (the big level has no such
tick: its columns are empty).  Prints a table and one JSON line per row (--out appends them to a file).  Needs the GPU and torch.

    python tools/reveal_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

FANS = ((64, 1.6), (256, 6.283185307179586))
RANGES = (10.0, 40.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--tick-ticks', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import closed_loop_cost
    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    n = a.players
    stream = torch.cuda.Stream()
    rows = []
    for scenario, path, slots in (('E1M1', ensure_wad(), [0]), ('E1M1-E1M3', ensure_wad(), [0, 1, 2]), ('big', ensure_big_wad(), [0])):
        wad = rd.Wad(path, META_PATH)
        tick_ms = closed_loop_cost.run(scenario, n, 320, 200, a.tick_ticks, 'device', min(n, 4096))[0] if scenario != 'big' else None
        built = [wad.build_level(i) for i in slots]
        rng = np.random.default_rng(n)
        lv = rng.integers(0, len(slots), n)
        if len(slots) == 1:
            world = wad.build_world(0)
            _, offs = world.game_state(n)
            levels = ()
        else:
            world = wad.build_world_set(slots)
            _, offs, lv_t = world.game_state(lv)
            levels = (lv_t,)
        n_lines = max(len(world.map_lines(*((s,) if levels else ()))) for s in range(len(slots)))
        for who in ('start', 'spread'):
            if who == 'start':  # closed_loop_cost's players
                pos, yaw = np.array([b.start()[0] for b in built], np.float32)[lv], np.array([b.start()[1] for b in built], np.float32)[lv]
                st = rd.player_states(pos, yaw + rng.normal(size=n).astype(np.float32))
            else:
                per = [rays_ref.players(b, 100 + s, count=n) for s, b in enumerate(built)]
                st = np.array([per[lv[p]][p] for p in range(n)], rd.PLAYER_STATE)
            states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
            seen = torch.zeros((n, world.seen_words()), dtype=torch.int32, device='cuda')
            new = torch.zeros(n, dtype=torch.int32, device='cuda')
            maps = torch.empty((n, 120, 160), dtype=torch.uint8, device='cuda')
            for rays, fov in FANS:
                fan = torch.from_numpy(rd.map_fan(rays, fov)).cuda()
                for max_range in RANGES:
                    def first():
                        seen.zero_()
                        world.reveal_lines(states, *levels, fan, max_range, offsets=offs, seen=seen, new_out=new, stream=stream)
                    zero_ms = _event_ms(lambda: seen.zero_(), stream, a.warmup, a.steps)[0]
                    first_ms = _event_ms(first, stream, a.warmup, a.steps)[0] - zero_ms
                    lines_seen = float(new.float().mean().item())
                    again = _event_ms(lambda: world.reveal_lines(states, *levels, fan, max_range, offsets=offs, seen=seen, new_out=new,
                                                                 stream=stream), stream, a.warmup, a.steps)
                    draw = _event_ms(lambda: world.draw_maps(states, *levels, 160, 120, 0.12, offsets=offs, out=maps, stream=stream,
                                                             seen=seen), stream, a.warmup, a.steps)
                    rows.append(dict(levels=scenario, lines=n_lines, players=n, who=who, rays=rays, fov=round(fov, 3), max_range=max_range,
                                     reveal_first_ms=first_ms, reveal_again_ms=again[0], reveal_again_ms_min=again[1],
                                     reveal_again_ms_max=again[2], lines_seen=lines_seen, draw_seen_160x120_ms=draw[0],
                                     tick_320x200_ms=tick_ms, share_of_tick=(first_ms / tick_ms if tick_ms else None)))
    print('%-10s %6s %-6s %5s %6s %10s %10s %11s %10s %14s %8s' % ('levels', 'lines', 'who', 'rays', 'range', 'first ms', 'again ms',
                                                                   'lines seen', 'draw ms', 'tick ms (320)', 'share'))
    for r in rows:
        tick = ('%14.3f %8.4f' % (r['tick_320x200_ms'], r['share_of_tick'])) if r['tick_320x200_ms'] else '%14s %8s' % ('', '')
        print('%-10s %6d %-6s %5d %6.0f %10.4f %10.4f %11.1f %10.4f %s' % (r['levels'], r['lines'], r['who'], r['rays'], r['max_range'],
                                                                          r['reveal_first_ms'], r['reveal_again_ms'], r['lines_seen'],
                                                                          r['draw_seen_160x120_ms'], tick))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
