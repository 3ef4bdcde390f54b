#!/usr/bin/env python3
"""What a top-down map costs (rdoom_world_draw_maps): draw_maps alone for 1024 players on E1M1 (World) and on
the E1M1..E1M3 world set, 160x120 and 320x200 pixels at 0.05 and 0.30 world units per pixel, timed with events on one stream --
the median of --steps launches after --warmup, each launch between its own pair of events.  Two sets of players: closed_loop_cost's
(everyone at the level's start, random yaws) and players spread over the level's floor (random centroids).  Next to each time, the
wall time tools/closed_loop_cost.py reports for one device-path tick (step_game -> render_players -> resolve_rgb) of the same
number of players at 320x200, and the map's share of it.  Prints a table and one JSON line per row (--out appends them to a
file).  Needs the GPU and torch.

    python tools/automap_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _event_ms(fn, stream, warmup, steps):
    import numpy as np
    import torch
    times = []
    with torch.cuda.stream(stream):
        for k in range(warmup + steps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            fn()
            end.record(stream)
            end.synchronize()
            if k >= warmup:
                times.append(start.elapsed_time(end))
    return float(np.median(times)), float(min(times)), float(max(times))


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
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    n = a.players
    wad = rd.Wad(ensure_wad(), META_PATH)
    stream = torch.cuda.Stream()
    rows = []
    for scenario, slots in (('E1M1', [0]), ('E1M1-E1M3', [0, 1, 2])):
        tick_ms, _ = closed_loop_cost.run(scenario, n, 320, 200, a.tick_ticks, 'device', min(n, 4096))
        built = [wad.build_level(i) for i in slots]
        rng = np.random.default_rng(n)
        lv = rng.integers(0, len(slots), n)
        if len(slots) == 1:
            world = wad.build_world(0)
            _, offs = world.game_state(n)
            levels = None
        else:
            world = wad.build_world_set(slots)
            _, offs, levels = world.game_state(lv)
        for who in ('start', 'spread'):
            if who == 'start':  # closed_loop_cost's players
                pos, yaw = np.array([b.start()[0] for b in built], np.float32)[lv], np.array([b.start()[1] for b in built], np.float32)[lv]
                st = rd.player_states(pos, yaw + rng.normal(size=n).astype(np.float32))
            else:
                per = [rays_ref.players(b, 100 + s, count=n) for s, b in enumerate(built)]
                st = np.array([per[lv[p]][p] for p in range(n)], rd.PLAYER_STATE)
            states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
            for w, h in ((160, 120), (320, 200)):
                out = torch.empty((n, h, w), dtype=torch.uint8, device='cuda')
                for scale in (0.05, 0.30):
                    if levels is None:
                        fn = lambda: world.draw_maps(states, w, h, scale, offsets=offs, out=out, stream=stream)
                    else:
                        fn = lambda: world.draw_maps(states, levels, w, h, scale, offsets=offs, out=out, stream=stream)
                    med, lo, hi = _event_ms(fn, stream, a.warmup, a.steps)
                    rows.append(dict(levels=scenario, players=n, who=who, width=w, height=h, scale=scale, draw_ms=med, draw_ms_min=lo,
                                     draw_ms_max=hi, ns_per_pixel=med * 1e6 / (n * w * h), line_pixels=float((out != 0).float().mean().item()),
                                     tick_320x200_ms=tick_ms, share_of_tick=med / tick_ms))
    print('%-10s %7s %-6s %9s %6s %10s %10s %12s %14s %8s' % ('levels', 'players', 'who', 'map', 'scale', 'draw ms', 'ns/pixel', 'drawn share',
                                                              'tick ms (320)', 'share'))
    for r in rows:
        print('%-10s %7d %-6s %9s %6.2f %10.4f %10.4f %12.3f %14.3f %8.4f' % (r['levels'], r['players'], r['who'], '%dx%d' % (r['width'], r['height']),
                                                                             r['scale'], r['draw_ms'], r['ns_per_pixel'], r['line_pixels'],
                                                                             r['tick_320x200_ms'], r['share_of_tick']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
