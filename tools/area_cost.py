#!/usr/bin/env python3
"""What keeping the explored area costs (rdoom_world_reveal_area): reveal_area alone for 1024 players spread over
the floor of E1M1 (World), of the E1M1..E1M3 world set and of the big level, with 64 rays over 1.6 rad at range 12 and 256 rays over
2 pi at range 40, at cells 0.25 and 0.0625 (n_steps = area_steps: half a cell between samples), timed with events on one stream --
the median of --steps launches after --warmup, each launch between its own pair of events.  Each launch is timed twice: onto zeroed
rows (every cell in sight is new: the first tick of an episode) and onto the rows it left (nothing is new: a player who stands
still).  Next to each time: the bands the kernel's window formula gives the players (mean and most), the cells marked,
draw_area_maps, reveal_lines and draw_maps of the same players and fan (maps of 160 x 120 pixels at 0.12 units per pixel), and the
wall time tools/closed_loop_cost.py reports for one device-path tick (step_game -> render_players -> resolve_rgb) of the same
number of players at 320x200 with the reveal's share of it (the big level has no such tick: its columns are empty).  Prints a table
and one JSON line per row (--out appends them to a file).  Needs the GPU and torch.

    python tools/area_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

FANS = ((64, 1.6, 12.0), (256, 6.283185307179586, 40.0))
CELLS = (0.25, 0.0625)


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

    import area_ref
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
        per = [rays_ref.players(b, 100 + s, count=n) for s, b in enumerate(built)]
        st = np.array([per[lv[p]][p] for p in range(n)], rd.PLAYER_STATE)
        states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        seen = torch.zeros((n, world.seen_words()), dtype=torch.int32, device='cuda')
        maps = torch.empty((n, 120, 160), dtype=torch.uint8, device='cuda')
        for rays, fov, max_range in FANS:
            fan_np = rd.map_fan(rays, fov)
            fan = torch.from_numpy(fan_np).cuda()
            lines_ms = _event_ms(lambda: world.reveal_lines(states, *levels, fan, max_range, offsets=offs, seen=seen, stream=stream), stream,
                                 a.warmup, a.steps)[0]
            draw_lines_ms = _event_ms(lambda: world.draw_maps(states, *levels, 160, 120, 0.12, offsets=offs, out=maps, stream=stream), stream,
                                      a.warmup, a.steps)[0]
            for cell in CELLS:
                grids = [world.area_grid(*((s,) if levels else ()), cell) for s in range(len(slots))]
                bands = np.concatenate([area_ref.bands(g, cell, st[lv == s], fan_np, max_range) for s, g in enumerate(grids)])
                area = torch.zeros((n, 2, world.area_words(cell)), dtype=torch.int32, device='cuda')
                new = torch.zeros((n, 2), dtype=torch.int32, device='cuda')

                def first():
                    area.zero_()
                    world.reveal_area(states, *levels, fan, max_range, cell, offsets=offs, area=area, new_out=new, stream=stream)
                zero_ms = _event_ms(lambda: area.zero_(), stream, a.warmup, a.steps)[0]
                first_ms = _event_ms(first, stream, a.warmup, a.steps)[0] - zero_ms
                marked = new.float().mean(0).tolist()
                again = _event_ms(lambda: world.reveal_area(states, *levels, fan, max_range, cell, offsets=offs, area=area, new_out=new,
                                                            stream=stream), stream, a.warmup, a.steps)
                draw = _event_ms(lambda: world.draw_area_maps(states, *levels, 160, 120, 0.12, area, cell, out=maps, stream=stream), stream,
                                 a.warmup, a.steps)
                rows.append(dict(levels=scenario, players=n, rays=rays, fov=round(fov, 3), max_range=max_range, cell=cell,
                                 n_steps=rd.area_steps(max_range, cell), words=int(area.shape[2]), bands_mean=float(bands.mean()),
                                 bands_max=int(bands.max()), area_first_ms=first_ms, area_again_ms=again[0], area_again_ms_min=again[1],
                                 area_again_ms_max=again[2], free_cells=marked[0], wall_cells=marked[1], draw_area_160x120_ms=draw[0],
                                 reveal_lines_ms=lines_ms, draw_maps_160x120_ms=draw_lines_ms, tick_320x200_ms=tick_ms,
                                 share_of_tick=(first_ms / tick_ms if tick_ms else None)))
    print('%-10s %5s %6s %7s %6s %6s %10s %10s %9s %8s %9s %9s %9s %14s %8s' % ('levels', 'rays', 'range', 'cell', 'steps', 'bands', 'first ms',
                                                                                'again ms', 'free', 'wall', 'draw ms', 'lines ms', 'maps ms',
                                                                                'tick ms (320)', 'share'))
    for r in rows:
        tick = ('%14.3f %8.4f' % (r['tick_320x200_ms'], r['share_of_tick'])) if r['tick_320x200_ms'] else '%14s %8s' % ('', '')
        print('%-10s %5d %6.0f %7.4f %6d %6.2f %10.4f %10.4f %9.1f %8.1f %9.4f %9.4f %9.4f %s' % (
            r['levels'], r['rays'], r['max_range'], r['cell'], r['n_steps'], r['bands_mean'], r['area_first_ms'], r['area_again_ms'],
            r['free_cells'], r['wall_cells'], r['draw_area_160x120_ms'], r['reveal_lines_ms'], r['draw_maps_160x120_ms'], tick))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
