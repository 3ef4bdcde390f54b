#!/usr/bin/env python3
"""What locating players and drawing filled sector maps costs (rdoom_world_locate_players, rdoom_world_draw_sector_maps, DESIGN
section 18): each alone for 1024 players on E1M1 (World), on the E1M1..E1M3 world set and on the big level, maps of 160 x 120 and
320 x 200 pixels at 0.05 and 0.30 units per pixel with all three planes, timed with events on one stream -- the median of --steps
launches after --warmup, each launch between its own pair of events.  Players are spread over the level's floor.  Next to each
time: draw_maps of the same view, and the wall time tools/closed_loop_cost.py reports for one device-path tick (step_game ->
render_players -> resolve_rgb) of the same number of players at 320x200 (the big level has no such tick: its column is empty).
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/sector_cost.jsonl).  Needs the GPU and torch.

    python tools/sector_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((160, 120), (320, 200))
SCALES = (0.05, 0.30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--tick-ticks', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sector_cost.jsonl'))
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
        n_sectors = max(len(world.map_sectors(*((s,) if levels else ())).sectors) for s in range(len(slots)))
        per = [rays_ref.players(b, 100 + s, count=n) for s, b in enumerate(built)]
        st = np.array([per[lv[p]][p] for p in range(n)], rd.PLAYER_STATE)
        states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        visited = torch.zeros((n, world.visited_words()), dtype=torch.int32, device='cuda')
        new = torch.zeros(n, dtype=torch.int32, device='cuda')
        where = torch.zeros(n, dtype=torch.int32, device='cuda')
        heights = torch.zeros((n, 2), dtype=torch.float32, device='cuda')
        locate = _event_ms(lambda: world.locate_players(states, *levels, offsets=offs, heights_out=heights, visited=visited, new_out=new,
                                                        out=where, stream=stream), stream, a.warmup, a.steps)
        for width, height in SIZES:
            sec = torch.empty((n, height, width), dtype=torch.int16, device='cuda')
            floor = torch.empty((n, height, width), dtype=torch.float32, device='cuda')
            ceil = torch.empty((n, height, width), dtype=torch.float32, device='cuda')
            maps = torch.empty((n, height, width), dtype=torch.uint8, device='cuda')
            for scale in SCALES:
                kw = dict(offsets=offs, rotate=True, top_down=True, stream=stream)
                planes = _event_ms(lambda: world.draw_sector_maps(states, *levels, width, height, scale, sector_out=sec, floor=floor,
                                                                  ceiling=ceil, **kw), stream, a.warmup, a.steps)
                alone = _event_ms(lambda: world.draw_sector_maps(states, *levels, width, height, scale, sector_out=sec, **kw), stream,
                                  a.warmup, a.steps)
                through = _event_ms(lambda: world.draw_sector_maps(states, *levels, width, height, scale, sector_out=sec, visited=visited,
                                                                   **kw), stream, a.warmup, a.steps)
                lines = _event_ms(lambda: world.draw_maps(states, *levels, width, height, scale, out=maps, **kw), stream, a.warmup, a.steps)
                rows.append(dict(levels=scenario, sectors=n_sectors, players=n, width=width, height=height, scale=scale,
                                 locate_ms=locate[0], locate_ms_min=locate[1], locate_ms_max=locate[2], sector_maps_3_planes_ms=planes[0],
                                 sector_maps_3_planes_ms_min=planes[1], sector_maps_3_planes_ms_max=planes[2], sector_plane_ms=alone[0],
                                 sector_plane_visited_ms=through[0], draw_maps_ms=lines[0], tick_320x200_ms=tick_ms))
    print('%-10s %7s %9s %6s %10s %11s %10s %11s %10s %14s' % ('levels', 'sectors', 'view', 'scale', 'locate ms', '3 planes ms', 'sector ms',
                                                              'visited ms', 'lines ms', 'tick ms (320)'))
    for r in rows:
        print('%-10s %7d %9s %6.2f %10.4f %11.4f %10.4f %11.4f %10.4f %14s' % (
            r['levels'], r['sectors'], '%dx%d' % (r['width'], r['height']), r['scale'], r['locate_ms'], r['sector_maps_3_planes_ms'],
            r['sector_plane_ms'], r['sector_plane_visited_ms'], r['draw_maps_ms'], '%.3f' % r['tick_320x200_ms'] if r['tick_320x200_ms'] else ''))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
