#!/usr/bin/env python3
"""What the walking distance to a goal costs: draw_area_planes (floor and ceiling) and flood_grids, forwards and
TOWARDS, for 1024 rows of E1M1 at cell 0.25 and for fewer rows at 0.125 and on the big level at 0.125, each row seeded at the cell of
a player spread over the level's floor; timed with a pair of events around each launch on one stream -- the median of --steps launches
after --warmup.  In the same run, on the 0.25 planes, which fit it: flood_maps, and what a user had before -- tools/flood_cost.py's
torch flood, here from the rows' seeds.  And the per-tick read: area_cells plus the gather from the field, next to locate_players.
Before anything is timed the kernel's distances are checked equal to the others': to flood_maps and the torch flood on the 0.25 planes,
and row 0 of every configuration, in both directions, to tests/goal_ref.py's breadth-first search.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/goal_cost.jsonl).  Needs the GPU and torch.

    python tools/goal_cost.py [--rows 1024] [--steps 20] [--warmup 3] [--torch-steps 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

# (level, cell, rows as a fraction of --rows)
CONFIGS = (('E1M1', 0.25, 1.0), ('E1M1', 0.125, 0.25), ('big', 0.125, 1.0 / 32))
MAX_STEP = 0.32  # the synthetic levels join most of their sectors by steps of 0.32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'goal_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import goal_ref
    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from flood_cost import torch_flood
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wads = {'E1M1': rd.Wad(ensure_wad(), META_PATH), 'big': rd.Wad(ensure_big_wad(), META_PATH)}
    rows = []
    for level, cell, share in CONFIGS:
        n = max(4, int(a.rows * share))
        wad = wads[level]
        world = wad.build_world(0)
        st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
        states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        height, width = world.area_plane_shape(cell)
        floor = torch.empty((n, height, width), dtype=torch.float32, device='cuda')
        ceiling = torch.empty_like(floor)
        dist = torch.empty((n, height, width), dtype=torch.int32, device='cuda')
        back = torch.empty_like(dist)
        count = torch.empty(n, dtype=torch.int32, device='cuda')
        cells = torch.empty((n, 2), dtype=torch.int32, device='cuda')
        draw = lambda: world.draw_area_planes(cell, n=n, floor=floor, ceiling=ceiling, stream=stream)
        locate = lambda: world.area_cells(states, cell, out=cells, stream=stream)
        flood = lambda: rd.flood_grids(floor, ceiling, cells, max_step=MAX_STEP, dist_out=dist, count_out=count, stream=stream)
        towards = lambda: rd.flood_grids(floor, ceiling, cells, towards=True, max_step=MAX_STEP, dist_out=back, count_out=count, stream=stream)
        with torch.cuda.stream(stream):
            draw(), locate(), flood(), towards()
        stream.synchronize()
        # the checks: row 0 against the search in both directions; at 0.25 every row against flood_maps and the torch flood
        f0, c0, s0 = floor[0].cpu().numpy(), ceiling[0].cpu().numpy(), cells[0].cpu().numpy()
        for got, way in ((dist, False), (back, True)):
            if not np.array_equal(got[0].cpu().numpy().view(np.uint32), goal_ref.flood(f0, c0, s0, way, max_step=MAX_STEP)):
                raise SystemExit('%s at %g: the kernel and the search differ (towards=%s)' % (level, cell, way))
        r = dict(level=level, cell=cell, rows=n, width=width, height=height, cells=width * height, max_step=MAX_STEP)
        if width * height <= rd.flood_max_cells():
            maps = rd.flood_maps(floor, ceiling, cells, max_step=MAX_STEP).to(torch.int32)
            if not torch.equal(torch.where(maps == rd.FLOOD_UNREACHED, -1, maps), dist):
                raise SystemExit('%s at %g: flood_grids and flood_maps differ' % (level, cell))
            want, iterations = torch_flood(floor, ceiling, cells, unreached=-1, max_step=MAX_STEP)
            if not torch.equal(want, dist):
                raise SystemExit('%s at %g: the torch flood and the kernel differ in %d cells' % (level, cell, int((want != dist).sum())))
            d16 = torch.empty((n, height, width), dtype=torch.uint16, device='cuda')
            maps_ms = _event_ms(lambda: rd.flood_maps(floor, ceiling, cells, max_step=MAX_STEP, dist_out=d16, stream=stream), stream, a.warmup, a.steps)
            torch_ms = _event_ms(lambda: torch_flood(floor, ceiling, cells, unreached=-1, max_step=MAX_STEP), torch.cuda.current_stream(), 1, a.torch_steps)
            r.update(flood_maps_ms=maps_ms[0], torch_flood_ms=torch_ms[0], torch_iterations=iterations)
        draw_ms = _event_ms(draw, stream, a.warmup, a.steps)
        flood_ms = _event_ms(flood, stream, a.warmup, a.steps)
        towards_ms = _event_ms(towards, stream, a.warmup, a.steps)
        # the tick: the players' cells and the gather from the field, negative cells mapped to unreached; next to it locate_players
        sector = torch.empty(n, dtype=torch.int32, device='cuda')
        rows_of = torch.arange(n, device='cuda')

        def read():
            locate()
            ok = (cells >= 0).all(1)
            return torch.where(ok, back[rows_of, cells[:, 1].clamp(min=0).long(), cells[:, 0].clamp(min=0).long()], -1)
        read_ms = _event_ms(read, stream, a.warmup, a.steps)
        cells_ms = _event_ms(locate, stream, a.warmup, a.steps)
        locate_ms = _event_ms(lambda: world.locate_players(states, out=sector, stream=stream), stream, a.warmup, a.steps)
        reached = count.cpu().numpy().view(np.uint32)
        far = back[back >= 0]
        r.update(draw_area_planes_2_planes_ms=draw_ms[0], flood_grids_ms=flood_ms[0], flood_grids_ms_min=flood_ms[1], flood_grids_ms_max=flood_ms[2],
                 flood_grids_towards_ms=towards_ms[0], flood_grids_ms_per_row=flood_ms[0] / n, flood_grids_towards_ms_per_row=towards_ms[0] / n,
                 area_cells_ms=cells_ms[0], area_cells_and_gather_ms=read_ms[0], locate_players_ms=locate_ms[0],
                 longest_distance=int(far.max().item()) if far.numel() else 0, cells_reached_mean=float(reached.mean()))
        if 'flood_maps_ms' in r:
            r['flood_grids_over_flood_maps'] = r['flood_grids_ms'] / r['flood_maps_ms']
        rows.append(r)
        del floor, ceiling, dist, back
    print('%-5s %6s %5s %11s %9s %9s %10s %9s %9s %9s %9s' % ('level', 'cell', 'rows', 'grid', 'planes ms', 'flood ms', 'towards ms', 'maps ms',
                                                                'torch ms', 'cells ms', 'locate ms'))
    for r in rows:
        print('%-5s %6.4f %5d %11s %9.4f %9.3f %10.3f %9s %9s %9.4f %9.4f' % (
            r['level'], r['cell'], r['rows'], '%dx%d' % (r['width'], r['height']), r['draw_area_planes_2_planes_ms'], r['flood_grids_ms'],
            r['flood_grids_towards_ms'], '%.3f' % r['flood_maps_ms'] if 'flood_maps_ms' in r else '-',
            '%.1f' % r['torch_flood_ms'] if 'torch_flood_ms' in r else '-', r['area_cells_ms'], r['locate_players_ms']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
