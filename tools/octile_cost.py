#!/usr/bin/env python3
"""What the octile distance costs: flood_grids_octile and descend_grids_octile next to flood_grids and
descend_grids on the same planes and seeds in the same run, for tools/goal_cost.py's configurations -- 1024 rows of E1M1 at cell 0.25,
fewer rows at 0.125 and on the big level at 0.125, each row seeded at the cell of a player spread over the level's floor, TOWARDS it;
the walks start at the next row's player, 8 moves (the README's tick) and the whole way.  And the diagonal phases on their own: a
band of open cells three wide along the main diagonal of a 300 x 300 and a 600 x 600 grid, next to a straight corridor three wide
along the middle rows of the same grids, each flooded from one end -- if the band's time grew faster with its length than the
corridor's, the diagonal phases would be relaxing a move a pass.  Every launch is timed with a pair of events on one stream, the
median of --steps launches after --warmup.  Before anything is timed, row 0 of every configuration is checked against
tests/octile_ref.py's Dijkstra and its descent.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/octile_cost.jsonl).  Needs the GPU and torch.

    python tools/octile_cost.py [--rows 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

# (level, cell, rows as a fraction of --rows): tools/goal_cost.py's
CONFIGS = (('E1M1', 0.25, 1.0), ('E1M1', 0.125, 0.25), ('big', 0.125, 1.0 / 32))
MAX_STEP = 0.32  # the synthetic levels join most of their sectors by steps of 0.32
BAND_ROWS = 16   # grids a launch of the band and the corridor
AHEAD = 8        # the README's waypoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'octile_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import flood_ref
    import octile_ref
    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    time = lambda fn: _event_ms(fn, stream, a.warmup, a.steps)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')
    wads = {'E1M1': rd.Wad(ensure_wad(), META_PATH), 'big': rd.Wad(ensure_big_wad(), META_PATH)}
    rows = []
    for level, cell, share in CONFIGS:
        n = max(4, int(a.rows * share))
        wad = wads[level]
        world = wad.build_world(0)
        st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
        states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        height, width = world.area_plane_shape(cell)
        floor, ceiling = world.draw_area_planes(cell, n=n, floor=True, ceiling=True)
        cells = world.area_cells(states, cell)
        starts = torch.roll(cells, -1, 0).contiguous()  # the next row's player: the planes are one level's, at rest
        four, eight, count = i32(n, height, width), i32(n, height, width), i32(n)
        at, made = i32(n, 2), i32(n)
        kw = dict(towards=True, max_step=MAX_STEP, stream=stream)
        flood4 = lambda: rd.flood_grids(floor, ceiling, cells, dist_out=four, count_out=count, **kw)
        flood8 = lambda: rd.flood_grids_octile(floor, ceiling, cells, dist_out=eight, count_out=count, **kw)
        walk4 = lambda m=None: rd.descend_grids(floor, ceiling, four, starts, max_moves=m, cells_out=at, moves_out=made, **kw)
        walk8 = lambda m=None: rd.descend_grids_octile(floor, ceiling, eight, starts, max_moves=m, cells_out=at, moves_out=made, **kw)
        with torch.cuda.stream(stream):
            flood4(), flood8(), walk8()
        stream.synchronize()
        # the checks: row 0 against the Dijkstra and its descent
        f0, c0, s0 = floor[0].cpu().numpy(), ceiling[0].cpu().numpy(), cells[0].cpu().numpy()
        want = octile_ref.flood(f0, c0, s0, True, max_step=MAX_STEP)
        if not np.array_equal(eight[0].cpu().numpy().view(np.uint32), want):
            raise SystemExit('%s at %g: the kernel and the Dijkstra differ' % (level, cell))
        cell0, moves0, _ = octile_ref.descend(f0, c0, want, starts[0].cpu().numpy(), True, max_step=MAX_STEP)
        if at[0].cpu().tolist() != list(cell0) or int(made[0].item()) != moves0:
            raise SystemExit('%s at %g: the walk and its reference differ' % (level, cell))
        moves8 = made.cpu().numpy().view(np.uint32).copy()
        r = dict(level=level, cell=cell, rows=n, width=width, height=height, cells=width * height, max_step=MAX_STEP)
        flood4_ms, flood8_ms = time(flood4), time(flood8)
        ahead4_ms, ahead8_ms = time(lambda: walk4(AHEAD)), time(lambda: walk8(AHEAD))
        whole8_ms, whole4_ms = time(walk8), time(walk4)
        moves4 = made.cpu().numpy().view(np.uint32)  # (walk4 ran last)
        reached = eight >= 0
        r.update(flood_grids_ms=flood4_ms[0], flood_grids_octile_ms=flood8_ms[0], flood_grids_octile_ms_min=flood8_ms[1],
                 flood_grids_octile_ms_max=flood8_ms[2], octile_over_flood_grids=flood8_ms[0] / flood4_ms[0],
                 descend_8_moves_ms=ahead4_ms[0], descend_octile_8_moves_ms=ahead8_ms[0], descend_ms=whole4_ms[0], descend_octile_ms=whole8_ms[0],
                 octile_over_descend_8_moves=ahead8_ms[0] / ahead4_ms[0], octile_over_descend=whole8_ms[0] / whole4_ms[0],
                 moves_mean=float(moves4.mean()), moves_octile_mean=float(moves8.mean()), moves_octile_max=int(moves8.max()),
                 cells_reached_mean=float(reached.reshape(n, -1).sum(1).float().mean().item()),
                 # the walk's length in cells by either metric, over the cells both reach: what the diagonals take off it
                 octile_length_over_moves=float((eight[reached].double().sum() / 5 / four[reached].double().sum().clamp(min=1)).item()))
        rows.append(r)
        del floor, ceiling, four, eight
    # the band and the corridor
    bands = []
    for length in (300, 600):
        for shape in ('band', 'corridor'):
            if shape == 'band':
                f, g = octile_ref.band(length)
            else:
                f, g = flood_ref.room(length, length, np.inf, -np.inf)
                f[length // 2 - 1:length // 2 + 2], g[length // 2 - 1:length // 2 + 2] = 0, 1
            seed = (0, 0) if shape == 'band' else (0, length // 2)
            want = octile_ref.flood(f, g, seed)
            floor = torch.from_numpy(np.repeat(f[None], BAND_ROWS, 0)).cuda()
            ceiling = torch.from_numpy(np.repeat(g[None], BAND_ROWS, 0)).cuda()
            seeds = torch.tensor([seed] * BAND_ROWS, dtype=torch.int32, device='cuda')
            four, eight = i32(BAND_ROWS, length, length), i32(BAND_ROWS, length, length)
            flood4 = lambda: rd.flood_grids(floor, ceiling, seeds, dist_out=four, stream=stream)
            flood8 = lambda: rd.flood_grids_octile(floor, ceiling, seeds, dist_out=eight, stream=stream)
            with torch.cuda.stream(stream):
                flood8()
            stream.synchronize()
            if not np.array_equal(eight[0].cpu().numpy().view(np.uint32), want):
                raise SystemExit('the %s of %d: the kernel and the Dijkstra differ' % (shape, length))
            flood4_ms, flood8_ms = time(flood4), time(flood8)
            bands.append(dict(shape=shape, length=length, rows=BAND_ROWS, width=length, height=length, farthest=int(want[want != octile_ref.UNREACHED].max()),
                              flood_grids_ms=flood4_ms[0], flood_grids_octile_ms=flood8_ms[0], flood_grids_octile_ms_min=flood8_ms[1],
                              flood_grids_octile_ms_max=flood8_ms[2]))
    by = {(b['shape'], b['length']): b['flood_grids_octile_ms'] for b in bands}
    growth = dict(band_600_over_300=by[('band', 600)] / by[('band', 300)], corridor_600_over_300=by[('corridor', 600)] / by[('corridor', 300)])
    growth['band_growth_over_corridor_growth'] = growth['band_600_over_300'] / growth['corridor_600_over_300']
    print('%-5s %6s %5s %11s %9s %10s %6s %9s %10s %9s %10s' % ('level', 'cell', 'rows', 'grid', 'flood ms', 'octile ms', 'ratio', 'walk8 ms',
                                                               'octile ms', 'walk ms', 'octile ms'))
    for r in rows:
        print('%-5s %6.4f %5d %11s %9.3f %10.3f %6.2f %9.4f %10.4f %9.4f %10.4f' % (
            r['level'], r['cell'], r['rows'], '%dx%d' % (r['width'], r['height']), r['flood_grids_ms'], r['flood_grids_octile_ms'],
            r['octile_over_flood_grids'], r['descend_8_moves_ms'], r['descend_octile_8_moves_ms'], r['descend_ms'], r['descend_octile_ms']))
    for b in bands:
        print('%-8s %4d: flood_grids %.3f ms, flood_grids_octile %.3f ms' % (b['shape'], b['length'], b['flood_grids_ms'], b['flood_grids_octile_ms']))
    print(json.dumps(growth))
    records = rows + bands + [dict(growth, what='the octile flood, 600 against 300 cells')]
    for r in records:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in records:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
