#!/usr/bin/env python3
"""What flooding every player's sector map costs (rdoom_flood_maps): flood_maps for 1024 players of E1M1 on the
planes draw_sector_maps drew of them, at 160 x 120 pixels and 0.12 units per pixel and at 77 x 53 and 0.30, timed with a pair of
events around each launch on one stream -- the median of --steps launches after --warmup.  Next to it, in the same run: the
draw_sector_maps launch (floor and ceiling) that feeds it, and what a user had before -- a straightforward torch flood on the same
planes, which masks and shifts the four ways, takes the minimum and iterates until torch.equal says nothing changed; its result
is checked equal to the kernel's before it is timed (--torch-steps times, it is slow).  Players are spread over the level's floor.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/flood_cost.jsonl).  Needs the GPU and torch.

    python tools/flood_cost.py [--players 1024] [--steps 20] [--warmup 3] [--torch-steps 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

VIEWS = ((160, 120, 0.12), (77, 53, 0.30))


def torch_flood(floor, ceiling, seeds=None, unreached=0xFFFF, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """(distances (n, H, W) int32 with `unreached` for unreached, iterations): the flood in plain torch, from seeds (n, 2) of
    (column, row) -- a negative pair seeds nothing -- or from the cell (W // 2, H // 2)"""
    import torch
    n, h, w = floor.shape
    far = 0x7FFFFFF0
    is_open = torch.isfinite(floor) & ((ceiling - floor) >= clearance)

    def enters(a, b):  # the move from the cells of slice a into those of slice b
        fa, fb, ga, gb = floor[a], floor[b], ceiling[a], ceiling[b]
        return is_open[a] & is_open[b] & ((fb - fa) <= max_step) & ((fa - fb) <= max_drop) & \
            ((torch.minimum(ga, gb) - torch.maximum(fa, fb)) >= clearance)
    lo, hi, every = slice(None, -1), slice(1, None), slice(None)
    ways = [((every, every, lo), (every, every, hi)), ((every, every, hi), (every, every, lo)),
            ((every, lo, every), (every, hi, every)), ((every, hi, every), (every, lo, every))]
    ways = [(a, b, enters(a, b)) for a, b in ways]
    dist = torch.full((n, h, w), far, dtype=torch.int32, device=floor.device)
    if seeds is None:
        seeds = torch.tensor([[w // 2, h // 2]], dtype=torch.int32, device=floor.device).expand(n, 2)
    rows = torch.arange(n, device=floor.device)
    valid = (seeds >= 0).all(1)
    r, c = seeds[:, 1].clamp(0, h - 1).long(), seeds[:, 0].clamp(0, w - 1).long()
    dist[rows, r, c] = torch.where(valid & is_open[rows, r, c], 0, far).to(torch.int32)
    iterations = 0
    while True:
        new = dist.clone()
        for a, b, ok in ways:
            new[b] = torch.where(ok, torch.minimum(new[b], dist[a] + 1), new[b])
        iterations += 1
        if torch.equal(new, dist):
            return torch.where(dist == far, unreached, dist), iterations
        dist = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flood_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    n = a.players
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    rows = []
    for width, height, scale in VIEWS:
        floor = torch.empty((n, height, width), dtype=torch.float32, device='cuda')
        ceiling = torch.empty_like(floor)
        dist = torch.empty((n, height, width), dtype=torch.uint16, device='cuda')
        count = torch.empty(n, dtype=torch.int32, device='cuda')
        draw = lambda: world.draw_sector_maps(states, width, height, scale, rotate=True, top_down=True, floor=floor, ceiling=ceiling, stream=stream)
        flood = lambda: rd.flood_maps(floor, ceiling, dist_out=dist, count_out=count, stream=stream)
        draw_ms = _event_ms(draw, stream, a.warmup, a.steps)
        flood_ms = _event_ms(flood, stream, a.warmup, a.steps)
        torch.cuda.synchronize()
        want, iterations = torch_flood(floor, ceiling)
        if not torch.equal(want, dist.to(torch.int32)):
            raise SystemExit('the torch flood and the kernel differ in %d cells' % int((want != dist.to(torch.int32)).sum()))
        torch_ms = _event_ms(lambda: torch_flood(floor, ceiling), torch.cuda.current_stream(), 1, a.torch_steps)
        reached = count.cpu().numpy().view(np.uint32)
        rows.append(dict(level='E1M1', players=n, width=width, height=height, scale=scale, flood_ms=flood_ms[0], flood_ms_min=flood_ms[1],
                         flood_ms_max=flood_ms[2], draw_sector_maps_2_planes_ms=draw_ms[0], torch_flood_ms=torch_ms[0],
                         torch_iterations=iterations, longest_distance=int(want[want != 0xFFFF].max().item()),
                         cells_reached_mean=float(reached.mean()), flood_over_draw=flood_ms[0] / draw_ms[0]))
    print('%-6s %9s %6s %9s %9s %13s %10s %9s' % ('level', 'view', 'scale', 'flood ms', 'draw ms', 'torch flood ms', 'torch its', 'longest'))
    for r in rows:
        print('%-6s %9s %6.2f %9.4f %9.4f %13.2f %10d %9d' % (r['level'], '%dx%d' % (r['width'], r['height']), r['scale'], r['flood_ms'],
                                                              r['draw_sector_maps_2_planes_ms'], r['torch_flood_ms'], r['torch_iterations'],
                                                              r['longest_distance']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
