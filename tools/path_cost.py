#!/usr/bin/env python3
"""What waypoints and frontiers cost: area_frontiers -- the nearest cell alone, and with the distance, the count and
the mask -- and descend_grids -- the waypoint 8 moves ahead on a field towards the level's start, and the whole path from the frontier
cell back to the player -- for 1024 rows of E1M1 at cell 0.25 and 256 rows at 0.125, every row a player spread over the level's floor
that has looked around four times; timed with a pair of events around each launch on one stream -- the median of --steps launches after
--warmup.  Next to them what a user had before: a torch formulation of the frontier (the bits unpacked, shifted ORs, a masked argmin),
and, for scale, the tick's read of a field, area_cells plus a gather.  Before anything is timed, row 0 of every output is checked equal
to tests/path_ref.py's, and the torch frontier equal to the kernel's in every row.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/path_cost.jsonl).  Needs the GPU and torch.

    python tools/path_cost.py [--rows 1024] [--steps 20] [--warmup 3] [--out FILE]
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
CONFIGS = (('E1M1', 0.25, 1.0), ('E1M1', 0.125, 0.25))
MAX_STEP = 0.32  # the synthetic levels join most of their sectors by steps of 0.32
WAYPOINT = 8
PATH_LEN = 512


def torch_frontiers(area, grid, dist):
    """(cells (n, 2) int32, dists (n,) int32 with -1 for none, counts (n,) int32, masks (n, H, W) uint8): the frontier in plain torch
    from reveal_area's rows (n, 2, stride) int32 and the distances (n, H, W) int32 with -1 for unreached"""
    import torch
    n, h, w = dist.shape
    ix = torch.arange(grid.gw, device=dist.device)
    planes = area[:, :, :grid.words].reshape(n, 2, grid.gh, grid.pitch)
    bits = (planes[:, :, :, ix >> 5] >> (ix & 31)) & 1  # (n, 2, gh, gw)
    unknown = (bits[:, 0] | bits[:, 1]) == 0
    near = torch.zeros_like(unknown)
    near[:, :, 1:] |= unknown[:, :, :-1]
    near[:, :, :-1] |= unknown[:, :, 1:]
    near[:, 1:, :] |= unknown[:, :-1, :]
    near[:, :-1, :] |= unknown[:, 1:, :]
    inside = dist[:, :grid.gh, :grid.gw]
    front = near & (inside >= 0)
    masks = torch.zeros((n, h, w), dtype=torch.uint8, device=dist.device)
    masks[:, :grid.gh, :grid.gw] = front
    far = 0x7FFFFFFF
    keyed = torch.where(front, inside, far).reshape(n, -1)
    at = keyed.argmin(1)  # the first of the smallest: the smallest iz, then ix
    best = keyed[torch.arange(n, device=dist.device), at]
    none = best == far
    cells = torch.stack([at % grid.gw, at // grid.gw], 1).to(torch.int32)
    cells[none] = -1
    return cells, torch.where(none, -1, best).to(torch.int32), front.reshape(n, -1).sum(1).to(torch.int32), masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'path_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import goal_ref
    import path_ref
    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    pos, yaw = wad.build_level(0).start()
    rows = []
    for level, cell, share in CONFIGS:
        n = max(4, int(a.rows * share))
        g = world.area_grid(cell)
        st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
        to_dev = lambda s: torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).reshape(-1).copy()).cuda()
        states = to_dev(st)
        fan = torch.from_numpy(rd.map_fan(64, 1.6)).cuda()
        area, turned = None, st.copy()
        for _ in range(4):
            area = world.reveal_area(to_dev(turned), fan, 12.0, cell, area=area)
            turned['yaw'] += np.float32(1.6)
        height, width = world.area_plane_shape(cell)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')
        # the exploring tick's field: forwards from the players' cells over what each has seen; the goal's: towards the start, whole level
        floor, ceiling = world.draw_area_planes(cell, area=area, floor=True, ceiling=True)
        cells = world.area_cells(states, cell)
        dist = rd.flood_grids(floor, ceiling, cells, max_step=MAX_STEP)
        whole_floor, whole_ceiling = world.draw_area_planes(cell, n=n, floor=True, ceiling=True)
        goal = world.area_cells(to_dev(rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.full(n, yaw, np.float32))), cell)
        to_goal = rd.flood_grids(whole_floor, whole_ceiling, goal, towards=True, max_step=MAX_STEP)
        front, front_dist, count, step, moves, path = i32(n, 2), i32(n), i32(n), i32(n, 2), i32(n), i32(n, PATH_LEN, 2)
        mask = torch.empty((n, height, width), dtype=torch.uint8, device='cuda')
        nearest = lambda: world.area_frontiers(area, dist, cell, cell_out=front, stream=stream)
        everything = lambda: world.area_frontiers(area, dist, cell, cell_out=front, dist_out=front_dist, count_out=count, mask_out=mask, stream=stream)
        waypoint = lambda: rd.descend_grids(whole_floor, whole_ceiling, to_goal, cells, towards=True, max_moves=WAYPOINT, max_step=MAX_STEP,
                                            cells_out=step, moves_out=moves, stream=stream)
        whole_path = lambda: rd.descend_grids(floor, ceiling, dist, front, max_step=MAX_STEP, cells_out=step, moves_out=moves, path_out=path,
                                              stream=stream)
        # the checks: row 0 of every output against the reference; the torch frontier against the kernel's, every row
        with torch.cuda.stream(stream):
            everything()
        stream.synchronize()
        host = lambda t: t.cpu().numpy()
        f0, c0, d0, a0 = host(floor[:1]), host(ceiling[:1]), host(dist[:1]).view(np.uint32), host(area[:1]).view(np.uint32)
        want = path_ref.area_frontiers(a0, g, d0)
        for got, ref, what in ((front, want[0], 'cell'), (front_dist, want[1], 'distance'), (count, want[2], 'count'), (mask, want[3], 'mask')):
            if not np.array_equal(host(got[:1]).view(ref.dtype), ref):
                raise SystemExit('%s at %g: the frontier kernel and the reference differ in the %s' % (level, cell, what))
        for got, ref, what in zip(torch_frontiers(area, g, dist), (front, front_dist, count, mask), ('cell', 'distance', 'count', 'mask')):
            if not torch.equal(got, ref):
                raise SystemExit('%s at %g: the torch frontier and the kernel differ in the %s' % (level, cell, what))
        with torch.cuda.stream(stream):
            whole_path()
        stream.synchronize()
        ref = path_ref.descend_grids(f0, c0, d0, want[0], path_len=PATH_LEN, max_step=MAX_STEP)
        if not all(np.array_equal(host(got[:1]).view(r.dtype), r) for got, r in zip((step, moves, path), ref)):
            raise SystemExit('%s at %g: the walk back from the frontier and the reference differ' % (level, cell))
        longest = int(moves.max().item())
        with torch.cuda.stream(stream):
            waypoint()
        stream.synchronize()
        ref = path_ref.descend_grids(host(whole_floor[:1]), host(whole_ceiling[:1]), host(to_goal[:1]).view(np.uint32), host(cells[:1]), towards=True,
                                     max_moves=WAYPOINT, max_step=MAX_STEP)
        if not all(np.array_equal(host(got[:1]).view(r.dtype), r) for got, r in zip((step, moves), ref[:2])):
            raise SystemExit('%s at %g: the waypoint and the reference differ' % (level, cell))
        r = dict(level=level, cell=cell, rows=n, width=width, height=height, cells=width * height, max_step=MAX_STEP,
                 frontier_cells_mean=float(count.float().mean().item()), rows_with_a_frontier=int((count > 0).sum().item()),
                 waypoint_moves_mean=float(moves.float().mean().item()), longest_path=longest, path_len=PATH_LEN)
        rows_of = torch.arange(n, device='cuda')
        at = i32(n, 2)

        def read():  # the tick's read of a field: the players' cells and a gather, negative cells mapped to unreached
            world.area_cells(states, cell, out=at, stream=stream)
            ok = (at >= 0).all(1)
            return torch.where(ok, to_goal[rows_of, at[:, 1].clamp(min=0).long(), at[:, 0].clamp(min=0).long()], -1)
        for name, call, on in (('area_frontiers_cell_ms', nearest, stream), ('area_frontiers_all_outputs_ms', everything, stream),
                               ('descend_waypoint_8_ms', waypoint, stream), ('descend_whole_path_ms', whole_path, stream),
                               ('torch_frontiers_ms', lambda: torch_frontiers(area, g, dist), torch.cuda.current_stream()),
                               ('area_cells_and_gather_ms', read, stream)):
            ms = _event_ms(call, on, a.warmup, a.steps)
            r[name] = ms[0]
            r[name + '_min'], r[name + '_max'] = ms[1], ms[2]
        r['torch_over_area_frontiers'] = r['torch_frontiers_ms'] / r['area_frontiers_all_outputs_ms']
        rows.append(r)
        del floor, ceiling, dist, whole_floor, whole_ceiling, to_goal, mask
    print('%-5s %6s %5s %9s %9s %9s %11s %9s %9s %9s' % ('level', 'cell', 'rows', 'grid', 'cell ms', 'all ms', 'waypoint ms', 'path ms', 'torch ms',
                                                         'read ms'))
    for r in rows:
        print('%-5s %6.4f %5d %9s %9.4f %9.4f %11.4f %9.4f %9.3f %9.4f' % (
            r['level'], r['cell'], r['rows'], '%dx%d' % (r['width'], r['height']), r['area_frontiers_cell_ms'], r['area_frontiers_all_outputs_ms'],
            r['descend_waypoint_8_ms'], r['descend_whole_path_ms'], r['torch_frontiers_ms'], r['area_cells_and_gather_ms']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
