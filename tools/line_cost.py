#!/usr/bin/env python3
"""What straight walks cost: walk_lines -- from every player's cell to the goal alone, and to 64 cells of the level
-- and straighten_paths -- the any-angle waypoint alone, and eight corners with the length, of an octile descent's path of 64 -- for
1024 rows of E1M1 at cell 0.25 and 256 rows at 0.125, every row a player spread over the level's floor; timed with a pair of events
around each launch on one stream -- the median of --steps launches after --warmup.  Next to them the descent that lists the path,
descend_grids_octile on the same rows, and what a user had before: a torch formulation of walk_lines, the cells of every crossing
from the closed forms of DESIGN section 27, one gather of the planes at them and the move comparisons over the whole batch.  Before
anything is timed, row 0 of every output is checked equal to tests/line_ref.py's, and the torch flags equal to the kernel's in every
row.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/line_cost.jsonl).  Needs the GPU and torch.

    python tools/line_cost.py [--rows 1024] [--steps 20] [--warmup 3] [--out FILE]
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
PATH_LEN = 64
TARGETS = 64
CORNERS = 8


def torch_walk_lines(floor, ceiling, starts, targets, reversed=False, max_step=0.24, max_drop=float('inf'), clearance=0.56):
    """the (n, q) uint8 flags of walk_lines in plain torch: every step of every line at once, padded to the longest line"""
    import torch
    n, h, w = floor.shape
    q = targets.shape[1]
    a, b = starts[:, None, :].expand(n, q, 2).long(), targets.long()
    inside = ((a >= 0) & (b >= 0) & (a[..., :1] < w) & (b[..., :1] < w) & (a[..., 1:] < h) & (b[..., 1:] < h)).all(-1)
    a, b = torch.where(inside[..., None], a, 0), torch.where(inside[..., None], b, 0)
    d = b - a
    sx, sy, dx, dy = d[..., 0].sign(), d[..., 1].sign(), d[..., 0].abs(), d[..., 1].abs()
    across = dx >= dy
    zero = torch.zeros_like(sx)
    long_c, long_r, short_c, short_r = torch.where(across, sx, zero), torch.where(across, zero, sy), torch.where(across, zero, sx), torch.where(across, sy, zero)
    dl, ds = torch.where(across, dx, dy)[..., None], torch.where(across, dy, dx)[..., None]
    steps = torch.arange(int(dl.max().item()) if dl.numel() else 0, device=floor.device)  # (L,)
    live = steps < dl
    two = (2 * dl).clamp(min=1)
    big = (2 * steps + 1) * ds + dl
    quot, rem = big // two, big % two
    corner = live & (rem == 0)
    before = quot - corner.long()
    made = torch.where(steps == 0, 0, quot - (rem < 2 * ds).long())
    c0 = a[..., :1] + steps * long_c[..., None] + made * short_c[..., None]
    r0 = a[..., 1:] + steps * long_r[..., None] + made * short_r[..., None]
    short = live & (made < before)
    c1, r1 = c0 + short * short_c[..., None], r0 + short * short_r[..., None]     # after the short crossing, if any
    cl, rl = c1 + long_c[..., None], r1 + long_r[..., None]                        # across the long one
    cs, rs = c1 + short_c[..., None], r1 + short_r[..., None]                      # the corner's other side
    cd, rd_ = cl + short_c[..., None], rl + short_r[..., None]                     # and beyond it
    base = (torch.arange(n, device=floor.device) * (h * w))[:, None, None]
    f, g = floor.reshape(-1), ceiling.reshape(-1)

    def at(c, r, valid):
        k = torch.where(valid, base + r * w + c, 0)
        return f[k], g[k]

    def is_open(fa, ga):
        return (fa < float('inf')) & (fa > -float('inf')) & (ga - fa >= clearance)

    def refused(xc, xr, yc, yr, valid):
        (fx, gx), (fy, gy) = at(xc, xr, valid), at(yc, yr, valid)
        if reversed:
            fx, gx, fy, gy = fy, gy, fx, gx
        ok = is_open(fx, gx) & is_open(fy, gy) & (fy - fx <= max_step) & (fx - fy <= max_drop) & (torch.fmin(gx, gy) - torch.fmax(fx, fy) >= clearance)
        return (valid & ~ok).any(-1)

    bad = refused(c0, r0, c1, r1, short) | refused(c1, r1, cl, rl, live) | refused(cl, rl, cd, rd_, corner) | refused(c1, r1, cs, rs, corner) | \
        refused(cs, rs, cd, rd_, corner)
    fa, ga = at(a[..., :1], a[..., 1:], inside[..., None])  # the start's own cell
    fa, ga = fa[..., 0], ga[..., 0]
    return (inside & is_open(fa, ga) & ~bad).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'line_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import line_ref
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
        height, width = world.area_plane_shape(cell)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')
        floor, ceiling = world.draw_area_planes(cell, n=n, floor=True, ceiling=True)
        cells = world.area_cells(to_dev(st), cell)
        goal = world.area_cells(to_dev(rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.full(n, yaw, np.float32))), cell)
        to_goal = rd.flood_grids_octile(floor, ceiling, goal, towards=True, max_step=MAX_STEP)
        rng = np.random.default_rng(27)
        many = torch.from_numpy(np.stack([rng.integers(0, g.gw, (n, TARGETS)), rng.integers(0, g.gh, (n, TARGETS))], 2).astype(np.int32)).cuda()
        many[:, 0] = goal
        one = goal[:, None, :].contiguous()
        step, moves, path = i32(n, 2), i32(n), i32(n, PATH_LEN, 2)
        clear1, clear64 = (torch.empty((n, q), dtype=torch.uint8, device='cuda') for q in (1, TARGETS))
        stop64, corner1, corners, count = i32(n, TARGETS, 2), i32(n, 1, 2), i32(n, CORNERS, 2), i32(n)
        length = torch.empty(n, dtype=torch.float32, device='cuda')
        kw = dict(max_step=MAX_STEP, stream=stream)
        descent = lambda: rd.descend_grids_octile(floor, ceiling, to_goal, cells, towards=True, max_moves=PATH_LEN, cells_out=step, moves_out=moves,
                                                  path_out=path, **kw)
        lines_1 = lambda: rd.walk_lines(floor, ceiling, cells, one, clear_out=clear1, **kw)
        lines_64 = lambda: rd.walk_lines(floor, ceiling, cells, many, clear_out=clear64, **kw)
        lines_64_stops = lambda: rd.walk_lines(floor, ceiling, cells, many, clear_out=clear64, stop_out=stop64, **kw)
        waypoint = lambda: rd.straighten_paths(floor, ceiling, cells, path, towards=True, corners=corner1, count_out=count, **kw)
        pulled = lambda: rd.straighten_paths(floor, ceiling, cells, path, towards=True, corners=corners, count_out=count, length_out=length, **kw)
        # the checks: row 0 of every output against the reference; the torch flags against the kernel's, every row
        with torch.cuda.stream(stream):
            descent(), lines_1(), lines_64_stops(), pulled()
        stream.synchronize()
        host = lambda t: t.cpu().numpy()
        ref_moves = [line_ref.moves_of(host(floor[0]), host(ceiling[0]), max_step=MAX_STEP)]
        want = line_ref.walk_lines(None, None, host(cells[:1]), host(many[:1]), moves=ref_moves)
        if not (np.array_equal(host(clear64[:1]), want[0]) and np.array_equal(host(stop64[:1]), want[1]) and host(clear1[0, 0]) == want[0][0, 0]):
            raise SystemExit('%s at %g: walk_lines and the reference differ' % (level, cell))
        want = line_ref.straighten_paths(None, None, host(cells[:1]), host(path[:1]), True, 64, CORNERS, moves=ref_moves)
        got = (host(corners[:1]), host(count[:1]).view(np.uint32), host(length[:1]))
        if not all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want)):
            raise SystemExit('%s at %g: straighten_paths and the reference differ' % (level, cell))
        for targets, flags in ((one, clear1), (many, clear64)):
            if not torch.equal(torch_walk_lines(floor, ceiling, cells, targets, max_step=MAX_STEP), flags):
                raise SystemExit('%s at %g: the torch lines and the kernel differ' % (level, cell))
        walked = moves > 0
        r = dict(level=level, cell=cell, rows=n, width=width, height=height, cells=width * height, max_step=MAX_STEP, path_len=PATH_LEN,
                 targets=TARGETS, corners=CORNERS, rows_that_walk=int(walked.sum().item()), moves_mean=float(moves[walked].float().mean().item()),
                 corners_mean=float(count[walked].float().mean().item()), rows_that_see_the_goal=int(clear1.sum().item()),
                 clear_of_64_mean=float(clear64.float().sum(1).mean().item()),
                 crossings_of_64_mean=float((many - cells[:, None, :]).abs().sum(2).float().mean().item()))
        for name, call, on in (('descend_octile_path_64_ms', descent, stream), ('walk_lines_1_ms', lines_1, stream),
                               ('walk_lines_64_ms', lines_64, stream), ('walk_lines_64_with_stops_ms', lines_64_stops, stream),
                               ('straighten_waypoint_ms', waypoint, stream), ('straighten_8_corners_length_ms', pulled, stream),
                               ('torch_walk_lines_1_ms', lambda: torch_walk_lines(floor, ceiling, cells, one, max_step=MAX_STEP), torch.cuda.current_stream()),
                               ('torch_walk_lines_64_ms', lambda: torch_walk_lines(floor, ceiling, cells, many, max_step=MAX_STEP), torch.cuda.current_stream())):
            ms = _event_ms(call, on, a.warmup, a.steps)
            r[name] = ms[0]
            r[name + '_min'], r[name + '_max'] = ms[1], ms[2]
        r['torch_over_walk_lines_64'] = r['torch_walk_lines_64_ms'] / r['walk_lines_64_ms']
        rows.append(r)
        del floor, ceiling, to_goal
    print('%-5s %6s %5s %9s %10s %9s %9s %11s %10s %10s %10s' % ('level', 'cell', 'rows', 'grid', 'descent ms', 'line ms', '64 ms', 'waypoint ms',
                                                              'pulled ms', 'torch 1', 'torch 64'))
    for r in rows:
        print('%-5s %6.4f %5d %9s %10.4f %9.4f %9.4f %11.4f %10.4f %10.3f %10.3f' % (
            r['level'], r['cell'], r['rows'], '%dx%d' % (r['width'], r['height']), r['descend_octile_path_64_ms'], r['walk_lines_1_ms'],
            r['walk_lines_64_ms'], r['straighten_waypoint_ms'], r['straighten_8_corners_length_ms'], r['torch_walk_lines_1_ms'],
            r['torch_walk_lines_64_ms']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
