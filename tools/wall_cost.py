#!/usr/bin/env python3
"""What the wall distance costs: rdoom_wall_distance on the planes draw_area_planes draws -- 1024 rows of E1M1 at
cell 0.25, fewer rows at 0.125 and on the big level at 0.125, section 23's table -- at close_d2 = 2 (radius 2) and at the radii 8
and 32 with close_d2 = R * R, each for the distances alone, the planes alone and both; timed with a pair of events around each
launch on one stream -- the median of --steps launches after --warmup.  Next to each, from the same run: the draw_area_planes launch
that wrote the planes, which writes as many bytes as the inflation does and so is the yardstick for memory traffic, and at
close_d2 = 2 what a user had before -- the same dilation in torch, max_pool2d of the closed mask and two torch.where.
Before anything is timed, row 0 of every configuration and radius is checked equal to tests/walls_ref.py's two-phase form, planes
and distances, and the torch dilation equal to the kernel's planes in every row.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/wall_cost.jsonl).  Needs the GPU and torch.

    python tools/wall_cost.py [--rows 1024] [--steps 20] [--warmup 3] [--out FILE]
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
# (radius of the launch, the body's radius in cells that gives it: close_d2 = floor(body * body))
RADII = ((2, 1.5), (8, 8.0), (32, 32.0))
CLEARANCE = 0.56


def torch_inflate(floor, ceiling):
    """close_d2 = 2 in torch: a cell is shut when a closed cell, or the grid's edge, is among its eight neighbours or itself"""
    import torch
    closed = ~(torch.isfinite(floor) & (ceiling - floor >= CLEARANCE))
    padded = torch.nn.functional.pad(closed.to(torch.float16)[:, None], (1, 1, 1, 1), value=1.0)
    shut = torch.nn.functional.max_pool2d(padded, 3, stride=1)[:, 0] > 0
    return torch.where(shut, float('inf'), floor), torch.where(shut, float('-inf'), ceiling)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wall_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import rust_doom_amd as rd
    import walls_ref
    from automap_cost import _event_ms
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wads = {'E1M1': rd.Wad(ensure_wad(), META_PATH), 'big': rd.Wad(ensure_big_wad(), META_PATH)}
    rows = []
    for level, cell, share in CONFIGS:
        n = max(4, int(a.rows * share))
        world = wads[level].build_world(0)
        height, width = world.area_plane_shape(cell)
        floor = torch.empty((n, height, width), dtype=torch.float32, device='cuda')
        ceiling = torch.empty_like(floor)
        fo, co = torch.empty_like(floor), torch.empty_like(floor)
        d2 = torch.empty((n, height, width), dtype=torch.uint16, device='cuda')
        draw = lambda: world.draw_area_planes(cell, n=n, floor=floor, ceiling=ceiling, stream=stream)
        with torch.cuda.stream(stream):
            draw()
        stream.synchronize()
        f0, c0 = floor[0].cpu().numpy(), ceiling[0].cpu().numpy()
        draw_ms = _event_ms(draw, stream, a.warmup, a.steps)
        tiles = -(-width // rd.WALL_TILE[0]) * -(-height // rd.WALL_TILE[1])
        for radius, body in RADII:
            shut = rd.wall_close_d2(body, 1.0)
            assert shut == (2 if radius == 2 else radius * radius)
            distances = lambda: rd.wall_distances(floor, ceiling, radius, dist2_out=d2, stream=stream)
            planes = lambda: rd.inflate_grids(floor, ceiling, body, 1.0, floor_out=fo, ceiling_out=co, stream=stream)
            both = lambda: rd.inflate_grids(floor, ceiling, body, 1.0, floor_out=fo, ceiling_out=co, dist2_out=d2, stream=stream)
            # the check: row 0 against the two-phase form, from each of the three launches
            want = walls_ref.capped(f0, c0, radius)
            want_planes = walls_ref.inflate(f0, c0, want, shut)
            for name, call, has_d2, has_planes in (('distances', distances, True, False), ('planes', planes, False, True), ('both', both, True, True)):
                d2.view(torch.int16).fill_(7), fo.fill_(7.0), co.fill_(7.0)
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    call()
                stream.synchronize()
                if has_d2 and not np.array_equal(d2[0].cpu().numpy(), want):
                    raise SystemExit('%s at %g, radius %d, %s: the kernel\'s distances and the reference differ' % (level, cell, radius, name))
                if has_planes and not (np.array_equal(fo[0].cpu().numpy().view(np.uint32), want_planes[0].view(np.uint32)) and
                                       np.array_equal(co[0].cpu().numpy().view(np.uint32), want_planes[1].view(np.uint32))):
                    raise SystemExit('%s at %g, radius %d, %s: the kernel\'s planes and the reference differ' % (level, cell, radius, name))
            r = dict(level=level, cell=cell, rows=n, width=width, height=height, cells=width * height, tiles=tiles, radius=radius, close_d2=shut,
                     draw_area_planes_2_planes_ms=draw_ms[0])
            if radius == 2:
                tf, tc = torch_inflate(floor, ceiling)
                if not (torch.equal(tf.view(torch.int32), fo.view(torch.int32)) and torch.equal(tc.view(torch.int32), co.view(torch.int32))):
                    raise SystemExit('%s at %g: the torch dilation and the kernel differ' % (level, cell))
                del tf, tc
                r['torch_max_pool2d_ms'] = _event_ms(lambda: torch_inflate(floor, ceiling), torch.cuda.current_stream(), a.warmup, a.steps)[0]
            d_ms, p_ms, b_ms = (_event_ms(call, stream, a.warmup, a.steps) for call in (distances, planes, both))
            r.update(distances_ms=d_ms[0], planes_ms=p_ms[0], planes_ms_min=p_ms[1], planes_ms_max=p_ms[2], both_ms=b_ms[0],
                     planes_over_draw_area_planes=p_ms[0] / draw_ms[0], both_over_draw_area_planes=b_ms[0] / draw_ms[0],
                     planes_us_per_row=1000.0 * p_ms[0] / n, shut_share=float(torch.isinf(fo).float().mean().item()))
            rows.append(r)
        del floor, ceiling, fo, co, d2
    print('%-5s %6s %5s %11s %3s %9s %12s %9s %9s %9s %9s' % ('level', 'cell', 'rows', 'grid', 'R', 'draw ms', 'distances ms', 'planes ms', 'both ms',
                                                                'x draw', 'torch ms'))
    for r in rows:
        print('%-5s %6.4f %5d %11s %3d %9.4f %12.4f %9.4f %9.4f %9.2f %9s' % (
            r['level'], r['cell'], r['rows'], '%dx%d' % (r['width'], r['height']), r['radius'], r['draw_area_planes_2_planes_ms'], r['distances_ms'],
            r['planes_ms'], r['both_ms'], r['planes_over_draw_area_planes'], '%.3f' % r['torch_max_pool2d_ms'] if 'torch_max_pool2d_ms' in r else '-'))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
