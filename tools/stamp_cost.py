#!/usr/bin/env python3
"""What stamping the solid things into the area planes costs: stamp_things on E1M1's planes -- the level's own
thing table at cell 0.125 with 256 rows and at cell 0.25 with 1024 rows, and a scattered table of 600 solid things at 0.125 with 256
rows -- in place, out of place and out of place with the index plane, timed with a pair of events around each launch on one stream:
the median of --steps launches after --warmup.  Next to it, in the same run, draw_area_planes (the yardstick: it writes the two
planes this launch writes) and inflate_grids.  Before anything is timed the kernel's planes and indices are checked equal to
tests/stamp_ref.py's on row 0 and to a torch formulation's -- one dense rows x things x cells tensor expression of the same
contract, a few rows at a time so that its temporaries fit -- on every row.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/stamp_cost.jsonl).  Needs the GPU and torch.

    python tools/stamp_cost.py [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

BODY = 0.19
TORCH_ELEMENTS = 1 << 27  # of one temporary of the torch formulation: the rows of a chunk x the things x the cells
CONFIGS = (('own', 0.125, 256), ('own', 0.25, 1024), ('600', 0.125, 256))


def torch_stamp(table, own, candidate, grid, cell, floor, grow, below, above):
    """the index plane (n, H, W) int32 of the header's contract in plain torch: every candidate thing against every cell of every
    row at once.  table: (T, 4) x, z, radius, height; own: (T, 2) int64 own cells, -1 for none; candidate: (n, T) bool; floor:
    (n, H, W).  Every operation is one rounded binary32 operation, in the header's order"""
    import torch
    dev = floor.device
    n, h, w = floor.shape
    t_n = table.shape[0]
    ix, iz = torch.arange(w, device=dev), torch.arange(h, device=dev)
    xc = ((ix.to(torch.int32) + grid.ix0).to(torch.float32) + 0.5) * cell
    zc = ((iz.to(torch.int32) + grid.iz0).to(torch.float32) + 0.5) * cell
    r = table[:, 2] + grow
    ex, ez = xc[None, :] - table[:, 0, None], zc[None, :] - table[:, 1, None]
    covers = ((ex * ex)[:, None, :] + (ez * ez)[:, :, None] <= (r * r)[:, None, None]) | \
        ((ix[None, None, :] == own[:, 0, None, None]) & (iz[None, :, None] == own[:, 1, None, None]))  # (T, H, W)
    covers[:, grid.gh:, :] = False
    covers[:, :, grid.gw:] = False
    number = torch.arange(t_n, dtype=torch.int32, device=dev)[None, :, None, None]
    none = torch.tensor(0x7FFFFFFF, dtype=torch.int32, device=dev)
    chunk = max(1, TORCH_ELEMENTS // (h * w * t_n))
    out = []
    for at in range(0, n, chunk):
        dy = floor[at:at + chunk, None] - table[None, :, 3, None, None]
        blocks = covers[None] & candidate[at:at + chunk, :, None, None] & (dy >= -below) & (dy <= above)
        best = torch.where(blocks, number, none).amin(1)
        out.append(torch.where(best == none, -1, best))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stamp_cost.jsonl'))
    a = ap.parse_args()

    import numpy as np
    import torch

    import rust_doom_amd as rd
    import stamp_ref
    import things_ref
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines, own_table = world.map_lines(), world.map_things()
    rng = np.random.default_rng(32)
    near = np.stack([own_table['x'], own_table['z']], 1)
    big = things_ref.make_table(rng, 600, things_ref.bounds_of(lines), near)
    inf = float('inf')
    rows = []
    for name, cell, n in CONFIGS:
        table = own_table if name == 'own' else big
        solid_bits = world.thing_obstacles() if name == 'own' else np.ones(len(table), bool)
        things = rd.DeviceThings(table)
        words = things.words()
        grid = world.area_grid(cell)
        rand = lambda: rng.integers(0, 1 << 32, (n, words), dtype=np.uint64).astype(np.uint32)
        hidden = rand() & rand() & rand()  # an eighth of the things collected, row by row
        hidden[0] = 0
        solid = rd.pack_things(solid_bits, words).view(np.uint32)[None]
        d_solid, d_hidden = (torch.from_numpy(r.view(np.int32).copy()).cuda() for r in (solid, hidden))
        kw = dict(solid=d_solid, hidden=d_hidden)
        with torch.cuda.stream(stream):
            floor, ceiling = world.draw_area_planes(cell, n=n, floor=True, ceiling=True, stream=stream)
            fo, co, index = world.stamp_things(floor, ceiling, things, cell, index_out=True, stream=stream, **kw)
            fi, ci = floor.clone(), ceiling.clone()
            world.stamp_things(fi, ci, things, cell, floor_out=fi, ceiling_out=ci, stream=stream, **kw)
        stream.synchronize()
        # the checks: row 0 against the restatement, every row against the torch formulation, in place against out of place
        f0, c0 = floor[:1].cpu().numpy(), ceiling[:1].cpu().numpy()
        want = stamp_ref.stamp(table, grid, cell, f0, c0, solid=solid, hidden=hidden[:1])
        for what, got, ref in (('floor', fo, want[0]), ('ceiling', co, want[1]), ('index', index, want[2])):
            if not np.array_equal(got[:1].cpu().numpy().view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)):
                raise SystemExit('%s at %g: row 0 of the %s plane and the reference differ' % (name, cell, what))
        candidate = np.stack([solid_bits & ~rd.unpack_things(hidden[p], len(table)) for p in range(n)])
        t_table = torch.from_numpy(np.stack([table['x'], table['z'], table['radius'], table['base']], 1).astype(np.float32)).cuda()
        t_own = torch.from_numpy(stamp_ref.own_cells(table, grid, cell).astype(np.int64)).cuda()
        dense = torch_stamp(t_table, t_own, torch.from_numpy(candidate).cuda(), grid, cell, floor, 0.0, inf, inf)
        torch.cuda.synchronize()
        if not torch.equal(dense, index):
            raise SystemExit('%s at %g: the torch formulation and the kernel differ in %d indices' % (name, cell, int((dense != index).sum())))
        blocked = index >= 0
        pos, neg = torch.tensor(inf, device='cuda'), torch.tensor(-inf, device='cuda')
        if not (torch.equal(torch.where(blocked, pos, floor).view(torch.int32), fo.view(torch.int32)) and
                torch.equal(torch.where(blocked, neg, ceiling).view(torch.int32), co.view(torch.int32)) and
                torch.equal(fi.view(torch.int32), fo.view(torch.int32)) and torch.equal(ci.view(torch.int32), co.view(torch.int32))):
            raise SystemExit('%s at %g: the planes do not follow the index plane, or in place differs from out of place' % (name, cell))
        tx, ty = rd.STAMP_TILE
        h, w = floor.shape[1:]
        tiles = blocked.new_zeros((n, -(-h // ty) * ty, -(-w // tx) * tx))
        tiles[:, :h, :w] = blocked
        touched = tiles.view(n, -1, ty, tiles.shape[2] // tx, tx).any(4).any(2)  # tiles that hold a blocked cell
        r = dict(level='E1M1', table=name, rows=n, things=len(table), solid=int(solid_bits.sum()), cell=cell, width=w, height=h,
                 tiles=int(touched[0].numel()), tiles_with_a_blocked_cell=float(touched.float().mean()), blocked_cells=float(blocked.float().mean()))
        calls = (('in_place_ms', lambda: world.stamp_things(fi, ci, things, cell, floor_out=fi, ceiling_out=ci, stream=stream, **kw)),
                 ('out_of_place_ms', lambda: world.stamp_things(floor, ceiling, things, cell, floor_out=fo, ceiling_out=co, stream=stream, **kw)),
                 ('with_index_ms', lambda: world.stamp_things(floor, ceiling, things, cell, floor_out=fo, ceiling_out=co, index_out=index,
                                                              stream=stream, **kw)),
                 ('draw_area_planes_ms', lambda: world.draw_area_planes(cell, n=n, floor=fo, ceiling=co, stream=stream)),
                 ('inflate_grids_ms', lambda: rd.inflate_grids(floor, ceiling, BODY, cell, floor_out=fo, ceiling_out=co, stream=stream)))
        for key, call in calls:
            r[key], r[key + '_min'], r[key + '_max'] = _event_ms(call, stream, a.warmup, a.steps)
        for key in ('in_place', 'out_of_place', 'with_index'):
            r[key + '_over_planes'] = r[key + '_ms'] / r['draw_area_planes_ms']
        rows.append(r)
        things.close()
    print('%-5s %6s %5s %6s %9s %7s %9s %9s %9s %9s %9s' % ('table', 'cell', 'rows', 'things', 'cells', 'tiles+', 'in place', 'out', 'index', 'planes', 'inflate'))
    for r in rows:
        print('%-5s %6g %5d %6d %4dx%-4d %7.3f %9.4f %9.4f %9.4f %9.4f %9.4f' % (
            r['table'], r['cell'], r['rows'], r['things'], r['width'], r['height'], r['tiles_with_a_blocked_cell'], r['in_place_ms'],
            r['out_of_place_ms'], r['with_index_ms'], r['draw_area_planes_ms'], r['inflate_grids_ms']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
