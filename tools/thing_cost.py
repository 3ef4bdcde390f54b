#!/usr/bin/env python3
"""What sensing the things costs: sense_things with all five outputs for 1024 players of E1M1 -- spread over the
level's floor -- against the level's own thing table and against a table of 600 things, timed with a pair of events around each launch
on one stream -- the median of --steps launches after --warmup.  Next to it reveal_lines with 64 rays on the same players, and what a
user had before: a torch formulation, one dense players x things x lines tensor expression of the same contract (the yaw's sine and
cosine handed to it, the players taken --torch-chunk at a time so that its temporaries fit).  Before anything is timed, row 0 of every
output is checked equal to tests/things_ref.py's, and the torch formulation's visible and touched bits equal to the kernel's in every
row.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/thing_cost.jsonl).  Needs the GPU and torch.

    python tools/thing_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

MAX_RANGE, FOV, TOUCH = 20.0, 2.0, 0.19
RAYS = 64


def torch_sense(lines, block, table, pos, sin, cos, max_range, cos_half_fov, touch_radius, chunk):
    """(visible, touched) bool (n, T) tensors of the header's contract in plain torch, every object at rest and nothing collected:
    every thing of every player against every line at once.  lines: (L, 4) a.x, a.z, b.x, b.z; block: (L,) bool; table: (T, 4) x, z,
    base, radius; pos: (n, 3); sin, cos: (n,)"""
    import torch
    ax, az, bx, bz = (lines[:, k][None, None, :] for k in range(4))
    ldx, ldz = bx - ax, bz - az
    len2 = ldx * ldx + ldz * ldz
    vis, tch = [], []
    for at in range(0, pos.shape[0], chunk):
        p, s, c = pos[at:at + chunk], sin[at:at + chunk, None], cos[at:at + chunk, None]
        dx, dz = table[None, :, 0] - p[:, None, 0], table[None, :, 1] - p[:, None, 2]
        d2 = dx * dx + dz * dz
        dy = p[:, None, 1] - (table[None, :, 2] + 0.0)
        tr = touch_radius + table[None, :, 3]
        tch.append((d2 <= tr * tr) & (dy >= -float('inf')) & (dy <= float('inf')))
        fx, fz = -s, -c
        in_view = (dx * fx + dz * fz >= cos_half_fov * torch.sqrt(d2)) if cos_half_fov > -1.0 else torch.ones_like(d2, dtype=torch.bool)
        cand = (d2 <= max_range * max_range) & in_view
        vx, vz = dx[:, :, None], dz[:, :, None]
        wx, wz = ax - p[:, None, None, 0], az - p[:, None, None, 2]
        den = vx * ldz - vz * ldx
        t = (wx * ldz - wz * ldx) / den
        u = (wx * vz - wz * vx) / den
        hit = (len2 > 0) & (den != 0) & (u >= 0) & (u <= 1) & (t >= 0) & (t <= 1) & block[None, None, :]
        limit = torch.where(hit, t, torch.ones_like(t)).amin(2)
        vis.append(cand & (limit == 1.0))
    return torch.cat(vis), torch.cat(tch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-chunk', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'thing_cost.jsonl'))
    a = ap.parse_args()
    import math

    import numpy as np
    import torch

    import rays_ref
    import reveal_ref
    import rust_doom_amd as rd
    import things_ref
    import world_ref
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines, own = world.map_lines(), world.map_things()
    n = a.players
    st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
    rng = np.random.default_rng(28)
    big = things_ref.make_table(rng, 600, things_ref.bounds_of(lines), np.stack([st['pos'][:, 0], st['pos'][:, 2]], 1))
    states = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
    fan = torch.from_numpy(rd.map_fan(RAYS, FOV)).cuda()
    seen = torch.zeros((n, world.seen_words()), dtype=torch.int32, device='cuda')
    reveal = lambda: world.reveal_lines(states, fan, MAX_RANGE, seen=seen, stream=stream)
    # what the torch formulation is handed: the table's end points, which lines block at rest, the positions and the project's sincos
    t_lines = torch.from_numpy(np.concatenate([lines['a'], lines['b']], 1).astype(np.float32)).cuda()
    t_block = torch.from_numpy(reveal_ref.blocking(lines)).cuda()
    t_pos = torch.from_numpy(st['pos'].astype(np.float32)).cuda()
    sc = np.array([world_ref.sincos(float(y)) for y in st['yaw']], np.float32)
    t_sin, t_cos = torch.from_numpy(sc[:, 0].copy()).cuda(), torch.from_numpy(sc[:, 1].copy()).cuda()
    cos_half = float(np.float32(math.cos(0.5 * FOV)))
    prm = things_ref.params(MAX_RANGE, fov=FOV, touch_radius=TOUCH)
    rows = []
    for name, table in (('own', own), ('600', big)):
        things = rd.DeviceThings(table)
        words = things.words()
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device='cuda')
        col, vis, tch, new = i32(n, words), i32(n, words), i32(n, words), i32(n, 8)
        near = torch.zeros((n, 8, 4), dtype=torch.float32, device='cuda')
        sense = lambda: world.sense_things(states, things, MAX_RANGE, fov=FOV, touch_radius=TOUCH, collected=col, visible_out=vis, touched_out=tch,
                                           nearest_out=near, new_out=new, stream=stream)
        t_table = torch.from_numpy(np.stack([table['x'], table['z'], table['base'], table['radius']], 1).astype(np.float32)).cuda()
        dense = lambda: torch_sense(t_lines, t_block, t_table, t_pos, t_sin, t_cos, MAX_RANGE, cos_half, TOUCH, a.torch_chunk)
        # the checks: row 0 of every output against the reference; the torch bits against the kernel's, every row
        with torch.cuda.stream(stream):
            sense()
        stream.synchronize()
        want = things_ref.sense(lines, table, st[:1], prm)
        for key, got in (('collected', col), ('visible', vis), ('touched', tch), ('nearest', near), ('new', new)):
            if not np.array_equal(got[:1].cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(want[key]).view(np.uint32).reshape(-1)):
                raise SystemExit('%s: %s of row 0 and the reference differ' % (name, key))
        t_vis, t_tch = dense()
        torch.cuda.synchronize()
        for key, rows_t, bits in (('visible', vis, t_vis), ('touched', tch, t_tch)):
            got = np.stack([rd.unpack_things(r, len(table)) for r in rows_t.cpu().numpy()])
            if not np.array_equal(got, bits.cpu().numpy()):
                raise SystemExit('%s: the torch formulation and the kernel differ in %d %s bits' % (name, int((got != bits.cpu().numpy()).sum()), key))
        visible = np.stack([rd.unpack_things(r, len(table)) for r in vis.cpu().numpy()])
        r = dict(level='E1M1', table=name, players=n, things=len(table), lines=len(lines), max_range=MAX_RANGE, fov=FOV, rays=RAYS,
                 torch_chunk=a.torch_chunk, visible_pairs=float(visible.mean()), players_that_see_something=int(visible.any(1).sum()))
        for key, call, on in (('sense_things_ms', sense, stream), ('reveal_lines_64_ms', reveal, stream),
                              ('torch_ms', dense, torch.cuda.current_stream())):
            ms = _event_ms(call, on, a.warmup, a.steps)
            r[key], r[key + '_min'], r[key + '_max'] = ms
        r['torch_over_kernel'] = r['torch_ms'] / r['sense_things_ms']
        rows.append(r)
        things.close()
    print('%-6s %7s %7s %6s %10s %10s %10s %8s' % ('table', 'players', 'things', 'lines', 'sense ms', 'reveal ms', 'torch ms', 'torch/k'))
    for r in rows:
        print('%-6s %7d %7d %6d %10.4f %10.4f %10.3f %8.1f' % (r['table'], r['players'], r['things'], r['lines'], r['sense_things_ms'],
                                                             r['reveal_lines_64_ms'], r['torch_ms'], r['torch_over_kernel']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
