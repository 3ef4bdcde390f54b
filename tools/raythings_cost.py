#!/usr/bin/env python3
"""What seeing things costs a range sensor (rdoom_world_cast_rays_things): tests/rays_ref.py's players (random
floor centroids, seeded yaws and pitches) on E1M1 (synthetic IWAD) with a fan of 64 rays each, at 4 096 and 65 536 players, against the level's
own thing table and against tables of 256 and 4 096 things scattered over the level's extent.  Three figures a row, each the
median of --steps launches after --warmup, host clock around torch.cuda.synchronize:

  cast     World.cast_rays on the same rays: what the sensor cost before
  things   World.cast_rays_things on the fractions cast_rays wrote (every thing, nothing hidden, at rest), with the indices
  torch    what a user had before: a torch formulation of the same contract on the device, one players x rays x things
           broadcast from cast_rays' own origin_out / vel_out, the players taken --torch-chunk at a time so that its
           temporaries fit

Before anything is timed, the launch's first 8 players are checked equal to tests/raythings_ref.py's, and the torch formulation's
fractions and indices are compared with the launch's over every player (the share that is equal is reported: torch's division and
square root need not be the correctly rounded ones).
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/raythings_cost.jsonl).  Needs the GPU
and torch.

    python tools/raythings_cost.py [--steps 5] [--warmup 1] [--skip-torch] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

RAYS, MAX_RANGE, FOV, HEIGHT = 64, 30.0, 2.0, 0.56


def torch_cast(origin, vel, table, frac, height, chunk):
    """(frac_out, thing_out) of the header's contract in plain torch, every thing standing at rest, selected and seen: every ray of
    every player against every thing at once.  origin, vel: (n, R, 3); table: (T, 4) x, z, base, radius; frac: (n, R)"""
    import torch
    inf = float('inf')
    x, z, base, radius = (table[:, k][None, None, :] for k in range(4))
    rr = radius * radius
    top = base + height
    index = torch.arange(table.shape[0], device=table.device, dtype=torch.int32)[None, None, :]
    none = torch.iinfo(torch.int32).max
    outs, things = [], []
    for at in range(0, origin.shape[0], chunk):
        o, v, cur = origin[at:at + chunk], vel[at:at + chunk], frac[at:at + chunk]
        ox, oy, oz = (o[:, :, k, None] for k in range(3))
        vx, vy, vz = (v[:, :, k, None] for k in range(3))
        ok = torch.isfinite(o).all(2, keepdim=True) & torch.isfinite(v).all(2, keepdim=True) & (v != 0).any(2, keepdim=True)
        cx, cz = ox - x, oz - z
        a = vx * vx + vz * vz
        b = cx * vx + cz * vz
        cc = (cx * cx + cz * cz) - rr
        disc = b * b - a * cc
        s = torch.sqrt(disc)
        slanted = a > 0
        h0 = torch.where(slanted, (-b - s) / a, torch.full_like(s, -inf))
        h1 = torch.where(slanted, (-b + s) / a, torch.full_like(s, inf))
        plan = torch.where(slanted, disc >= 0, cc <= 0)
        u0, u1 = (base - oy) / vy, (top - oy) / vy
        rising = vy != 0
        v0 = torch.where(rising, torch.minimum(u0, u1), torch.full_like(u0, -inf))
        v1 = torch.where(rising, torch.maximum(u0, u1), torch.full_like(u0, inf))
        in_height = rising | ((oy >= base) & (oy <= top))
        t = torch.clamp_min(torch.where(h0 < v0, v0, h0), 0.0)
        e = torch.where(v1 < h1, v1, h1)
        hit = plan & in_height & (t <= e) & (t <= 1) & (radius > 0) & ok
        t = torch.where(hit, t, torch.full_like(t, inf))
        best = t.amin(2)
        who = torch.where((t == best[:, :, None]) & hit, index, torch.full_like(index, none)).amin(2)
        replaces = best < cur
        outs.append(torch.where(replaces, best, cur))
        things.append(torch.where(replaces, who, torch.full_like(who, -1)))
    return torch.cat(outs), torch.cat(things)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--players', type=int, nargs='*', default=[4096, 65536])
    ap.add_argument('--torch-cells', type=int, default=1 << 26, help='players x rays x things the torch formulation takes at a time')
    ap.add_argument('--skip-torch', action='store_true', help='time cast and things only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'raythings_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import raythings_ref as rt
    import rust_doom_amd as rd
    import things_ref
    from ray_cost import _median_ms
    import rays_ref
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built, world = wad.build_level(0), wad.build_world(0)
    own = world.map_things()
    x0, x1, z0, z1 = things_ref.bounds_of(world.map_lines())
    rng = np.random.default_rng(33)
    tables = [('own', own)]
    for size in (256, 4096):
        tables.append((str(size), rt.table_of(rng.uniform(x0, x1, size), rng.uniform(z0, z1, size), rng.choice(own['base'], size),
                                              rng.uniform(0.08, 0.3, size), rng.integers(0, 8, size))))
    fan_np = rd.ray_fan(RAYS, FOV)
    fan = torch.from_numpy(fan_np).cuda()
    rows = []
    for n in a.players:
        st = np.array(rays_ref.players(built, n, count=n), rd.PLAYER_STATE)
        states = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
        world_frac = torch.empty((n, RAYS), dtype=torch.float32, device='cuda')
        origin = torch.empty((n, RAYS, 3), dtype=torch.float32, device='cuda')
        vel = torch.empty_like(origin)
        world.cast_rays(states, fan, MAX_RANGE, frac_out=world_frac, origin_out=origin, vel_out=vel)
        spare = torch.empty_like(world_frac)
        cast = _median_ms(lambda: world.cast_rays(states, fan, MAX_RANGE, frac_out=spare), a.warmup, a.steps)
        for name, table in tables:
            things = rd.DeviceThings(table)
            frac = torch.empty_like(world_frac)
            thing = torch.empty((n, RAYS), dtype=torch.int32, device='cuda')
            launch = lambda: world.cast_rays_things(states, things, fan, MAX_RANGE, heights=HEIGHT, frac=world_frac, frac_out=frac, thing_out=thing)
            launch()
            torch.cuda.synchronize()
            want = rt.cast(table, st[:8], fan_np, MAX_RANGE, heights=HEIGHT, frac=world_frac[:8].cpu().numpy())
            if not (np.array_equal(frac[:8].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and
                    np.array_equal(thing[:8].cpu().numpy(), want[1])):
                raise SystemExit('%s, %d players: the launch and the reference differ' % (name, n))
            t_table = torch.from_numpy(np.stack([table['x'], table['z'], table['base'], table['radius']], 1).astype(np.float32)).cuda()
            chunk = max(1, a.torch_cells // (RAYS * len(table)))
            dense = lambda: torch_cast(origin, vel, t_table, world_frac, HEIGHT, chunk)
            same_frac = same_thing = None
            dense_ms = (float('nan'),) * 3
            kernel = _median_ms(launch, a.warmup, a.steps)
            if not a.skip_torch:
                t_frac, t_thing = dense()
                torch.cuda.synchronize()
                same_frac = float((t_frac.view(torch.int32) == frac.view(torch.int32)).float().mean().item())
                same_thing = float((t_thing == thing).float().mean().item())
                del t_frac, t_thing
                dense_ms = _median_ms(dense, a.warmup, a.steps)
            rays = n * RAYS
            rows.append(dict(level='E1M1', table=name, things=len(table), players=n, rays=RAYS, max_range=MAX_RANGE, height=HEIGHT,
                             cast_ms=cast[0], cast_ms_min=cast[1], cast_ms_max=cast[2], things_ms=kernel[0], things_ms_min=kernel[1],
                             things_ms_max=kernel[2], torch_ms=dense_ms[0], torch_ms_min=dense_ms[1], torch_ms_max=dense_ms[2],
                             torch_chunk=chunk, things_ns_per_ray=kernel[0] * 1e6 / rays, things_over_cast=kernel[0] / cast[0],
                             torch_over_things=dense_ms[0] / kernel[0], rays_on_things=float((thing >= 0).float().mean().item()),
                             torch_same_frac=same_frac, torch_same_thing=same_thing))
            things.close()
    print('%-5s %7s %8s %9s %10s %10s %12s %10s %9s' % ('table', 'things', 'players', 'cast ms', 'things ms', 'torch ms', 'things/cast',
                                                        'torch/thgs', 'on things'))
    for r in rows:
        print('%-5s %7d %8d %9.3f %10.3f %10.3f %12.3f %10.1f %9.3f' % (r['table'], r['things'], r['players'], r['cast_ms'], r['things_ms'],
                                                                       r['torch_ms'], r['things_over_cast'], r['torch_over_things'],
                                                                       r['rays_on_things']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
