#!/usr/bin/env python3
"""What a range sensor costs (rdoom_world_cast_rays, DESIGN section "Range-sensor rays"): tools/player_step_cost.py's players
(random floor centroids, random yaws) with a fan of 64 rays each, on E1M1 (synthetic IWAD) and on the 10x level, at 4 096 and
65 536 players.  Three ways to the same distances, each the median of --steps launches after --warmup, host clock around
torch.cuda.synchronize:

  cast        World.cast_rays on the device states
  sweep       the existing path on the same rays, generously: World.sweep at radius 0 on spheres / velocities already resident
              on the device (cast_rays' own origin_out / vel_out), so it pays no host build
  sweep+host  the full old path: states copied off the device, n x R spheres and velocities built on the host (numpy), uploaded,
              swept

Prints a table and one JSON line per row (nanoseconds per ray; --out appends the lines to a file).  Needs the GPU and torch.

    python tools/ray_cost.py [--steps K] [--warmup W] [--rays R] [--range M] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _median_ms(fn, warmup, steps):
    import numpy as np
    import torch
    times = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def _host_rays(states, fan, max_range):
    """the rays of every player built on the host in numpy: the eye 0.12 above the player along its up, the fan turned by
    (yaw, pitch) -- the construction a caller of World.sweep has to do from copied states (not bit for bit the device's)"""
    import numpy as np
    yaw, pitch = states['yaw'].astype(np.float32), states['pitch'].astype(np.float32)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    # R = Ry(yaw) Rx(pitch), rows
    r0 = np.stack([cy, sy * sp, sy * cp], 1)
    r1 = np.stack([np.zeros_like(cy), cp, -sp], 1)
    r2 = np.stack([-sy, cy * sp, cy * cp], 1)
    rot = np.stack([r0, r1, r2], 1)  # (n, 3, 3)
    eye = states['pos'] + rot[:, :, 1] * np.float32(0.12)
    vel = np.einsum('nij,rj->nri', rot, fan).astype(np.float32) * np.float32(max_range)
    spheres = np.zeros((len(states), len(fan), 4), np.float32)
    spheres[:, :, :3] = eye[:, None, :]
    return spheres.reshape(-1, 4), vel.reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rays', type=int, default=64)
    ap.add_argument('--range', type=float, default=30.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import rust_doom_amd as rd
    from test_gpu_world import _players
    from util import META_PATH, ensure_big_wad, ensure_wad
    rd.set_device(0)
    fan_np = rd.ray_fan(a.rays, 2.0)
    fan = torch.from_numpy(fan_np).cuda()
    rows = []
    for label, path in (('E1M1', ensure_wad()), ('10x', ensure_big_wad())):
        wad = rd.Wad(path, META_PATH)
        built = wad.build_level(0)
        world = wad.build_world(0)
        for n in (4096, 65536):
            st = _players(built, n, seed=n)
            states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
            frac = torch.empty((n, a.rays), dtype=torch.float32, device='cuda')
            origin = torch.empty((n, a.rays, 3), dtype=torch.float32, device='cuda')
            vel = torch.empty_like(origin)
            world.cast_rays(states, fan, a.range, frac_out=frac, origin_out=origin, vel_out=vel)
            spheres = torch.cat([origin.view(-1, 3), torch.zeros((n * a.rays, 1), dtype=torch.float32, device='cuda')], 1).contiguous()
            vels = vel.view(-1, 3).contiguous()
            cast = _median_ms(lambda: world.cast_rays(states, fan, a.range, frac_out=frac), a.warmup, a.steps)
            sweep = _median_ms(lambda: world.sweep(spheres, vels), a.warmup, a.steps)

            def old_path():
                host = states.cpu().numpy().view(rd.PLAYER_STATE).reshape(-1)
                s, v = _host_rays(host, fan_np, a.range)
                world.sweep(torch.from_numpy(s).cuda(), torch.from_numpy(v).cuda())
            full = _median_ms(old_path, a.warmup, a.steps)
            swept = world.sweep(spheres, vels)[:, 0]
            torch.cuda.synchronize()
            same = float((torch.where(swept <= 1.0, swept, torch.full_like(swept, float('inf'))).view(torch.int32)
                          == frac.view(-1).view(torch.int32)).float().mean().item())
            rays = n * a.rays
            rows.append(dict(level=label, players=n, rays=a.rays, max_range=a.range, cast_ms=cast[0], cast_ms_min=cast[1],
                             cast_ms_max=cast[2], sweep_ms=sweep[0], sweep_ms_min=sweep[1], sweep_ms_max=sweep[2],
                             sweep_with_host_ms=full[0], cast_ns_per_ray=cast[0] * 1e6 / rays, sweep_ns_per_ray=sweep[0] * 1e6 / rays,
                             sweep_with_host_ns_per_ray=full[0] * 1e6 / rays, sweep_over_cast=sweep[0] / cast[0],
                             hit_share=float(torch.isfinite(frac).float().mean().item()), same_as_sweep=same))
    print('%-6s %8s %5s %10s %12s %12s %14s %12s' % ('level', 'players', 'rays', 'cast ms', 'cast ns/ray', 'sweep ns/ray',
                                                      'sweep+host ns', 'sweep / cast'))
    for r in rows:
        print('%-6s %8d %5d %10.3f %12.3f %12.3f %14.3f %12.2f' % (r['level'], r['players'], r['rays'], r['cast_ms'], r['cast_ns_per_ray'],
                                                                 r['sweep_ns_per_ray'], r['sweep_with_host_ns_per_ray'],
                                                                 r['sweep_over_cast']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
