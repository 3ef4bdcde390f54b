#!/usr/bin/env python3
"""Cost of one closed-loop tick -- step_game (1 tick) -> render -> resolve_rgb -- for N players, through the host path (states,
levels and offsets copied to the host, one camera and one object-matrix call per player, constants rebuilt and uploaded by the
renderer) and through Batch.render_players (nothing leaves the device).  E1M1 alone (World) and the E1M1..E1M3 world set.  Prints
the median wall ms per tick and the host CPU ms per tick (process time, every thread).  Frames are rendered in chunks of a batch
of as many poses as fit a 1 GiB frame budget, each chunk resolved to RGB into one preallocated tensor.  GPU box.

    python tools/closed_loop_cost.py [--players 4096,65536] [--sizes 320x200,1920x1080] [--ticks 3] [--paths host,device]

The new kernel's share of the render: run once under `rocprofv3 --kernel-trace --stats -- python tools/closed_loop_cost.py
--paths device ...` and compare player_frames_kernel's total with the other render kernels' (DESIGN section 12).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import rust_doom_amd as rd  # noqa: E402
from util import META_PATH, ensure_wad  # noqa: E402

FRAME_BUDGET = 1 << 30  # bytes of palette-index frames per chunk


def inputs(n, ticks, seed):
    rng = np.random.default_rng(seed)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    inp['movement'][..., 1] = -1.0
    inp['look'][..., 0] = rng.normal(scale=0.02, size=(ticks, n)).astype(np.float32)
    act = (rng.random((ticks, n)) < 0.05).astype(np.uint8) * rd.ACTION_PUSH
    return inp, act


def run(scenario, n, w, h, ticks, path, chunk):
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0] if scenario == 'E1M1' else [0, 1, 2]
    built = [wad.build_level(i) for i in slots]
    level = rd.DeviceLevel(built[0]) if len(slots) == 1 else rd.DeviceLevelSet(built)
    n_obj = level.num_objects()
    rng = np.random.default_rng(n)
    if len(slots) == 1:
        world = wad.build_world(0)
        pos, yaw = built[0].start()
        st = rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.float32(yaw) + rng.normal(size=n).astype(np.float32))
        game, offs = world.game_state(n)
        levels = None
    else:
        world = wad.build_world_set(slots)
        lv = rng.integers(0, 3, n)
        st = world.start_states(lv)
        st['yaw'] += rng.normal(size=n).astype(np.float32)
        game, offs, levels = world.game_state(lv)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    inp, act = inputs(n, ticks + 1, 7)
    ti = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda()
    ta = torch.from_numpy(act.reshape(-1).copy()).cuda()
    table = np.stack([b.lights_at(0.0) for b in built])
    lights = torch.from_numpy(table).cuda()
    batch = rd.Batch(level, w, h, chunk)
    rgb = torch.empty((chunk, h, w, 3), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()

    def step(k, s):
        a = dict(actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=s)
        if levels is None:
            world.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, **a)
        else:
            world.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, levels, **a)

    def tick_host(k):
        step(k, None)
        lop = levels.cpu().numpy().astype(np.uint32) if levels is not None else np.zeros(n, np.uint32)
        sh = states.cpu().numpy().view(rd.PLAYER_STATE)
        poses = rd.poses_from_players(sh, w, h)
        mvs = rd.object_modelviews_from_players(sh, offs)[:, :n_obj]
        for c in range(0, n, chunk):
            m = min(chunk, n - c)
            kw = dict(object_modelviews=mvs[c:c + m])
            if levels is not None:
                kw['level_of_pose'] = lop[c:c + m]
            batch.render(poses[c:c + m], table[lop[c:c + m]] if levels is not None else table[0], **kw)
            batch.resolve_rgb(rgb[:m])
        torch.cuda.synchronize()

    def tick_device(k):
        step(k, stream)
        for c in range(0, n, chunk):
            m = min(chunk, n - c)
            batch.render_players(states[c * 40:(c + m) * 40], lights, levels=levels[c:c + m] if levels is not None else None,
                                 offsets=offs[c:c + m], stream=stream)
            batch.resolve_rgb(rgb[:m], stream=stream)
        stream.synchronize()

    tick = tick_host if path == 'host' else tick_device
    torch.cuda.synchronize()
    tick(0)  # warm-up: first-use allocations
    walls, cpus = [], []
    for k in range(1, ticks + 1):
        t0, c0 = time.perf_counter(), time.process_time()
        tick(k)
        walls.append((time.perf_counter() - t0) * 1e3)
        cpus.append((time.process_time() - c0) * 1e3)
    batch.finish()
    return float(np.median(walls)), float(np.median(cpus))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', default='4096,65536')
    ap.add_argument('--sizes', default='320x200,1920x1080')
    ap.add_argument('--scenarios', default='E1M1,E1M1-E1M3')
    ap.add_argument('--paths', default='host,device')
    ap.add_argument('--ticks', type=int, default=3)
    args = ap.parse_args()
    rd.set_device(0)
    print('%-12s %7s %10s %-7s %7s %12s %12s' % ('levels', 'players', 'frame', 'path', 'chunk', 'wall ms/tick', 'cpu ms/tick'))
    for scenario in args.scenarios.split(','):
        for n in [int(x) for x in args.players.split(',')]:
            for size in args.sizes.split(','):
                w, h = (int(x) for x in size.split('x'))
                chunk = min(n, max(64, FRAME_BUDGET // (w * h)))
                for path in args.paths.split(','):
                    wall, cpu = run(scenario, n, w, h, args.ticks, path, chunk)
                    print('%-12s %7d %10s %-7s %7d %12.2f %12.2f' % (scenario, n, size, path, chunk, wall, cpu), flush=True)


if __name__ == '__main__':
    main()
