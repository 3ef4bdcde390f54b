#!/usr/bin/env python3
"""Cost of a clock per player: one E1M1 tick -- step_game (1 tick) -> render_players -> resolve_rgb -- for N players, three ways:

  a  frozen   render_players with the light table of time 0 uploaded once (what the device loop did before the clocked render)
  b  host     the same, with BuiltLevel.lights_at(t) evaluated on the host and uploaded every tick, one time for all players
  c  clocked  render_players(states, DeviceLights, times=...): `times += dt` on the stream, tables evaluated by the light kernel

closed_loop_cost.py's method: frames in chunks of a 1 GiB frame budget, one warm-up tick, the median wall ms of `--ticks` ticks.
`a` runs twice (a, a2): their difference is the run-to-run spread the other differences are read against.  One JSON line per
measurement; DESIGN section 15 quotes profiles/clock_cost.jsonl.  GPU box.

    python tools/clock_cost.py [--players 4096,65536] [--sizes 320x200,1920x1080] [--ticks 3] [--out profiles/clock_cost.jsonl]
"""
import argparse
import json
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
from closed_loop_cost import FRAME_BUDGET, inputs  # noqa: E402
from util import META_PATH, ensure_wad  # noqa: E402

DT = 1.0 / 60.0


def run(n, w, h, ticks, variant, chunk):
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    level = rd.DeviceLevel(built)
    world = wad.build_world(0)
    rng = np.random.default_rng(n)
    pos, yaw = built.start()
    st = rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.float32(yaw) + rng.normal(size=n).astype(np.float32))
    game, offs = world.game_state(n)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    inp, act = inputs(n, ticks + 1, 7)
    ti = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda()
    ta = torch.from_numpy(act.reshape(-1).copy()).cuda()
    lights = torch.from_numpy(built.lights_at(0.0).copy()).cuda()
    staging = torch.empty(256, dtype=torch.uint8).pin_memory()
    dlights = rd.DeviceLights([built])
    times = torch.from_numpy(rng.uniform(0.0, 60.0, n).astype(np.float32)).cuda()
    batch = rd.Batch(level, w, h, chunk)
    rgb = torch.empty((chunk, h, w, 3), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()

    def tick(k):
        t = k * DT
        with torch.cuda.stream(stream):
            if variant == 'b':
                staging.copy_(torch.from_numpy(built.lights_at(t)))
                lights.copy_(staging, non_blocking=True)
            elif variant == 'c':
                times.add_(DT)
        world.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=stream)
        for c in range(0, n, chunk):
            m = min(chunk, n - c)
            if variant == 'c':
                batch.render_players(states[c * 40:(c + m) * 40], dlights, offsets=offs[c:c + m], times=times[c:c + m], stream=stream)
            else:
                batch.render_players(states[c * 40:(c + m) * 40], lights, offsets=offs[c:c + m], time=t if variant == 'b' else 0.0,
                                     stream=stream)
            batch.resolve_rgb(rgb[:m], stream=stream)
        stream.synchronize()

    torch.cuda.synchronize()
    tick(0)  # warm-up: first-use allocations
    walls = []
    for k in range(1, ticks + 1):
        t0 = time.perf_counter()
        tick(k)
        walls.append((time.perf_counter() - t0) * 1e3)
    batch.finish()
    return float(np.median(walls)), walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', default='4096,65536')
    ap.add_argument('--sizes', default='320x200,1920x1080')
    ap.add_argument('--ticks', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rd.set_device(0)
    out = open(args.out, 'a') if args.out else None
    for n in [int(x) for x in args.players.split(',')]:
        for size in args.sizes.split(','):
            w, h = (int(x) for x in size.split('x'))
            chunk = min(n, max(64, FRAME_BUDGET // (w * h)))
            for name, variant in (('a', 'a'), ('b', 'b'), ('c', 'c'), ('a2', 'a')):
                wall, walls = run(n, w, h, args.ticks, variant, chunk)
                line = json.dumps(dict(level='E1M1', players=n, frame=size, variant=name, chunk=chunk, ticks=args.ticks,
                                       wall_ms_per_tick=round(wall, 3), walls_ms=[round(x, 3) for x in walls]))
                print(line, flush=True)
                if out:
                    out.write(line + '\n')
                    out.flush()


if __name__ == '__main__':
    main()
