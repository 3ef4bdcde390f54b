#!/usr/bin/env python3
"""The fragment kernel's own census of its listed quads (hook frag_count=1 -> rdoom_batch_path_stats) for the sweep bench.py renders:
E1M1 (synthetic IWAD), 1024 poses, 1920 x 1080, rendered once with half lanes (the default) and once with the hook no_half_runs=1
(both quads of every run an edge crosses are listed, as before round 8).  One JSON line: half lanes that finished their uniform
quad, half lanes that fell back, listed quads of both renders and their ratio.  Needs the GPU.

    python tools/half_runs_census.py [--poses N] [--width W] [--height H] [--big]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=1024)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--big', action='store_true', help='the 10x-E1M1 synthetic level')
    a = ap.parse_args()
    import rust_doom_amd as rd
    from util import META_PATH, ensure_big_wad, ensure_wad
    sharding = importlib.import_module('rust-doom_amd.sharding')
    rd.set_device(0)
    w, h, n = a.width, a.height, a.poses
    built = rd.Wad(ensure_big_wad() if a.big else ensure_wad(), META_PATH).build_level(0)
    level = rd.DeviceLevel(built)
    poses, lights = sharding.pose_sweep(rd, built, n, w, h), built.lights_at(0.0)
    out = {'poses': n, 'width': w, 'height': h, 'big': a.big}
    for name, hooks in (('half_lanes', {}), ('no_half_runs', {'no_half_runs': 1})):
        try:
            rd.debug_set('frag_count', 1)
            for k, v in hooks.items():
                rd.debug_set(k, v)
            batch = rd.Batch(level, w, h, n)
            batch.render(poses, lights)
            st = batch.path_stats()
        finally:
            rd.debug_set('reset')
        out[name] = {k: st[k] for k in ('half_runs', 'half_fallbacks', 'listed_quads')}
        del batch
    runs = n * (w // 8) * h
    hl, old = out['half_lanes'], out['no_half_runs']
    mixed = hl['half_runs'] + hl['half_fallbacks']  # (mixed runs with a uniform quad; those without one are not counted apart)
    out['runs'] = runs
    out['half_lane_pct_of_runs'] = round(100.0 * mixed / runs, 3)
    out['listed_quads_ratio'] = round(hl['listed_quads'] / max(1, old['listed_quads']), 4)
    out['quads_per_half_lane'] = round((2 * mixed - hl['half_runs']) / max(1, mixed), 4)  # 2.0 before; the CPU census predicted 1.045 per mixed run
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
