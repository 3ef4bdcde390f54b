#!/usr/bin/env python3
"""What the depth / label / primitive planes cost on the GPU (rdoom_batch_resolve_plane alone), modelled on
tools/rgb_cost.py and meant to be run beside it in one session: E1M1 (synthetic IWAD), the pose sweep bench.py renders, rendered
once; then K resolves of every frame's plane into one device buffer, bracketed by rdoom_batch_finish, repeated R times.  Prints
one JSON line per plane: median / min / max ms per pass over the repetitions, and the effective bytes per second counting what
the pass must move -- the visibility words read in the quadrants the table does not describe (2 B/px there) and the plane
written (depth 4, label 2, primitive 4 B/px); the record gathers come on top and are not counted.  Needs the GPU and torch.

    python tools/plane_cost.py [--steps K] [--warmup W] [--reps R] [--poses N] [--width W --height H]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plane_cost.py --steps 3 --reps 1     (the kernels' own times)
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--poses', type=int, default=1024)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    a = ap.parse_args()
    import torch

    import rust_doom_amd as rd
    from util import META_PATH, ensure_wad
    sharding = importlib.import_module('rust-doom_amd.sharding')
    rd.set_device(0)
    w, h, n = a.width, a.height, a.poses
    built = rd.Wad(ensure_wad(), META_PATH).build_level(0)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    batch.render(sharding.pose_sweep(rd, built, n, w, h), built.lights_at(0.0))
    batch.finish()
    st = batch.path_stats()
    px = n * w * h
    vis_px = px * (st['quadrants'] - st['described_quadrants']) / max(1, st['quadrants'])
    out = torch.empty(px, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    for name, plane, elem in (('depth', rd.PLANE_DEPTH, 4), ('label', rd.PLANE_LABEL, 2), ('primitive', rd.PLANE_PRIMITIVE, 4)):
        ptr = out.data_ptr()
        for _ in range(a.warmup):
            batch.resolve_plane(ptr, plane)
        batch.finish()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                batch.resolve_plane(ptr, plane)
            batch.finish()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = statistics.median(ms)
        moved = vis_px * 2 + px * elem
        print(json.dumps({'plane': name, 'poses': n, 'width': w, 'height': h, 'steps': a.steps, 'reps': a.reps,
                          'ms_per_pass': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3),
                          'bytes_per_pixel': round(moved / px, 3), 'bytes_per_pass': int(moved),
                          'effective_TB_per_s': round(moved / med / 1e9, 3),
                          'described_quadrants_pct': round(100.0 * st['described_quadrants'] / max(1, st['quadrants']), 1),
                          'timing': 'host clock around %d passes ended by rdoom_batch_finish, median of %d' % (a.steps, a.reps)}), flush=True)


if __name__ == '__main__':
    main()
