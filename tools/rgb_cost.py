#!/usr/bin/env python3
"""What the RGB resolve costs on the GPU (rdoom_batch_resolve_rgb alone, DESIGN section "RGB frames"): E1M1 (synthetic IWAD), the
1024-pose 1920 x 1080 sweep bench.py renders, rendered once; then K resolves of all its frames into one device buffer, bracketed
by rdoom_batch_finish, for RGB8 and RGBA8.  Prints one JSON line per format: ms per resolve and the effective bytes per second,
counting what the pass must move -- the palette indices read (1 B/px), the visibility words read in the quadrants the table does
not describe (2 or 4 B/px there), the frames written (3 / 4 B/px).  Needs the GPU and torch (the output buffer).

    python tools/rgb_cost.py [--steps K] [--warmup W] [--poses N]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rgb_cost.py --steps 3     (the kernels' own times)
"""
import argparse
import importlib
import json
import os
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
    # visibility words are read in the quadrants the table does not describe (16-bit words: the level has < 65535 triangles)
    vis_px = px * (st['quadrants'] - st['described_quadrants']) / max(1, st['quadrants'])
    out = torch.empty(px * 4, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    for alpha in (False, True):
        bpp = 4 if alpha else 3
        view = out[:px * bpp]
        for _ in range(a.warmup):
            batch.resolve_rgb(view, alpha=alpha)
        batch.finish()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            batch.resolve_rgb(view, alpha=alpha)
        batch.finish()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        moved = px * 1 + vis_px * 2 + px * bpp
        print(json.dumps({'format': 'RGBA8' if alpha else 'RGB8', 'poses': n, 'width': w, 'height': h, 'steps': a.steps,
                          'ms_per_resolve': round(ms, 3), 'bytes_per_resolve': int(moved), 'effective_TB_per_s': round(moved / ms / 1e9, 3),
                          'described_quadrants_pct': round(100.0 * st['described_quadrants'] / max(1, st['quadrants']), 1),
                          'timing': 'host clock around %d resolves ended by rdoom_batch_finish' % a.steps}), flush=True)


if __name__ == '__main__':
    main()
