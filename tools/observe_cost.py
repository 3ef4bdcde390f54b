#!/usr/bin/env python3
"""What the reduced-size observations cost on the GPU (rdoom_batch_resolve_observation), in the style of
tools/rgb_cost.py / tools/plane_cost.py: E1M1 (synthetic IWAD), the pose sweep bench.py renders, 1024 poses at 1920 x 1080 and
1024 at 640 x 400, rendered once.  Then, per size, every format at factors 2, 4 and 8, and next to them what they replace:
resolve_rgb and resolve_depth alone, and each followed by the torch pooling into the same shape (avg_pool2d of the float frame,
-max_pool2d(-depth)).  Every figure is the median of --reps single passes after --warmup, each bracketed by an event pair on
one stream.  Prints one JSON line per figure and writes them to profiles/observe_cost.jsonl.  Needs the GPU and torch.

    python tools/observe_cost.py [--reps 20] [--warmup 3] [--poses 1024] [--sizes 1920x1080,640x400]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/observe_cost.py --reps 3 --sizes 1920x1080    (the kernels' own times)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--poses', type=int, default=1024)
    ap.add_argument('--sizes', default='1920x1080,640x400')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'observe_cost.jsonl'))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import rust_doom_amd as rd
    from util import META_PATH, ensure_wad
    sharding = importlib.import_module('rust-doom_amd.sharding')
    rd.set_device(0)
    n = a.poses
    built = rd.Wad(ensure_wad(), META_PATH).build_level(0)
    level = rd.DeviceLevel(built)
    stream = torch.cuda.current_stream()
    lines = []

    def timed(what, fn, **fields):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec = dict(what=what, poses=n, **fields, ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                   timing='event pair on one stream around one pass, median of %d after %d warm-ups' % (a.reps, a.warmup))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for size in a.sizes.split(','):
        w, h = (int(v) for v in size.split('x'))
        batch = rd.Batch(level, w, h, n)
        batch.render(sharding.pose_sweep(rd, built, n, w, h), built.lights_at(0.0))
        batch.finish()
        st = batch.path_stats()
        common = dict(width=w, height=h, described_quadrants_pct=round(100.0 * st['described_quadrants'] / max(1, st['quadrants']), 1))
        rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda')
        depth = torch.empty((n, h, w), dtype=torch.float32, device='cuda')
        timed('resolve_rgb', lambda: batch.resolve_rgb(rgb, stream=stream), **common)
        timed('resolve_depth', lambda: batch.resolve_depth(depth, stream=stream), **common)
        for f in (2, 4, 8):
            def rgb_pool():
                batch.resolve_rgb(rgb, stream=stream)
                return F.avg_pool2d(rgb.permute(0, 3, 1, 2).float(), f).add_(0.5).to(torch.uint8)

            def depth_pool():
                batch.resolve_depth(depth, stream=stream)
                return -F.max_pool2d(-depth, f)

            timed('resolve_rgb + avg_pool2d', rgb_pool, factor=f, **common)
            timed('resolve_depth + max_pool2d', depth_pool, factor=f, **common)
            for name, fmt in (('OBS_RGB8', rd.OBS_RGB8), ('OBS_RGB8_PLANAR', rd.OBS_RGB8_PLANAR), ('OBS_GRAY8', rd.OBS_GRAY8),
                              ('OBS_DEPTH_MIN', rd.OBS_DEPTH_MIN)):
                shape = (n,) + rd.observation_shape(fmt, w, h, f)
                out = torch.empty(shape, dtype=torch.float32 if fmt == rd.OBS_DEPTH_MIN else torch.uint8, device='cuda')
                timed('resolve_observation ' + name, lambda: batch.resolve_observation(out, fmt, f, stream=stream), factor=f, **common)
                del out
        del rgb, depth
        batch.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
