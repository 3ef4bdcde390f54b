#!/usr/bin/env python3
"""What things in the frame cost on the GPU, modelled on tools/plane_cost.py: E1M1 (synthetic IWAD), the pose
sweep bench.py renders, rendered once; then K passes of each call, bracketed by a wait for the device, repeated R times; the median
over the repetitions.  Two groups of JSON lines, one per call:

  resolve_thing_plane next to resolve_plane(LABEL) and resolve_plane(PRIMITIVE) on the same frames -- the yardsticks: the same
  reads of the table and the visibility words, the label with the same second gather, 2 and 4 B/px written;

  frame_things with and without the depth plane next to a device copy of the bytes it reads, and next to a torch formulation of
  the same contract (bincount of frame * max_things + id, scatter_reduce amin / amax of columns, rows and depth bits), which is
  first checked equal to the kernel on 8 frames.  The torch formulation makes int64 keys and coordinates of every pixel in range, so
  it is timed on --torch-frames frames and its row says so (ms_per_pass is of those frames; ms_scaled is scaled to all).

    python tools/framethings_cost.py [--steps K] [--warmup W] [--reps R] [--poses N] [--width W --height H] [--out FILE]
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

INF_BITS = 0x7F800000
INT32_MAX = 0x7FFFFFFF


def torch_frame_things(torch, ids, depth, max_things, min_pixels):
    """the contract of rdoom_frame_things in torch: (table (n, max_things, 6) int32, bits (n, words) int32)"""
    n, h, w = ids.shape
    dev = ids.device
    valid = (ids >= 0) & (ids < max_things)
    frame = torch.arange(n, device=dev).view(n, 1, 1) * max_things
    key = (frame + ids)[valid]
    ys = torch.arange(h, device=dev).view(1, h, 1).expand(n, h, w)[valid]
    xs = torch.arange(w, device=dev).view(1, 1, w).expand(n, h, w)[valid]
    total = n * max_things
    count = torch.bincount(key, minlength=total)

    def fold(init, values, how, k=key):
        return torch.full((total,), init, dtype=torch.int64, device=dev).scatter_reduce(0, k, values, how)
    cols = [count, fold(INT32_MAX, xs, 'amin'), fold(INT32_MAX, ys, 'amin'), fold(-1, xs, 'amax'), fold(-1, ys, 'amax')]
    if depth is None:
        cols.append(torch.full((total,), INF_BITS, dtype=torch.int64, device=dev))
    else:
        d = depth.view(torch.int32)[valid].to(torch.int64)
        ok = (d >= 0) & (d < INF_BITS)  # the bit pattern, as a uint32, below +inf's: finite and not negative
        cols.append(fold(INF_BITS, d[ok], 'amin', key[ok]))
    table = torch.stack(cols, 1).to(torch.int32).view(n, max_things, 6)
    words = (max_things + 31) // 32
    flags = torch.zeros((n, words * 32), dtype=torch.int64, device=dev)
    flags[:, :max_things] = (count.view(n, max_things) >= min_pixels).to(torch.int64)
    bits = (flags.view(n, words, 32) << torch.arange(32, device=dev)).sum(2)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return table, bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--poses', type=int, default=1024)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--torch-frames', type=int, default=32)
    ap.add_argument('--min-pixels', type=int, default=12)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    import torch

    import rust_doom_amd as rd
    from util import META_PATH, ensure_wad
    sharding = importlib.import_module('rust-doom_amd.sharding')
    rd.set_device(0)
    w, h, n = a.width, a.height, a.poses
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    max_things = 32 * ((len(wad.build_world(0, device=False).map_things()) + 31) // 32)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    batch.render(sharding.pose_sweep(rd, built, n, w, h), built.lights_at(0.0))
    batch.finish()
    st = batch.path_stats()
    px = n * w * h
    common = {'poses': n, 'width': w, 'height': h, 'steps': a.steps, 'reps': a.reps,
              'described_quadrants_pct': round(100.0 * st['described_quadrants'] / max(1, st['quadrants']), 1)}

    def emit(row):
        line = json.dumps(dict(row, **common))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')

    def timed(fn, wait):
        for _ in range(a.warmup):
            fn()
        wait()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            wait()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        return {'ms_per_pass': round(statistics.median(ms), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3)}

    thing_px = torch.empty((n, h, w), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    # ---- the plane, next to the label and the primitive plane of the same frames
    ptr = thing_px.data_ptr()
    rows = {}
    for name, fn, elem in (('label', lambda: batch.resolve_plane(ptr, rd.PLANE_LABEL), 2),
                           ('primitive', lambda: batch.resolve_plane(ptr, rd.PLANE_PRIMITIVE), 4),
                           ('thing', lambda: batch.resolve_thing_plane(ptr, top_down=True), 4)):
        rows[name] = dict(timed(fn, batch.finish), call='resolve_' + name + '_plane', bytes_written_per_pixel=elem,
                          timing='host clock around %d passes ended by rdoom_batch_finish, median of %d' % (a.steps, a.reps))
    for name in ('label', 'primitive', 'thing'):
        rows[name]['thing_over_this'] = round(rows['thing']['ms_per_pass'] / rows[name]['ms_per_pass'], 3)
        emit(rows[name])
    # ---- the reduction, next to a device copy of what it reads and a torch formulation
    depth = torch.empty((n, h, w), dtype=torch.float32, device='cuda')
    batch.resolve_thing_plane(thing_px, top_down=True)
    batch.resolve_depth(depth, top_down=True)
    batch.finish()
    in_range = int(((thing_px >= 0) & (thing_px < max_things)).sum())
    table = torch.empty((n, max_things, 6), dtype=torch.int32, device='cuda')
    bits = torch.empty((n, max_things // 32), dtype=torch.int32, device='cuda')
    k = min(8, n)
    for d in (None, depth[:k]):  # the torch formulation is the kernel's contract: equal on 8 frames
        t_k, b_k = rd.frame_things(thing_px[:k], d, max_things=max_things, min_pixels=a.min_pixels)
        t_t, b_t = torch_frame_things(torch, thing_px[:k], d, max_things, a.min_pixels)
        torch.cuda.synchronize()
        assert torch.equal(t_k, t_t) and torch.equal(b_k, b_t), 'the torch formulation differs from the kernel'
    copy_ids, copy_depth = torch.empty_like(thing_px), torch.empty_like(depth)
    wait = torch.cuda.synchronize
    timing = 'host clock around %d passes ended by a device synchronize, median of %d' % (a.steps, a.reps)
    res = {}
    res['copy_ids'] = dict(timed(lambda: copy_ids.copy_(thing_px), wait), call='device copy of the ids', bytes_read=4 * px)
    res['copy_ids_depth'] = dict(timed(lambda: (copy_ids.copy_(thing_px), copy_depth.copy_(depth)), wait), call='device copy of ids and depth',
                                 bytes_read=8 * px)
    del copy_ids, copy_depth
    kw = dict(max_things=max_things, min_pixels=a.min_pixels, table_out=table, bits_out=bits)
    res['frame_things'] = dict(timed(lambda: rd.frame_things(thing_px, None, **kw), wait), call='frame_things without depth', bytes_read=4 * px)
    res['frame_things_depth'] = dict(timed(lambda: rd.frame_things(thing_px, depth, **kw), wait), call='frame_things with depth', bytes_read=8 * px)
    res['frame_things']['over_copy'] = round(res['frame_things']['ms_per_pass'] / res['copy_ids']['ms_per_pass'], 3)
    res['frame_things_depth']['over_copy'] = round(res['frame_things_depth']['ms_per_pass'] / res['copy_ids_depth']['ms_per_pass'], 3)
    tf = min(a.torch_frames, n)
    for name, d in (('torch', None), ('torch_depth', depth[:tf])):
        r = timed(lambda: torch_frame_things(torch, thing_px[:tf], d, max_things, a.min_pixels), wait)
        res[name] = dict(r, call='torch formulation' + (' with depth' if d is not None else ''), frames_timed=tf,
                         ms_scaled=round(r['ms_per_pass'] * n / tf, 3))
    res['torch']['over_kernel'] = round(res['torch']['ms_scaled'] / res['frame_things']['ms_per_pass'], 1)
    res['torch_depth']['over_kernel'] = round(res['torch_depth']['ms_scaled'] / res['frame_things_depth']['ms_per_pass'], 1)
    for name in ('copy_ids', 'frame_things', 'torch', 'copy_ids_depth', 'frame_things_depth', 'torch_depth'):
        emit(dict(res[name], max_things=max_things, min_pixels=a.min_pixels, pixels_in_range_pct=round(100.0 * in_range / px, 2), timing=timing))


if __name__ == '__main__':
    main()
