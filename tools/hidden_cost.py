#!/usr/bin/env python3
"""What hiding things per player costs the render: render_players of 1024 players of E1M1 -- spread over the
level's floor -- at 320 x 200 and at the benchmark's frame size, three ways: without rows, with all-zero rows, and with the bits of
half the level's things set in every row.  Each is timed with a pair of events around the render on one stream -- the median of
--steps renders after --warmup.  Before anything is timed, the frames with all-zero rows are checked equal to the frames without.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/hidden_cost.jsonl).  Needs the GPU and torch.

    python tools/hidden_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((320, 200), (1920, 1080))  # the small frame of BASELINE config 2; bench.py's default


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hidden_cost.jsonl'))
    a = ap.parse_args()
    import numpy as np
    import torch

    import rays_ref
    import rust_doom_amd as rd
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    level = rd.DeviceLevel(built)
    table = built.decor_things()
    n = a.players
    st = np.array(rays_ref.players(built, 100, count=n), rd.PLAYER_STATE)
    states = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
    lights = torch.from_numpy(built.lights_at(0.0).copy()).cuda()
    words = (int(table.max()) >> 5) + 1
    zero = torch.zeros((n, words), dtype=torch.int32, device='cuda')
    half_row = np.zeros(words, np.uint32)
    for t in table[::2].tolist():  # every other drawn thing
        half_row[t >> 5] |= np.uint32(1 << (t & 31))
    half = torch.from_numpy(np.repeat(half_row[None], n, 0).view(np.int32).copy()).cuda()
    rows = []
    for w, h in SIZES:
        batch = rd.Batch(level, w, h, n)
        render = lambda: batch.render_players(states, lights, stream=stream)
        frames = {}
        r = dict(level='E1M1', players=n, width=w, height=h, decor_quads=len(table), hidden_quads_half=len(table[::2]), words=words)
        for key, hidden in (('no_rows', None), ('zero_rows', zero), ('half_hidden', half)):
            batch.set_hidden_things(hidden)
            ms = _event_ms(render, stream, a.warmup, a.steps)
            r[key + '_ms'], r[key + '_ms_min'], r[key + '_ms_max'] = ms
            batch.finish()
            frames[key] = batch.read_framebuffer(0, min(n, 16))
        if not np.array_equal(frames['no_rows'], frames['zero_rows']):
            raise SystemExit('%dx%d: the frames with all-zero rows differ from the frames without rows' % (w, h))
        r['frames_changed_by_half'] = int((frames['no_rows'] != frames['half_hidden']).any((1, 2)).sum())
        r['zero_rows_over_no_rows'] = r['zero_rows_ms'] / r['no_rows_ms']
        r['half_hidden_over_no_rows'] = r['half_hidden_ms'] / r['no_rows_ms']
        rows.append(r)
        batch.close()
    print('%-10s %7s %10s %10s %10s %8s %8s' % ('frame', 'players', 'none ms', 'zero ms', 'half ms', 'zero/none', 'half/none'))
    for r in rows:
        print('%-10s %7d %10.4f %10.4f %10.4f %8.4f %8.4f' % ('%dx%d' % (r['width'], r['height']), r['players'], r['no_rows_ms'], r['zero_rows_ms'],
                                                             r['half_hidden_ms'], r['zero_rows_over_no_rows'], r['half_hidden_over_no_rows']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
