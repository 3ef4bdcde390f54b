#!/usr/bin/env python3
"""What drawing the things on the map costs: draw_thing_maps for 1024 players of E1M1 -- spread over the level's
floor -- at 160 x 120 and 320 x 200 pixels, 0.12 units a pixel, rotated and top-down, with hidden and known rows, against the level's
own thing table and against a scattered table of 600 things, timed with a pair of events around each launch on one stream -- the
median of --steps launches after --warmup.  The timed launch is the README tick's: RDOOM_THING_MARKS_OVER on the buffer draw_maps
filled.  Next to it draw_maps on the same players and view, and what a user had before: a torch formulation, one dense players x
pixels x things tensor expression of the same contract (the yaw's sine and cosine handed to it, the players taken a few at a time so
that its temporaries fit).  Before anything is timed, the kernel's bytes and indices are checked equal to the torch formulation's in
every map, and to tests/thingmap_ref.py's on row 0.
Prints a table and one JSON line per row, and appends the rows to --out (default profiles/thingmap_cost.jsonl).  Needs the GPU and
torch.

    python tools/thingmap_cost.py [--players 1024] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

SCALE, MIN_RADIUS = 0.12, 2.0
SIZES = ((160, 120), (320, 200))
TORCH_ELEMENTS = 1 << 27  # of one temporary of the torch formulation: the players of a chunk x the pixels x the things


def torch_draw(table, drawn, pos, sin, cos, width, height, scale, min_radius, codes):
    """(out uint8, index int32), both (n, height, width), of the header's contract in plain torch, rotated and top-down: every thing
    against every pixel of every player at once.  table: (T, 3) x, z, radius; drawn: (n, T) bool; pos: (n, 3); sin, cos: (n,);
    codes: (T,) int32.  Every operation is one rounded binary32 operation, in the header's order"""
    import torch
    t_n = table.shape[0]
    i = torch.arange(width, dtype=torch.float32, device=pos.device)
    j = torch.arange(height - 1, -1, -1, dtype=torch.float32, device=pos.device)  # top-down: row 0 is j = height - 1
    u = (((i + 0.5) - width * 0.5) * scale)[None, None, :]
    v = (((j + 0.5) - height * 0.5) * scale)[None, :, None]
    rp = torch.tensor(min_radius, dtype=torch.float32, device=pos.device) * scale
    r = torch.where(table[:, 2] > rp, table[:, 2], rp)
    r2 = (r * r)[None, :, None, None]
    key = (codes << 20) | (0xFFFFF - torch.arange(t_n, dtype=torch.int32, device=pos.device))
    chunk = max(1, TORCH_ELEMENTS // (width * height * t_n))
    outs = []
    for at in range(0, pos.shape[0], chunk):
        p, s, c = pos[at:at + chunk], sin[at:at + chunk, None, None], cos[at:at + chunk, None, None]
        qx = (p[:, 0, None, None] + c * u) + (-s) * v
        qz = (p[:, 2, None, None] + (-s) * u) + (-c) * v
        ex = qx[:, None] - table[None, :, 0, None, None]
        ez = qz[:, None] - table[None, :, 1, None, None]
        covers = (ex * ex + ez * ez <= r2) & drawn[at:at + chunk, :, None, None]
        outs.append(torch.where(covers, key[None, :, None, None], 0).amax(1))
    best = torch.cat(outs)
    return (best >> 20).to(torch.uint8), torch.where(best != 0, 0xFFFFF - (best & 0xFFFFF), -1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--players', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'thingmap_cost.jsonl'))
    a = ap.parse_args()

    import numpy as np
    import torch

    import rays_ref
    import rust_doom_amd as rd
    import things_ref
    import thingmap_ref
    import world_ref
    from automap_cost import _event_ms
    from util import META_PATH, ensure_wad
    rd.set_device(0)
    stream = torch.cuda.Stream()
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines, own = world.map_lines(), world.map_things()
    n = a.players
    st = np.array(rays_ref.players(wad.build_level(0), 100, count=n), rd.PLAYER_STATE)
    rng = np.random.default_rng(30)
    big = things_ref.make_table(rng, 600, things_ref.bounds_of(lines), np.stack([st['pos'][:, 0], st['pos'][:, 2]], 1))
    states = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
    t_pos = torch.from_numpy(st['pos'].astype(np.float32)).cuda()
    sc = np.array([world_ref.sincos(float(y)) for y in st['yaw']], np.float32)
    t_sin, t_cos = torch.from_numpy(sc[:, 0].copy()).cuda(), torch.from_numpy(sc[:, 1].copy()).cuda()
    rows = []
    for name, table in (('own', own), ('600', big)):
        things = rd.DeviceThings(table)
        words = things.words()
        rand = lambda: rng.integers(0, 1 << 32, (n, words), dtype=np.uint64).astype(np.uint32)
        hidden, known = rand() & rand() & rand(), rand() | rand()  # an eighth collected, three quarters seen so far
        d_hidden, d_known = (torch.from_numpy(r.view(np.int32)).cuda() for r in (hidden, known))
        is_drawn = np.stack([thingmap_ref.drawn(table, thingmap_ref.DEFAULT_CODES, hidden[p], known[p])[0] for p in range(n)])
        t_table = torch.from_numpy(np.stack([table['x'], table['z'], table['radius']], 1).astype(np.float32)).cuda()
        t_codes = torch.from_numpy((rd.MAP_THING + (table['category'] & 0xFF)).astype(np.int32)).cuda()
        t_drawn = torch.from_numpy(is_drawn).cuda()
        for width, height in SIZES:
            view = thingmap_ref.view_of(width, height, SCALE, rotate=True, top_down=True)
            kw = dict(hidden=d_hidden, known=d_known, min_radius=MIN_RADIUS, rotate=True, top_down=True)
            maps = torch.zeros((n, height, width), dtype=torch.uint8, device='cuda')
            index = torch.zeros((n, height, width), dtype=torch.int32, device='cuda')
            dense = lambda: torch_draw(t_table, t_drawn, t_pos, t_sin, t_cos, width, height, SCALE, MIN_RADIUS, t_codes)
            # the checks: every map against the torch formulation, row 0 against the reference
            with torch.cuda.stream(stream):
                world.draw_thing_maps(states, things, width, height, SCALE, out=maps, index_out=index, stream=stream, **kw)
            stream.synchronize()
            t_out, t_index = dense()
            torch.cuda.synchronize()
            for what, got, want in (('bytes', maps, t_out), ('indices', index, t_index)):
                if not torch.equal(got, want):
                    raise SystemExit('%s %dx%d: the torch formulation and the kernel differ in %d %s' % (name, width, height, int((got != want).sum()), what))
            want = thingmap_ref.draw(table, st[:1], view, min_radius=MIN_RADIUS, hidden=hidden[:1], known=known[:1])
            if not (np.array_equal(maps[:1].cpu().numpy(), want[0]) and np.array_equal(index[:1].cpu().numpy(), want[1])):
                raise SystemExit('%s %dx%d: row 0 and the reference differ' % (name, width, height))
            marked = float((index >= 0).float().mean())
            lines_only = lambda: world.draw_maps(states, width, height, SCALE, rotate=True, top_down=True, out=maps, stream=stream)
            marks = lambda: world.draw_thing_maps(states, things, width, height, SCALE, over=True, out=maps, stream=stream, **kw)
            with torch.cuda.stream(stream):
                lines_only()
            r = dict(level='E1M1', table=name, players=n, things=len(table), lines=len(lines), width=width, height=height, scale=SCALE,
                     min_radius=MIN_RADIUS, marked_pixels=marked, drawn_things=float(is_drawn.mean()))
            for key, call, on, steps, warmup in (('draw_thing_maps_ms', marks, stream, a.steps, a.warmup), ('draw_maps_ms', lines_only, stream, a.steps, a.warmup),
                                                 ('torch_ms', dense, torch.cuda.current_stream(), max(3, a.steps // 4), 1)):
                ms = _event_ms(call, on, warmup, steps)
                r[key], r[key + '_min'], r[key + '_max'] = ms
            r['torch_over_kernel'] = r['torch_ms'] / r['draw_thing_maps_ms']
            r['marks_over_lines'] = r['draw_thing_maps_ms'] / r['draw_maps_ms']
            rows.append(r)
        things.close()
    print('%-6s %7s %7s %9s %10s %10s %10s %8s' % ('table', 'players', 'things', 'pixels', 'marks ms', 'lines ms', 'torch ms', 'torch/k'))
    for r in rows:
        print('%-6s %7d %7d %4dx%-4d %10.4f %10.4f %10.3f %8.1f' % (r['table'], r['players'], r['things'], r['width'], r['height'],
                                                                  r['draw_thing_maps_ms'], r['draw_maps_ms'], r['torch_ms'], r['torch_over_kernel']))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
