"""Child process of tests/test_gpu_stamp.py (prints one RESULT line): draw_area_planes, stamp_things, inflate_grids and flood_grids on
a side stream given as a torch stream and as a raw handle, into the caller's tensors and through raw device pointers; two players
who walk over one solid thing a tick apart, with sense_things and stamp_things(hidden=collected) queued tick after tick on one
stream and no host wait; and a captured graph of planes, stamp, inflation and flood -- those four launches and nothing else --
replayed twice with the hidden rows changed between the replays.  Every plane is held against tests/stamp_ref.py.  torch is
initialised BEFORE the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import goal_ref
import rust_doom_amd as rd
import sector_ref
import stamp_cases as sc
import stamp_ref

U = np.uint32
F = np.float32
N = 3


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    cell = sc.E2E_CELL
    wad = sc.e1m1_wad()
    world = wad.build_world(0)
    host = wad.build_world(0, device=False)
    tables, g = sector_ref.Tables(host), world.area_grid(cell)
    at = [goal_ref.level_sectors(tables, g, cell)]
    table = world.map_things()
    things = rd.DeviceThings(table)
    words = things.words()
    solid_np = rd.pack_things(world.thing_obstacles()).view(U)[None]
    rng = np.random.default_rng(4)
    off = sector_ref.random_offsets(rng, N, world.game_objects)
    off[0] = 0
    seeds = np.tile(np.array([sc.E2E_SEED], np.int32), (N, 1))
    hides = [sc.bit_rows([[], [0], list(sc.E1M1_BARRELS)], words), sc.bit_rows([list(sc.E1M1_BARRELS), [], [1, 4]], words)]
    _, floor_np, ceiling_np = goal_ref.planes(tables, g, cell, N, offsets=off, at_centres=at)
    want = []
    for hidden in hides:
        stamped = stamp_ref.stamp(table, g, cell, floor_np, ceiling_np, solid=solid_np, hidden=hidden, offsets=off)
        planes, flood = sc.flood_to_start(stamped[0], stamped[1], seeds)
        want.append(stamped + planes + flood)
    assert (want[0][2] != want[1][2]).any() and (want[0][5] != want[1][5]).any() and (want[0][6] > 1000).all()

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    u32 = lambda t: t.cpu().numpy().view(U)
    offsets, cells, solid = dev(off), dev(seeds), dev(solid_np.view(np.int32))
    hidden = dev(hides[0].view(np.int32))
    h, w = world.area_plane_shape(cell)
    floor, ceiling = torch.full((N, h, w), 7.0, device='cuda'), torch.full((N, h, w), 7.0, device='cuda')
    fi, ci = torch.full((N, h, w), 7.0, device='cuda'), torch.full((N, h, w), 7.0, device='cuda')
    index = torch.full((N, h, w), 7, dtype=torch.int32, device='cuda')
    dist = torch.full((N, h, w), 7, dtype=torch.int32, device='cuda')
    cnt = torch.full((N,), 7, dtype=torch.int32, device='cuda')

    def same(ref, what, with_index=True):
        for got, k in ((floor, 0), (ceiling, 1), (index, 2), (fi, 3), (ci, 4), (dist, 5), (cnt, 6)):
            if got is index and not with_index:
                continue
            assert np.array_equal(u32(got), np.ascontiguousarray(ref[k]).view(U)), (what, k)

    def reset():
        for t in (floor, ceiling, fi, ci, index, dist, cnt):
            t.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False, with_index=True):
        """the reset-time recipe: planes, the stamp in place, inflation, the flood"""
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        world.draw_area_planes(cell, offsets=offsets, floor=floor, ceiling=ceiling, stream=stream)
        got = world.stamp_things(floor, ceiling, things, cell, solid=ptr(solid), hidden=ptr(hidden), offsets=ptr(offsets), floor_out=ptr(floor),
                                 ceiling_out=ptr(ceiling), index_out=ptr(index) if with_index else None, stream=stream,
                                 n_objects=int(offsets.shape[1]) if raw else None, stride=words if raw else None)
        assert len(got) == (3 if with_index else 2) and (raw or (got[0] is floor and got[1] is ceiling))
        rd.inflate_grids(floor, ceiling, sc.BODY, cell, floor_out=fi, ceiling_out=ci, stream=stream)
        rd.flood_grids(fi, ci, cells, towards=True, max_step=sc.E2E_STEP, dist_out=dist, count_out=cnt, stream=stream)

    # ---- a side stream, the caller's tensors, raw pointers and a raw stream handle
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    tick(side)
    side.synchronize()
    same(want[0], 'a side stream, the caller\'s tensors')
    reset()
    tick(side.cuda_stream, raw=True)
    side.synchronize()
    same(want[0], 'raw pointers, the stream as a raw handle')
    reset()
    tick(side, with_index=False)
    side.synchronize()
    same(want[0], 'the planes alone', with_index=False)
    assert (index.cpu().numpy() == 7).all()  # not asked for, not written

    # ---- two players walk over one solid thing a tick apart: each row's cell opens in its player's own tick and not before
    candle = 17
    assert table['thing_type'][candle] == 34 and (table['category'][candle] & 0xFF) == rd.THING_AMMO
    t = table[candle]
    ticks, step = 24, 0.05
    walk = np.zeros((ticks, 2), rd.PLAYER_STATE)
    for k in range(ticks):
        for p in range(2):  # towards -z, player 1 one tick behind player 0
            pos = F([[t['x'], t['base'] + 0.33, t['z'] + 0.8 - step * max(k - p, 0)]])
            walk[k, p] = rd.player_states(pos, F([0.0]))[0]
    firm = dev(sc.bit_rows([[candle]], words).view(np.int32))  # the candle alone is solid here
    own = goal_ref.cells(g, cell, rd.player_states(F([[t['x'], 0.0, t['z']]]), F([0.0])))[0]
    assert floor_np[0, own[1], own[0]] < np.inf  # the candle stands on open floor
    steps = torch.from_numpy(walk.view(np.uint8).reshape(ticks, -1).copy()).cuda()
    states = torch.zeros_like(steps[0])
    collected = torch.zeros((2, words), dtype=torch.int32, device='cuda')
    base_f, base_c = dev(floor_np[:2]), dev(ceiling_np[:2])
    keep = dict(rows=torch.zeros((ticks, 2, words), dtype=torch.int32, device='cuda'), floor=torch.zeros((ticks, 2, h, w), device='cuda'),
                ceiling=torch.zeros((ticks, 2, h, w), device='cuda'), index=torch.zeros((ticks, 2, h, w), dtype=torch.int32, device='cuda'))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k in range(ticks):
            states.copy_(steps[k])
            world.sense_things(states, things, max_range=10.0, touch_below=1.0, touch_above=1.0, collect=(rd.THING_AMMO,), collected=collected,
                               stream=stream)
            world.stamp_things(base_f, base_c, things, cell, solid=firm, hidden=collected, floor_out=keep['floor'][k], ceiling_out=keep['ceiling'][k],
                               index_out=keep['index'][k], stream=stream)
            keep['rows'][k].copy_(collected)
    stream.synchronize()
    got_rows = u32(keep['rows'])
    got_it = (got_rows[:, :, candle >> 5] >> (candle & 31)) & 1  # (ticks, 2)
    assert got_it[0].tolist() == [0, 0] and got_it[-1].tolist() == [1, 1], got_it.T.tolist()
    first = [int(np.argmax(got_it[:, p])) for p in range(2)]
    assert first[1] == first[0] + 1 and (np.diff(got_it.astype(np.int64), axis=0) >= 0).all(), first
    kept_index, kept_floor = keep['index'].cpu().numpy(), keep['floor'].cpu().numpy()
    shut = np.isposinf(kept_floor[:, :, own[1], own[0]])  # (ticks, 2): the candle's own cell
    assert np.array_equal(shut, got_it == 0), (shut.T.tolist(), got_it.T.tolist())  # shut until its player's own tick, and not after
    assert shut[first[0] - 1].tolist() == [True, True] and shut[first[0]].tolist() == [False, True] and shut[first[1]].tolist() == [False, False]
    assert np.array_equal(kept_index[:, :, own[1], own[0]] == candle, shut)
    for k in sorted({0, first[0] - 1, first[0], first[1], ticks - 1}):  # whole planes around the pick-ups
        ref = stamp_ref.stamp(table, g, cell, floor_np[:2], ceiling_np[:2], solid=sc.bit_rows([[candle]], words), hidden=got_rows[k])
        for got, r in ((keep['floor'][k], ref[0]), (keep['ceiling'][k], ref[1]), (keep['index'][k], ref[2])):
            assert np.array_equal(u32(got), np.ascontiguousarray(r).view(U)), ('walk', k)

    # ---- a captured graph of the four launches (a call that waited or allocated could not be captured), replayed with the hidden
    # rows changed in between
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    reset()
    graph.replay()
    torch.cuda.synchronize()
    same(want[0], 'first replay')
    hidden.copy_(dev(hides[1].view(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    same(want[1], 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
