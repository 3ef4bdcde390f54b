"""Child process of tests/test_gpu_octile.py (prints one RESULT line): flood_grids_octile and descend_grids_octile on a side stream
given as a torch stream and as a raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a
captured graph of planes, flood and descent replayed twice with the doors' and lifts' offsets changed between the replays.  torch is
initialised BEFORE the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import goal_ref
import octile_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad

PATH_LEN = 9
STEP = 0.32  # tests/test_gpu_goal.py: the synthetic E1M1 joins most of its sectors by steps of 0.32


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    index, cell, n = 0, 0.25, 4
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(index)
    host = wad.build_world(index, device=False)
    tables, g = sector_ref.Tables(host), world.area_grid(cell)
    at = [goal_ref.level_sectors(tables, g, cell)]
    pos, yaw = wad.build_level(index).start()
    goal = goal_ref.cells(g, cell, rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.full(n, yaw, np.float32)))
    rng = np.random.default_rng(7)
    offs = [sector_ref.random_offsets(rng, n, host.game_objects) for _ in range(2)]
    offs[0][0] = 0  # row 0 of the first replay: all at rest
    # the starts: cells that reach the goal at rest
    _, floor, ceiling = goal_ref.planes(tables, g, cell, 1, at_centres=at)
    rows, cols = np.nonzero(octile_ref.flood(floor[0], ceiling[0], goal[0], True, max_step=STEP) != octile_ref.UNREACHED)
    pick = rng.integers(0, len(rows), n)
    starts = np.stack([cols[pick], rows[pick]], 1).astype(np.int32)
    want = []
    for off in offs:
        _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=off, at_centres=at)
        dist, count = octile_ref.flood_grids(floor, ceiling, goal, True, max_step=STEP)
        walk = octile_ref.descend_grids(floor, ceiling, dist, starts, path_len=PATH_LEN, towards=True, max_step=STEP, max_moves=12)
        want.append((floor, ceiling, dist, count) + walk)
    assert (want[0][2] != want[1][2]).any() and (want[0][3] > 500).all()  # the offsets count, and the fields are worth having
    assert (want[0][5] > PATH_LEN).any()  # walks longer than the path

    h, w = world.area_plane_shape(cell)
    off_t = torch.from_numpy(offs[0]).cuda()
    goal_t, starts_t = torch.from_numpy(goal).cuda(), torch.from_numpy(starts).cuda()
    floor, ceiling = torch.full((n, h, w), 7.0, device='cuda'), torch.full((n, h, w), 7.0, device='cuda')
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device='cuda')
    dist, count, cells, moves, path = i32(n, h, w), i32(n), i32(n, 2), i32(n), i32(n, PATH_LEN, 2)
    outs = (floor, ceiling, dist, count, cells, moves, path)

    def same(want, what):
        for k, (got, ref) in enumerate(zip(outs, want)):
            got = got.cpu().numpy()
            assert np.array_equal(got.view(ref.dtype), ref), (what, k)

    def reset():
        for t in outs:
            t.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False):
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        world.draw_area_planes(cell, offsets=off_t, floor=floor, ceiling=ceiling, stream=stream)
        got = rd.flood_grids_octile(floor, ceiling, goal_t, towards=True, max_step=STEP, dist_out=ptr(dist), count_out=ptr(count), stream=stream)
        assert raw or (got[0] is dist and got[1] is count)
        got = rd.descend_grids_octile(floor, ceiling, dist, starts_t, towards=True, max_step=STEP, max_moves=12, cells_out=ptr(cells),
                                      moves_out=ptr(moves), path_out=path, stream=stream)
        assert got[2] is path and (raw or (got[0] is cells and got[1] is moves))

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    tick(side)
    side.synchronize()
    same(want[0], 'a side stream, the caller\'s tensors')
    reset()
    tick(side.cuda_stream, raw=True)
    side.synchronize()
    same(want[0], 'raw pointers, the stream as a raw handle')
    # new tensors: the distances alone; a path allocated by its length
    alone = rd.flood_grids_octile(floor, ceiling, goal_t, towards=True, max_step=STEP)
    assert alone.dtype == torch.int32 and np.array_equal(alone.cpu().numpy().view(np.uint32), want[0][2])
    got = rd.descend_grids_octile(floor, ceiling, alone, starts_t, towards=True, max_step=STEP, max_moves=12, path_out=PATH_LEN)
    assert len(got) == 3 and all(np.array_equal(t.cpu().numpy().view(ref.dtype), ref) for t, ref in zip(got, want[0][4:]))
    # tensors that do not fit are refused before anything is queued, and costs outside their limits by the library
    flood = dict(floor=floor, ceiling=ceiling, seeds=goal_t)
    walk = dict(floor=floor, ceiling=ceiling, dist=dist, starts=starts_t)
    for call, args, kw in ((rd.flood_grids_octile, flood, dict(floor=floor.double())), (rd.flood_grids_octile, flood, dict(ceiling=ceiling[:, :-1])),
                           (rd.flood_grids_octile, flood, dict(seeds=goal_t.long())), (rd.flood_grids_octile, flood, dict(seeds=goal_t[:-1])),
                           (rd.flood_grids_octile, flood, dict(dist_out=i32(n, h, w - 1))), (rd.flood_grids_octile, flood, dict(dist_out=floor)),
                           (rd.flood_grids_octile, flood, dict(count_out=i32(n + 1))),
                           (rd.descend_grids_octile, walk, dict(dist=dist.float())), (rd.descend_grids_octile, walk, dict(dist=dist[:, :-1])),
                           (rd.descend_grids_octile, walk, dict(starts=starts_t.long())), (rd.descend_grids_octile, walk, dict(starts=None)),
                           (rd.descend_grids_octile, walk, dict(cells_out=i32(n, 3))), (rd.descend_grids_octile, walk, dict(moves_out=i32(n + 1))),
                           (rd.descend_grids_octile, walk, dict(path_out=i32(n, PATH_LEN, 3)))):
        try:
            call(**dict(args, **kw))
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    for call, args in ((rd.flood_grids_octile, flood), (rd.descend_grids_octile, walk)):
        for costs in ((0, 0), (5, 4), (5, 11), (1 << 24, 1 << 24)):
            try:
                call(axial_cost=costs[0], diagonal_cost=costs[1], **args)
            except rd.RdoomError as e:
                assert e.status == -1 and 'axial_cost' in str(e)
            else:
                raise AssertionError('accepted costs %s' % (costs,))
    # a captured graph (a call that waited or allocated could not be captured), replayed with the offsets changed in between
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    reset()
    graph.replay()
    torch.cuda.synchronize()
    same(want[0], 'first replay')
    off_t.copy_(torch.from_numpy(offs[1]))
    graph.replay()
    torch.cuda.synchronize()
    same(want[1], 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
