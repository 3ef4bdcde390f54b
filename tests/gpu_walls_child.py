"""Child process of tests/test_gpu_walls.py (prints one RESULT line): draw_area_planes, inflate_grids and flood_grids on a side stream
given as a torch stream and as a raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a
captured graph of planes, inflation and flood replayed twice with the offsets changed between the replays.  torch is initialised
BEFORE the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import goal_ref
import rust_doom_amd as rd
import sector_ref
import walls_ref
from util import META_PATH, ensure_wad

BODY, STEP = 0.19, 0.32


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    index, cell, n = 0, 0.125, 3
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(index)
    tables, g = sector_ref.Tables(wad.build_world(index, device=False)), world.area_grid(cell)
    at = [goal_ref.level_sectors(tables, g, cell)]
    pos, yaw = wad.build_level(index).start()
    st = rd.player_states(np.repeat(np.asarray(pos, np.float32)[None], n, 0), np.full(n, yaw, np.float32))
    seeds = goal_ref.cells(g, cell, st)
    rng = np.random.default_rng(4)
    off = [sector_ref.random_offsets(rng, n, world.game_objects) for _ in range(2)]
    want = []
    for o in off:
        _, floor, ceiling = goal_ref.planes(tables, g, cell, n, offsets=o, at_centres=at)
        fi, ci, d2 = walls_ref.inflate_grids(floor, ceiling, BODY, cell)
        want.append((fi, ci, d2) + goal_ref.flood_grids(fi, ci, seeds, True, max_step=STEP))
    assert (want[0][3] != want[1][3]).any() and (want[0][4] > 1000).all() and (want[0][2] != want[1][2]).any()
    assert (want[0][0].view(np.uint32) != goal_ref.planes(tables, g, cell, n, offsets=off[0], at_centres=at)[1].view(np.uint32)).any()

    offsets = torch.from_numpy(off[0]).cuda()
    cells = torch.from_numpy(seeds).cuda()
    h, w = world.area_plane_shape(cell)
    floor, ceiling = torch.full((n, h, w), 7.0, device='cuda'), torch.full((n, h, w), 7.0, device='cuda')
    fi, ci = torch.full((n, h, w), 7.0, device='cuda'), torch.full((n, h, w), 7.0, device='cuda')
    d2 = torch.empty((n, h, w), dtype=torch.uint16, device='cuda')
    d2.view(torch.int16).fill_(7)
    dist = torch.full((n, h, w), 7, dtype=torch.int32, device='cuda')
    cnt = torch.full((n,), 7, dtype=torch.int32, device='cuda')

    def same(want, what, with_d2=True):
        for got, ref, view in ((fi, want[0], np.uint32), (ci, want[1], np.uint32), (d2, want[2], np.uint16), (dist, want[3], np.uint32),
                               (cnt, want[4], np.uint32)):
            if got is d2 and not with_d2:
                continue
            assert np.array_equal(got.cpu().numpy().view(view), ref.view(view)), what

    def reset():
        for t in (floor, ceiling, fi, ci, dist, cnt):
            t.fill_(7)
        d2.view(torch.int16).fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False, with_d2=True):
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        world.draw_area_planes(cell, offsets=offsets, floor=floor, ceiling=ceiling, stream=stream)
        got = rd.inflate_grids(floor, ceiling, BODY, cell, floor_out=ptr(fi), ceiling_out=ptr(ci), dist2_out=ptr(d2) if with_d2 else None,
                               stream=stream)
        assert len(got) == (3 if with_d2 else 2) and (raw or (got[0] is fi and got[1] is ci and (not with_d2 or got[2] is d2)))
        rd.flood_grids(fi, ci, cells, towards=True, max_step=STEP, dist_out=dist, count_out=cnt, stream=stream)

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
    tick(side, with_d2=False)
    side.synchronize()
    same(want[0], 'the planes alone', with_d2=False)
    assert (d2.cpu().numpy() == 7).all()  # not asked for, not written
    # the distances alone, into the caller's tensor and into a new one
    assert rd.wall_distances(floor, ceiling, 2, dist2_out=d2, stream=side) is d2
    side.synchronize()
    assert np.array_equal(d2.cpu().numpy(), want[0][2])
    alone = rd.wall_distances(floor, ceiling, 2)
    assert alone.dtype == torch.uint16 and tuple(alone.shape) == (n, h, w) and np.array_equal(alone.cpu().numpy(), want[0][2])
    # tensors that do not fit are refused before anything is queued
    for call, kw in ((rd.inflate_grids, dict(floor=floor.cpu())), (rd.inflate_grids, dict(floor=floor.double())),
                     (rd.inflate_grids, dict(ceiling=ceiling[:-1])), (rd.inflate_grids, dict(floor_out=torch.zeros((n, h, w - 1), device='cuda'))),
                     (rd.inflate_grids, dict(ceiling_out=torch.zeros((n, h, w), dtype=torch.float64, device='cuda'))),
                     (rd.inflate_grids, dict(floor_out=torch.zeros((n, h, w), dtype=torch.int32, device='cuda'))),
                     (rd.inflate_grids, dict(dist2_out=torch.zeros((n, h, w), dtype=torch.int32, device='cuda'))),
                     (rd.inflate_grids, dict(dist2_out=torch.zeros((n, h, w), dtype=torch.float16, device='cuda'))),
                     (rd.inflate_grids, dict(radius=5.0)),  # forty cells: above WALL_MAX_RADIUS
                     (rd.wall_distances, dict(dist2_out=torch.zeros((n, h + 1, w), dtype=torch.uint16, device='cuda'))),
                     (rd.wall_distances, dict(ceiling=ceiling.half()))):
        args = dict(floor=floor, ceiling=ceiling, radius=BODY, cell=cell) if call is rd.inflate_grids else dict(floor=floor, ceiling=ceiling,
                                                                                                                 radius_cells=2)
        args.update(kw)
        try:
            call(**args)
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    # a radius the library refuses, and an output on an input
    for call in (lambda: rd.wall_distances(floor, ceiling, 0), lambda: rd.wall_distances(floor, ceiling, 33),
                 lambda: rd.inflate_grids(floor, ceiling, BODY, cell, floor_out=ceiling)):
        try:
            call()
        except rd.RdoomError as e:
            assert e.status == -1
        else:
            raise AssertionError('accepted a bad radius or an output on an input')
    # a captured graph (a call that waited or allocated could not be captured), replayed with the offsets changed in between
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    reset()
    graph.replay()
    torch.cuda.synchronize()
    same(want[0], 'first replay')
    offsets.copy_(torch.from_numpy(off[1]))
    graph.replay()
    torch.cuda.synchronize()
    same(want[1], 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
