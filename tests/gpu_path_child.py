"""Child process of tests/test_gpu_path.py (prints one RESULT line): area_frontiers and descend_grids on a side stream given as a torch
stream and as a raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a captured graph of
planes, flood, frontier and walk replayed twice with the explored area grown between the replays.  torch is initialised BEFORE the
library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import goal_ref
import path_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad

PATH_LEN = 6


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    index, cell, n = 0, 0.25, 6
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(index)
    tables, g = sector_ref.Tables(wad.build_world(index, device=False)), world.area_grid(cell)
    at = [goal_ref.level_sectors(tables, g, cell)]
    st, _ = sector_ref.players(wad, index, n, np.random.default_rng(34), outside=0, nan=0)
    seeds = goal_ref.cells(g, cell, st)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    states = to_dev(st)
    fan = torch.from_numpy(rd.map_fan(64, 1.6)).cuda()
    # the explored area after four looks around, as tests/test_gpu_path.py takes them
    area, turned = None, st.copy()
    for _ in range(4):
        area = world.reveal_area(to_dev(turned), fan, 12.0, cell, area=area)
        turned['yaw'] += np.float32(1.6)
    torch.cuda.synchronize()
    areas = [area.cpu().numpy().view(np.uint32)]
    want = []
    for k in range(2):
        rows = areas[k]
        _, floor, ceiling = goal_ref.planes(tables, g, cell, n, area=rows, at_centres=at)
        dist, _ = goal_ref.flood_grids(floor, ceiling, seeds)
        front = path_ref.area_frontiers(rows, g, dist)
        want.append(front + path_ref.descend_grids(floor, ceiling, dist, front[0], path_len=PATH_LEN, stop_dist=1))
        if k == 0:  # the second area: the five by five cells around every row's nearest frontier cell seen free as well
            more = rows.copy()
            for p, (cx, cz) in enumerate(front[0].tolist()):
                for iz in range(max(cz - 2, 0), min(cz + 3, g.gh)):
                    for ix in range(max(cx - 2, 0), min(cx + 3, g.gw)):
                        more[p, 0, iz * g.pitch + ix // 32] |= np.uint32(1 << (ix % 32))
            areas.append(more)
    assert (want[0][2] > 10).sum() >= 4 and (want[0][3] != want[1][3]).any() and (want[0][0] != want[1][0]).any()
    assert (want[0][5] > PATH_LEN).any() and (want[0][5] < PATH_LEN).any()  # walks longer and shorter than the path

    h, w = world.area_plane_shape(cell)
    area = torch.from_numpy(areas[0].view(np.int32)).cuda()
    floor, ceiling = torch.full((n, h, w), 7.0, device='cuda'), torch.full((n, h, w), 7.0, device='cuda')
    cells = world.area_cells(states, cell)
    dist = torch.full((n, h, w), 7, dtype=torch.int32, device='cuda')
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device='cuda')
    front, front_dist, count, step, moves, path = i32(n, 2), i32(n), i32(n), i32(n, 2), i32(n), i32(n, PATH_LEN, 2)
    mask = torch.full((n, h, w), 7, dtype=torch.uint8, device='cuda')
    outs = (front, front_dist, count, mask, step, moves, path)

    def same(want, what):
        for k, (got, ref) in enumerate(zip(outs, want)):
            got = got.cpu().numpy()
            assert np.array_equal(got.view(ref.dtype) if got.dtype.itemsize == ref.dtype.itemsize else got, ref), (what, k)

    def reset():
        for t in outs + (floor, ceiling, dist):
            t.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False):
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        world.draw_area_planes(cell, area=area, floor=floor, ceiling=ceiling, stream=stream)
        rd.flood_grids(floor, ceiling, cells, dist_out=dist, stream=stream)
        got = world.area_frontiers(area, dist, cell, cell_out=front, dist_out=ptr(front_dist), count_out=ptr(count), mask_out=mask, stream=stream)
        assert got[0] is front and got[3] is mask and (raw or (got[1] is front_dist and got[2] is count))
        got = rd.descend_grids(floor, ceiling, dist, front, stop_dist=1, cells_out=ptr(step), moves_out=ptr(moves), path_out=path, stream=stream)
        assert got[2] is path and (raw or (got[0] is step and got[1] is moves))

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    tick(side)
    side.synchronize()
    same(want[0], 'a side stream, the caller\'s tensors')
    reset()
    tick(side.cuda_stream, raw=True)
    side.synchronize()
    same(want[0], 'raw pointers, the stream as a raw handle')
    # new tensors: the cells alone; a path allocated by its length
    alone = world.area_frontiers(area, dist, cell)
    assert alone.dtype == torch.int32 and np.array_equal(alone.cpu().numpy(), want[0][0])
    got = rd.descend_grids(floor, ceiling, dist, alone, stop_dist=1, path_out=PATH_LEN)
    assert len(got) == 3 and all(np.array_equal(t.cpu().numpy().view(ref.dtype), ref) for t, ref in zip(got, want[0][4:]))
    # tensors that do not fit are refused before anything is queued
    walk = dict(floor=floor, ceiling=ceiling, dist=dist, starts=front)
    frontier = dict(area=area, dist=dist, cell=cell)
    for call, args, kw in ((rd.descend_grids, walk, dict(dist=dist.float())), (rd.descend_grids, walk, dict(dist=dist[:, :-1])),
                           (rd.descend_grids, walk, dict(dist=dist.cpu())), (rd.descend_grids, walk, dict(starts=front.long())),
                           (rd.descend_grids, walk, dict(starts=front[:-1])), (rd.descend_grids, walk, dict(starts=None)),
                           (rd.descend_grids, walk, dict(cells_out=i32(n, 3))), (rd.descend_grids, walk, dict(cells_out=torch.zeros((n, 2), device='cuda'))),
                           (rd.descend_grids, walk, dict(moves_out=i32(n + 1))), (rd.descend_grids, walk, dict(path_out=i32(n, PATH_LEN, 3))),
                           (rd.descend_grids, walk, dict(path_out=i32(n - 1, PATH_LEN, 2))), (rd.descend_grids, walk, dict(path_out=torch.zeros((n, 4, 2), device='cuda'))),
                           (world.area_frontiers, frontier, dict(dist=dist.float())), (world.area_frontiers, frontier, dict(dist=dist[0])),
                           (world.area_frontiers, frontier, dict(area=area[:-1])), (world.area_frontiers, frontier, dict(area=area[:, :, :g.words - 1].contiguous())),
                           (world.area_frontiers, frontier, dict(cell_out=i32(n, 3))), (world.area_frontiers, frontier, dict(dist_out=i32(n + 1))),
                           (world.area_frontiers, frontier, dict(count_out=torch.zeros(n, device='cuda'))),
                           (world.area_frontiers, frontier, dict(mask_out=i32(n, h, w))), (world.area_frontiers, frontier, dict(mask_out=mask[:, :-1]))):
        try:
            call(**dict(args, **kw))
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    # distances smaller than the grid are the library's to refuse
    try:
        world.area_frontiers(area, dist[:, :h - 1].contiguous(), cell)
    except rd.RdoomError as e:
        assert e.status == -1 and 'distances of' in str(e)
    else:
        raise AssertionError('accepted distances smaller than the grid')
    # a captured graph (a call that waited or allocated could not be captured), replayed with the area changed in between
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    reset()
    graph.replay()
    torch.cuda.synchronize()
    same(want[0], 'first replay')
    area.copy_(torch.from_numpy(areas[1].view(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    same(want[1], 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
