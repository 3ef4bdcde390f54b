"""Child process of tests/test_gpu_goal.py (prints one RESULT line): draw_area_planes, area_cells and flood_grids on a side stream
given as a torch stream and as a raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a
captured graph of planes, cells and flood replayed twice with the offsets changed between the replays.  torch is initialised BEFORE
the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import goal_ref
import rust_doom_amd as rd
import sector_ref
from util import META_PATH, ensure_wad


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
    st, _ = sector_ref.players(wad, index, n, np.random.default_rng(2), outside=1, nan=1)
    rng = np.random.default_rng(3)
    off = [sector_ref.random_offsets(rng, n, world.game_objects) for _ in range(2)]
    seeds = goal_ref.cells(g, cell, st)
    want = []
    for o in off:
        planes = goal_ref.planes(tables, g, cell, n, offsets=o, at_centres=at)
        want.append(planes + goal_ref.flood_grids(planes[1], planes[2], seeds, True, max_step=0.32))
    assert (want[0][3] != want[1][3]).any() and (want[0][4][:n - 2] > 100).sum() >= 3 and (want[0][4][n - 2:] == 0).all()
    assert (want[0][3] == goal_ref.UNREACHED).any()

    states = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()
    offsets = torch.from_numpy(off[0]).cuda()
    h, w = world.area_plane_shape(cell)
    sector = torch.full((n, h, w), 7, dtype=torch.int16, device='cuda')
    floor, ceiling = torch.full((n, h, w), 7.0, device='cuda'), torch.full((n, h, w), 7.0, device='cuda')
    cells = torch.full((n, 2), 7, dtype=torch.int32, device='cuda')
    dist = torch.full((n, h, w), 7, dtype=torch.int32, device='cuda')
    cnt = torch.full((n,), 7, dtype=torch.int32, device='cuda')

    def same(want, what):
        for got, ref, view in ((sector, want[0], np.uint16), (floor, want[1], np.uint32), (ceiling, want[2], np.uint32), (dist, want[3], np.uint32),
                               (cnt, want[4], np.uint32)):
            assert np.array_equal(got.cpu().numpy().view(view), ref.view(view)), what
        assert np.array_equal(cells.cpu().numpy(), seeds), what

    def reset():
        for t in (sector, floor, ceiling, cells, dist, cnt):
            t.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False):
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        got = world.draw_area_planes(cell, offsets=offsets, sector_out=sector, floor=floor, ceiling=ceiling, stream=stream)
        assert got[0] is sector and got[1] is floor and got[2] is ceiling
        assert world.area_cells(states, cell, out=cells, stream=stream) is cells
        rd.flood_grids(floor, ceiling, cells, towards=True, max_step=0.32, dist_out=ptr(dist), count_out=ptr(cnt), stream=stream)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    tick(side)
    side.synchronize()
    same(want[0], 'a side stream, the caller\'s tensors')
    reset()
    tick(side.cuda_stream, raw=True)
    side.synchronize()
    same(want[0], 'raw pointers, the stream as a raw handle')
    # new tensors, no counts
    alone = rd.flood_grids(floor, ceiling, cells, towards=True, max_step=0.32)
    assert alone.dtype == torch.int32 and tuple(alone.shape) == (n, h, w) and np.array_equal(alone.cpu().numpy().view(np.uint32), want[0][3])
    # tensors that do not fit are refused before anything is queued
    for call, kw in ((rd.flood_grids, dict(floor=floor.cpu())), (rd.flood_grids, dict(floor=floor.double())), (rd.flood_grids, dict(ceiling=ceiling[:-1])),
                     (rd.flood_grids, dict(seeds=cells.long())), (rd.flood_grids, dict(seeds=cells[:-1])),
                     (rd.flood_grids, dict(dist_out=torch.zeros((n, h, w), dtype=torch.int16, device='cuda'))),
                     (rd.flood_grids, dict(dist_out=torch.zeros((n, h, w), dtype=torch.float32, device='cuda'))),
                     (rd.flood_grids, dict(dist_out=torch.zeros((n, h, w - 1), dtype=torch.int32, device='cuda'))),
                     (rd.flood_grids, dict(count_out=torch.zeros(n + 1, dtype=torch.int32, device='cuda'))),
                     (world.draw_area_planes, dict(floor=torch.zeros((n, h, w), dtype=torch.float64, device='cuda'))),
                     (world.draw_area_planes, dict(sector_out=torch.zeros((n, h, w), dtype=torch.int32, device='cuda'))),
                     (world.draw_area_planes, dict(floor=torch.zeros((n, h, w), device='cuda'), ceiling=torch.zeros((n, h, w + 1), device='cuda'))),
                     (world.draw_area_planes, dict(offsets=offsets[:-1], n=n)),
                     (world.draw_area_planes, dict(area=torch.zeros((n, 2, g.words - 1), dtype=torch.int32, device='cuda'))),
                     (world.area_cells, dict(out=torch.zeros((n, 2), dtype=torch.int64, device='cuda'))),
                     (world.area_cells, dict(out=torch.zeros((n - 1, 2), dtype=torch.int32, device='cuda')))):
        if call is rd.flood_grids:
            args = dict(floor=floor, ceiling=ceiling, seeds=cells)
        elif call == world.area_cells:
            args = dict(states=states, cell=cell)
        else:
            args = dict(cell=cell, n=n)
        args.update(kw)
        try:
            call(**args)
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    # planes smaller than the grid are the library's to refuse
    try:
        world.draw_area_planes(cell, offsets=offsets, floor=torch.zeros((n, h - 1, w), device='cuda'))
    except rd.RdoomError as e:
        assert e.status == -1 and 'planes of' in str(e)
    else:
        raise AssertionError('accepted planes smaller than the grid')
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
