"""Child process of tests/test_gpu_flood.py (prints one RESULT line): flood_maps on a side stream given as a torch stream and as a
raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a captured graph replayed twice with
the planes changed between the replays.  torch is initialised BEFORE the library is loaded, as bench.py does: torch and the library
then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import flood_ref
import rust_doom_amd as rd


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    rng = np.random.default_rng(5)
    n, h, w = 6, 21, 37
    # rooms with random pillars and a few raised cells: some of every outcome
    floor = np.where(rng.random((n, h, w)) < 0.15, 0.3, 0.0).astype(np.float32)
    ceiling = np.where(rng.random((n, h, w)) < 0.12, 0.2, 1.5).astype(np.float32)
    seeds = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], 1).astype(np.int32)
    for p in range(n):  # the seed's own cell is open
        floor[p, seeds[p, 1], seeds[p, 0]], ceiling[p, seeds[p, 1], seeds[p, 0]] = 0.0, 1.5
    want, count = flood_ref.flood_maps(floor, ceiling, seeds)
    assert (want == flood_ref.UNREACHED).any() and (count > 20).all() and len(set(count.tolist())) > 1
    f, g, s = torch.from_numpy(floor).cuda(), torch.from_numpy(ceiling).cuda(), torch.from_numpy(seeds).cuda()

    def same(dist, cnt, want, count, what):
        assert np.array_equal(dist.cpu().numpy().view(np.uint16), want), what
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), count), what

    side = torch.cuda.Stream()
    dist = torch.full((n, h, w), 7, dtype=torch.uint16, device='cuda')
    cnt = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    res = rd.flood_maps(f, g, s, dist_out=dist, count_out=cnt, stream=side)
    assert res[0] is dist and res[1] is cnt
    side.synchronize()
    same(dist, cnt, want, count, 'a side stream, the caller\'s tensors')
    # int16 storage, raw pointers, the stream as a raw handle
    dist16 = torch.full((n, h, w), 7, dtype=torch.int16, device='cuda')
    cnt.fill_(7)
    torch.cuda.synchronize()
    rd.flood_maps(f, g, s, dist_out=dist16.data_ptr(), count_out=cnt.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    same(dist16, cnt, want, count, 'raw pointers')
    # a new tensor, no counts, the default seeds
    alone = rd.flood_maps(f, g)
    assert alone.dtype == torch.uint16 and tuple(alone.shape) == (n, h, w)
    assert np.array_equal(alone.cpu().numpy(), flood_ref.flood_maps(floor, ceiling)[0])
    got = rd.flood_maps(f, g, s, count_out=True)
    same(got[0], got[1], want, count, 'count_out=True')
    # tensors that do not fit are refused before anything is queued
    for kw in (dict(floor=f.cpu()), dict(floor=f.double()), dict(floor=f[:, :, :-1]), dict(ceiling=g[:-1]), dict(seeds=s.long()), dict(seeds=s[:-1]),
               dict(dist_out=torch.zeros((n, h, w), dtype=torch.int32, device='cuda')), dict(dist_out=torch.zeros((n, h, w), dtype=torch.float16, device='cuda')),
               dict(dist_out=torch.zeros((n, h, w - 1), dtype=torch.int16, device='cuda')), dict(count_out=torch.zeros(n + 1, dtype=torch.int32, device='cuda')),
               dict(count_out=torch.zeros(n, dtype=torch.float32, device='cuda'))):
        args = dict(floor=f, ceiling=g, seeds=s)
        args.update(kw)
        try:
            rd.flood_maps(**args)
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    # a captured graph (a call that waited or allocated could not be captured), replayed with the planes changed in between
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rd.flood_maps(f, g, s, dist_out=dist, count_out=cnt, stream=torch.cuda.current_stream())
    dist.fill_(3)
    cnt.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    same(dist, cnt, want, count, 'first replay')
    floor2, ceiling2 = floor.copy(), ceiling.copy()
    floor2[:, ::3, 5:9], ceiling2[:, 4:7, ::4] = 0.6, 0.1
    for p in range(n):
        floor2[p, seeds[p, 1], seeds[p, 0]], ceiling2[p, seeds[p, 1], seeds[p, 0]] = 0.0, 1.5
    want2, count2 = flood_ref.flood_maps(floor2, ceiling2, seeds)
    assert (want2 != want).any() and (count2 != count).any()
    f.copy_(torch.from_numpy(floor2))
    g.copy_(torch.from_numpy(ceiling2))
    graph.replay()
    torch.cuda.synchronize()
    same(dist, cnt, want2, count2, 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
