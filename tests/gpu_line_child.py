"""Child process of tests/test_gpu_line.py (prints one RESULT line): walk_lines and straighten_paths on a side stream given as a torch
stream and as a raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a captured graph of
flood, descent, straightening and lines replayed twice with the planes changed between the replays.  torch is initialised BEFORE the
library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import line_ref
import octile_ref
import rust_doom_amd as rd

W, H, N, Q = 61, 37, 4, 5
PATH_LEN, CORNERS = 48, 6


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    rng = np.random.default_rng(3)
    # two sets of four sparse rooms; a goal near the middle and a start near a corner of each, on the floor
    sets = [[line_ref.sparse_room(W, H, 10 * k + p, 0.03) for p in range(N)] for k in range(2)]
    goal, starts = np.zeros((N, 2), np.int32), np.zeros((N, 2), np.int32)
    for p in range(N):
        free = (sets[0][p][0] == 0) & (sets[1][p][0] == 0)
        rows, cols = np.nonzero(free)
        k = np.argmin((rows - H // 2) ** 2 + (cols - W // 2) ** 2)
        goal[p] = cols[k], rows[k]
        k = np.argmin((rows - (H - 2) * (p & 1)) ** 2 + (cols - (W - 2) * (p >> 1)) ** 2)
        starts[p] = cols[k], rows[k]
    targets = np.stack([rng.integers(-1, W + 1, (N, Q)), rng.integers(-1, H + 1, (N, Q))], 2).astype(np.int32)
    targets[:, 0] = goal
    want = []
    for rooms in sets:
        floor, ceiling = np.stack([r[0] for r in rooms]), np.stack([r[1] for r in rooms])
        moves = [line_ref.moves_of(floor[p], ceiling[p]) for p in range(N)]
        dist, _ = octile_ref.flood_grids(floor, ceiling, goal, True)
        _, made, path = octile_ref.descend_grids(floor, ceiling, dist, starts, path_len=PATH_LEN, towards=True)
        corners, count, length = line_ref.straighten_paths(None, None, starts, path, True, 64, CORNERS, moves=moves)
        clear, stop, _ = line_ref.walk_lines(None, None, starts, targets, True, moves=moves)
        want.append((floor, ceiling, corners, count, length, clear, stop))
        assert (made > 15).all() and (count >= 1).all() and (count < made).all()
    assert any((a != b).any() for a, b in zip(want[0][2:], want[1][2:]))  # the planes count

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    floor, ceiling = dev(want[0][0]), dev(want[0][1])
    goal_t, starts_t, targets_t = dev(goal), dev(starts), dev(targets)
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device='cuda')
    dist, cells, moves_made, path = i32(N, H, W), i32(N, 2), i32(N), i32(N, PATH_LEN, 2)
    corners, count, length = i32(N, CORNERS, 2), i32(N), torch.full((N,), 7.0, device='cuda')
    clear, stop = torch.full((N, Q), 7, dtype=torch.uint8, device='cuda'), i32(N, Q, 2)
    outs = (corners, count, length, clear, stop)

    def same(want, what):
        for k, (got, ref) in enumerate(zip(outs, want[2:])):
            got = got.cpu().numpy()
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (what, k)

    def reset():
        for t in outs:
            t.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False):
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        rd.flood_grids_octile(floor, ceiling, goal_t, towards=True, dist_out=dist, stream=stream)
        rd.descend_grids_octile(floor, ceiling, dist, starts_t, towards=True, cells_out=cells, moves_out=moves_made, path_out=path, stream=stream)
        got = rd.straighten_paths(floor, ceiling, starts_t, path, towards=True, corners=corners, count_out=ptr(count), length_out=ptr(length),
                                  stream=stream)
        assert got[0] is corners and (raw or (got[1] is count and got[2] is length))
        got = rd.walk_lines(floor, ceiling, starts_t, targets_t, reversed=True, clear_out=ptr(clear), stop_out=ptr(stop), stream=stream)
        assert raw or (got[0] is clear and got[1] is stop)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    tick(side)
    side.synchronize()
    same(want[0], 'a side stream, the caller\'s tensors')
    reset()
    tick(side.cuda_stream, raw=True)
    side.synchronize()
    same(want[0], 'raw pointers, the stream as a raw handle')
    # new tensors: the flags alone; corners allocated by their number, with and without the length
    alone = rd.walk_lines(floor, ceiling, starts_t, targets_t, reversed=True)
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.uint8 and np.array_equal(alone.cpu().numpy(), want[0][5])
    got = rd.walk_lines(floor, ceiling, starts_t, targets_t, reversed=True, stop_out=True)
    assert got[1].dtype == torch.int32 and np.array_equal(got[1].cpu().numpy(), want[0][6])
    got = rd.straighten_paths(floor, ceiling, starts_t, path, towards=True, corners=CORNERS)
    assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), want[0][2]) and np.array_equal(got[1].cpu().numpy().view(np.uint32), want[0][3])
    got = rd.straighten_paths(floor, ceiling, starts_t, path, towards=True, corners=CORNERS, length_out=True)
    assert len(got) == 3 and got[2].dtype == torch.float32 and np.array_equal(got[2].cpu().numpy().view(np.uint32), want[0][4].view(np.uint32))
    # tensors that do not fit are refused before anything is queued, and limits outside their range by the library
    lines = dict(floor=floor, ceiling=ceiling, starts=starts_t, targets=targets_t)
    pull = dict(floor=floor, ceiling=ceiling, starts=starts_t, path=path)
    for call, args, kw in ((rd.walk_lines, lines, dict(floor=floor.double())), (rd.walk_lines, lines, dict(ceiling=ceiling[:, :-1])),
                           (rd.walk_lines, lines, dict(starts=starts_t.long())), (rd.walk_lines, lines, dict(starts=starts_t[:-1])),
                           (rd.walk_lines, lines, dict(targets=targets_t[:-1])), (rd.walk_lines, lines, dict(targets=targets_t[:, 0])),
                           (rd.walk_lines, lines, dict(targets=targets_t.float())), (rd.walk_lines, lines, dict(targets=None)),
                           (rd.walk_lines, lines, dict(clear_out=i32(N, Q))), (rd.walk_lines, lines, dict(clear_out=clear[:, :-1])),
                           (rd.walk_lines, lines, dict(stop_out=i32(N, Q, 3))), (rd.walk_lines, lines, dict(stop_out=length)),
                           (rd.straighten_paths, pull, dict(path=path.long())), (rd.straighten_paths, pull, dict(path=path[:-1])),
                           (rd.straighten_paths, pull, dict(starts=None)), (rd.straighten_paths, pull, dict(corners=i32(N, CORNERS, 3))),
                           (rd.straighten_paths, pull, dict(corners=i32(N + 1, CORNERS, 2))), (rd.straighten_paths, pull, dict(count_out=i32(N + 1))),
                           (rd.straighten_paths, pull, dict(length_out=count)), (rd.straighten_paths, pull, dict(length_out=length[:-1]))):
        try:
            call(**dict(args, **kw))
        except ValueError:
            continue
        raise AssertionError('accepted %s' % sorted(kw))
    for kw, word in ((dict(max_look=0), 'max_look'), (dict(max_look=1025), 'max_look'), (dict(clearance=-1.0), 'clearance')):
        try:
            rd.straighten_paths(**dict(pull, **kw))
        except rd.RdoomError as e:
            assert e.status == -1 and word in str(e)
        else:
            raise AssertionError('accepted %s' % (kw,))
    # a captured graph (a call that waited or allocated could not be captured), replayed with the planes changed in between
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    reset()
    graph.replay()
    torch.cuda.synchronize()
    same(want[0], 'first replay')
    floor.copy_(dev(want[1][0]))
    ceiling.copy_(dev(want[1][1]))
    graph.replay()
    torch.cuda.synchronize()
    same(want[1], 'second replay')
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
