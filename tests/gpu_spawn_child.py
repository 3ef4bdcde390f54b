"""Child process of tests/test_gpu_spawn.py (prints one RESULT line): spawn_players on a side stream given as a torch stream and as a
raw handle, with the mask, the episodes and the tries as raw device pointers, on a world and on a world set, and a captured graph
replayed twice with the episodes bumped between the replays, each checked against tests/spawn_ref.py.  torch is initialised BEFORE
the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import rust_doom_amd as rd
import spawn_ref


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    wad, _, level = spawn_ref.real(0)
    world = wad.build_world(0)
    n, seed = 96, 0x1234567890ABCDEF
    blank = spawn_ref.blank_states(n)
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    episode = (np.arange(n) % 5).astype(np.uint32)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def same(states, tries, want, what):
        assert states.cpu().numpy().tobytes() == want[0].tobytes(), what
        assert np.array_equal(tries.cpu().numpy().view(np.uint32), want[1]), what

    states, d_mask = dev(blank), dev(mask)
    d_episode = torch.from_numpy(episode.view(np.int32).copy()).cuda()
    tries = torch.full((n,), 9, dtype=torch.int32, device='cuda')
    want = spawn_ref.spawn(level, blank, seed, mask=mask, episode=episode, tries=np.full(n, 9, np.uint32))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = world.spawn_players(states, seed, mask=d_mask, episode=d_episode, tries_out=tries, stream=side)
    assert res is states
    side.synchronize()
    same(states, tries, want, 'a side stream, tensors')
    # raw pointers, the stream as a raw handle
    states.copy_(dev(blank))
    tries.fill_(9)
    torch.cuda.synchronize()
    world.spawn_players(states, seed, mask=d_mask.data_ptr(), episode=d_episode.data_ptr(), tries_out=tries.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    same(states, tries, want, 'raw pointers')
    # a world set on the side stream
    ws = wad.build_world_set([3, 0])
    slots = (np.arange(n) % 2).astype(np.uint32)
    d_slots = torch.from_numpy(slots.view(np.int32).copy()).cuda()
    levels = [spawn_ref.Level(ws, 0), spawn_ref.Level(ws, 1)]
    states.copy_(dev(blank))
    tries.fill_(9)
    torch.cuda.synchronize()
    ws.spawn_players(states, d_slots, seed, mask=d_mask.data_ptr(), episode=d_episode, tries_out=tries, stream=side)
    side.synchronize()
    same(states, tries, spawn_ref.spawn(levels, blank, seed, level_of=slots, mask=mask, episode=episode, tries=np.full(n, 9, np.uint32)), 'a set')
    # a captured graph (a call that waited or allocated could not be captured), replayed with the episodes bumped in between
    graph = torch.cuda.CUDAGraph()
    states.copy_(dev(blank))
    tries.fill_(9)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        world.spawn_players(states, seed, mask=d_mask, episode=d_episode, tries_out=tries, stream=torch.cuda.current_stream())
    graph.replay()
    torch.cuda.synchronize()
    same(states, tries, want, 'first replay')
    d_episode.add_(d_mask.to(torch.int32))
    states.copy_(dev(blank))
    tries.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    want2 = spawn_ref.spawn(level, blank, seed, mask=mask, episode=episode + mask, tries=np.full(n, 9, np.uint32))
    assert (want2[0]['pos'][mask != 0] != want[0]['pos'][mask != 0]).any(1).all()
    same(states, tries, want2, 'second replay')
    assert np.array_equal(d_episode.cpu().numpy().view(np.uint32), episode + mask)
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
