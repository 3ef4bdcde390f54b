"""Child process of tests/test_gpu_things.py (prints one RESULT line): sense_things on a side stream given as a torch stream and as a
raw handle, into the caller's tensors and into raw device pointers, tensors that do not fit, and a captured graph of a game step, the
sensing and the episode reset of `collected`, replayed twice with the states changed between the replays.  torch is initialised
BEFORE the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import rust_doom_amd as rd
import things_ref
from util import META_PATH, ensure_wad

N = 6
U = np.uint32
KW = dict(max_range=12.0, fov=2.0, touch_radius=0.6, collect=tuple(range(8)))


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines, table = world.map_lines(), world.map_things()
    things = rd.DeviceThings(table)
    words = things.words()
    prm = things_ref.params(**KW)
    rng = np.random.default_rng(2)
    # two sets of players, each next to a thing of the level
    sets = [things_ref.players_near(table, N, rng, spread=0.4) for _ in range(2)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    u32 = lambda t: t.cpu().numpy().view(U)

    def same(outs, want, what):
        for key, t in outs.items():
            got = u32(t)
            assert np.array_equal(got.reshape(-1), np.ascontiguousarray(want[key]).view(U).reshape(-1)), (what, key)

    def fresh():
        return dict(collected=torch.zeros((N, words), dtype=torch.int32, device='cuda'),
                    visible=torch.full((N, words), 7, dtype=torch.int32, device='cuda'),
                    touched=torch.full((N, words), 7, dtype=torch.int32, device='cuda'),
                    nearest=torch.full((N, 8, 4), 7.0, dtype=torch.float32, device='cuda'),
                    new=torch.full((N, 8), 7, dtype=torch.int32, device='cuda'))

    def sense(states, o, stream, raw=False):
        if raw:  # raw device pointers and a raw stream handle
            return world.sense_things(states.data_ptr(), things, collected=o['collected'].data_ptr(), visible_out=o['visible'].data_ptr(),
                                      touched_out=o['touched'].data_ptr(), nearest_out=o['nearest'].data_ptr(), new_out=o['new'].data_ptr(),
                                      stream=stream.cuda_stream, n=N, stride=words, **KW)
        return world.sense_things(states, things, collected=o['collected'], visible_out=o['visible'], touched_out=o['touched'],
                                  nearest_out=o['nearest'], new_out=o['new'], stream=stream, **KW)

    want = [things_ref.sense(lines, table, st, prm) for st in sets]
    assert all(w['visible'].any() and w['new'].any(1).all() for w in want) and (want[0]['visible'] != want[1]['visible']).any()
    side = torch.cuda.Stream()
    for raw in (False, True):
        for k, st in enumerate(sets):
            states, o = dev(st), fresh()
            side.wait_stream(torch.cuda.current_stream())
            sense(states, o, side, raw)
            side.synchronize()
            same(o, want[k], ('side stream', raw, k))
    # tensors that do not fit
    states, o = dev(sets[0]), fresh()
    for key, bad in (('visible_out', torch.zeros((N, words), dtype=torch.float32, device='cuda')),
                     ('collected', torch.zeros((N + 1, words), dtype=torch.int32, device='cuda')),
                     ('new_out', torch.zeros((N, 7), dtype=torch.int32, device='cuda')),
                     ('nearest_out', torch.zeros((N, 8, 4), dtype=torch.float32))):
        try:
            world.sense_things(states, things, **{key: bad}, **KW)
        except ValueError:
            continue
        raise AssertionError('%s was accepted' % key)
    try:
        world.sense_things(states, things, visible_out=torch.zeros((N, words - 1), dtype=torch.int32, device='cuda'), **KW)
        raise AssertionError('a short stride was accepted')
    except rd.RdoomError as e:
        assert e.status == -1 and 'stride' in str(e)

    # a captured graph of a tick -- the game step, the sensing, the episode reset -- replayed with the states changed in between
    game, offsets = world.game_state(N)
    inputs = dev(np.zeros((1, N), rd.PLAYER_INPUT))
    done = torch.zeros(N, dtype=torch.bool, device='cuda')
    done[1] = True
    o = fresh()

    def tick(stream):
        world.step_game(states, inputs, game, offsets, n_ticks=1, stream=stream)
        sense(states, o, stream)
        o['collected'].masked_fill_(done[:, None], 0)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    for k, st in enumerate(sets):
        states.copy_(dev(st))
        o['collected'].zero_()
        graph.replay()
        torch.cuda.synchronize()
        stepped = states.cpu().numpy().view(rd.PLAYER_STATE)
        ref = things_ref.sense(lines, table, stepped, prm, offsets.cpu().numpy())
        assert ref['visible'].any() and ref['collected'][1].any()
        ref['collected'][1] = 0  # the episode of player 1 ended
        same(o, ref, ('replay', k))
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
