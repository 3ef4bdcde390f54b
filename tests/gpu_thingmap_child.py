"""Child process of tests/test_gpu_thingmap.py (prints one RESULT line): draw_thing_maps on a side stream given as a torch stream and
as a raw handle, into the caller's tensors and into raw device pointers; two players who walk over one candle a tick apart, with
step, sense, the OR into `known` and the draw queued tick after tick on one stream and no host wait; and a captured graph of such a
tick, replayed twice with the states changed between the replays.  Every map is held against tests/thingmap_ref.py.  torch is
initialised BEFORE the library is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import rust_doom_amd as rd
import things_ref
import thingmap_ref
from util import META_PATH, ensure_wad

N = 6
U = np.uint32
F = np.float32
VIEW = thingmap_ref.view_of(77, 53, 0.05, rotate=True, top_down=True)
W, H, SCALE = VIEW['width'], VIEW['height'], VIEW['scale']
FLAGS = dict(rotate=True, top_down=True)
SENSE = dict(max_range=10.0, fov=1.6, touch_below=1.0, touch_above=1.0, collect=(rd.THING_AMMO,))


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    table = world.map_things()
    things = rd.DeviceThings(table)
    words = things.words()
    rng = np.random.default_rng(2)
    sets = [things_ref.players_near(table, N, rng, spread=0.4) for _ in range(2)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    u32 = lambda t: t.cpu().numpy().view(U)
    hidden = rng.integers(0, 1 << 32, (N, words), dtype=np.uint64).astype(U) & rng.integers(0, 1 << 32, (N, words), dtype=np.uint64).astype(U)
    rows = torch.from_numpy(hidden.view(np.int32)).cuda()

    def same(out, index, want, what):
        assert np.array_equal(out.cpu().numpy(), want[0]), (what, 'out')
        assert np.array_equal(index.cpu().numpy(), want[1]), (what, 'index')

    # ---- a side stream, the caller's tensors, raw pointers and a raw stream handle
    want = [thingmap_ref.draw(table, st, VIEW, hidden=hidden) for st in sets]
    assert all(w[0].any() and (w[1].reshape(N, -1).max(1) >= 0).sum() >= N // 2 for w in want) and (want[0][0] != want[1][0]).any()
    side = torch.cuda.Stream()
    for raw in (False, True):
        for k, st in enumerate(sets):
            states = dev(st)
            out = torch.full((N, H, W), 0xEE, dtype=torch.uint8, device='cuda')
            index = torch.full((N, H, W), 7, dtype=torch.int32, device='cuda')
            side.wait_stream(torch.cuda.current_stream())
            if raw:
                got = world.draw_thing_maps(states.data_ptr(), things, W, H, SCALE, hidden=rows.data_ptr(), out=out.data_ptr(),
                                            index_out=index.data_ptr(), stream=side.cuda_stream, n=N, stride=words, **FLAGS)
                assert got == (out.data_ptr(), index.data_ptr())
            else:
                got = world.draw_thing_maps(states, things, W, H, SCALE, hidden=rows, out=out, index_out=index, stream=side, **FLAGS)
                assert got[0] is out and got[1] is index
            side.synchronize()
            same(out, index, want[k], ('side stream', raw, k))

    # ---- two players walk over one candle a tick apart: each map loses it in its player's own tick
    candle = 17
    assert table['thing_type'][candle] == 34 and (table['category'][candle] & 0xFF) == rd.THING_AMMO
    t = table[candle]
    st = rd.player_states(np.repeat(F([[t['x'], t['base'] + 0.33, t['z'] + 0.8]]), 2, 0), F([0.0, 0.0]))
    settle, ticks = 30, 30
    inp = np.zeros((settle + ticks + 1, 2), rd.PLAYER_INPUT)
    inp['movement'][settle:, 0, 1] = -1.0      # forwards: towards -z, the candle
    inp['movement'][settle + 1:, 1, 1] = -1.0  # the same walk, one tick later
    game, offs = world.game_state(2)
    states, ti = dev(st), dev(inp)
    collected = torch.zeros((2, words), dtype=torch.int32, device='cuda')
    visible = torch.zeros_like(collected)
    known = torch.zeros_like(collected)
    keep = dict(rows=torch.zeros((ticks, 2, words), dtype=torch.int32, device='cuda'), known=torch.zeros((ticks, 2, words), dtype=torch.int32, device='cuda'),
                states=torch.zeros((ticks, states.numel()), dtype=torch.uint8, device='cuda'),
                out=torch.zeros((ticks, 2, H, W), dtype=torch.uint8, device='cuda'), index=torch.zeros((ticks, 2, H, W), dtype=torch.int32, device='cuda'))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        world.step_game(states, ti[:settle * 40], game, offs, n_ticks=settle, stream=stream)  # both come to rest on the floor
        for k in range(ticks):
            at = (settle + k) * 40
            world.step_game(states, ti[at:at + 40], game, offs, n_ticks=1, stream=stream)
            world.sense_things(states, things, offsets=offs, collected=collected, visible_out=visible, stream=stream, **SENSE)
            known |= visible  # what the player has seen so far
            world.draw_thing_maps(states, things, W, H, SCALE, hidden=collected, known=known, out=keep['out'][k], index_out=keep['index'][k],
                                  stream=stream, **FLAGS)
            keep['rows'][k].copy_(collected), keep['known'][k].copy_(known), keep['states'][k].copy_(states)
    stream.synchronize()
    got_rows, got_known = u32(keep['rows']), u32(keep['known'])
    got_it = (got_rows[:, :, candle >> 5] >> (candle & 31)) & 1  # (ticks, 2)
    assert got_it[0].tolist() == [0, 0] and got_it[-1].tolist() == [1, 1], got_it.T.tolist()
    first = [int(np.argmax(got_it[:, p])) for p in range(2)]
    assert first[1] == first[0] + 1 and (np.diff(got_it, axis=0) >= 0).all(), first
    index = keep['index'].cpu().numpy()
    shows = np.array([[bool((index[k, p] == candle).any()) for p in range(2)] for k in range(ticks)])
    assert shows[first[0] - 1].tolist() == [True, True] and shows[first[0]].tolist() == [False, True] and shows[first[1]].tolist() == [False, False]
    assert np.array_equal(shows, got_it == 0), (shows.T.tolist(), got_it.T.tolist())  # there until its player's own tick, and not after
    assert ((got_known[0] & ~got_known[-1]) == 0).all() and got_known[-1].any(1).all()  # what is known stays known
    for k in sorted({0, first[0] - 1, first[0], first[1], ticks - 1}):  # whole maps around the pick-ups
        stepped = keep['states'][k].cpu().numpy().view(rd.PLAYER_STATE)
        same(keep['out'][k], keep['index'][k], thingmap_ref.draw(table, stepped, VIEW, hidden=got_rows[k], known=got_known[k]), ('walk', k))

    # ---- a captured graph of a tick, replayed with the states changed in between
    game, offsets = world.game_state(N)
    inputs = dev(np.zeros((1, N), rd.PLAYER_INPUT))
    states = dev(sets[0])
    collected = torch.zeros((N, words), dtype=torch.int32, device='cuda')
    visible, known = torch.zeros_like(collected), torch.zeros_like(collected)
    out = torch.zeros((N, H, W), dtype=torch.uint8, device='cuda')
    index = torch.zeros((N, H, W), dtype=torch.int32, device='cuda')
    sense = dict(SENSE, touch_radius=0.6, collect=tuple(range(8)))

    def tick(stream):
        world.step_game(states, inputs, game, offsets, n_ticks=1, stream=stream)
        world.sense_things(states, things, offsets=offsets, collected=collected, visible_out=visible, stream=stream, **sense)
        known.bitwise_or_(visible)
        world.draw_thing_maps(states, things, W, H, SCALE, hidden=collected, known=known, out=out, index_out=index, stream=stream, **FLAGS)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick(torch.cuda.current_stream())
    for k, st in enumerate(sets):
        states.copy_(dev(st))
        collected.zero_(), known.zero_(), out.fill_(0xEE), index.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        stepped = states.cpu().numpy().view(rd.PLAYER_STATE)
        ref = things_ref.sense(world.map_lines(), table, stepped, things_ref.params(**sense), offsets.cpu().numpy())
        assert np.array_equal(u32(collected), ref['collected']) and np.array_equal(u32(known), ref['visible'])
        assert ref['collected'].any() and ref['visible'].any() and (ref['visible'] & ~ref['collected']).any()
        same(out, index, thingmap_ref.draw(table, stepped, VIEW, hidden=ref['collected'], known=ref['visible']), ('replay', k))
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if main() else 1)
