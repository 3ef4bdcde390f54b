"""Child process of tests/test_gpu_raythings.py (prints one RESULT line): cast_rays and cast_rays_things on a side stream given as
a torch stream and as a raw handle, into the caller's tensors and through raw device pointers; a step_game -> cast_rays ->
cast_rays_things loop queued tick after tick on one stream with no host wait, every tick's rays kept on the device and held
against the references afterwards; and a captured graph of cast_rays and cast_rays_things -- those two launches and nothing else
-- replayed twice with the hidden rows changed between the replays.  Every fraction and index is held against
tests/raythings_ref.py, the world's fractions against tests/rays_ref.py.  torch is initialised BEFORE the library is loaded, as
bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import rays_ref
import raythings_ref as rt
import rust_doom_amd as rd
import stamp_cases as sc
import world_ref

U = np.uint32
F = np.float32
RANGE, RAYS, HEIGHT = 30.0, 64, 0.42


def main():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    wad = sc.e1m1_wad()
    world = wad.build_world(0)
    ref_world = world_ref.RefWorld(wad, 0)
    table = world.map_things()
    things = rd.DeviceThings(table)
    words = things.words()
    solid_np = rd.pack_things(world.thing_obstacles()).view(U)[None]
    barrels = list(sc.E1M1_BARRELS)
    n = len(barrels)
    pos = np.stack([table['x'][barrels] - F(0.7), table['base'][barrels] + F(0.33), table['z'][barrels]], 1).astype(F)
    st = rd.player_states(pos, np.linspace(0.0, 3.0, n).astype(F))
    dirs = rd.ray_fan(RAYS, 2 * np.pi, pitch=-0.3)
    hides = [sc.bit_rows([[]] * n, words), sc.bit_rows([[b] for b in barrels], words)]  # nothing; every player's own barrel
    hides[1][0] = 0  # but player 0's

    def wanted(states_np, hidden, offsets=None):
        world_frac = rays_ref.cast(ref_world, states_np, dirs, RANGE, offsets=offsets)['frac']
        return rt.cast(table, states_np, dirs, RANGE, heights=HEIGHT, select=solid_np, hidden=hidden,
                       offsets=offsets, frac=world_frac)

    want = [wanted(st, h) for h in hides]
    assert all((want[0][1][p] == b).any() for p, b in enumerate(barrels))
    assert (want[1][1][0] == barrels[0]).any() and not any((want[1][1][p] == b).any() for p, b in enumerate(barrels) if p)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    u32 = lambda t: t.cpu().numpy().view(U)
    states = dev(np.ascontiguousarray(st, rd.PLAYER_STATE).view(np.uint8).reshape(-1))
    fan, solid, hidden = dev(dirs), dev(solid_np.view(np.int32)), dev(hides[0].view(np.int32))
    frac = torch.full((n, RAYS), 7.0, device='cuda')
    thing = torch.full((n, RAYS), 7, dtype=torch.int32, device='cuda')

    def same(ref, what):
        assert np.array_equal(u32(frac), ref[0].view(U)), (what, 'frac')
        assert np.array_equal(u32(thing), ref[1].view(U)), (what, 'thing')

    def reset():
        frac.fill_(7.0), thing.fill_(7)
        torch.cuda.synchronize()

    def tick(stream, raw=False):
        """the two lines of the README's tick: the world cast, then the things, in place"""
        ptr = (lambda t: t.data_ptr()) if raw else (lambda t: t)
        world.cast_rays(states, fan, RANGE, frac_out=frac, stream=stream)
        got = world.cast_rays_things(ptr(states), things, fan, RANGE, heights=HEIGHT, select=ptr(solid), hidden=ptr(hidden), frac=ptr(frac),
                                     frac_out=ptr(frac), thing_out=ptr(thing), stream=stream, n=n if raw else None,
                                     stride=words if raw else None)
        assert raw or (got[0] is frac and got[1] is thing)

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

    # ---- a stepping loop with no host wait: the players walk forward, every tick's rays stay on the device
    ticks = 12
    game, offsets = world.game_state(n)
    script = np.zeros((ticks, n), rd.PLAYER_INPUT)
    script['movement'][:, :, 1] = 1.0
    script['look'][:, :, 0] = 0.02
    inputs = dev(script.view(np.uint8).reshape(ticks, -1))
    walk = states.clone()
    keep = dict(states=torch.zeros((ticks,) + tuple(walk.shape), dtype=torch.uint8, device='cuda'),
                offsets=torch.zeros((ticks,) + tuple(offsets.shape), device='cuda'),
                frac=torch.zeros((ticks, n, RAYS), device='cuda'), thing=torch.zeros((ticks, n, RAYS), dtype=torch.int32, device='cuda'))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k in range(ticks):
            world.step_game(walk, inputs[k], game, offsets, n_ticks=1, stream=stream)
            world.cast_rays(walk, fan, RANGE, offsets=offsets, frac_out=keep['frac'][k], stream=stream)
            world.cast_rays_things(walk, things, fan, RANGE, heights=HEIGHT, select=solid, offsets=offsets, frac=keep['frac'][k],
                                   frac_out=keep['frac'][k], thing_out=keep['thing'][k], stream=stream)
            keep['states'][k].copy_(walk)
            keep['offsets'][k].copy_(offsets)
    stream.synchronize()
    moved = keep['states'].cpu().numpy().view(rd.PLAYER_STATE).reshape(ticks, n)
    assert np.abs(moved[-1]['pos'] - moved[0]['pos']).max() > 0.05  # they walked
    for k in (0, ticks // 2, ticks - 1):
        ref = wanted(moved[k], None, keep['offsets'][k].cpu().numpy())
        assert np.array_equal(u32(keep['frac'][k]), ref[0].view(U)) and np.array_equal(u32(keep['thing'][k]), ref[1].view(U)), ('walk', k)

    # ---- a captured graph of the two launches (a call that waited or allocated could not be captured), replayed with the hidden
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
