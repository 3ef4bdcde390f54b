"""The spawn on the GPU (spawn.hip spawn_players_kernel and its world-set form) against tests/spawn_ref.py: every byte of every state
and every tries value, zero tolerance.  The hand-made levels with 1 to 15 players a launch; E1M1 with 64 players and with 1024; a
three-level set with mixed slots and one out of range; a mask over states filled with a byte pattern; episodes given and not; a door
of E1M4 raised in half of the games; the spawned states through locate_players, a game tick and a render; a side stream, raw
pointers and a captured graph in a child process; every argument error, with nothing queued."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rust_doom_amd as rd
import sector_ref
import spawn_ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _ints(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32).copy()).cuda()


def _run(world, blank, seed, levels=None, mask=None, episode=None, offsets=None, tries=9, **kw):
    """spawn_players of numpy inputs on the device: (states, tries) as numpy; tries_out starts as `tries` everywhere"""
    st = _dev(blank)
    out = torch.full((len(blank),), tries, dtype=torch.int32, device='cuda')
    args = dict(mask=torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda() if mask is not None else None,
                episode=_ints(episode) if episode is not None else None,
                offsets=torch.from_numpy(np.ascontiguousarray(offsets, F)).cuda() if offsets is not None else None, tries_out=out)
    args.update(kw)
    res = world.spawn_players(st, seed, **args) if levels is None else world.spawn_players(st, _ints(levels), seed, **args)
    assert res is st
    return st.cpu().numpy().view(rd.PLAYER_STATE), out.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    st, tries = got
    assert st.shape == want[0].shape and np.array_equal(tries, want[1]), (what, tries, want[1])
    bad = st.view(np.uint8).reshape(len(st), -1) != want[0].view(np.uint8).reshape(len(st), -1)  # bytes: every float bit for bit
    assert not bad.any(), (what, int(bad.any(1).sum()), np.argwhere(bad)[:3], st[bad.any(1)][:2], want[0][bad.any(1)][:2])


@pytest.mark.parametrize('name', spawn_ref.HAND)
def test_the_hand_made_levels_one_to_fifteen_players_a_launch(name):
    rd.set_device(0)
    wad, world = spawn_ref.hand_world(name, device=True)
    level = spawn_ref.Level(world)
    for n, seed, kw in ((1, 3, {}), (2, 4, {}), (7, 5 | 9 << 32, {}), (15, 6, {}), (15, 7, dict(max_step=0.6)), (15, 8, dict(clearance=0.5)),
                        (15, 9, dict(margin=0.1, flags=rd.PLAYER_CLIP | rd.PLAYER_FLY)), (13, 10, dict(margin=0.0, max_step=0.0))):
        blank = spawn_ref.blank_states(n)
        want = spawn_ref.spawn(level, blank, seed, tries=np.full(n, 9, np.uint32), **kw)
        _same(_run(world, blank, seed, **kw), want, (name, n, kw))
        if name in ('thin', 'low') and not kw:
            assert (want[1] == 0).all()
        if name == 'square' and not kw:
            assert (want[1] > 0).all()


def test_e1m1_with_64_players_and_with_1024():
    rd.set_device(0)
    wad, _, level = spawn_ref.real(0)
    world = wad.build_world(0)
    wants = {}
    for n, seed in ((64, 1993), (1024, 1993), (1024, 0xFFFFFFFFFFFFFFFF)):
        blank = spawn_ref.blank_states(n)
        want = wants[n, seed] = spawn_ref.spawn(level, blank, seed)
        assert (want[1] > 1).any() and (want[1] == 1).any()
        _same(_run(world, blank, seed, tries=0), want, (n, seed))
    # a state is the same in any batch
    assert wants[64, 1993][0].tobytes() == wants[1024, 1993][0][:64].tobytes()
    _same(_run(world, spawn_ref.blank_states(3), 1993), (wants[64, 1993][0][:3], wants[64, 1993][1][:3]), 'three players')


def test_a_world_set_with_mixed_slots_and_one_out_of_range():
    rd.set_device(0)
    wad = spawn_ref.real(0)[0]
    ws = wad.build_world_set([0, 3, 1])
    levels = [spawn_ref.Level(ws, slot) for slot in range(3)]
    n = 200
    rng = np.random.default_rng(12)
    slots = rng.integers(0, 3, n).astype(np.uint32)
    slots[17], slots[130] = 3, 0xFFFFFFFF
    blank = spawn_ref.blank_states(n)
    offsets = sector_ref.random_offsets(rng, n, ws.n_objects)
    for kw in (dict(), dict(offsets=offsets), dict(offsets=offsets, episode=rng.integers(0, 2 ** 32, n, dtype=np.uint64))):
        want = spawn_ref.spawn(levels, blank, 31, level_of=slots, tries=np.full(n, 9, np.uint32), **kw)
        assert want[0][17].tobytes() == blank[17].tobytes() and want[1][17] == 0 and want[1][130] == 0
        _same(_run(ws, blank, 31, levels=slots, **kw), want, sorted(kw))
    # a wave whose players are all on one level, and the start of each level for players without a candidate
    one = np.full(64, 1, np.uint32)
    _same(_run(ws, blank[:64], 5, levels=one), spawn_ref.spawn(levels, blank[:64], 5, level_of=one), 'one level')
    want = spawn_ref.spawn(levels, blank, 31, level_of=slots, margin=50.0, tries=np.full(n, 9, np.uint32))
    inside = slots < 3
    assert (want[1] == 0).all() and want[0][inside].tobytes() == ws.start_states(slots[inside]).tobytes()
    _same(_run(ws, blank, 31, levels=slots, margin=50.0), want, 'no candidate')


def test_a_mask_leaves_the_other_players_untouched_and_episodes_move_the_points():
    rd.set_device(0)
    wad, _, level = spawn_ref.real(0)
    world = wad.build_world(0)
    n = 130
    blank = spawn_ref.blank_states(n, 0x5A)
    mask = (np.arange(n) % 2 == 0).astype(np.uint8)
    mask[64:128:2] = 7  # any non-zero byte
    mask[3] = 1
    want = spawn_ref.spawn(level, blank, 77, mask=mask, tries=np.full(n, 9, np.uint32))
    got = _run(world, blank, 77, mask=mask)
    _same(got, want, 'mask')
    off = mask == 0
    assert off.sum() > 30 and got[0][off].tobytes() == blank[off].tobytes() and (got[1][off] == 9).all() and (got[1][~off] != 9).all()
    _same(_run(world, blank, 77, mask=mask != 0), want, 'a mask of bools')
    # episodes: NULL is zero, a player with another episode gets another point, and the launch does not write the episodes
    full = spawn_ref.spawn(level, blank, 77)
    _same(_run(world, blank, 77, episode=np.zeros(n, np.uint32)), full, 'episode zero')
    episode = (np.arange(n) % 3).astype(np.uint32)
    episode[5] = 0xFFFFFFFF
    want = spawn_ref.spawn(level, blank, 77, episode=episode)
    assert (want[0]['pos'][episode != 0] != full[0]['pos'][episode != 0]).any(1).all()
    ep = _ints(episode)
    st = _dev(blank)
    world.spawn_players(st, 77, episode=ep)
    assert st.cpu().numpy().view(rd.PLAYER_STATE).tobytes() == want[0].tobytes()
    assert np.array_equal(ep.cpu().numpy().view(np.uint32), episode)
    ep.add_(torch.from_numpy((mask != 0).astype(np.int32)).cuda())  # the next reset of the masked players
    episode2 = episode + (mask != 0)
    _same(_run(world, blank, 77, mask=mask, episode=ep.cpu().numpy().view(np.uint32)),
          spawn_ref.spawn(level, blank, 77, mask=mask, episode=episode2, tries=np.full(n, 9, np.uint32)), 'bumped')


def test_a_door_raised_in_half_of_the_games_takes_players_in_those_games_only():
    rd.set_device(0)
    door, offsets, want, sector = spawn_ref.door_case()
    inside = (want[1] > 0) & (sector == door)
    assert inside[1::2].any() and not inside[0::2].any()  # on the reference first
    wad = spawn_ref.real(3)[0]
    world = wad.build_world(3)
    got = _run(world, spawn_ref.blank_states(len(offsets)), 77, offsets=offsets)
    _same(got, want, 'the door')
    located = world.locate_players(_dev(got[0]), offsets=torch.from_numpy(offsets).cuda()).cpu().numpy().view(np.uint32)
    assert np.array_equal(located, sector)


def test_spawned_players_are_located_stepped_and_rendered():
    rd.set_device(0)
    wad, _, level = spawn_ref.real(0)
    world = wad.build_world(0)
    n, w, h = 64, 64, 40
    game, offsets = world.game_state(n)
    states = _dev(spawn_ref.blank_states(n))
    tries = torch.zeros(n, dtype=torch.int32, device='cuda')
    world.spawn_players(states, 2024, offsets=offsets, tries_out=tries)
    heights = torch.empty((n, 2), dtype=torch.float32, device='cuda')
    sector = world.locate_players(states, offsets=offsets, heights_out=heights).cpu().numpy().view(np.uint32)
    accepted = tries.cpu().numpy() > 0
    assert accepted.sum() > 56 and (sector[accepted] != sector_ref.NONE).all()
    st = states.cpu().numpy().view(rd.PLAYER_STATE)
    hs = heights.cpu().numpy()
    assert (st['pos'][accepted, 1] == hs[accepted, 0] + F(0.5)).all() and (hs[accepted, 1] - hs[accepted, 0] >= F(0.56)).all()
    inputs = _dev(np.zeros((1, n), rd.PLAYER_INPUT))
    world.step_game(states, inputs, game, offsets, n_ticks=1)
    built = wad.build_level(0)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    batch.render_players(states, built.lights_at(0.0), offsets=offsets)
    batch.finish()
    fb = batch.read_framebuffer()
    assert fb.shape[0] == n and (fb != 0).mean() > 0.3
    after = states.cpu().numpy().view(rd.PLAYER_STATE)
    assert np.isfinite(after['pos']).all() and not (after['flags'] & rd.PLAYER_DIVERGED).any()
    assert (np.abs(after['pos'][:, [0, 2]] - st['pos'][:, [0, 2]]) < 0.05).all()  # a tick of standing still


def test_a_side_stream_raw_pointers_and_a_graph_in_one_child():
    """tests/gpu_spawn_child.py in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_spawn_child.py')], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0 and out[-1] == 'RESULT ok=1', p.stdout[-3000:] + p.stderr[-3000:]


def test_argument_errors_by_status_and_text():
    rd.set_device(0)
    L = rd.lib()
    wad, _, level = spawn_ref.real(0)
    world = wad.build_world(0)
    ws = wad.build_world_set([0, 3])
    host_only = wad.build_world(0, device=False)
    n = 5
    blank = spawn_ref.blank_states(n)
    states = _dev(blank)
    tries = torch.full((n,), 9, dtype=torch.int32, device='cuda')
    slots = _ints(np.zeros(n, np.uint32))
    small = torch.zeros((n, 1, 3), dtype=torch.float32, device='cuda')
    v = ctypes.c_void_p
    nan = float('nan')

    def call(h=world._h, st=states.data_ptr(), n=n, off=None, n_obj=0, params=(0.19, 0.56, 0.24, rd.PLAYER_CLIP)):
        p = ctypes.byref(rd.SpawnParams(*params)) if params is not None else None
        return L.rdoom_world_spawn_players(h, v(st), n, v(off), n_obj, None, ctypes.c_uint64(9), None, p, v(tries.data_ptr()), None)

    def call_set(h=ws._h, st=states.data_ptr(), lv=slots.data_ptr(), n=n, off=None, n_obj=0, params=(0.19, 0.56, 0.24, rd.PLAYER_CLIP)):
        p = ctypes.byref(rd.SpawnParams(*params)) if params is not None else None
        return L.rdoom_worldset_spawn_players(h, v(st), v(lv), n, v(off), n_obj, None, ctypes.c_uint64(9), None, p, v(tries.data_ptr()), None)

    for fn, noun in ((call, 'world'), (call_set, 'world set')):
        def fails(word, **kw):
            assert fn(**kw) == -1, kw
            assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

        fails('null ' + noun, h=None)
        fails('null params', params=None)
        fails('null states', st=None)
        for k, name in enumerate(('margin', 'clearance', 'max_step')):
            for bad in (nan, -0.5):
                params = [0.19, 0.56, 0.24, 0]
                params[k] = bad
                fails(name, params=tuple(params))
        fails('n_objects 1 is smaller', off=small.data_ptr(), n_obj=1)
    assert call_set(lv=None) == -1 and 'null levels' in L.rdoom_last_error().decode()
    assert call(h=host_only._h) == -1 and 'RDOOM_WORLD_HOST_ONLY' in L.rdoom_last_error().decode()
    with pytest.raises(rd.RdoomError) as e:
        world.spawn_players(states, 1, max_step=nan)
    assert e.value.status == -1 and 'max_step' in str(e.value)
    with pytest.raises(rd.RdoomError):
        world.spawn_players(states, 1, offsets=small)
    for kw in (dict(mask=torch.zeros(n, dtype=torch.int32, device='cuda')), dict(mask=torch.zeros(n + 1, dtype=torch.uint8, device='cuda')),
               dict(episode=torch.zeros(n, dtype=torch.float32, device='cuda')), dict(episode=torch.zeros(n, dtype=torch.int64, device='cuda')),
               dict(tries_out=torch.zeros(n - 1, dtype=torch.int32, device='cuda')), dict(mask=torch.zeros(n, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            world.spawn_players(states, 1, **kw)
    with pytest.raises(ValueError):
        world.spawn_players(states, -1)
    with pytest.raises(ValueError):
        world.spawn_players(states.cpu(), 1)
    # nothing was queued by any of them, and n == 0 queues nothing either
    assert call(n=0) == 0 and call(n=0, st=None) == 0 and call_set(n=0, st=None, lv=None) == 0
    torch.cuda.synchronize()
    assert states.cpu().numpy().tobytes() == blank.tobytes() and (tries == 9).all()
    assert call() == 0  # the same arguments, valid
    torch.cuda.synchronize()
    want = spawn_ref.spawn(level, blank, 9)
    assert states.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(tries.cpu().numpy().view(np.uint32), want[1])
