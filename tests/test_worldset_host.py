"""World sets on the host (CPU, no GPU): each slot's collision arrays and trigger list are rdoom_world_create's of the same
level, bit for bit; starts are rdoom_built_start's; the destination table; the set's object count; bad arguments."""
import ctypes

import numpy as np
import pytest

import rust_doom_amd as rd
from util import META_PATH, ensure_wad

NONE = rd.WORLDSET_NO_DESTINATION


@pytest.fixture(scope='module')
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


@pytest.mark.parametrize('indices', [list(range(9)), [2, 0, 1]], ids=['all', 'shuffled'])
def test_each_slot_is_the_levels_world(wad, indices):
    ws = wad.build_world_set(indices, device=False)
    assert ws.n_levels == len(indices)
    table = ws.levels()
    for s, index in enumerate(indices):
        world = wad.build_world(index, device=False)
        got, want = ws.arrays(s), world.arrays()
        for k in ('nodes', 'chunks', 'triangles', 'verts', 'dynamics'):
            assert got[k].tobytes() == want[k].tobytes(), (index, k)
        for k in ('n_static_triangles', 'n_objects', 'node_depth'):
            assert got[k] == want[k], (index, k)
        gt, wt = ws.triggers(s), world.triggers()
        assert gt['triggers'].tobytes() == wt['triggers'].tobytes() and gt['effects'].tobytes() == wt['effects'].tobytes()
        assert gt['n_objects'] == wt['n_objects'] == table['n_objects'][s]
        assert table['archive_index'][s] == index and table['n_triggers'][s] == len(wt['triggers'])
        assert table['node_depth'][s] == want['node_depth']
        pos, yaw = wad.build_level(index).start()
        assert table['start_pos'][s].tobytes() == np.asarray(pos, np.float32).tobytes()
        assert table['start_yaw'][s].tobytes() == np.float32(yaw).tobytes()
    # the set's object count covers every level's game and render objects
    assert ws.n_objects == max(table['n_objects'])
    assert ws.n_objects >= max(int(wad.build_level(i).counters()['num_objects']) for i in indices)


@pytest.mark.parametrize('indices,dest', [([0, 1, 2], [1, 2, NONE]), ([2, 0, 1], [NONE, 2, 0]), ([0, 2], [NONE, NONE]),
                                          ([8], [NONE]), ([7, 8, 6], [1, NONE, 0])])
def test_destinations(wad, indices, dest):
    ws = wad.build_world_set(indices, device=False)
    assert ws.levels()['destination'].tolist() == dest


def test_start_states_are_the_reset(wad):
    ws = wad.build_world_set([1, 0], device=False)
    st = ws.start_states([0, 1, 1])
    table = ws.levels()
    assert np.array_equal(st['pos'], table['start_pos'][[0, 1, 1]]) and np.array_equal(st['yaw'], table['start_yaw'][[0, 1, 1]])
    assert (st['pitch'] == np.float32(1e-8)).all() and (st['vel'] == 0).all() and (st['last_height_diff'] == 0).all()
    assert (st['flags'] == rd.PLAYER_CLIP).all()


def test_game_bytes_is_the_largest_levels(wad):
    indices = [1, 0, 2]
    ws = wad.build_world_set(indices, device=False)
    assert ws.game_bytes() == max(wad.build_world(i, device=False).game_bytes() for i in indices)
    assert ws.game_bytes() % 16 == 0


def test_bad_arguments(wad):
    L = rd.lib()
    h = ctypes.c_void_p()
    n_levels = wad.num_levels()

    def create(idx, flags=rd.WORLD_HOST_ONLY, out=True):
        a = np.asarray(idx, np.uint32)
        return L.rdoom_worldset_create(wad._h, a.ctypes.data_as(ctypes.c_void_p) if len(a) else None, len(a), flags,
                                       ctypes.byref(h) if out else None)

    assert create([]) == -1                  # an empty list
    assert create([0, n_levels]) == -1       # out of range
    assert create([0, 2, 0]) == -1           # a duplicate
    assert b'twice' in L.rdoom_last_error()
    assert create([0], flags=0x80) == -1     # unknown flags
    assert create([0], out=False) == -1
    assert L.rdoom_worldset_create(None, None, 0, 0, ctypes.byref(h)) == -1
    idx = np.zeros(1, np.uint32)
    assert L.rdoom_worldset_create(None, idx.ctypes.data_as(ctypes.c_void_p), 1, 0, ctypes.byref(h)) == -1
    assert L.rdoom_worldset_create(wad._h, None, 2, 0, ctypes.byref(h)) == -1
    with pytest.raises(rd.RdoomError) as e:
        wad.build_world_set([3, 3], device=False)
    assert e.value.status == -1
    ws = wad.build_world_set([0, 1], device=False)
    v = ctypes.c_void_p
    assert L.rdoom_worldset_info(None, None, None) == -1
    assert L.rdoom_worldset_level(ws._h, 2, v(1 << 20)) == -1  # no such slot
    assert L.rdoom_worldset_level(ws._h, 0, None) == -1
    assert L.rdoom_worldset_level(None, 0, v(1 << 20)) == -1
    assert L.rdoom_worldset_game_bytes(ws._h, None) == -1
    assert L.rdoom_worldset_game_bytes(None, v(1 << 20)) == -1
    # a fake, aligned device pointer: every check below fails before anything reaches the device
    fake = v(1 << 20)
    n_obj = ws.n_objects
    f = ctypes.c_float(1.0 / 60.0)
    assert L.rdoom_worldset_game_reset(None, fake, fake, n_obj, fake, 4, None, None) == -1
    assert L.rdoom_worldset_game_reset(ws._h, None, fake, n_obj, fake, 4, None, None) == -1
    assert L.rdoom_worldset_game_reset(ws._h, fake, None, n_obj, fake, 4, None, None) == -1
    assert L.rdoom_worldset_game_reset(ws._h, fake, fake, n_obj, None, 4, None, None) == -1          # no levels
    assert L.rdoom_worldset_game_reset(ws._h, v((1 << 20) + 4), fake, n_obj, fake, 4, None, None) == -1  # misaligned
    assert L.rdoom_worldset_game_reset(ws._h, fake, fake, n_obj - 1, fake, 4, None, None) == -1      # n_objects too small
    assert L.rdoom_worldset_game_reset(ws._h, fake, fake, n_obj, fake, 4, None, None) == -1          # host-only set
    args = lambda game, offs, n_objects, levels: (ws._h, fake, fake, None, game, offs, n_objects, levels, 4, 10, None, f, None)
    assert L.rdoom_worldset_step_game(*args(fake, fake, n_obj - 1, fake)) == -1
    assert L.rdoom_worldset_step_game(*args(None, fake, n_obj, fake)) == -1
    assert L.rdoom_worldset_step_game(*args(fake, None, n_obj, fake)) == -1
    assert L.rdoom_worldset_step_game(*args(fake, fake, n_obj, None)) == -1
    assert L.rdoom_worldset_step_game(*args(fake, fake, n_obj, fake)) == -1
    assert L.rdoom_worldset_step_game(None, fake, fake, None, fake, fake, n_obj, fake, 4, 10, None, f, None) == -1
    assert L.rdoom_worldset_step_game(ws._h, None, fake, None, fake, fake, n_obj, fake, 4, 10, None, f, None) == -1
    assert L.rdoom_worldset_step_game(ws._h, fake, fake, None, fake, fake, n_obj, fake, 4, 10, None, ctypes.c_float(-1.0), None) == -1
