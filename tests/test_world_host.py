"""The collision world's host half (CPU, no GPU): rdoom_world_create's arrays -- game::world::WorldBuilder restated in
csrc/host/game_world.cpp -- equal an independent restatement's (tests/world_restatement.c) fed from the same level walk, on
every level of the synthetic IWADs; map-side invariants; the restatement's sincos; the C ABI's bad-argument paths; and world
creation from four host threads."""
import ctypes
import hashlib
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rust_doom_amd as rd
import world_ref
from util import META_PATH, ensure_big_wad, ensure_wad

_syn = __import__('importlib').import_module('rust-doom_amd.synthetic')


def _levels():
    out = [(ensure_wad(), i) for i in range(9)]
    out += [(_syn.ensure_rich_wad(), 0), (ensure_big_wad(), 0)]
    return out


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('path,index', _levels(), ids=lambda v: str(v).rsplit('/', 1)[-1] if isinstance(v, str) else str(v))
def test_world_arrays_equal_the_restatement(path, index):
    wad = rd.Wad(path, META_PATH)
    got = wad.build_world(index, device=False).arrays()
    want = world_ref.RefWorld(wad, index).arrays()
    for key in ('nodes', 'chunks', 'triangles', 'verts', 'dynamics'):
        assert _same(got[key], want[key]), key
    assert got['n_static_triangles'] == want['n_static_triangles'] and got['n_objects'] == want['n_objects']
    assert len(got['nodes']) > 0 and 1 <= got['node_depth'] <= len(got['nodes'])


@pytest.mark.parametrize('index', [0, 2, 5])
def test_map_side_invariants(index):
    wad = rd.Wad(ensure_wad(), META_PATH)
    ref = world_ref.RefWorld(wad, index)  # (its visitor counts the events WorldBuilder sees)
    a = wad.build_world(index, device=False).arrays()
    feed = ref.feed
    # two triangles per blocker quad and per sky quad, n - 2 per flat polygon of n vertices; nothing else
    expect = 2 * feed.blocker_quads + 2 * feed.sky_quads + sum(max(n - 2, 0) for n in feed.flat_vertex_counts)
    assert len(a['triangles']) == expect and feed.other_quads > 0  # (the level has non-blocking walls: they were left out)
    verts = a['verts'].astype(np.float64)
    normals = verts[a['triangles'][:, 3]]
    assert np.all(np.abs(np.linalg.norm(normals, axis=1) - 1.0) < 1e-6)
    flat = normals[:, 1] != 0
    assert np.all(np.abs(normals[flat, 1]) == 1.0) and np.all(normals[~flat, 1] == 0.0)
    n_static = a['n_static_triangles']
    for start, end in a['chunks']:
        assert start <= end <= n_static
    dyn = a['dynamics']
    if len(dyn):
        assert dyn[0, 1] == n_static and dyn[-1, 2] == len(a['triangles'])
        assert np.all(dyn[1:, 1] == dyn[:-1, 2]) and np.all(np.diff(dyn[:, 0].astype(np.int64)) > 0)
        assert a['n_objects'] == int(dyn[-1, 0]) + 1
    # the packed children point at existing nodes / chunks; children are never the root
    nodes = a['nodes']
    for c in np.concatenate([nodes['positive'], nodes['negative']]):
        assert (0 < c < len(nodes)) or (0 <= -c < len(a['chunks']))


def _ulps(got, want):
    """|got - want| in units of the last place of the binary32 nearest to want (want a float64)"""
    w = np.float32(want)
    ulp = np.spacing(np.abs(w)) if w != 0 else np.float32(1.4e-45)
    return abs(float(got) - want) / float(ulp)


def test_restatement_sincos_within_two_ulp():
    """the project-owned binary32 sincos (its twin is csrc/hip/world.hip: sincos_rd) against float64 math.sin / math.cos on
    |x| <= 64 pi: random arguments, the neighbourhoods of the multiples of pi / 4, and the small arguments the look input makes"""
    rng = np.random.default_rng(5)
    xs = list(rng.uniform(-64 * math.pi, 64 * math.pi, 40000).astype(np.float32))
    for k in range(-256, 257):
        x = np.float32(k * math.pi / 4)
        xs += [x, np.nextafter(x, np.float32(1e9)), np.nextafter(x, np.float32(-1e9))]
    xs += list(rng.uniform(-0.1, 0.1, 4000).astype(np.float32)) + [np.float32(0.0), np.float32(1e-8), np.float32(-3e-5)]
    worst = 0.0
    for x in xs:
        s, c = world_ref.sincos(float(x))
        ws, wc = math.sin(float(x)), math.cos(float(x))
        # relative to the result where it is not tiny; near a zero, relative to the reduction's absolute error floor
        es = _ulps(s, ws) if abs(ws) > 1e-5 else abs(float(s) - ws) / 1e-12
        ec = _ulps(c, wc) if abs(wc) > 1e-5 else abs(float(c) - wc) / 1e-12
        worst = max(worst, es, ec)
    assert worst <= 2.0, worst


def test_bad_arguments_are_rejected():
    L = rd.lib()
    wad = rd.Wad(ensure_wad(), META_PATH)
    h = ctypes.c_void_p()
    assert L.rdoom_world_create(None, 0, 0, ctypes.byref(h)) == -1
    assert L.rdoom_world_create(wad._h, 0, 0, None) == -1
    assert L.rdoom_world_create(wad._h, 0, 0x80, ctypes.byref(h)) == -1 and b'flags' in L.rdoom_last_error()
    assert L.rdoom_world_create(wad._h, 99, rd.WORLD_HOST_ONLY, ctypes.byref(h)) < 0  # no such level
    assert L.rdoom_world_host_arrays(None, None) == -1
    assert L.rdoom_player_config_default(None) == -1
    world = wad.build_world(0, device=False)
    assert world.n_objects > 1
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is rejected before a launch)
    # null arrays with n > 0
    assert L.rdoom_world_sweep(world._h, None, fake, 4, None, 0, None, fake) == -1 and b'null' in L.rdoom_last_error()
    assert L.rdoom_world_sweep(world._h, fake, fake, 4, None, 0, None, None) == -1
    assert L.rdoom_world_sweep(None, fake, fake, 4, None, 0, None, fake) == -1
    assert L.rdoom_world_step_players(world._h, None, fake, 4, 1, None, ctypes.c_float(0), None, 0, None) == -1
    assert L.rdoom_world_step_players(world._h, fake, None, 4, 1, None, ctypes.c_float(0), None, 0, None) == -1
    assert L.rdoom_world_step_players(world._h, fake, fake, 4, 1, None, ctypes.c_float(-1.0), None, 0, None) == -1
    # offsets for fewer objects than the world has
    assert L.rdoom_world_sweep(world._h, fake, fake, 4, fake, world.n_objects - 1, None, fake) == -1
    assert b'n_objects' in L.rdoom_last_error()
    assert L.rdoom_world_step_players(world._h, fake, fake, 4, 1, None, ctypes.c_float(0), fake, 1, None) == -1
    assert b'n_objects' in L.rdoom_last_error()
    # a host-only world has no device copy
    assert L.rdoom_world_sweep(world._h, fake, fake, 4, None, 0, None, fake) == -1 and b'HOST_ONLY' in L.rdoom_last_error()
    cfg = rd.player_config_default()
    assert cfg['radius'] == np.float32(0.19) and cfg['height'] == np.float32(0.21) and cfg['move_force'] == 60.0


def _digest(path, indices):
    wad = rd.Wad(path, META_PATH)  # every thread its own handle (wad/src/archive.rs:21: an Archive is !Sync)
    h = hashlib.sha256()
    for i in indices:
        for _ in range(2):
            a = wad.build_world(i, device=False).arrays()
            for k in ('nodes', 'chunks', 'triangles', 'verts', 'dynamics'):
                h.update(np.ascontiguousarray(a[k]).tobytes())
    return h.hexdigest()


def test_worlds_from_four_host_threads():
    path = ensure_wad()
    alone = _digest(path, range(9))
    with ThreadPoolExecutor(4) as ex:  # (ctypes releases the GIL inside rdoom_world_create)
        got = list(ex.map(lambda _: _digest(path, range(9)), range(4)))
    assert got == [alone] * 4
