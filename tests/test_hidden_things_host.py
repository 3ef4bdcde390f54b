"""Hidden things on the host, with no GPU: BuiltLevel.decor_things() of every synthetic level against the level's thing table and its
decor vertices; the yardstick of the GPU tests -- a twin level, tests/hidden_ref.py -- against the oracle on arrays with the hidden
triangles deleted; the prototypes; and every argument error of the three calls that is found before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import hidden_ref
import rust_doom_amd as rd
from oracle import raster
from util import META_PATH, ensure_wad

BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 200


@pytest.fixture(scope='module')
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


@pytest.mark.parametrize('level', range(9))
def test_decor_things_name_the_thing_of_every_quad(wad, level):
    built = wad.build_level(level)
    table = built.decor_things()
    things = wad.build_world(level, device=False).map_things()
    verts = built.arrays()['decor_vertices']
    assert table.dtype == np.uint32 and len(verts) % 4 == 0 and len(table) == len(verts) // 4 > 0
    assert (np.diff(table.astype(np.int64)) > 0).all() and int(table[-1]) < len(things)
    for q, i in enumerate(table.tolist()):
        assert verts[4 * q]['a_pos'][0] == things[i]['x'] and verts[4 * q]['a_pos'][2] == things[i]['z'], (q, i)
        for k in range(1, 4):  # the quad's four vertices stand on the thing
            assert verts[4 * q + k]['a_pos'][0] == things[i]['x'] and verts[4 * q + k]['a_pos'][2] == things[i]['z']
    assert not (things['thing_type'][table] == 9999).any()  # the metadata lacks the type: the thing is in the table and draws nothing
    # every decor triangle lies in one quad: what rdoom_level_set_decor_things asks of a descriptor
    tris = built.arrays()['decor_indices'].reshape(-1, 3) // 4
    assert (tris == tris[:, :1]).all() and set(tris[:, 0].tolist()) == set(range(len(table)))


def test_the_thing_table_is_not_needed_for_the_indices(wad):
    """the index counts the things of the decor branch whether or not a table is recorded: a level holds a type-9999 thing in
    front of drawn ones, so an ordinal among the DRAWN things would differ from the table's"""
    built = wad.build_level(0)
    table, things = built.decor_things(), wad.build_world(0, device=False).map_things()
    undrawn = np.flatnonzero(things['thing_type'] == 9999)
    assert len(undrawn) and (table > undrawn[0]).any() and not np.isin(undrawn, table).any()
    assert not np.array_equal(table, np.arange(len(table)))


def decor_ids(arrays):
    """the primitive id of the first triangle of every decor quad (the quad's two triangles follow each other in a draw)"""
    first, at = {}, 0
    for kind, _obj, start, count in np.asarray(arrays['draws']).reshape(-1, 4).tolist():
        if kind == 2:
            for t in range(count // 3):
                first.setdefault(int(arrays['decor_indices'][start + 3 * t]) // 4, at + t)
        at += count // 3
    return first


def facing_poses(built, arrays):
    """two poses at the level's start that face things: the two of sixteen yaws that show the most decor quads, and those quads"""
    ro = raster.RasterOracle(arrays)
    pos, _yaw = built.start()
    lights = built.lights_at(0.0)
    ids = decor_ids(arrays)
    quad_of = {}
    for q, t in ids.items():
        quad_of[t], quad_of[t + 1] = q, q
    found = []
    for k in range(16):
        p = rd.pose_look((pos[0], pos[1] + 0.12, pos[2]), k * np.pi / 8, 0.0, W, H, 0.0)
        _fb, prim = ro.render(p['modelview'], p['projection'], 0.0, lights, W, H, want_prim=True)
        seen = sorted({quad_of[t] for t in np.unique(prim).tolist() if t in quad_of})
        found.append((len(seen), k, p, seen))
    found.sort(key=lambda f: (-f[0], f[1]))
    return [(p, seen) for _n, _k, p, seen in found[:2]], lights


def test_the_twin_level_is_the_level_without_the_hidden_triangles(wad):
    """RasterOracle on the twin == RasterOracle on arrays with those triangles deleted: the frame, and the ids through the remap"""
    built = wad.build_level(0)
    arrays = built.arrays()
    poses, lights = facing_poses(built, arrays)
    base = raster.RasterOracle(arrays)
    for pose, seen in poses:
        assert len(seen) >= 2, seen
        quads = seen[::2] + [q for q in range(len(built.decor_things())) if q % 5 == 0]  # some that show, some anywhere
        tw = hidden_ref.twin(arrays, quads)
        assert np.array_equal(tw['draws'], arrays['draws']) and len(tw['decor_indices']) == len(arrays['decor_indices'])
        gone, old_id = hidden_ref.deleted(arrays, quads)
        assert len(gone['decor_indices']) == len(arrays['decor_indices']) - 6 * len(set(quads))
        args = (pose['modelview'], pose['projection'], 0.0, lights, W, H)
        fb_t, prim_t = raster.RasterOracle(tw).render(*args, want_prim=True)
        fb_d, prim_d = raster.RasterOracle(gone).render(*args, want_prim=True)
        fb_0, prim_0 = base.render(*args, want_prim=True)
        assert np.array_equal(fb_t, fb_d)
        assert np.array_equal(prim_t, hidden_ref.remap(prim_d, old_id))
        ids = decor_ids(arrays)
        hidden_ids = {ids[q] for q in quads} | {ids[q] + 1 for q in quads}
        assert hidden_ids & set(np.unique(prim_0).tolist()) and not hidden_ids & set(np.unique(prim_t).tolist())
        assert (fb_t != fb_0).any()


def test_hidden_quads_of_a_row():
    table = np.array([3, 0, hidden_ref.NO_THING, 33, 31, 3, 64], np.uint32)
    assert hidden_ref.hidden_quads(hidden_ref.row_of([3, 31, 33], 2), table).tolist() == [0, 3, 4, 5]
    assert hidden_ref.hidden_quads(np.array([0xFFFFFFFF], np.uint32), table).tolist() == [0, 1, 4, 5]  # 33 and 64 lie beyond one word
    assert hidden_ref.hidden_quads(np.array([-1, -1, -1], np.int32), table).tolist() == [0, 1, 3, 4, 5, 6]  # never NO_THING
    assert hidden_ref.hidden_quads(np.zeros(2, np.uint32), table).tolist() == []


# ---- the interface ----
def prototype(name):
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, header, flags=re.M)
    assert m, name
    return m.group(1).strip(), [' '.join(a.split()) for a in m.group(2).split(',')]


def test_the_prototypes_argument_by_argument():
    assert prototype('rdoom_built_decor_things') == ('rdoom_status', ['const rdoom_built *built', 'const uint32_t **out', 'uint32_t *out_n'])
    assert prototype('rdoom_level_set_decor_things') == \
        ('rdoom_status', ['rdoom_level *level', 'uint32_t slot', 'const uint32_t *thing_of_quad', 'uint32_t n_quads'])
    assert prototype('rdoom_batch_set_hidden_things') == ('rdoom_status', ['rdoom_batch *batch', 'const uint32_t *d_hidden', 'uint32_t stride'])
    header = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert re.search(r'^#define RDOOM_NO_THING 0xFFFFFFFFu$', header, flags=re.M) and rd.NO_THING == hidden_ref.NO_THING == 0xFFFFFFFF
    for name in ('rdoom_built_decor_things', 'rdoom_level_set_decor_things', 'rdoom_batch_set_hidden_things'):
        assert name in rd.API_SYMBOLS and getattr(rd.lib(), name).restype is ctypes.c_int32


def test_the_calls_check_their_arguments_before_they_touch_a_device(wad):
    """a level and a batch live on a device, so what can be refused without one is a NULL handle -- with every other argument in
    order and never followed -- and the NULL outputs of the built level's call (tests/test_gpu_hidden_things.py has the rest)"""
    L = rd.lib()
    built = wad.build_level(1)
    p, n = ctypes.c_void_p(), ctypes.c_uint32(7)
    fake = ctypes.c_void_p(0x1000)
    assert L.rdoom_built_decor_things(None, ctypes.byref(p), ctypes.byref(n)) == BAD and 'null' in L.rdoom_last_error().decode()
    assert L.rdoom_built_decor_things(built._h, None, ctypes.byref(n)) == BAD
    assert L.rdoom_built_decor_things(built._h, ctypes.byref(p), None) == BAD
    assert p.value is None and n.value == 7  # nothing was written
    assert L.rdoom_built_decor_things(built._h, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 1 and p.value
    assert L.rdoom_level_set_decor_things(None, 0, fake, 1) == BAD and 'null' in L.rdoom_last_error().decode()
    assert L.rdoom_level_set_decor_things(None, 0, None, 0) == BAD
    assert L.rdoom_batch_set_hidden_things(None, fake, 1) == BAD and 'null' in L.rdoom_last_error().decode()
    assert L.rdoom_batch_set_hidden_things(None, None, 0) == BAD
