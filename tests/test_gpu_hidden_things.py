"""GPU: hidden things (rdoom_batch_set_hidden_things; setup.hip cull_kernel<true>).  A render with rows of thing bits must be, bit for
bit, the render of the TWIN level of every pose (tests/hidden_ref.py: the hidden quads' triangles collapsed to a point, which the
determinant test culls) -- against the oracle on the twin, frame and primitive ids, and against a second device level made of the
twins and rendered without rows, which also covers the depth and the label plane.  320 x 200 frames, at most 16 poses a case."""
import ctypes
import functools

import numpy as np
import pytest

import hidden_ref
import rust_doom_amd as rd
from hidden_ref import NO_THING
from oracle import raster
from util import META_PATH, ensure_wad, render_checked

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
W, H = 320, 200
NO_DECOR = rd.ALL_KINDS & ~(1 << rd.KIND_DECOR)


@functools.lru_cache(maxsize=None)
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


@functools.lru_cache(maxsize=None)
def level(index):
    """a built level, its arrays, its decor-thing table and its thing table (computed once and left unchanged)"""
    built = wad().build_level(index)
    return dict(built=built, arrays=built.arrays(), table=built.decor_things(), things=wad().build_world(index, device=False).map_things(),
                lights=built.lights_at(0.0))


def look_at(eye, target):
    """the pose at `eye` that looks at `target` (forward is (-sin yaw, -cos yaw) on the map)"""
    d = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    return rd.pose_look(tuple(float(x) for x in eye), float(np.arctan2(-d[0], -d[2])), float(np.arctan2(d[1], np.hypot(d[0], d[2]))), W, H, 0.0)


def poses_at_things(lv, n, seed):
    """n poses, each 0.9 from a drawn thing of the level and a little above it, looking at it"""
    rng = np.random.default_rng(seed)
    drawn = lv['things'][lv['table']]
    poses = np.zeros(n, rd.POSE)
    for p in range(n):
        t = drawn[(p * 5 + seed) % len(drawn)]
        a = rng.uniform(0, 2 * np.pi)
        eye = (t['x'] + 0.9 * np.cos(a), t['base'] + 0.45, t['z'] + 0.9 * np.sin(a))
        poses[p] = look_at(eye, (t['x'], t['base'] + 0.2, t['z']))
    return poses


def rows_tensor(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, U).view(np.int32).copy()).cuda()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = got.view(bits) != want.view(bits)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def oracle_frames(arrays_of, tables_of, rows, poses, lights, lop, om=None):
    """per pose: the twin of its level under its row, and the oracle's frame and primitive ids of it"""
    twins, fbs, prims = [], [], []
    for p in range(len(poses)):
        k = int(lop[p])
        tw = hidden_ref.twin(arrays_of[k], hidden_ref.hidden_quads(rows[p], tables_of[k]))
        li = lights[p] if np.ndim(lights) == 2 else lights
        fb, prim = raster.RasterOracle(tw).render(poses[p]['modelview'], poses[p]['projection'], float(poses[p]['time']), li, W, H,
                                                  want_prim=True, object_modelviews=None if om is None else om[p])
        twins.append(tw), fbs.append(fb), prims.append(prim)
    return twins, np.stack(fbs), np.stack(prims)


def check(dev_level, arrays_of, tables_of, rows, poses, lights, lop=None, om=None, stride=None):
    """the render of `poses` on a batch of dev_level with `rows` hidden: against the oracle on every pose's twin and against a device
    level set of the twins rendered without rows.  Returns (frames, primitive ids) for the caller's own assertions"""
    n = len(poses)
    rows = np.ascontiguousarray(rows, U)
    assert rows.shape[0] == n and (stride is None or stride == rows.shape[1])
    lop_ = np.zeros(n, U) if lop is None else np.asarray(lop, U)
    twins, ofb, oprim = oracle_frames(arrays_of, tables_of, rows, poses, lights, lop_, om)
    kw = {}
    if lop is not None:
        kw['level_of_pose'] = lop_
    if om is not None:
        kw['object_modelviews'] = om
    batch = rd.Batch(dev_level, W, H, n)
    dev_rows = rows_tensor(rows)
    batch.set_hidden_things(dev_rows)
    fb_plain, fb_ids, prim = render_checked(batch, poses, lights, **kw)
    depth, label = batch.read_depth(), batch.read_plane(rd.PLANE_LABEL)
    same(fb_plain, ofb, 'frames without ids against the oracle on the twins')
    same(fb_ids, ofb, 'frames with ids against the oracle on the twins')
    same(prim, oprim, 'primitive ids against the oracle on the twins')
    # the twins as a level set of their own, one level per pose, no rows
    second = rd.Batch(rd.DeviceLevelSet(twins), W, H, n)
    second.enable_primitive_ids()
    tkw = dict(kw, level_of_pose=np.arange(n, dtype=U))
    second.render(poses, lights, **tkw)
    same(fb_ids, second.read_framebuffer(), 'frames against the twin levels')
    same(prim, second.read_primitive_ids(), 'primitive ids against the twin levels')
    same(depth, second.read_depth(), 'depth against the twin levels')
    same(label, second.read_plane(rd.PLANE_LABEL), 'labels against the twin levels')
    batch.finish()
    return fb_ids, prim


def decor_prims(arrays):
    """{quad: (its two primitive ids)}"""
    out, at = {}, 0
    for kind, _obj, start, count in np.asarray(arrays['draws']).reshape(-1, 4).tolist():
        if kind == rd.KIND_DECOR:
            for t in range(count // 3):
                out.setdefault(int(arrays['decor_indices'][start + 3 * t]) // 4, []).append(at + t)
        at += count // 3
    return out


def quads_shown(arrays, prim):
    """the decor quads with a pixel in the primitive ids of one frame or of several"""
    seen = set(np.unique(prim).tolist())
    return sorted(q for q, ids in decor_prims(arrays).items() if seen & set(ids))


def plain_render(dev_level, poses, lights, **kw):
    batch = rd.Batch(dev_level, W, H, len(poses))
    batch.enable_primitive_ids()
    batch.render(poses, lights, **kw)
    return batch.read_framebuffer(), batch.read_primitive_ids()


# ---- E1M1: rows of every kind -------------------------------------------------------------------------------------------------------

def test_every_pose_has_a_row_of_its_own():
    rd.set_device(0)
    lv = level(0)
    n = 16
    poses = poses_at_things(lv, n, 3)
    rows = np.random.default_rng(7).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(U)
    assert len({r.tobytes() for r in rows}) == n
    dev = rd.DeviceLevel(lv['built'])
    fb, prim = check(dev, [lv['arrays']], [lv['table']], rows, poses, lv['lights'])
    fb0, prim0 = plain_render(dev, poses, lv['lights'])
    changed = [(fb[p] != fb0[p]).any() for p in range(n)]
    assert sum(changed) >= n // 2, changed  # the poses face things: half of them, at random, are gone
    for p in range(n):  # what a pose still shows of the decor is what its row leaves
        hidden = set(hidden_ref.hidden_quads(rows[p], lv['table']).tolist())
        assert not hidden & set(quads_shown(lv['arrays'], prim[p])) and set(quads_shown(lv['arrays'], prim0[p])) - hidden <= set(quads_shown(lv['arrays'], prim[p]))


def test_zero_rows_no_rows_and_rows_switched_off_are_todays_render():
    rd.set_device(0)
    lv = level(0)
    n = 8
    poses = poses_at_things(lv, n, 5)
    dev = rd.DeviceLevel(lv['built'])
    fb0, prim0 = plain_render(dev, poses, lv['lights'])
    assert quads_shown(lv['arrays'], prim0)
    fb, prim = check(dev, [lv['arrays']], [lv['table']], np.zeros((n, 2), U), poses, lv['lights'])
    same(fb, fb0, 'all-zero rows')
    same(prim, prim0, 'all-zero rows, ids')
    batch = rd.Batch(dev, W, H, n)
    batch.enable_primitive_ids()
    batch.set_hidden_things(rows_tensor(np.full((n, 2), 0xFFFFFFFF, U)))
    batch.render(poses, lv['lights'])
    assert (batch.read_framebuffer() != fb0).any()
    batch.set_hidden_things(None)  # the full frame is back
    batch.render(poses, lv['lights'])
    same(batch.read_framebuffer(), fb0, 'rows switched off')
    same(batch.read_primitive_ids(), prim0, 'rows switched off, ids')


def test_all_bits_set_hides_every_decoration():
    rd.set_device(0)
    lv = level(0)
    n = 8
    poses = poses_at_things(lv, n, 9)
    dev = rd.DeviceLevel(lv['built'])
    fb, prim = check(dev, [lv['arrays']], [lv['table']], np.full((n, 2), 0xFFFFFFFF, U), poses, lv['lights'])
    assert not quads_shown(lv['arrays'], prim)
    fb_k, prim_k = plain_render(dev, poses, lv['lights'], kinds=NO_DECOR)
    same(fb, fb_k, 'all bits against kinds without decor')
    same(prim, prim_k, 'ids')


def test_bits_that_no_quad_maps_to_change_nothing():
    """bits at and beyond the level's thing count, and the bits of the things that draw nothing (type 9999, no metadata)"""
    rd.set_device(0)
    lv = level(0)
    n = 4
    poses = poses_at_things(lv, n, 11)
    t_n = len(lv['things'])
    undrawn = np.flatnonzero(lv['things']['thing_type'] == 9999)
    assert 32 < t_n < 64 and len(undrawn) and not np.isin(undrawn, lv['table']).any()
    rows = np.stack([hidden_ref.row_of(range(t_n, 64), 2), hidden_ref.row_of(undrawn, 2), hidden_ref.row_of(list(undrawn) + list(range(t_n, 64)), 2),
                     hidden_ref.row_of([63], 2)])
    dev = rd.DeviceLevel(lv['built'])
    fb, prim = check(dev, [lv['arrays']], [lv['table']], rows, poses, lv['lights'])
    fb0, prim0 = plain_render(dev, poses, lv['lights'])
    assert quads_shown(lv['arrays'], prim0)
    same(fb, fb0, 'bits no quad maps to')
    same(prim, prim0, 'ids')


def test_a_wider_stride_and_a_stride_of_one_word():
    rd.set_device(0)
    # two words more than the level needs, random everywhere
    lv = level(0)
    n = 8
    poses = poses_at_things(lv, n, 13)
    rows = np.random.default_rng(17).integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(U)
    check(rd.DeviceLevel(lv['built']), [lv['arrays']], [lv['table']], rows, poses, lv['lights'], stride=4)
    # one word on a level with more than 32 drawn things: the quads of things 32 and above stay
    lv = level(5)
    assert len(lv['table']) > 32 and (lv['table'] >= 32).sum() >= 4
    late = lv['things'][lv['table'][lv['table'] >= 32]]
    poses = np.zeros(n, rd.POSE)
    for p in range(n):
        t = late[p % len(late)]
        a = 0.8 * p
        poses[p] = look_at((t['x'] + 0.9 * np.cos(a), t['base'] + 0.45, t['z'] + 0.9 * np.sin(a)), (t['x'], t['base'] + 0.2, t['z']))
    dev = rd.DeviceLevel(lv['built'])
    fb, prim = check(dev, [lv['arrays']], [lv['table']], np.full((n, 1), 0xFFFFFFFF, U), poses, lv['lights'], stride=1)
    shown = quads_shown(lv['arrays'], prim)
    assert shown and (lv['table'][shown] >= 32).all()
    _fb0, prim0 = plain_render(dev, poses, lv['lights'])
    assert (lv['table'][quads_shown(lv['arrays'], prim0)] < 32).any()  # without rows the frames show earlier things as well


# ---- a hand-made level: a table that is no identity ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hand_made():
    """E1M1's arrays with 70 small decor quads appended in a 10 x 7 grid 1.2 in front of the start pose, and a table that is a
    permutation of the level's own followed by one with repeats: several quads map to one thing, one entry is NO_THING, and some
    lie beyond the two words of the rows"""
    lv = level(0)
    arrays = dict(lv['arrays'])
    pos, yaw = lv['built'].start()
    fwd = np.array([-np.sin(yaw), -np.cos(yaw)])
    right = np.array([np.cos(yaw), -np.sin(yaw)])
    verts = [arrays['decor_vertices']]
    n0 = len(arrays['decor_vertices']) // 4
    proto = arrays['decor_vertices'][:4]
    new_idx = []
    for q in range(70):
        col, row = q % 10, q // 10
        c = np.array([pos[0], pos[2]]) + 1.2 * fwd + (col - 4.5) * 0.09 * right
        v = proto.copy()
        v['a_pos'][:, 0], v['a_pos'][:, 2] = F(c[0]), F(c[1])
        v['a_pos'][:2, 1], v['a_pos'][2:, 1] = F(pos[1] - 0.25 + 0.09 * row), F(pos[1] - 0.25 + 0.09 * row + 0.07)
        v['a_local_x'] = F([-0.035, 0.035, 0.035, -0.035])
        verts.append(v)
        b = 4 * (n0 + q)
        new_idx += [b, b + 1, b + 3, b + 1, b + 2, b + 3]
    arrays['decor_vertices'] = np.concatenate(verts)
    draws = np.array(arrays['draws'], U, copy=True).reshape(-1, 4)
    decor = np.flatnonzero(draws[:, 0] == rd.KIND_DECOR)
    assert len(decor) == 1 and draws[decor[0], 2] + draws[decor[0], 3] == len(arrays['decor_indices'])  # one decor draw: it grows at its end
    draws[decor[0], 3] += len(new_idx)
    arrays['draws'] = draws
    arrays['decor_indices'] = np.concatenate([arrays['decor_indices'], np.array(new_idx, U)])
    own = np.random.default_rng(23).permutation(n0).astype(U) + 64  # the level's own quads: things 64 .. 94, beyond the rows
    mapped = np.array([(q * 7) % 64 if q % 3 else (0, 31, 32, 33, 63)[(q // 3) % 5] for q in range(70)], U)
    mapped[40] = NO_THING
    table = np.concatenate([own, mapped])
    assert not np.array_equal(table, np.arange(len(table))) and len(set(mapped.tolist())) < 70
    return dict(arrays=arrays, table=table, n0=n0, start=(pos, yaw))


def test_a_hand_made_level_with_a_table_that_is_no_identity():
    rd.set_device(0)
    c, lv = hand_made(), level(0)
    pos, yaw = c['start']
    n = 6
    poses = np.zeros(n, rd.POSE)
    for p in range(n):
        poses[p] = rd.pose_look((pos[0], pos[1] + 0.12, pos[2]), float(yaw) + 0.08 * (p - 2), -0.1, W, H, 0.0)
    rows = np.stack([hidden_ref.row_of([0, 31, 32, 33, 63], 2), hidden_ref.row_of([0], 2), hidden_ref.row_of([31, 32], 2),
                     hidden_ref.row_of([33, 63, 7, 14, 21], 2), np.full(2, 0xFFFFFFFF, U), np.zeros(2, U)])
    dev = rd.DeviceLevel(c['arrays'])
    batch = rd.Batch(dev, W, H, n)
    with pytest.raises(rd.RdoomError) as e:  # decor triangles and no table yet
        batch.set_hidden_things(rows_tensor(rows))
    assert e.value.status == -1 and 'thing table' in str(e.value)
    dev.set_decor_things(np.zeros(len(c['table']), U))
    dev.set_decor_things(c['table'])  # calling again replaces the table
    fb, prim = check(dev, [c['arrays']], [c['table']], rows, poses, lv['lights'])
    _fb0, prim0 = plain_render(dev, poses, lv['lights'])
    new = [q for q in quads_shown(c['arrays'], prim0[5]) if q >= c['n0']]
    assert len(new) >= 40, len(new)  # the grid is in front of the start pose
    for p in range(5):
        hidden = set(hidden_ref.hidden_quads(rows[p], c['table']).tolist())
        assert hidden & set(new) and not hidden & set(quads_shown(c['arrays'], prim[p])), p
    # under a row of all ones the quad of NO_THING and the level's own quads (things 64 and above) stay, and nothing else
    stay = {q for q in range(len(c['table'])) if q < c['n0'] or q == c['n0'] + 40}
    assert c['n0'] + 40 in quads_shown(c['arrays'], prim[4]) and set(quads_shown(c['arrays'], prim[4])) <= stay


# ---- a level set, moving objects -----------------------------------------------------------------------------------------------------

def test_a_level_set_where_one_row_means_different_things_per_level():
    rd.set_device(0)
    idx = (0, 5, 2)
    lvs = [level(i) for i in idx]
    lop = np.array([0, 1, 2, 2, 1, 0, 1, 0, 2, 0, 1, 2], U)
    n = len(lop)
    poses = np.zeros(n, rd.POSE)
    for k in range(3):
        sel = np.flatnonzero(lop == k)
        poses[sel] = poses_at_things(lvs[k], len(sel), 31 + k)
    lights = np.stack([lvs[k]['lights'] for k in lop])
    row = np.array([0x5A5AA5A5, 0x0000FF0F], U)  # one pattern for every pose
    rows = np.repeat(row[None], n, 0)
    hid = [set(l['table'][hidden_ref.hidden_quads(row, l['table'])].tolist()) for l in lvs]
    assert all(hid) and len({tuple(sorted(h)) for h in hid}) == 3
    dev = rd.DeviceLevelSet([l['built'] for l in lvs])  # (the three tables are attached by the constructor)
    fb, prim = check(dev, [l['arrays'] for l in lvs], [l['table'] for l in lvs], rows, poses, lights, lop=lop)
    fb0, _prim0 = plain_render(dev, poses, lights, level_of_pose=lop)
    assert all((fb[lop == k] != fb0[lop == k]).any() for k in range(3))


def test_a_lift_that_carries_a_thing():
    """E1M2's one thing stands on object 1: object_modelviews lift it, and the row hides it in the even poses only"""
    rd.set_device(0)
    lv = level(1)
    assert lv['table'].tolist() == [0] and lv['things']['object_id'][0] == 1
    dev = rd.DeviceLevel(lv['built'])
    n_obj = dev.num_objects()
    t = lv['things'][0]
    n = 6
    poses, om = np.zeros(n, rd.POSE), np.zeros((n, n_obj, 16), F)
    for p in range(n):
        a, lift = 1.0 * p, 0.15 * p
        poses[p] = look_at((t['x'] + 0.9 * np.cos(a), t['base'] + 0.45 + lift, t['z'] + 0.9 * np.sin(a)), (t['x'], t['base'] + 0.2 + lift, t['z']))
        view = np.asarray(poses[p]['modelview'], np.float64).reshape(4, 4).T
        for o in range(n_obj):
            m = np.eye(4)
            m[1, 3] = lift if o == 1 else 0.0
            om[p, o] = (view @ m).T.astype(F).reshape(16)
    rows = np.array([[1 - p % 2] for p in range(n)], U)
    fb, prim = check(dev, [lv['arrays']], [lv['table']], rows, poses, lv['lights'], om=om)
    shown = [bool(quads_shown(lv['arrays'], prim[p])) for p in range(n)]
    assert shown == [False, True] * 3, shown


# ---- sensed, collected and gone, on one stream ---------------------------------------------------------------------------------------

def test_two_players_collect_one_candle_a_tick_apart():
    """step_game -> sense_things(collect=ammo) -> render_players with the collected rows, tick after tick on one stream with no host
    wait.  Player 1's inputs trail player 0's by a tick, so it reaches the candle a tick later: each frame loses the candle in its
    player's own tick.  The frames of every tick are held against renders, without rows, of the level and of the candle's twin."""
    rd.set_device(0)
    lv = level(0)
    things = lv['things']
    candle = 17
    assert things['thing_type'][candle] == 34 and (things['category'][candle] & 0xFF) == rd.THING_AMMO
    quad = int(np.flatnonzero(lv['table'] == candle)[0])
    ids = decor_prims(lv['arrays'])[quad]
    t = things[candle]
    st = rd.player_states(np.repeat(F([[t['x'], t['base'] + 0.33, t['z'] + 0.8]]), 2, 0), F([0.0, 0.0]), pitch=-0.9)
    settle, ticks = 30, 30
    inp = np.zeros((settle + ticks + 1, 2), rd.PLAYER_INPUT)
    inp['movement'][settle:, 0, 1] = -1.0      # forwards: towards -z, the candle
    inp['movement'][settle + 1:, 1, 1] = -1.0  # the same walk, one tick later
    world = wad().build_world(0)
    dev_things = rd.DeviceThings(things)
    words = dev_things.words()
    dev = rd.DeviceLevel(lv['built'])
    twin_dev = rd.DeviceLevel(hidden_ref.twin(lv['arrays'], [quad]))
    batch = rd.Batch(dev, W, H, 2)
    batch.enable_primitive_ids()
    game, offs = world.game_state(2)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda()
    lights = torch.from_numpy(lv['lights'].copy()).cuda()
    collected = torch.zeros((2, words), dtype=torch.int32, device='cuda')
    batch.set_hidden_things(collected)
    keep_rows = torch.zeros((ticks, 2, words), dtype=torch.int32, device='cuda')
    keep_states = torch.zeros((ticks, states.numel()), dtype=torch.uint8, device='cuda')
    keep_prim = torch.zeros((ticks, 2, H, W), dtype=torch.int32, device='cuda')
    keep_depth = torch.zeros((ticks, 2, H, W), dtype=torch.float32, device='cuda')
    keep_rgb = torch.zeros((ticks, 2, H, W, 3), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        world.step_game(states, ti[:settle * 40], game, offs, n_ticks=settle, stream=stream)  # both come to rest on the floor
        for k in range(ticks):
            at = (settle + k) * 40
            world.step_game(states, ti[at:at + 40], game, offs, n_ticks=1, stream=stream)
            world.sense_things(states, dev_things, max_range=10.0, touch_below=1.0, touch_above=1.0, collect=(rd.THING_AMMO,), offsets=offs,
                               collected=collected, stream=stream)
            batch.render_players(states, lights, offsets=offs, stream=stream)
            batch.resolve_plane(keep_prim[k], rd.PLANE_PRIMITIVE, stream=stream)
            batch.resolve_depth(keep_depth[k], stream=stream)
            batch.resolve_rgb(keep_rgb[k], stream=stream)
            keep_rows[k].copy_(collected)
            keep_states[k].copy_(states)
    stream.synchronize()
    batch.finish()
    rows = keep_rows.cpu().numpy().view(U)
    got_it = (rows[:, :, candle >> 5] >> (candle & 31)) & 1  # (ticks, 2)
    assert got_it[0].tolist() == [0, 0] and got_it[-1].tolist() == [1, 1], got_it.T.tolist()
    first = [int(np.argmax(got_it[:, p])) for p in range(2)]
    assert first[1] == first[0] + 1, first
    assert (np.diff(got_it, axis=0) >= 0).all()  # never given back
    prim = keep_prim.cpu().numpy().view(U)
    shows = np.array([[bool(np.isin(prim[k, p], ids).any()) for p in range(2)] for k in range(ticks)])
    # each player's frame loses the candle in its own tick and not in the other's
    assert shows[first[0] - 1].tolist() == [True, True] and shows[first[0]].tolist() == [False, True] and shows[first[1]].tolist() == [False, False]
    assert (shows == (got_it == 0))[:first[1] + 3].all(), (shows.T.tolist(), got_it.T.tolist())
    # the three ticks around the pick-ups, whole frames: the level where the player still has the candle to take, the twin where not
    full, gone = rd.Batch(dev, W, H, 2), rd.Batch(twin_dev, W, H, 2)
    depth, rgb = keep_depth.cpu().numpy(), keep_rgb.cpu().numpy()
    for k in (first[0] - 1, first[0], first[1]):
        for b in (full, gone):
            b.enable_primitive_ids()
            b.render_players(keep_states[k], lights, offsets=offs)
        for p in range(2):
            ref = gone if got_it[k, p] else full
            same(prim[k, p], ref.read_plane(rd.PLANE_PRIMITIVE, p, 1)[0], ('ids', k, p))
            same(depth[k, p], ref.read_depth(p, 1)[0], ('depth', k, p))
            same(rgb[k, p], ref.read_rgb(p, 1)[0], ('rgb', k, p))
    assert (full.read_rgb() != gone.read_rgb()).any()


# ---- the errors that need a device -----------------------------------------------------------------------------------------------

def test_the_argument_errors_that_need_a_device():
    rd.set_device(0)
    L = rd.lib()
    lv, small = level(0), level(1)
    dev = rd.DeviceLevel(lv['arrays'])  # from arrays: no table attached
    n_quads = len(lv['table'])
    table = np.ascontiguousarray(lv['table'], U)
    ptr = table.ctypes.data_as(ctypes.c_void_p)

    def fails(word, status):
        assert status == -1 and word in L.rdoom_last_error().decode(), (word, status, L.rdoom_last_error())

    fails('null', L.rdoom_level_set_decor_things(dev._h, 0, None, n_quads))
    fails('slot', L.rdoom_level_set_decor_things(dev._h, 1, ptr, n_quads))
    fails('n_quads', L.rdoom_level_set_decor_things(dev._h, 0, ptr, n_quads - 1))
    fails('n_quads', L.rdoom_level_set_decor_things(dev._h, 0, ptr, n_quads + 1))
    fails('n_quads', L.rdoom_level_set_decor_things(dev._h, 0, None, 0))
    spans = dict(lv['arrays'])
    spans['decor_indices'] = np.array(lv['arrays']['decor_indices'], U, copy=True)
    spans['decor_indices'][2] = 4  # triangle 0: vertices 0, 1 and 4 -- two quads
    bad = rd.DeviceLevel(spans)
    fails('one quad', L.rdoom_level_set_decor_things(bad._h, 0, ptr, n_quads))
    lset = rd.DeviceLevelSet([lv['arrays'], small['arrays']])
    fails('slot', L.rdoom_level_set_decor_things(lset._h, 2, ptr, n_quads))
    lset.set_decor_things(0, lv['table'])
    rows = torch.zeros((4, 2), dtype=torch.int32, device='cuda')
    batch, set_batch = rd.Batch(dev, 64, 64, 4), rd.Batch(lset, 64, 64, 4)
    fails('thing table', L.rdoom_batch_set_hidden_things(batch._h, ctypes.c_void_p(rows.data_ptr()), 2))
    fails('level 1', L.rdoom_batch_set_hidden_things(set_batch._h, ctypes.c_void_p(rows.data_ptr()), 2))  # slot 0 has its table, slot 1 not
    dev.set_decor_things(lv['table'])
    lset.set_decor_things(1, small['table'])
    fails('stride', L.rdoom_batch_set_hidden_things(batch._h, ctypes.c_void_p(rows.data_ptr()), 0))
    fails('aligned', L.rdoom_batch_set_hidden_things(batch._h, ctypes.c_void_p(rows.data_ptr() + 2), 2))
    assert L.rdoom_batch_set_hidden_things(batch._h, None, 0) == 0  # off: the stride is not looked at
    assert L.rdoom_batch_set_hidden_things(batch._h, ctypes.c_void_p(rows.data_ptr()), 2) == 0
    assert L.rdoom_batch_set_hidden_things(set_batch._h, ctypes.c_void_p(rows.data_ptr()), 2) == 0
    # the wrapper: a tensor that does not fit, and fewer rows than a render has poses
    for wrong in (torch.zeros((4, 2), dtype=torch.float32, device='cuda'), torch.zeros((4, 2), dtype=torch.int32), torch.zeros(8, dtype=torch.int32, device='cuda'),
                  torch.zeros((4, 2), dtype=torch.int16, device='cuda')):
        with pytest.raises(ValueError):
            batch.set_hidden_things(wrong)
    with pytest.raises(ValueError):
        batch.set_hidden_things(rows, stride=3)
    with pytest.raises(ValueError):
        batch.set_hidden_things(rows.data_ptr())  # a raw pointer needs its stride
    batch.set_hidden_things(rows[:2])
    poses = poses_at_things(lv, 4, 1)
    with pytest.raises(ValueError):
        batch.render(poses, lv['lights'])
    batch.render(poses[:2], lv['lights'])
    batch.finish()
