"""Child process of tests/test_gpu_framethings.py (rdoom_debug_set is process-wide; prints one RESULT line).  Every expected plane is
tests/framethings_ref.py's, from the ORACLE's winners; every render goes through util.render_checked, so follows a dirtying render;
every comparison is array_equal.  Frames of at most 321 x 200, at most 16 poses.
  hooks      E1M1's two facing poses at 320 x 200 and 321 x 200 under every equivalent-path test hook in turn: the thing plane in both
             row orders, on the plain and on the id path, a first / count sub-range into a tensor, and frame_things of it with and
             without the depth plane resolve_depth wrote
  levels     a level set of three levels with level_of_pose mixed: the indices are per level
  handmade   E1M1 plus a 10 x 7 grid of quads before the start pose, with a table that is a permutation with repeats, one NO_THING
             and indices at and above 32; the same from so close that a quadrant is one decor triangle's; rows of hidden things;
             and the handle before a table is attached
  synthetic  frame_things on tensors of the smallest shapes where it can go wrong
  graph      frame_things alone captured into a graph and replayed twice
  lift       E1M2, whose one thing rides object 1: render_players with offsets
  tick       4 players for 3 ticks of the closed loop on one side stream
  errors     the argument errors that need a device, the wrappers' refusals, raw device pointers"""
import sys

import numpy as np
import torch  # before the library is loaded: torch and the library then share one HIP runtime

import conftest  # noqa: F401  (sys.path)
import framethings_ref as fr
import hidden_ref
import rust_doom_amd as rd
from oracle import raster
from util import META_PATH, ensure_wad, render_checked

HOOKS = [{}, {'vis32': 1}, {'no_qtab': 1}, {'keep_vis': 1}, {'leak_mod': 97}, {'no_bins': 1}, {'entry_cap': 300}]
H = 200
U = np.uint32
BAD = [0]
CHECKS = [0]


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    CHECKS[0] += 1
    if got.shape != want.shape or got.dtype.itemsize != want.dtype.itemsize or not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        n = -1 if got.shape != want.shape else int((got != want).sum())
        print('MISMATCH %s: %d elements' % (what, n))
        BAD[0] += 1


def oracle_prims(arrays, poses, lights, w, h, om=None):
    ro = raster.RasterOracle(arrays)
    return np.stack([ro.render(poses[p]['modelview'], poses[p]['projection'], float(poses[p]['time']),
                               lights[p] if np.ndim(lights) == 2 else lights, w, h, want_prim=True,
                               object_modelviews=None if om is None else om[p])[1] for p in range(len(poses))])


def check_reduce(ids_t, depth_t, max_things, min_pixels, stride, what, **kw):
    """frame_things of device tensors against the numpy reduction of the same tensors"""
    ids = ids_t.cpu().numpy()
    depth = None if depth_t is None else depth_t.cpu().numpy()
    words = (max_things + 31) // 32
    bits_out = None if stride in (None, words) else torch.full((ids.shape[0], stride), 0x55AA55AA, dtype=torch.int32, device='cuda')
    table, bits = rd.frame_things(ids_t, depth_t, max_things=max_things, min_pixels=min_pixels, bits_out=bits_out, **kw)
    torch.cuda.synchronize()
    want_t, want_b = fr.reduce(ids, depth, max_things, min_pixels, stride or words)
    same(table.cpu().numpy(), fr.as_words(want_t), what + ': table')
    same(bits.cpu().numpy().view(U), want_b, what + ': bits')
    return want_t


def check_batch(batch, want, poses, lights, what, stride_things=64, **kw):
    """the thing plane of `poses` on both paths and in both row orders against `want`; frame_things of it"""
    n, h, w = want.shape
    for path in ('plain', 'ids'):
        render_checked(batch, poses, lights, want_prim=(path == 'ids'), **kw)
        for td in (False, True):
            same(batch.read_thing_plane(top_down=td), want[:, ::-1] if td else want, '%s (%s path, top_down=%s)' % (what, path, td))
        # a sub-range into a tensor on a side stream, top-down; then the reduction, with the depth plane and without
        s = torch.cuda.Stream()
        first, count = (1, n - 1) if n > 1 else (0, 1)
        px = torch.full((count, h, w), 7, dtype=torch.int32, device='cuda')
        depth = torch.zeros((count, h, w), dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        batch.resolve_thing_plane(px, first=first, count=count, top_down=True, stream=s)
        batch.resolve_depth(depth, first=first, count=count, top_down=True, stream=s)
        with torch.cuda.stream(s):
            table, bits = rd.frame_things(px, depth, max_things=stride_things, min_pixels=12, stream=s)
        s.synchronize()
        batch.finish()
        same(px.cpu().numpy(), want[first:first + count, ::-1], '%s (%s path, sub-range)' % (what, path))
        want_t, want_b = fr.reduce(px.cpu().numpy(), depth.cpu().numpy(), stride_things, 12, (stride_things + 31) // 32)
        same(table.cpu().numpy(), fr.as_words(want_t), '%s (%s path): table with depth' % (what, path))
        same(bits.cpu().numpy().view(U), want_b, '%s (%s path): bits' % (what, path))
        shown = want_t['count'] > 0
        if shown.any() and not (np.isfinite(want_t['depth_min'][shown]).all() and (want_t['depth_min'][shown] > 0).all()):
            print('MISMATCH %s: a thing in the frame has no depth' % what)
            BAD[0] += 1
        check_reduce(px, None, stride_things, 1, None, '%s (%s path), no depth' % (what, path))


def e1m1():
    from test_hidden_things_host import facing_poses
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    arrays = built.arrays()
    found, lights = facing_poses(built, arrays)
    pos, _yaw = built.start()
    eye = (pos[0], pos[1] + 0.12, pos[2])
    yaws = []
    for p, _seen in found:  # the yaw of each facing pose, to look the same way in a frame of another width
        ks = [k for k in range(16) if np.array_equal(rd.pose_look(eye, k * np.pi / 8, 0.0, 320, H, 0.0)['modelview'], p['modelview'])]
        assert len(ks) == 1
        yaws.append(ks[0] * np.pi / 8)
    return wad, built, arrays, lights, eye, yaws


def hooks_case():
    _wad, built, arrays, lights, eye, yaws = e1m1()
    table = built.decor_things()
    level = rd.DeviceLevel(built)
    for w in (320, 321):
        poses = np.zeros(2, rd.POSE)
        for i, yaw in enumerate(yaws):
            poses[i] = rd.pose_look(eye, yaw, 0.0, w, H, 0.0)
        want = fr.thing_plane(arrays, table, oracle_prims(arrays, poses, lights, w, H))
        for f in range(2):
            assert len(set(want[f][want[f] >= 0].tolist())) >= 2, 'a facing pose shows fewer than two things'
        for hooks in HOOKS:
            rd.debug_set('reset')
            for name, value in hooks.items():
                rd.debug_set(name, value)
            batch = rd.Batch(level, w, H, 2)  # (vis32 / entry_cap are read here)
            check_batch(batch, want, poses, lights, 'E1M1 %d x %d hooks=%r' % (w, H, hooks))
            batch.close()
        rd.debug_set('reset')


def levels_case():
    import importlib
    tg = importlib.import_module('test_gpu_hidden_things')
    idx = (0, 5, 2)
    lvs = [tg.level(i) for i in idx]
    lop = np.array([0, 1, 2, 2, 1, 0], U)
    poses = np.zeros(len(lop), rd.POSE)
    for k in range(3):
        sel = np.flatnonzero(lop == k)
        poses[sel] = tg.poses_at_things(lvs[k], len(sel), 31 + k)
    lights = np.stack([lvs[k]['lights'] for k in lop])
    want = np.stack([fr.thing_plane(lvs[k]['arrays'], lvs[k]['table'], oracle_prims(lvs[k]['arrays'], poses[p:p + 1], lights[p], 320, H)[0])
                     for p, k in enumerate(lop.tolist())])
    per_level = [set(want[lop == k][want[lop == k] >= 0].tolist()) for k in range(3)]
    assert all(per_level) and len({tuple(sorted(s)) for s in per_level}) == 3, per_level
    dev = rd.DeviceLevelSet([l['built'] for l in lvs])
    check_batch(rd.Batch(dev, 320, H, len(lop)), want, poses, lights, 'level set', stride_things=128, level_of_pose=lop)


def handmade_case():
    import importlib
    tg = importlib.import_module('test_gpu_hidden_things')
    c, lv = tg.hand_made(), tg.level(0)
    arrays, table = c['arrays'], c['table']
    pos, yaw = c['start']
    lights = lv['lights']
    n = 4
    poses = np.zeros(n, rd.POSE)
    for p in range(n):
        poses[p] = rd.pose_look((pos[0], pos[1] + 0.12, pos[2]), float(yaw) + 0.08 * (p - 1), -0.1, 320, H, 0.0)
    prims = oracle_prims(arrays, poses, lights, 320, H)
    want = fr.thing_plane(arrays, table, prims)
    quad = fr.quad_of_primitive(arrays)
    drawn = prims != 0xFFFFFFFF
    quads = set(np.unique(quad[prims[drawn]]).tolist())
    shown = set(want[want >= 0].tolist())
    # the carrier of indices >= 32, of two quads of one thing, and of NO_THING, from the reference
    assert any(t >= 32 for t in shown), shown
    assert c['n0'] + 40 in quads and table[c['n0'] + 40] == hidden_ref.NO_THING
    assert any(len([q for q in quads if q >= 0 and table[q] == t]) >= 2 for t in shown)
    dev = rd.DeviceLevel(arrays)
    batch = rd.Batch(dev, 320, H, n)
    # a handle without a table: every element is -1
    render_checked(batch, poses, lights, want_prim=False)
    for td in (False, True):
        same(batch.read_thing_plane(top_down=td), np.full((n, H, 320), -1, np.int32), 'no table (top_down=%s)' % td)
    dev.set_decor_things(table)
    check_batch(batch, want, poses, lights, 'hand-made level', stride_things=96)
    # hidden rows, random per pose: no hidden index appears, and the plane is the reference's on the twin level
    rows = np.random.default_rng(41).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(U)
    want_h = np.stack([fr.thing_plane(arrays, table, oracle_prims(hidden_ref.twin(arrays, hidden_ref.hidden_quads(rows[p], table)),
                                                                  poses[p:p + 1], lights, 320, H)[0]) for p in range(n)])
    for p in range(n):
        hidden = {int(t) for t in range(64) if (int(rows[p][t >> 5]) >> (t & 31)) & 1}
        assert not hidden & set(want_h[p][want_h[p] >= 0].tolist())
    assert (want_h != want).any()
    dev_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    batch.set_hidden_things(dev_rows)
    check_batch(batch, want_h, poses, lights, 'hand-made level, hidden rows', stride_things=96)
    batch.set_hidden_things(None)
    # close enough that one decor triangle owns an aligned 32 x 32 quadrant: the described-quadrant path
    fwd = np.array([-np.sin(yaw), -np.cos(yaw)])
    right = np.array([np.cos(yaw), -np.sin(yaw)])
    close = np.zeros(3, rd.POSE)
    for p, d in enumerate((1.1, 1.14, 1.16)):  # the grid stands 1.2 ahead; the eye before the middle of column 5, row 3
        eye = (pos[0] + d * fwd[0] + 0.045 * right[0], pos[1] - 0.25 + 0.09 * 3 + 0.035, pos[2] + d * fwd[1] + 0.045 * right[1])
        close[p] = rd.pose_look(eye, float(yaw), 0.0, 320, H, 0.0)
    cprims = oracle_prims(arrays, close, lights, 320, H)
    want_c = fr.thing_plane(arrays, table, cprims)
    blocks = cprims[:, :H // 32 * 32].reshape(3, H // 32, 32, 10, 32)
    whole = (blocks == blocks[:, :, :1, :, :1]).all(axis=(2, 4)) & (quad[np.where(blocks[:, :, 0, :, 0] != 0xFFFFFFFF, blocks[:, :, 0, :, 0], 0)] >= 0) \
        & (blocks[:, :, 0, :, 0] != 0xFFFFFFFF)
    print('quadrants won entirely by one decor triangle: %d' % int(whole.sum()))
    FOUND['whole'] = int(whole.sum())
    assert whole.sum() >= 8 and len(set(want_c[want_c >= 0].tolist())) >= 3
    check_batch(batch, want_c, close, lights, 'hand-made level, close', stride_things=96)


FOUND = {'whole': -1}


def errors_case():
    """the argument errors that need a device, the wrappers' refusals, and raw device pointers in place of tensors"""
    import ctypes
    _wad, built, _arrays, lights, eye, yaws = e1m1()
    w, h, n = 64, 40, 3
    poses = np.zeros(n, rd.POSE)
    for i in range(n):
        poses[i] = rd.pose_look(eye, yaws[0] + 0.1 * i, 0.0, w, h, 0.0)
    batch = rd.Batch(rd.DeviceLevel(built), w, h, n)

    def refused(word, fn, *args, **kw):
        CHECKS[0] += 1
        try:
            fn(*args, **kw)
        except rd.RdoomError as e:
            if e.status == -1 and word in str(e):
                return
            print('MISMATCH: refused with %r, expected %r' % (str(e), word))
        else:
            print('MISMATCH: not refused (%r)' % word)
        BAD[0] += 1

    refused('nothing rendered', batch.read_thing_plane, count=1)
    batch.render(poses, lights)
    for first, count in ((0, 4), (3, 1), (2, 2), (4, 0)):
        refused('range', batch.read_thing_plane, first=first, count=count)
    assert batch.read_thing_plane(first=3, count=0).shape == (0, h, w)
    host = np.zeros((n, h, w), np.int32)
    refused('device memory', batch.resolve_thing_plane, host.ctypes.data)
    px = torch.zeros((n, h, w), dtype=torch.int32, device='cuda')
    refused('aligned', batch.resolve_thing_plane, px.data_ptr() + 2, count=1)
    L = rd.lib()
    v = ctypes.c_void_p
    assert L.rdoom_batch_resolve_thing_plane(batch._h, 0, 1, 0, None, None) == -1
    assert L.rdoom_batch_resolve_thing_plane(batch._h, 0, 1, 1, v(px.data_ptr()), None) == -1 and 'flag' in L.rdoom_last_error().decode()
    assert L.rdoom_batch_resolve_plane(batch._h, 0, 1, 4, v(px.data_ptr()), None) == -1  # the plane family keeps refusing 4
    on_host, wrong_type = torch.zeros((n, h, w), dtype=torch.int32), torch.zeros((n, h, w), dtype=torch.float32, device='cuda')
    wrong_size = torch.zeros((n, h, w + 1), dtype=torch.int32, device='cuda')
    strided = wrong_size[..., :w]
    for fn, tensors in ((batch.resolve_thing_plane, (on_host, wrong_type, wrong_size, strided)),
                        (lambda t: rd.frame_things(t, max_things=8), (on_host, wrong_type, strided))):  # (a plane of any width reduces)
        for bad in tensors:
            CHECKS[0] += 1
            try:
                fn(bad)
            except ValueError:
                continue
            print('MISMATCH: a tensor that does not fit was taken')
            BAD[0] += 1
    # nothing of that leaks: the plane by tensor, by raw pointer and by the synchronous read agree, and so does the reduction
    want = batch.read_thing_plane(top_down=True)
    batch.resolve_thing_plane(px, top_down=True)
    raw = torch.full((n, h, w), 9, dtype=torch.int32, device='cuda')
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    batch.resolve_thing_plane(raw.data_ptr(), top_down=True, stream=s.cuda_stream)
    table = torch.zeros((n, 64, 6), dtype=torch.int32, device='cuda')
    bits = torch.zeros((n, 2), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    rd.frame_things(raw.data_ptr(), None, max_things=64, min_pixels=1, table_out=table.data_ptr(), bits_out=bits.data_ptr(), stream=s.cuda_stream,
                    shape=(n, h, w))
    s.synchronize()
    batch.finish()
    same(px.cpu().numpy(), want, 'by tensor')
    same(raw.cpu().numpy(), want, 'by raw pointer')
    want_t, want_b = fr.reduce(want, None, 64, 1, 2)
    same(table.cpu().numpy(), fr.as_words(want_t), 'raw pointers: table')
    same(bits.cpu().numpy().view(U), want_b, 'raw pointers: bits')
    assert (want >= 0).any()


def lift_case():
    """E1M2's one thing stands on object 1.  The synthetic E1M2 has no trigger that starts it, so after a step_game tick the
    offsets of object 1 are written as a lift in motion would leave them, a height per player, and render_players draws the
    players from device state with those offsets; expected: the oracle's winners under the object modelviews"""
    import importlib
    import frames_ref
    tg = importlib.import_module('test_gpu_hidden_things')
    lv = tg.level(1)
    assert lv['table'].tolist() == [0] and lv['things']['object_id'][0] == 1
    world = tg.wad().build_world(1)
    dev = rd.DeviceLevel(lv['built'])
    t = lv['things'][0]
    n, w, h = 4, 320, H
    st = rd.player_states(np.float32([[t['x'] + 0.9 * np.cos(a), t['base'] + 0.33, t['z'] + 0.9 * np.sin(a)] for a in (0.0, 1.0, 2.0, 3.0)]),
                          np.float32([np.arctan2(np.cos(a), np.sin(a)) for a in (0.0, 1.0, 2.0, 3.0)]), pitch=-0.5)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    game, offs = world.game_state(n)
    world.step_game(states, np.zeros((1, n), rd.PLAYER_INPUT), game, offs)
    torch.cuda.synchronize()
    lifts = torch.tensor([0.0, 0.1, 0.25, 0.4], dtype=torch.float32, device='cuda')
    offs[:, 1, 1] = lifts
    torch.cuda.synchronize()
    o = offs.cpu().numpy()
    host_states = states.cpu().numpy().view(rd.PLAYER_STATE).copy().reshape(-1)
    poses, mvs = frames_ref.cameras(host_states, w, h, 0.0, o)
    poses, mvs = poses.reshape(-1), mvs[:, :dev.num_objects()]
    prims = oracle_prims(lv['arrays'], poses, lv['lights'], w, h, om=mvs)
    want = fr.thing_plane(lv['arrays'], lv['table'], prims)
    at_rest = frames_ref.cameras(host_states, w, h, 0.0, o * 0)[1][:, :dev.num_objects()]
    rest = fr.thing_plane(lv['arrays'], lv['table'], oracle_prims(lv['arrays'], poses, lv['lights'], w, h, om=at_rest))
    assert all((want[p] == 0).any() for p in range(n)) and (want[1:] != rest[1:]).any()  # the thing shows, and where the lift put it
    batch = rd.Batch(dev, w, h, n)
    for ids in (False, True):
        if ids:
            batch.enable_primitive_ids()
        batch.render(np.roll(poses, 1), lv['lights'])  # a dirtying render of other poses
        batch.render_players(states, lv['lights'], offsets=offs, time=0.0)
        for td in (False, True):
            same(batch.read_thing_plane(top_down=td), want[:, ::-1] if td else want, 'lift (ids=%s, top_down=%s)' % (ids, td))


def tick_case():
    """4 players for 3 ticks: step_game, sense_things(collect=...), render_players with the collected rows hidden, resolve_depth,
    resolve_thing_plane and frame_things on one side stream with no host wait; each tick's table against the reference afterwards"""
    import importlib
    import frames_ref
    import planes_ref
    tg = importlib.import_module('test_gpu_hidden_things')
    lv = tg.level(0)
    things = lv['things']
    candle = 17
    assert things['thing_type'][candle] == 34 and (things['category'][candle] & 0xFF) == rd.THING_AMMO
    t = things[candle]
    n, ticks, settle, w, h = 4, 3, 30, 160, 100
    st = rd.player_states(np.repeat(np.float32([[t['x'], t['base'] + 0.33, t['z'] + 0.8]]), n, 0), np.float32([0.0, 0.1, -0.1, 0.2]), pitch=-0.9)
    inp = np.zeros((settle + ticks, n), rd.PLAYER_INPUT)
    inp['movement'][settle:, :, 1] = -1.0
    world = tg.wad().build_world(0)
    dev_things = rd.DeviceThings(things)
    words = dev_things.words()
    max_things = 32 * words
    batch = rd.Batch(rd.DeviceLevel(lv['built']), w, h, n)
    game, offs = world.game_state(n)
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    ti = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).cuda()
    lights = torch.from_numpy(lv['lights'].copy()).cuda()
    start_rows = np.zeros((n, words), U)
    start_rows[1] = hidden_ref.row_of([candle], words)  # player 1 took the candle before: its frames never show it
    collected = torch.from_numpy(start_rows.view(np.int32).copy()).cuda()
    batch.set_hidden_things(collected)
    thing_px = torch.zeros((n, h, w), dtype=torch.int32, device='cuda')
    depth = torch.zeros((n, h, w), dtype=torch.float32, device='cuda')
    keep_table = torch.zeros((ticks, n, max_things, 6), dtype=torch.int32, device='cuda')
    keep_bits = torch.zeros((ticks, n, words), dtype=torch.int32, device='cuda')
    keep_rows = torch.zeros((ticks, n, words), dtype=torch.int32, device='cuda')
    keep_states = torch.zeros((ticks, states.numel()), dtype=torch.uint8, device='cuda')
    step = n * rd.PLAYER_INPUT.itemsize
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        world.step_game(states, ti[:settle * step], game, offs, n_ticks=settle, stream=stream)
        for k in range(ticks):
            at = (settle + k) * step
            world.step_game(states, ti[at:at + step], game, offs, n_ticks=1, stream=stream)
            world.sense_things(states, dev_things, max_range=10.0, touch_below=1.0, touch_above=1.0, collect=(rd.THING_AMMO,), offsets=offs,
                               collected=collected, stream=stream)
            batch.render_players(states, lights, offsets=offs, stream=stream)
            batch.resolve_depth(depth, top_down=True, stream=stream)
            batch.resolve_thing_plane(thing_px, top_down=True, stream=stream)
            rd.frame_things(thing_px, depth, max_things=max_things, min_pixels=12, table_out=keep_table[k], bits_out=keep_bits[k], stream=stream)
            keep_rows[k].copy_(collected)
            keep_states[k].copy_(states)
    stream.synchronize()
    batch.finish()
    assert not offs.cpu().numpy().any()  # nothing moved: the oracle's depth takes no object matrices
    rows = keep_rows.cpu().numpy().view(U)
    seen = 0
    for k in range(ticks):
        hs = keep_states[k].cpu().numpy().view(rd.PLAYER_STATE).copy().reshape(-1)
        poses, _ = frames_ref.cameras(hs, w, h, 0.0, None)
        poses = poses.reshape(-1)
        ids, dep = [], []
        for p in range(n):
            tw = hidden_ref.twin(lv['arrays'], hidden_ref.hidden_quads(rows[k, p], lv['table']))
            e = planes_ref.expected_planes(raster.RasterOracle(tw), tw, poses[p], lv['lights'], w, h)
            ids.append(fr.thing_plane(tw, lv['table'], e['primitive'])[::-1]), dep.append(e['depth'][::-1])
        want_t, want_b = fr.reduce(np.stack(ids), np.stack(dep), max_things, 12, words)
        same(keep_table[k].cpu().numpy(), fr.as_words(want_t), 'tick %d: table' % k)
        same(keep_bits[k].cpu().numpy().view(U), want_b, 'tick %d: bits' % k)
        seen += int(want_t['count'][0, candle] > 0)
        assert want_t['count'][1, candle] == 0
    assert seen, 'player 0 never has the candle in its frame'


def synthetic_case():
    rng = np.random.default_rng(5)
    widths, heights, things = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 321), (1, 2, 33), (1, 31, 32, 33, 65)
    k = 0
    for w in widths:
        for h in heights:
            n, max_things = 1 + k % 3, things[k % 5]
            k += 1
            ids = torch.from_numpy(rng.integers(-2, max_things + 3, (n, h, w)).astype(np.int32)).cuda()
            depth = torch.from_numpy(fr.synthetic_depth(rng, (n, h, w))).cuda()
            words = (max_things + 31) // 32
            for d in (None, depth):
                for min_pixels, stride in ((1, words), (2, words + 2), (64001, words)):
                    check_reduce(ids, d, max_things, min_pixels, stride, 'synthetic %d x %d x %d, %d things, min %d, stride %d, depth %s'
                                 % (n, h, w, max_things, min_pixels, stride, d is not None))
    for max_things in things:  # every max_things at a width with a tail, sparse ids as a frame has them
        ids_h = np.full((2, 33, 65), -1, np.int32)
        sel = rng.random(ids_h.shape) < 0.05
        ids_h[sel] = rng.integers(-2, max_things + 3, int(sel.sum()))
        check_reduce(torch.from_numpy(ids_h).cuda(), None, max_things, 1, None, 'sparse, %d things' % max_things)
    # one id throughout a 320 x 200 frame: the contention case
    one = torch.full((1, 200, 320), 3, dtype=torch.int32, device='cuda')
    depth = torch.from_numpy(fr.synthetic_depth(rng, (1, 200, 320))).cuda()
    for min_pixels in (1, 64000, 64001):
        t = check_reduce(one, depth, 33, min_pixels, 2, 'one id throughout, min %d' % min_pixels)
        assert t[0, 3]['count'] == 64000 and (t[0, 3]['x0'], t[0, 3]['y0'], t[0, 3]['x1'], t[0, 3]['y1']) == (0, 0, 319, 199)
    # 200 distinct ids in 2 x 2 blocks: more ids in a band of rows than the table in LDS has slots
    blocks = np.arange(200, dtype=np.int32).reshape(10, 20)
    many = torch.from_numpy(np.repeat(np.repeat(blocks, 2, 0), 2, 1)[None].copy()).cuda()
    t = check_reduce(many, torch.from_numpy(fr.synthetic_depth(rng, (1, 20, 40))).cuda(), 200, 4, 7, '200 ids in 2 x 2 blocks')
    assert (t['count'] == 4).all()
    t = check_reduce(many, None, 65, 5, 3, '200 ids in 2 x 2 blocks, 65 records')
    # ids far out of range on every side
    wild = torch.from_numpy(np.array([[[-2 ** 31, 2 ** 31 - 1, 1 << 20, 0, -1, 5, 4, 2 ** 30]]], np.int32)).cuda()
    check_reduce(wild, None, 5, 1, 1, 'ids far out of range')


def graph_case():
    rng = np.random.default_rng(9)
    n, h, w, max_things = 2, 33, 65, 33
    ids = torch.from_numpy(rng.integers(-2, max_things + 3, (n, h, w)).astype(np.int32)).cuda()
    depth = torch.from_numpy(fr.synthetic_depth(rng, (n, h, w))).cuda()
    table = torch.zeros((n, max_things, 6), dtype=torch.int32, device='cuda')
    bits = torch.zeros((n, 2), dtype=torch.int32, device='cuda')
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # three launches in one linear chain on one stream
            rd.frame_things(ids, depth, max_things=max_things, min_pixels=3, table_out=table, bits_out=bits, stream=s)
    for k in range(2):
        if k:
            ids.copy_(torch.from_numpy(rng.integers(-2, max_things + 3, (n, h, w)).astype(np.int32)).cuda())
        table.fill_(0x11111111), bits.fill_(0x22222222)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_t, want_b = fr.reduce(ids.cpu().numpy(), depth.cpu().numpy(), max_things, 3, 2)
        same(table.cpu().numpy(), fr.as_words(want_t), 'graph replay %d: table' % k)
        same(bits.cpu().numpy().view(U), want_b, 'graph replay %d: bits' % k)


if __name__ == '__main__':
    rd.set_device(0)
    {'hooks': hooks_case, 'levels': levels_case, 'handmade': handmade_case, 'synthetic': synthetic_case, 'graph': graph_case,
     'lift': lift_case, 'tick': tick_case, 'errors': errors_case}[sys.argv[1]]()
    print('RESULT bad=%d checks=%d whole=%d' % (BAD[0], CHECKS[0], FOUND['whole']))
    sys.exit(0 if BAD[0] == 0 else 1)
