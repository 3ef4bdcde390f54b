"""Child process of tests/test_gpu_lights.py: one case per process, so that each GPU step runs under the parent's time limit and a
fault ends that case alone.  Prints what it measured and exits 0 when every assertion of the case held.

  tables     DeviceLights.tables against the restatement (tests/lights_ref.py) and, by the sinf rule, against the host
  one_time   the clocked render with every clock at t == render_players(time=t, lights=tables(t)), bit for bit
  many_times 8 clocks in one render == 8 unclocked renders, and the frames do change with the clock
  oracle     players at distinct times against the oracle's rasteriser with the oracle's fill_buffer_at(time)
  loop       a clocked closed loop on a side stream without a host wait == the same loop synchronised; a captured graph
  errors     the argument checks return RDOOM_BAD_ARG and queue nothing"""
import ctypes
import importlib
import sys
import tempfile

import numpy as np

import conftest  # noqa: F401  (sys.path)
import frames_ref
import lights_ref
import rust_doom_amd as rd
import worldset_ref
from test_game_host import patched_variant
from test_gpu_game import _script, _setup
from test_gpu_worldset import SET, _players
from util import META_PATH, ensure_big_wad, ensure_wad

import torch

synthetic = importlib.import_module('rust-doom_amd.synthetic')
F = np.float32
TIMES8 = np.array([0.0, 0.31, 0.75, 1.7, 2.5, 7.3, 12.5, 100.25], F)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def all_levels():
    out = [rd.Wad(ensure_wad(), META_PATH).build_level(i) for i in range(9)]
    out.append(rd.Wad(ensure_big_wad(), META_PATH).build_level(0))
    out.append(rd.Wad(synthetic.ensure_rich_wad(), META_PATH).build_level(0))
    return out


class Census:
    """entries compared, and entries left out because the binary64 sine lies within 2^-48 of a binary32 midpoint"""

    def __init__(self):
        self.compared, self.excluded = 0, 0

    def same(self, infos, times, got, what):
        want = lights_ref.tables(infos, times)
        near = np.zeros(got.shape, bool)
        args = lights_ref.random_args(infos, times)
        near[:, :args.shape[1]] = lights_ref.near_midpoint(np.nan_to_num(args)) & ~np.isnan(args)
        self.compared += int(len(infos)) * len(times)
        self.excluded += int(near.sum())
        bad = (got != want) & ~near
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist())
        return want


def tables_case():
    census = Census()
    rng = np.random.default_rng(15)
    built = all_levels()
    host_diff = 0
    for i, b in enumerate(built):
        infos = b.light_infos()
        times = rng.uniform(0.0, 3600.0, 4096).astype(F)
        times[:4] = (0.0, 0.75, 99999.0, 123456.79)
        got = rd.DeviceLights([b]).tables(dev(times)).cpu().numpy()
        census.same(infos, times, got, 'level %d' % i)
        assert not got[:, len(infos):].any()
        host = np.stack([b.lights_at(float(t)) for t in times])
        n_diff, bad = lights_ref.explained(infos, times, host, got)
        assert not bad, ('host, level %d' % i, bad[:8])
        host_diff += n_diff
    print('device tables differ from the host in %d bytes, each a Random entry where sinf is not the correctly rounded sine' % host_diff)
    # a three-level set: grouped by level, then shuffled
    three = [built[0], built[4], built[8]]
    dl = rd.DeviceLights(three)
    n = 4096 + 77
    times = rng.uniform(0.0, 3600.0, n).astype(F)
    for name, lv in (('grouped', np.sort(rng.integers(0, 3, n))), ('shuffled', rng.integers(0, 3, n))):
        got = dl.tables(dev(times), levels=dev(lv.astype(np.int32))).cpu().numpy()
        for s in range(3):
            census.same(three[s].light_infos(), times[lv == s], got[lv == s], '%s, slot %d' % (name, s))
    # the hand-written table, the degenerate Glow, arrays instead of levels, an empty level
    hw, dg = lights_ref.handwritten_infos(), lights_ref.degenerate_glow()
    dl2 = rd.DeviceLights([hw, dg, np.zeros(0, rd.LIGHT_INFO)])
    times = np.concatenate([lights_ref.host_times(), rng.uniform(0.0, 3600.0, 4000).astype(F)])
    for s, infos in enumerate((hw, dg, np.zeros(0, rd.LIGHT_INFO))):
        got = dl2.tables(dev(times), levels=torch.full((len(times),), s, dtype=torch.int32, device='cuda')).cpu().numpy()
        census.same(infos, times, got, 'table %d' % s)
        if s:
            assert not got.any()  # Rust's NaN as u8; no infos at all
    # n = 1, levels=None, a caller's out tensor
    one = dl.tables(dev(np.array([1.7], F)))
    assert one.shape == (1, 256)
    census.same(three[0].light_infos(), np.array([1.7], F), one.cpu().numpy(), 'n = 1')
    # a slot outside the set: a row of zeros, the neighbours intact, nothing else written
    n = 77
    times = rng.uniform(0.0, 100.0, n).astype(F)
    lv = rng.integers(0, 3, n).astype(np.int64)
    lv[[0, 13, 76]] = (3, 0xFFFFFFFF, 1000)
    out = torch.full((n + 1, 256), 0xAB, dtype=torch.uint8, device='cuda')
    res = dl.tables(dev(times), levels=dev(lv.astype(np.uint32).view(np.int32)), out=out[:n])
    assert res.data_ptr() == out.data_ptr()
    got = out.cpu().numpy()
    assert (got[n] == 0xAB).all()
    for p in range(n):
        if p in (0, 13, 76):
            assert not got[p].any(), p
        else:
            census.same(three[lv[p]].light_infos(), times[p:p + 1], got[p:p + 1], 'player %d' % p)
    print('entries compared: %d, excluded as too near a midpoint: %d' % (census.compared, census.excluded))
    assert census.compared > 10 ** 6 and census.excluded * 10 ** 6 < census.compared


def e1m1_with_doors(n, seed, ticks=200):
    """players in front of the patched E1M1's triggers, stepped with pushes: (built, world, level, states, offsets)"""
    d = tempfile.mkdtemp(prefix='lights_patched_')
    wad_path, meta_path = patched_variant(d)
    wad, world, ref, t, st, _ = _setup(wad_path, meta_path, n, seed)
    st = st[:len(st) - len(st) % 8]
    assert len(st) >= 8
    n = len(st)
    inp, act = _script(n, ticks, seed + 1, push=0.1)
    game, offs = world.game_state(n)
    states = dev(st.view(np.uint8).copy())
    world.step_game(states, inp, game, offs, actions=act)
    torch.cuda.synchronize()
    assert (offs.cpu().numpy() != 0).any()
    built = wad.build_level(0)
    return built, world, rd.DeviceLevel(built), states, offs, game


def exit_set(n, seed, ticks=300):
    exits = worldset_ref.exit_variant(tempfile.mkdtemp(prefix='lights_exits_'))
    ws, st, lv, inp, act = _players(exits, n, seed)
    game, offs, levels = ws.game_state(lv)
    states = dev(st.view(np.uint8).copy())
    ws.step_game(states, inp[:ticks], game, offs, levels, actions=act[:ticks])
    torch.cuda.synchronize()
    wad = rd.Wad(exits[0], exits[1])
    built = [wad.build_level(i) for i in SET]
    return built, ws, rd.DeviceLevelSet(built), states, offs, levels, game, (inp, act)


def render_both(level, n, w, h, clocked_kw, plain_kw):
    """(frames, primitive ids, poses) of a clocked and an unclocked render on fresh batches with primitive ids"""
    out = []
    for kw in (clocked_kw, plain_kw):
        b = rd.Batch(level, w, h, n)
        b.enable_primitive_ids()
        poses = torch.zeros((n, rd.POSE.itemsize // 4), dtype=torch.float32, device='cuda')
        b.render_players(poses_out=poses, **kw)
        b.finish()
        out.append((b.read_framebuffer(), b.read_primitive_ids(), poses.cpu().numpy().view(np.uint32)))
    return out


def one_time_case():
    w, h = 160, 100
    built, world, level, states, offs, _ = e1m1_with_doors(256, 21)
    n = states.numel() // rd.PLAYER_STATE.itemsize
    dl = rd.DeviceLights([built])
    for t in (0.0, 0.75, 7.3):
        times = torch.full((n,), t, dtype=torch.float32, device='cuda')
        table = dl.tables(times[:1])[0].contiguous()
        (cf, cp, cposes), (pf, pp, pposes) = render_both(
            level, n, w, h, dict(states=states, lights=dl, offsets=offs, times=times),
            dict(states=states, lights=table, offsets=offs, time=t))
        assert np.array_equal(cf, pf) and np.array_equal(cp, pp) and np.array_equal(cposes, pposes), t
        assert (cf != 0).mean() > 0.3
    built3, ws, lset, states, offs, levels, _, _ = exit_set(512, 23)
    n = 512
    assert len(set(levels.cpu().numpy().tolist())) == 3 and (offs.cpu().numpy() != 0).any()
    dl3 = rd.DeviceLights(built3)
    t = 12.5
    times = torch.full((n,), t, dtype=torch.float32, device='cuda')
    table = dl3.tables(times[:3], levels=torch.arange(3, dtype=torch.int32, device='cuda')).contiguous()
    (cf, cp, cposes), (pf, pp, pposes) = render_both(
        lset, n, w, h, dict(states=states, lights=dl3, levels=levels, offsets=offs, times=times),
        dict(states=states, lights=table, levels=levels, offsets=offs, time=t))
    assert np.array_equal(cf, pf) and np.array_equal(cp, pp) and np.array_equal(cposes, pposes)
    # the cameras alone, per player
    times = dev(np.resize(TIMES8, n))
    poses, mvs = rd.poses_from_players_device(states, w, h, offsets=offs, times=times)
    p0, m0 = rd.poses_from_players_device(states, w, h, 0.0, offsets=offs)
    got, base = poses.cpu().numpy().view(rd.POSE).reshape(-1), p0.cpu().numpy().view(rd.POSE).reshape(-1)
    assert np.array_equal(got['time'], np.resize(TIMES8, n)) and torch.equal(mvs, m0)
    assert np.array_equal(got['modelview'], base['modelview']) and np.array_equal(got['projection'], base['projection'])
    print('clocked == unclocked at one time: E1M1 with moved doors (%d players, 3 times), a three-level set (%d players)'
          % (states.numel() // 40, n))


def many_times_case():
    w, h = 160, 100
    built, world, level, states, offs, _ = e1m1_with_doors(64, 31)
    st = states.cpu().numpy().view(rd.PLAYER_STATE).reshape(-1)[:8]
    o = offs.cpu().numpy()[:8]
    n = 64  # player p: state p % 8 at time TIMES8[p // 8]
    states = dev(np.tile(st, 8).view(np.uint8).copy())
    offs = dev(np.tile(o, (8, 1, 1)))
    times = dev(np.repeat(TIMES8, 8))
    dl = rd.DeviceLights([built])
    b = rd.Batch(level, w, h, n)
    b.render_players(states, dl, offsets=offs, times=times)
    got = b.read_framebuffer()
    plain = rd.Batch(level, w, h, 8)
    for k, t in enumerate(TIMES8):
        table = dl.tables(dev(np.array([t], F)))[0].contiguous()
        plain.render_players(states[:8 * 40], table, offsets=offs[:8], time=float(t))
        assert np.array_equal(plain.read_framebuffer(), got[8 * k:8 * k + 8]), t
    by_time = got.reshape(8, 8, h, w)
    differing = sum(not np.array_equal(by_time[a, s], by_time[c, s]) for s in range(8) for a in range(8) for c in range(a))
    tables = dl.tables(dev(TIMES8)).cpu().numpy()
    print('(state, time pair) frames that differ: %d of %d; distinct light tables among the 8 times: %d'
          % (differing, 8 * 28, len({t.tobytes() for t in tables})))
    assert differing > 0 and len({t.tobytes() for t in tables}) > 1


def oracle_case():
    from oracle import raster, wad_oracle
    w, h = 160, 100
    built, world, level, states, offs, _ = e1m1_with_doors(64, 41)
    n = 16
    states, offs = states[:n * 40].contiguous(), offs[:n].contiguous()
    tvals = np.concatenate([TIMES8, np.array([0.5, 1.0, 3.3, 5.75, 9.9, 20.2, 33.3, 61.0], F)])
    times = dev(tvals)
    dl = rd.DeviceLights([built])
    poses_t = torch.zeros((n, rd.POSE.itemsize // 4), dtype=torch.float32, device='cuda')
    mvs_t = torch.zeros((n, offs.shape[1], 16), dtype=torch.float32, device='cuda')
    b = rd.Batch(level, w, h, n)
    b.render_players(states, dl, offsets=offs, times=times, poses_out=poses_t, modelviews_out=mvs_t)
    fb = b.read_framebuffer()
    poses, mvs = poses_t.cpu().numpy().view(rd.POSE).reshape(-1), mvs_t.cpu().numpy()
    tables = dl.tables(times).cpu().numpy()
    lv = wad_oracle.build_level(*patched_variant(tempfile.mkdtemp(prefix='lights_oracle_')), 0)
    ro = raster.RasterOracle(built.arrays())
    n_obj = level.num_objects()
    h0, c0 = frames_ref.sky_angles(poses['projection'][0], poses['modelview'])
    h1, c1 = frames_ref.sky_angles(poses['projection'][0], mvs[:, :n_obj])
    exact = (h0 == c0) & (h1 == c1).all(1)
    checked = 0
    for p in range(n):
        want_lights = lv.lights.fill_buffer_at(float(tvals[p]))
        if not exact[p] or not np.array_equal(want_lights, tables[p]):
            # section 12's rule: such a player is not held to the oracle bit for bit; each one is named with its reason
            why = []
            if not exact[p]:
                why.append('a sky angle from libm atan2f is not the correctly rounded one')
            if not np.array_equal(want_lights, tables[p]):
                n_diff, bad = lights_ref.explained(built.light_infos(), tvals[p:p + 1], want_lights[None], tables[p:p + 1])
                assert not bad, (p, bad)
                why.append('%d Random light entries differ by the sinf rule' % n_diff)
            print('player %d (time %.2f) not compared: %s' % (p, float(tvals[p]), '; '.join(why)))
            continue
        want = ro.render(poses[p]['modelview'], poses[p]['projection'], float(tvals[p]), want_lights, w, h,
                         object_modelviews=mvs[p, :int(built.counters()['num_objects'])])
        assert np.array_equal(want, fb[p]), p
        checked += 1
    print('players bit-exact against the oracle at their own times: %d of %d' % (checked, n))
    assert checked >= n // 2


def loop_case():
    w, h, ticks, n = 160, 100, 40, 256
    dt = float(F(1.0 / 60.0))
    L = rd.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    results = []
    for synchronised in (False, True):
        built3, ws, lset, states, offs, levels, game, (inp, act) = exit_set(n, 51, ticks=60)
        dl = rd.DeviceLights(built3)
        ti = dev(inp[60:60 + ticks].view(np.uint8).reshape(-1).copy())
        ta = dev(act[60:60 + ticks].reshape(-1).copy())
        rng = np.random.default_rng(52)
        masks = dev(rng.random((ticks, n)) < 0.02)
        masks_u8 = masks.to(torch.uint8)
        times = dev(rng.uniform(0.0, 50.0, n).astype(F))
        batch = rd.Batch(lset, w, h, n)
        rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda')
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k in range(ticks):
            with torch.cuda.stream(stream):
                times += dt
                times.masked_fill_(masks[k], 0.0)
            # (the C entry point: WorldSet.reset_game waits for the stream before it lets go of a mask tensor)
            assert L.rdoom_worldset_game_reset(ws._h, vp(game), vp(offs), int(offs.shape[1]), vp(levels), n, vp(masks_u8[k]),
                                               ctypes.c_void_p(stream.cuda_stream)) == 0
            ws.step_game(states, ti[k * n * 20:(k + 1) * n * 20], game, offs, levels, actions=ta[k * n:(k + 1) * n], n_ticks=1, stream=stream)
            batch.render_players(states, dl, levels=levels, offsets=offs, times=times, stream=stream)
            batch.resolve_rgb(rgb, stream=stream)
            if synchronised:
                stream.synchronize()
                batch.finish()
        stream.synchronize()
        batch.finish()
        results.append((rgb.cpu().numpy(), times.cpu().numpy(), states.cpu().numpy()))
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    assert np.array_equal(results[0][0], results[1][0])
    assert (results[0][1] < 0.5).any() and (results[0][1] > 1.0).any()  # some clocks were reset on the way
    # the clocked render captured into a graph (it allocates nothing and waits for nothing), replayed at other times
    batch.render_players(states, dl, levels=levels, offsets=offs, times=times)
    want_a = batch.read_framebuffer()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch.render_players(states, dl, levels=levels, offsets=offs, times=times, stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    batch.finish()
    assert np.array_equal(batch.read_framebuffer(), want_a)
    times += 0.4
    g.replay()
    torch.cuda.synchronize()
    got_b = batch.read_framebuffer()
    fresh = rd.Batch(lset, w, h, n)
    fresh.render_players(states, dl, levels=levels, offsets=offs, times=times)
    assert np.array_equal(got_b, fresh.read_framebuffer())
    print('closed loop of %d ticks: asynchronous == synchronised; graph replay == direct render (frames changed by the clock: %s)'
          % (ticks, not np.array_equal(want_a, got_b)))


def errors_case():
    BAD = -1
    L = rd.lib()
    n, w, h = 16, 64, 40
    built3, ws, lset, states, offs, levels, _, _ = exit_set(n, 61, ticks=30)
    dl, dl1 = rd.DeviceLights(built3), rd.DeviceLights(built3[:1])
    times = torch.full((n,), 1.0, dtype=torch.float32, device='cuda')
    batch = rd.Batch(lset, w, h, n)
    batch.render_players(states, dl, levels=levels, offsets=offs, times=times)
    before = batch.read_framebuffer()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    n_obj = int(offs.shape[1])

    def call(b=batch._h, st=states, lv=levels, li=dl._h, tm=times, count=n, flags=0):
        return L.rdoom_batch_render_players_clocked(b, p(st), p(lv), p(offs), n_obj, li, p(tm), count, rd.ALL_KINDS, flags, None, None, None)
    for kw in (dict(li=None), dict(tm=None), dict(li=dl1._h), dict(b=None), dict(st=None), dict(lv=None), dict(count=0),
               dict(count=n + 1), dict(flags=2)):
        assert call(**kw) == BAD, kw
        assert L.rdoom_last_error()
    out = torch.full((n, 256), 0xAB, dtype=torch.uint8, device='cuda')
    assert L.rdoom_lightset_tables(dl._h, p(levels), None, n, p(out), None) == BAD
    assert L.rdoom_lightset_tables(dl._h, p(levels), p(times), n, None, None) == BAD
    assert L.rdoom_lightset_tables(None, p(levels), p(times), n, p(out), None) == BAD
    assert L.rdoom_lightset_tables(dl._h, p(levels), None, 0, None, None) == 0  # n == 0 queues nothing
    poses = torch.full((n, rd.POSE.itemsize // 4), -3.0, dtype=torch.float32, device='cuda')
    assert L.rdoom_poses_from_players_device_clocked(p(states), n, w, h, None, None, 0, p(poses), None, None) == BAD
    torch.cuda.synchronize()
    batch.finish()
    assert (out == 0xAB).all().item() and (poses == -3.0).all().item() and np.array_equal(batch.read_framebuffer(), before)
    # the light set's own checks
    h_ = ctypes.c_void_p()
    infos = np.zeros(256, rd.LIGHT_INFO)
    ptr = lambda a, k: ((ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_uint32 * 1)(k))
    assert L.rdoom_lightset_create(*ptr(infos, 256), 1, ctypes.byref(h_)) == BAD and not h_.value  # more than 255 infos
    assert L.rdoom_lightset_create(*ptr(infos, 255), 1, ctypes.byref(h_)) == 0 and h_.value
    L.rdoom_lightset_destroy(h_)
    for kind in (3, -1):
        infos[7]['has_effect'], infos[7]['effect_kind'] = 1, kind
        assert L.rdoom_lightset_create(*ptr(infos, 8), 1, ctypes.byref(h_)) == BAD and not h_.value
    assert L.rdoom_lightset_create(*ptr(infos, 7), 0, ctypes.byref(h_)) == BAD
    assert L.rdoom_lightset_create(None, None, 1, ctypes.byref(h_)) == BAD
    # the Python layer: times and a DeviceLights go together
    table = dl.tables(times[:3], levels=torch.arange(3, dtype=torch.int32, device='cuda'))
    for kw in (dict(lights=table, times=times), dict(lights=dl)):
        try:
            batch.render_players(states, levels=levels, offsets=offs, **kw)
        except ValueError:
            continue
        raise AssertionError('no ValueError for %r' % sorted(kw))
    batch.finish()
    assert np.array_equal(batch.read_framebuffer(), before)
    assert call() == 0
    batch.finish()
    print('every argument error is RDOOM_BAD_ARG / ValueError and queues nothing')


CASES = {'tables': tables_case, 'one_time': one_time_case, 'many_times': many_times_case, 'oracle': oracle_case, 'loop': loop_case,
         'errors': errors_case}

if __name__ == '__main__':
    rd.set_device(0)
    CASES[sys.argv[1]]()
    print('RESULT ok')
