"""Seen lines on the GPU (reveal.hip reveal_lines_kernel / worldset_reveal_lines_kernel, automap.hip's maps drawn through a set)
against the test-side restatement (tests/reveal_restatement.c, every ray against every line, twice): every word of every row, zero
tolerance.  E1M1, E1M8 and the big level with 256 players each, three fans, with and without per-player door offsets;
accumulation and the new-line count; a wide stride; a world set with slots out of range; a NaN position; streams, caller's
tensors and graph capture; every argument check of the header; the maps through seen, full and empty sets."""
import ctypes
import functools
import os

import numpy as np
import pytest

import automap_ref
import mapcheck
import rays_ref
import reveal_ref
import rust_doom_amd as rd
from util import META_PATH, ensure_big_wad, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
LEVELS = {'E1M1': (ensure_wad, 0, 101), 'E1M8': (ensure_wad, 7, 109), 'big': (ensure_big_wad, 0, 110)}  # (wad, index, seed)
PLAYERS = 256


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _rows(a):
    """a uint32 array as the int32 tensor reveal_lines takes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _fan(n_rays, fov):
    return torch.from_numpy(rd.map_fan(n_rays, fov)).cuda()


def _same(got, want, what):
    got = _u32(got) if not isinstance(got, np.ndarray) else got
    bad = got != want
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[bad][:8], want[bad][:8])


@functools.lru_cache(maxsize=None)
def inputs(level):
    """what the tests of one level share, computed once and left unchanged: the host table, 256 players at random floor
    centroids and yaws, random per-player object offsets, and the restatement's result for every fan with and without them"""
    ensure, index, seed = LEVELS[level]
    wad = rd.Wad(ensure(), META_PATH)
    host = wad.build_world(index, device=False)
    lines = host.map_lines()
    st = rays_ref.players(wad.build_level(index), seed, count=PLAYERS)
    off = reveal_ref.random_offsets(np.random.RandomState(seed), PLAYERS, host.game_objects)
    want = {(k, moved): reveal_ref.reveal(lines, st, rd.map_fan(rays, fov), rng, off if moved else None, detail=True)
            for k, (rays, fov, rng) in enumerate(reveal_ref.FANS) for moved in (False, True)}
    return dict(wad=wad, index=index, lines=lines, states=st, offsets=off, want=want)


def check_not_vacuous(level):
    """on the restatement's own result, before any comparison (runs on the CPU; the seeds of LEVELS were picked to meet it)"""
    d = inputs(level)
    n_lines = len(d['lines'])
    for (k, moved), w in d['want'].items():
        count = reveal_ref.popcount(w['seen'])
        assert np.array_equal(count, w['new'])
        assert (count >= 1).all() and (count < n_lines).all(), (level, k, moved)  # every player sees something, nobody everything
        assert (w['marks'] >= 2).any(), (level, k, moved)  # sight passes through an open two-sided line
        assert (w['stop'] == reveal_ref.STOP_ONE_SIDED).any() and (w['stop'] == reveal_ref.STOP_TWO_SIDED).any(), (level, k, moved)
    for moved in (False, True):  # rays that end in the open: of the short fans (E1M1 has no 40 units of open floor)
        assert all((d['want'][k, moved]['stop'] == reveal_ref.STOP_RANGE).any() for k in (0, 2)), (level, moved)
    for k in range(len(reveal_ref.FANS)):
        differs = (d['want'][k, False]['seen'] != d['want'][k, True]['seen']).any(1)
        assert differs.any() and not differs.all(), (level, k, int(differs.sum()))  # doors shut and open change some players' sets


@pytest.mark.parametrize('level', list(LEVELS))
def test_rows_and_counts_match_the_restatement(level):
    check_not_vacuous(level)
    rd.set_device(0)
    d = inputs(level)
    world = d['wad'].build_world(d['index'])
    words = world.seen_words()
    assert words == reveal_ref.words_of(len(d['lines']))
    states, offs = _dev(d['states']), torch.from_numpy(d['offsets']).cuda()
    for k, (rays, fov, rng) in enumerate(reveal_ref.FANS):
        for moved in (False, True):
            want = d['want'][k, moved]
            new = torch.full((PLAYERS,), 77, dtype=torch.int32, device='cuda')
            seen = world.reveal_lines(states, _fan(rays, fov), rng, offsets=offs if moved else None, new_out=new)
            assert seen.dtype == torch.int32 and tuple(seen.shape) == (PLAYERS, words)
            _same(seen, want['seen'], (level, k, moved))
            _same(new, want['new'], (level, k, moved, 'new'))


def test_a_second_pass_of_three_rays_that_look_backwards():
    """259 rays: the pass loop runs twice, and the second pass has 85 slices and a thread without one"""
    d = inputs('E1M1')
    n, fan, rng = reveal_ref.TAIL_PLAYERS, reveal_ref.tail_fan(), reveal_ref.TAIL_RANGE
    assert len(d['lines']) == 713 and fan.shape == (259, 2) and fan.dtype == F
    st = rays_ref.players(d['wad'].build_level(d['index']), LEVELS['E1M1'][2], count=n)
    off = reveal_ref.random_offsets(np.random.RandomState(LEVELS['E1M1'][2]), n, d['offsets'].shape[1])
    rd.set_device(0)
    world = d['wad'].build_world(d['index'])
    for o_np in (None, off):
        want = reveal_ref.reveal(d['lines'], st, fan, rng, o_np, detail=True)
        head = reveal_ref.reveal(d['lines'], st, fan[:256], rng, o_np)
        # on the restatement's own result: the tail pass sees lines of its own for every player, and every ray of it ends on a wall
        tail_only = (want['witness_ray'] >= 256) & (want['witness_ray'] != reveal_ref.NO_WITNESS)
        assert tail_only.any(1).all(), tail_only.sum(1)
        assert (want['seen'] != head['seen']).any(1).all() and (want['limit'][:, 256:] < 1).all()
        new = torch.full((n,), 77, dtype=torch.int32, device='cuda')
        seen = world.reveal_lines(_dev(st), torch.from_numpy(fan).cuda(), rng, offsets=None if o_np is None else torch.from_numpy(o_np).cuda(),
                                  new_out=new)
        _same(seen, want['seen'], ('tail', o_np is not None))
        _same(new, want['new'], ('tail', o_np is not None, 'new'))


def test_rows_accumulate_and_the_count_is_what_is_new():
    rd.set_device(0)
    d = inputs('E1M8')
    lines, n_lines = d['lines'], len(d['lines'])
    world = d['wad'].build_world(d['index'])
    rays, fov, rng = reveal_ref.FANS[0]
    fan = _fan(rays, fov)
    rs = np.random.RandomState(3)
    noise = (rs.randint(0, 1 << 32, d['want'][0, False]['seen'].shape, dtype=np.uint64).astype(np.uint32)
             & rs.randint(0, 1 << 32, d['want'][0, False]['seen'].shape, dtype=np.uint64).astype(np.uint32))  # a quarter of the bits
    tail = n_lines % 32
    if tail:
        noise[:, -1] &= np.uint32((1 << tail) - 1)
    before = d['want'][0, False]['seen'] | noise
    moved_states = rays_ref.players(d['wad'].build_level(d['index']), 999, count=PLAYERS)
    want = reveal_ref.reveal(lines, moved_states, rd.map_fan(rays, fov), rng, seen=before)
    fresh = reveal_ref.reveal(lines, moved_states, rd.map_fan(rays, fov), rng)
    assert np.array_equal(want['seen'], before | fresh['seen']) and np.array_equal(want['new'], reveal_ref.popcount(want['seen'] & ~before))
    assert (want['new'] > 0).sum() > PLAYERS // 2 and (want['new'] < fresh['new']).any()
    rows, new = _rows(before), torch.full((PLAYERS,), 77, dtype=torch.int32, device='cuda')
    assert world.reveal_lines(_dev(moved_states), fan, rng, seen=rows, new_out=new) is rows
    _same(rows, before | fresh['seen'], 'old OR restated')
    _same(new, reveal_ref.popcount(_u32(rows) & ~before), 'the count')
    world.reveal_lines(_dev(moved_states), fan, rng, seen=rows, new_out=new)  # a third, identical call finds nothing new
    _same(rows, want['seen'], 'third call')
    assert not new.any().item()


def test_padding_words_and_tail_bits_survive_a_wide_stride():
    rd.set_device(0)
    d = inputs('E1M1')
    n_lines = len(d['lines'])
    words = reveal_ref.words_of(n_lines)
    assert n_lines % 32 != 0
    tail = np.uint32(0xFFFFFFFF) << np.uint32(n_lines % 32)
    before = np.zeros((PLAYERS, words + 3), np.uint32)
    before[:, words:] = 0xDEADBEEF
    before[:, words - 1] = tail & np.uint32(0xA5A5A5A5)
    assert (before[:, words - 1] != 0).all()
    world = d['wad'].build_world(d['index'])
    rays, fov, rng = reveal_ref.FANS[1]
    rows = _rows(before)
    new = torch.zeros(PLAYERS, dtype=torch.int32, device='cuda')
    world.reveal_lines(_dev(d['states']), _fan(rays, fov), rng, seen=rows, new_out=new)
    got = _u32(rows)
    assert (got[:, words:] == 0xDEADBEEF).all() and np.array_equal(got[:, words - 1] & tail, before[:, words - 1])
    want = d['want'][1, False]
    _same(got[:, :words] & ~np.concatenate([np.zeros(words - 1, np.uint32), [tail]]), want['seen'], 'the rows')
    _same(new, want['new'], 'the counts')


def test_a_world_set_with_slots_out_of_range():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 7]
    ws = wad.build_world_set(slots)
    tables = [ws.map_lines(s) for s in range(3)]
    parts, lv = [], []
    for s, index in enumerate(slots):
        parts.append(rays_ref.players(wad.build_level(index), 60 + s, count=80))
        lv += [s] * 80
    rs = np.random.RandomState(9)
    order = rs.permutation(240)
    st, lv = np.concatenate(parts)[order], np.array(lv, np.uint32)[order]
    lv[::31] = 3 + (np.arange(len(lv[::31])) % 2) * 0x7FFFFFF0  # slots 3 and far beyond: out of the set
    outside = lv >= 3
    levels_t = torch.from_numpy(lv.view(np.int32).copy()).cuda()
    off = reveal_ref.random_offsets(rs, 240, ws.n_objects)
    words = ws.seen_words()
    assert words == max(reveal_ref.words_of(len(t)) for t in tables) and len({len(t) for t in tables}) == 3
    rays, fov, rng = reveal_ref.FANS[1]
    for o_np in (None, off):
        before = np.zeros((240, words), np.uint32)
        before[outside] = 0x5A5A5A5A
        want = reveal_ref.reveal(tables, st, rd.map_fan(rays, fov), rng, o_np, levels=lv, seen=before)
        assert (want['seen'][outside] == 0x5A5A5A5A).all() and not want['new'][outside].any() and (want['new'][~outside] > 0).all()
        rows, new = _rows(before), torch.full((240,), 77, dtype=torch.int32, device='cuda')
        ws.reveal_lines(_dev(st), levels_t, _fan(rays, fov), rng, offsets=None if o_np is None else torch.from_numpy(o_np).cuda(),
                        seen=rows, new_out=new)
        _same(rows, want['seen'], 'set rows')
        _same(new, want['new'], 'set counts')
    # a slot's players alone equal the single world's
    mine = lv == 2
    alone = wad.build_world(7).reveal_lines(_dev(st[mine]), _fan(rays, fov), rng)
    both = ws.reveal_lines(_dev(st), levels_t, _fan(rays, fov), rng)
    assert torch.equal(alone, both[torch.from_numpy(mine).cuda()][:, :alone.shape[1]])


def test_a_nan_position_marks_nothing():
    rd.set_device(0)
    d = inputs('E1M1')
    st = d['states'][:64].copy()
    st['pos'][5, 0] = np.nan
    st['pos'][6, 2] = np.nan
    st['yaw'][7] = np.nan
    world = d['wad'].build_world(d['index'])
    rays, fov, rng = reveal_ref.FANS[1]
    want = reveal_ref.reveal(d['lines'], st, rd.map_fan(rays, fov), rng)
    assert not want['seen'][5:8].any() and not want['new'][5:8].any() and (want['new'][:5] > 0).all()
    new = torch.full((64,), 77, dtype=torch.int32, device='cuda')
    seen = world.reveal_lines(_dev(st), _fan(rays, fov), rng, new_out=new)
    _same(seen, want['seen'], 'rows')
    _same(new, want['new'], 'counts')


def test_a_side_stream_the_callers_tensors_and_a_captured_graph():
    rd.set_device(0)
    d = inputs('E1M1')
    world = d['wad'].build_world(d['index'])
    rays, fov, rng = reveal_ref.FANS[0]
    want = d['want'][0, True]
    states, fan, offs = _dev(d['states']), _fan(rays, fov), torch.from_numpy(d['offsets']).cuda()
    rows = torch.zeros((PLAYERS, world.seen_words()), dtype=torch.int32, device='cuda')
    new = torch.full((PLAYERS,), 77, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert world.reveal_lines(states, fan, rng, offsets=offs, seen=rows, new_out=new, stream=side) is rows
    side.synchronize()
    _same(rows, want['seen'], 'side stream')
    _same(new, want['new'], 'side stream counts')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a call that waited or allocated could not be captured
        world.reveal_lines(states, fan, rng, offsets=offs, seen=rows, new_out=new, stream=torch.cuda.current_stream())
    rows.zero_()
    new.fill_(77)
    g.replay()
    torch.cuda.synchronize()
    _same(rows, want['seen'], 'graph replay')
    _same(new, want['new'], 'graph replay counts')
    g.replay()  # onto its own result: nothing new
    torch.cuda.synchronize()
    _same(rows, want['seen'], 'second replay')
    assert not new.any().item()


def test_argument_checks_queue_nothing():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(0), wad.build_world_set([0, 7])
    host_only, host_set = wad.build_world(0, device=False), wad.build_world_set([0, 7], device=False)
    n = 64
    states = _dev(rays_ref.players(wad.build_level(0), 6, count=n))
    lv = torch.zeros(n, dtype=torch.int32, device='cuda')
    fan = _fan(16, 1.0)
    words, set_words = world.seen_words(), ws.seen_words()
    rows = torch.full((n, set_words), 0x11111111, dtype=torch.int32, device='cuda')
    new = torch.full((n,), -1, dtype=torch.int32, device='cuda')  # no count is 2^32 - 1
    out = torch.full((n, 53, 77), 77, dtype=torch.uint8, device='cuda')
    small = torch.zeros((n, 1, 3), dtype=torch.float32, device='cuda')
    assert world.game_objects > 1 and ws.n_objects > 1 and set_words > words
    L = rd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    BAD = -1
    view = rd.MapView(77, 53, 0.12, 0.75, 3.0, 0)

    def one(h=world, st=states, k=n, dirs=fan, r=16, rng=10.0, off=None, no=0, seen=rows, stride=set_words, cnt=new):
        return L.rdoom_world_reveal_lines(h._h if h is not None else None, p(st), k, p(dirs), r, ctypes.c_float(rng), p(off), no, p(seen),
                                          stride, p(cnt), None)

    def many(h=ws, st=states, lv_=lv, k=n, dirs=fan, r=16, rng=10.0, off=None, no=0, seen=rows, stride=set_words, cnt=new):
        return L.rdoom_worldset_reveal_lines(h._h if h is not None else None, p(st), p(lv_), k, p(dirs), r, ctypes.c_float(rng), p(off), no,
                                             p(seen), stride, p(cnt), None)

    def draw_one(h=world, seen=rows, stride=set_words):
        return L.rdoom_world_draw_maps_seen(h._h if h is not None else None, p(states), n, None, 0, ctypes.byref(view), p(seen), stride, p(out), None)

    def draw_many(h=ws, seen=rows, stride=set_words, lv_=lv):
        return L.rdoom_worldset_draw_maps_seen(h._h if h is not None else None, p(states), p(lv_), n, None, 0, ctypes.byref(view), p(seen), stride,
                                               p(out), None)

    inf, nan = float('inf'), float('nan')
    for call, enough in ((one, words), (many, set_words)):
        for kw in [dict(h=None), dict(st=None), dict(seen=None), dict(dirs=None), dict(r=0), dict(rng=0.0), dict(rng=-3.0), dict(rng=inf),
                   dict(rng=nan), dict(stride=enough - 1), dict(stride=0), dict(off=small, no=1)]:
            assert call(**kw) == BAD, (call.__name__, list(kw))
            assert L.rdoom_last_error()
    assert many(lv_=None) == BAD and one(h=host_only) == BAD and many(h=host_set) == BAD
    assert draw_one(h=None) == BAD and draw_many(h=None) == BAD and draw_many(lv_=None) == BAD
    assert draw_one(stride=words - 1) == BAD and draw_many(stride=set_words - 1) == BAD
    assert draw_one(h=host_only) == BAD and draw_many(h=host_set) == BAD
    if rd.device_count() > 1:  # a handle that lives on another device
        rd.set_device(1)
        assert one() == BAD and many() == BAD and draw_one() == BAD and draw_many() == BAD
        rd.set_device(0)
    torch.cuda.synchronize()
    assert (rows == 0x11111111).all().item() and (new == -1).all().item() and (out == 77).all().item()  # nothing was queued
    assert one(k=0) == 0 and many(k=0) == 0 and one(k=0, st=None, seen=None, dirs=None) == 0
    torch.cuda.synchronize()
    assert (rows == 0x11111111).all().item() and (new == -1).all().item()
    assert one(stride=set_words) == 0 and many(cnt=None) == 0 and draw_one(seen=None, stride=0) == 0
    torch.cuda.synchronize()
    assert not (new == -1).any().item() and not (out == 77).any().item()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        world.reveal_lines(states.cpu(), fan, 10.0)
    with pytest.raises(ValueError):
        world.reveal_lines(states, torch.zeros((16, 3), device='cuda'), 10.0)
    with pytest.raises(ValueError):
        world.reveal_lines(states, fan, 10.0, seen=rows[:, :words - 1].contiguous())
    with pytest.raises(ValueError):
        world.reveal_lines(states, fan, 10.0, seen=rows.float())
    with pytest.raises(ValueError):
        world.reveal_lines(states, fan, 10.0, new_out=new[:5])
    with pytest.raises(ValueError):
        ws.reveal_lines(states, lv[:5], fan, 10.0)
    with pytest.raises(ValueError):
        world.draw_maps(states, 77, 53, 0.12, seen=rows[:5])
    with pytest.raises(rd.RdoomError):
        world.reveal_lines(states, fan, -1.0)


def _mapped_copy(directory):
    """a copy of the IWAD whose first level has flag 0x100 (already on the map) on every seventh linedef"""
    data, lumps = mapcheck.read_directory(ensure_wad())
    marker = mapcheck.level_markers(lumps)[0]
    _, pos, size = next(l for l in lumps[marker + 1:marker + 11] if l[0] == b'LINEDEFS')
    raw = np.frombuffer(data, np.uint8).copy()
    recs = raw[pos:pos + size].view('<u2').reshape(-1, 7)
    recs[::7, 2] |= rd.LINE_MAPPED
    path = os.path.join(directory, 'mapped.wad')
    with open(path, 'wb') as f:
        f.write(raw.tobytes())
    return path


DRAW_VIEWS = (automap_ref.VIEWS[1], automap_ref.VIEWS[2])  # one rotated (flat lines, a marker), one top_down (no marker)


def _draw(target, states, levels, kw, **more):
    extra = {k: v for k, v in kw.items() if k not in ('width', 'height', 'scale')}
    args = (states,) + ((levels,) if levels is not None else ()) + (kw['width'], kw['height'], kw['scale'])
    return target.draw_maps(*args, **extra, **more)


def test_maps_drawn_through_the_seen_set(tmp_path):
    """32 players of E1M1, on the IWAD as it is and on a copy with 0x100 on every seventh linedef: through the set a reveal left
    every byte is the restatement's map of the seen or flagged lines; through all-ones rows it is the plain map; through all-zero
    rows it shows the marker and the flagged lines only"""
    rd.set_device(0)
    rays, fov, rng = reveal_ref.FANS[0]
    for path, flagged in ((ensure_wad(), False), (_mapped_copy(str(tmp_path)), True)):
        wad = rd.Wad(path, META_PATH)
        world = wad.build_world(0)
        lines = world.map_lines()
        mapped = (lines['flags'] & rd.LINE_MAPPED) != 0
        assert mapped.any() == flagged
        st = rays_ref.players(wad.build_level(0), 21, count=32)
        off = reveal_ref.random_offsets(np.random.RandomState(21), 32, world.game_objects)
        states, offs = _dev(st), torch.from_numpy(off).cuda()
        seen = world.reveal_lines(states, _fan(rays, fov), rng, offsets=offs)
        seen_np = reveal_ref.reveal(lines, st, rd.map_fan(rays, fov), rng, off)['seen']
        _same(seen, seen_np, 'the set')
        ones, zeros = torch.full_like(seen, -1), torch.zeros_like(seen)
        for kw in DRAW_VIEWS:
            want = reveal_ref.draw_seen(lines, st, seen_np, off, **kw)
            full = automap_ref.draw(lines, st, off, **kw)
            assert ((want != full).reshape(32, -1).any(1)).sum() > 16 and (want <= full).all()  # the set hides lines, and only hides
            assert ((want >= rd.MAP_FLAT) & (want <= rd.MAP_ONE_SIDED)).reshape(32, -1).any(1).sum() > 16
            _same(_draw(world, states, None, kw, offsets=offs, seen=seen).cpu().numpy(), want, ('seen', flagged))
            plain = _draw(world, states, None, kw, offsets=offs)
            _same(plain.cpu().numpy(), full, ('plain', flagged))
            assert torch.equal(_draw(world, states, None, kw, offsets=offs, seen=ones), plain)
            empty = _draw(world, states, None, kw, offsets=offs, seen=zeros).cpu().numpy()
            _same(empty, reveal_ref.draw_seen(lines, st, np.zeros_like(seen_np), off, **kw), ('empty', flagged))
            codes = set(np.unique(empty).tolist())
            if flagged:
                assert codes - {rd.MAP_NONE, rd.MAP_PLAYER}, codes
            else:
                assert codes == ({rd.MAP_NONE, rd.MAP_PLAYER} if kw.get('marker', 3.0) > 0 else {rd.MAP_NONE}), codes


def test_world_set_maps_drawn_through_the_seen_set():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 7]
    ws = wad.build_world_set(slots)
    tables = [ws.map_lines(s) for s in range(3)]
    lv = np.array([0, 1, 2, 2, 1, 0, 3, 2] * 4, np.uint32)
    st = np.concatenate([rays_ref.players(wad.build_level(slots[min(int(s), 2)]), 300 + k, count=1) for k, s in enumerate(lv)])
    levels_t = torch.from_numpy(lv.view(np.int32).copy()).cuda()
    rays, fov, rng = reveal_ref.FANS[1]
    states = _dev(st)
    seen = ws.reveal_lines(states, levels_t, _fan(rays, fov), rng)
    seen_np = reveal_ref.reveal(tables, st, rd.map_fan(rays, fov), rng, levels=lv)['seen']
    _same(seen, seen_np, 'the set')
    for kw in DRAW_VIEWS:
        want = reveal_ref.draw_seen(tables, st, seen_np, levels=lv, **kw)
        assert (want[lv >= 3] == 0).all() and (want[lv < 3] != 0).reshape((lv < 3).sum(), -1).any(1).all()
        _same(_draw(ws, states, levels_t, kw, seen=seen).cpu().numpy(), want, 'seen')
        assert torch.equal(_draw(ws, states, levels_t, kw, seen=torch.full_like(seen, -1)), _draw(ws, states, levels_t, kw))
