"""The explored area on the GPU (area.hip reveal_area_kernel / worldset_reveal_area_kernel and the two draw kernels) against the
test-side restatement (tests/area_restatement.c: every ray against every line, every sample into byte-per-cell planes of the whole
grid): every word of every row and every byte of every map, zero tolerance.  E1M2 (one room of nine lines) and E1M1 with 64 players
each; a window that fits LDS, windows taken in two and in four bands, more than 256 samples a ray, a single ray; with and without
per-player door offsets; accumulation and the counts; a wide stride; a world set with slots out of range; NaNs; streams, caller's
tensors and graph capture; every argument check of the header; the maps against the restatement and against draw_maps."""
import ctypes
import functools

import numpy as np
import pytest

import area_ref
import rays_ref
import reveal_ref
import rust_doom_amd as rd
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
LEVELS = {'E1M2': (1, 102), 'E1M1': (0, 101)}  # (index, seed); E1M1's seed is tests/test_gpu_reveal.py's
PLAYERS = 64
BAND_CASES = (1, 2)  # of area_ref.CASES: on E1M1 their windows exceed the LDS window


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _rows(a):
    """a uint32 array as the int32 tensor reveal_area takes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _fan(n_rays, fov):
    return torch.from_numpy(rd.map_fan(n_rays, fov)).cuda()


def _same(got, want, what):
    got = _u32(got) if not isinstance(got, np.ndarray) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[bad][:8], want[bad][:8])


@functools.lru_cache(maxsize=None)
def wad():
    return rd.Wad(ensure_wad(), META_PATH)


@functools.lru_cache(maxsize=None)
def inputs(level):
    """what the tests of one level share, computed once and left unchanged: the host table, 64 players at random floor centroids
    and yaws, random per-player object offsets, and the restatement's result for every case with and without them"""
    index, seed = LEVELS[level]
    host = wad().build_world(index, device=False)
    lines = host.map_lines()
    st = rays_ref.players(wad().build_level(index), seed, count=PLAYERS)
    off = reveal_ref.random_offsets(np.random.RandomState(seed), PLAYERS, host.game_objects)
    want = {(k, moved): area_ref.reveal(lines, st, rd.map_fan(rays, fov), rng, cell, offsets=off if moved else None, detail=True)
            for k, (rays, fov, rng, cell) in enumerate(area_ref.CASES) for moved in (False, True)}
    return dict(index=index, lines=lines, states=st, offsets=off, want=want)


def check_not_vacuous(level):
    """on the restatement's own result, before any comparison (runs on the CPU; the seeds of LEVELS were picked to meet it)"""
    d = inputs(level)
    by_range = False
    for (k, moved), w in d['want'].items():
        rays, fov, rng, cell = area_ref.CASES[k]
        assert np.array_equal(area_ref.popcount(w['area']), w['new'])
        assert w['new'][:, 0].max() > (100 if rays > 1 else 10), (level, k, moved)  # some player marks more than 100 FREE cells
        assert (w['limit'] < 1).any() and w['new'][:, 1].max() > 0, (level, k, moved)  # some ray ends on a wall
        assert (w['area'][:, 0] & w['area'][:, 1]).any(), (level, k, moved)  # some cell carries both bits
        by_range = by_range or bool((w['limit'] >= 1).any())
        assert rd.area_steps(rng, cell) + 1 > 256 or k != 2  # more than 256 samples a ray
        if level == 'E1M1' and k in BAND_CASES:  # the kernel's own window formula: some player's window takes several bands
            bands = area_ref.bands(area_ref.grid(d['lines'], cell), cell, d['states'], rd.map_fan(rays, fov), rng)
            assert bands.max() >= (2 if k == 1 else 4) and bands.min() >= 1, (k, bands)
    # some ray ends by range: on E1M1 (E1M2 is one room, smaller than any range here)
    assert by_range == (level == 'E1M1')
    for k in range(len(area_ref.CASES)):
        differs = (d['want'][k, False]['area'] != d['want'][k, True]['area']).any((1, 2))
        assert differs.any() and not differs.all(), (level, k, int(differs.sum()))  # offsets change some players' rows


@pytest.mark.parametrize('level', list(LEVELS))
def test_rows_and_counts_match_the_restatement(level):
    check_not_vacuous(level)
    rd.set_device(0)
    d = inputs(level)
    world = wad().build_world(d['index'])
    states, offs = _dev(d['states']), torch.from_numpy(d['offsets']).cuda()
    for k, (rays, fov, rng, cell) in enumerate(area_ref.CASES):
        g = world.area_grid(cell)
        assert g == area_ref.grid(d['lines'], cell) and world.area_words(cell) == g.words
        for moved in (False, True):
            want = d['want'][k, moved]
            new = torch.full((PLAYERS, 2), 77, dtype=torch.int32, device='cuda')
            area = world.reveal_area(states, _fan(rays, fov), rng, cell, offsets=offs if moved else None, new_out=new)
            assert area.dtype == torch.int32 and tuple(area.shape) == (PLAYERS, 2, g.words)
            _same(area, want['area'], (level, k, moved))
            _same(new, want['new'], (level, k, moved, 'new'))


def test_a_second_pass_of_three_rays_that_look_backwards():
    """259 rays: the pass loop runs twice, and the second pass's sight limits come from 85 slices and a thread without one"""
    d = inputs('E1M1')
    n, fan, rng, cell = reveal_ref.TAIL_PLAYERS, reveal_ref.tail_fan(), reveal_ref.TAIL_RANGE, 0.25
    assert len(d['lines']) == 713 and fan.shape == (259, 2) and fan.dtype == F
    st = rays_ref.players(wad().build_level(d['index']), LEVELS['E1M1'][1], count=n)
    off = reveal_ref.random_offsets(np.random.RandomState(LEVELS['E1M1'][1]), n, d['offsets'].shape[1])
    rd.set_device(0)
    world = wad().build_world(d['index'])
    for o_np in (None, off):
        want = area_ref.reveal(d['lines'], st, fan, rng, cell, offsets=o_np, detail=True)
        head = area_ref.reveal(d['lines'], st, fan[:256], rng, cell, offsets=o_np)
        # on the restatement's own result: the tail pass marks cells of its own for every player, and every ray of it ends on a wall
        assert (want['area'] != head['area']).any((1, 2)).all() and (want['limit'][:, 256:] < 1).all()
        new = torch.full((n, 2), 77, dtype=torch.int32, device='cuda')
        area = world.reveal_area(_dev(st), torch.from_numpy(fan).cuda(), rng, cell, offsets=None if o_np is None else torch.from_numpy(o_np).cuda(),
                                 new_out=new)
        _same(area, want['area'], ('tail', o_np is not None))
        _same(new, want['new'], ('tail', o_np is not None, 'new'))


def test_rows_accumulate_and_the_counts_are_what_is_new():
    rd.set_device(0)
    d = inputs('E1M1')
    rays, fov, rng, cell = area_ref.CASES[1]  # a window in bands
    lines = d['lines']
    g = area_ref.grid(lines, cell)
    world = wad().build_world(d['index'])
    fan = _fan(rays, fov)
    first = d['want'][1, False]['area']
    rs = np.random.RandomState(3)
    noise = (rs.randint(0, 1 << 32, first.shape, dtype=np.uint64).astype(np.uint32)
             & rs.randint(0, 1 << 32, first.shape, dtype=np.uint64).astype(np.uint32))  # a quarter of the bits
    before = first | noise
    moved_states = rays_ref.players(wad().build_level(d['index']), 999, count=PLAYERS)
    want = area_ref.reveal(lines, moved_states, rd.map_fan(rays, fov), rng, cell, area=before)
    fresh = area_ref.reveal(lines, moved_states, rd.map_fan(rays, fov), rng, cell)
    assert np.array_equal(want['area'], before | fresh['area']) and np.array_equal(want['new'], area_ref.popcount(want['area'] & ~before))
    assert (want['new'][:, 0] > 0).sum() > PLAYERS // 2 and (want['new'] < fresh['new']).any()
    rows, new = _rows(before), torch.full((PLAYERS, 2), 77, dtype=torch.int32, device='cuda')
    assert world.reveal_area(_dev(moved_states), fan, rng, cell, area=rows, new_out=new) is rows
    _same(rows, before | fresh['area'], 'old OR restated')
    _same(new, area_ref.popcount(_u32(rows) & ~before), 'the counts')
    world.reveal_area(_dev(moved_states), fan, rng, cell, area=rows, new_out=new)  # a third, identical call finds nothing new
    _same(rows, want['area'], 'third call')
    assert not new.any().item()
    assert g.words == rows.shape[2]


def test_padding_words_and_row_tail_bits_survive_a_wide_stride():
    rd.set_device(0)
    d = inputs('E1M1')
    rays, fov, rng, cell = area_ref.CASES[2]
    g = area_ref.grid(d['lines'], cell)
    assert g.gw % 32 != 0
    tail = np.uint32(0xFFFFFFFF) << np.uint32(g.gw % 32)  # the bits of a grid row's last word beyond gw
    before = np.zeros((PLAYERS, 2, g.words + 3), np.uint32)
    before[:, :, g.words:] = 0xDEADBEEF
    before[:, :, g.pitch - 1:g.words:g.pitch] = tail & np.uint32(0xA5A5A5A5)
    assert (before[:, :, g.pitch - 1] != 0).all()
    world = wad().build_world(d['index'])
    rows = _rows(before)
    new = torch.zeros((PLAYERS, 2), dtype=torch.int32, device='cuda')
    world.reveal_area(_dev(d['states']), _fan(rays, fov), rng, cell, area=rows, new_out=new)
    got = _u32(rows)
    assert (got[:, :, g.words:] == 0xDEADBEEF).all()
    assert np.array_equal(got[:, :, g.pitch - 1:g.words:g.pitch] & tail, before[:, :, g.pitch - 1:g.words:g.pitch])
    mask = np.full(g.words, 0xFFFFFFFF, np.uint32)
    mask[g.pitch - 1::g.pitch] = ~tail
    want = d['want'][2, False]
    _same(got[:, :, :g.words] & mask, want['area'], 'the rows')
    _same(new, want['new'], 'the counts')


def test_a_world_set_with_slots_out_of_range_and_a_grid_per_level():
    rd.set_device(0)
    slots = [0, 1, 7]
    ws = wad().build_world_set(slots)
    tables = [ws.map_lines(s) for s in range(3)]
    parts, lv = [], []
    for s, index in enumerate(slots):
        parts.append(rays_ref.players(wad().build_level(index), 60 + s, count=24))
        lv += [s] * 24
    rs = np.random.RandomState(9)
    order = rs.permutation(72)
    st, lv = np.concatenate(parts)[order], np.array(lv, np.uint32)[order]
    lv[::13] = 3 + (np.arange(len(lv[::13])) % 2) * 0x7FFFFFF0  # slots 3 and far beyond: out of the set
    outside = lv >= 3
    levels_t = torch.from_numpy(lv.view(np.int32).copy()).cuda()
    off = reveal_ref.random_offsets(rs, 72, ws.n_objects)
    rays, fov, rng, cell = area_ref.CASES[1]
    grids = [area_ref.grid(t, cell) for t in tables]
    words = ws.area_words(cell)
    assert [ws.area_grid(s, cell) for s in range(3)] == grids and words == max(g.words for g in grids) and len({g.words for g in grids}) == 3
    for o_np in (None, off):
        before = np.zeros((72, 2, words), np.uint32)
        before[outside] = 0x5A5A5A5A
        want = area_ref.reveal(tables, st, rd.map_fan(rays, fov), rng, cell, offsets=o_np, levels=lv, area=before)
        assert (want['area'][outside] == 0x5A5A5A5A).all() and not want['new'][outside].any() and (want['new'][~outside, 0] > 0).all()
        rows, new = _rows(before), torch.full((72, 2), 77, dtype=torch.int32, device='cuda')
        ws.reveal_area(_dev(st), levels_t, _fan(rays, fov), rng, cell, offsets=None if o_np is None else torch.from_numpy(o_np).cuda(),
                       area=rows, new_out=new)
        _same(rows, want['area'], 'set rows')
        _same(new, want['new'], 'set counts')
    # a slot's players alone equal the single world's
    mine = lv == 1
    alone = wad().build_world(1).reveal_area(_dev(st[mine]), _fan(rays, fov), rng, cell)
    both = ws.reveal_area(_dev(st), levels_t, _fan(rays, fov), rng, cell)
    assert torch.equal(alone, both[torch.from_numpy(mine).cuda()][:, :, :alone.shape[2]])
    # and the set's maps: a slot outside the set draws nothing
    got = ws.draw_area_maps(_dev(st), levels_t, 40, 30, 0.12, both, cell, rotate=True).cpu().numpy()
    _same(got, area_ref.draw(tables, st, _u32(both), cell, 40, 30, 0.12, rotate=True, levels=lv), 'set maps')
    assert not got[outside].any() and got[~outside].reshape((~outside).sum(), -1).any(1).all()


def test_a_nan_position_or_yaw_marks_nothing():
    rd.set_device(0)
    d = inputs('E1M1')
    st = d['states'].copy()
    st['pos'][5, 0] = np.nan
    st['pos'][6, 2] = np.nan
    st['yaw'][7] = np.nan
    world = wad().build_world(d['index'])
    rays, fov, rng, cell = area_ref.CASES[0]
    want = area_ref.reveal(d['lines'], st, rd.map_fan(rays, fov), rng, cell)
    assert not want['area'][5:8].any() and not want['new'][5:8].any() and (want['new'][:5, 0] > 0).all()
    new = torch.full((PLAYERS, 2), 77, dtype=torch.int32, device='cuda')
    area = world.reveal_area(_dev(st), _fan(rays, fov), rng, cell, new_out=new)
    _same(area, want['area'], 'rows')
    _same(new, want['new'], 'counts')
    maps = world.draw_area_maps(_dev(st), 40, 30, 0.12, torch.full_like(area, -1), cell, rotate=True).cpu().numpy()
    assert not maps[5:8].any() and maps[:5].any()


def test_a_side_stream_the_callers_tensors_and_a_captured_graph():
    rd.set_device(0)
    d = inputs('E1M1')
    world = wad().build_world(d['index'])
    rays, fov, rng, cell = area_ref.CASES[1]
    want = d['want'][1, True]
    states, fan, offs = _dev(d['states']), _fan(rays, fov), torch.from_numpy(d['offsets']).cuda()
    rows = torch.zeros((PLAYERS, 2, world.area_words(cell)), dtype=torch.int32, device='cuda')
    new = torch.full((PLAYERS, 2), 77, dtype=torch.int32, device='cuda')
    maps = torch.full((PLAYERS, 30, 40), 77, dtype=torch.uint8, device='cuda')
    want_maps = area_ref.draw(d['lines'], d['states'], want['area'], cell, 40, 30, 0.12)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert world.reveal_area(states, fan, rng, cell, offsets=offs, area=rows, new_out=new, stream=side) is rows
    assert world.draw_area_maps(states, 40, 30, 0.12, rows, cell, out=maps, stream=side) is maps
    side.synchronize()
    _same(rows, want['area'], 'side stream')
    _same(new, want['new'], 'side stream counts')
    _same(maps.cpu().numpy(), want_maps, 'side stream maps')
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a call that waited or allocated could not be captured
        world.reveal_area(states, fan, rng, cell, offsets=offs, area=rows, new_out=new, stream=torch.cuda.current_stream())
        world.draw_area_maps(states, 40, 30, 0.12, rows, cell, out=maps, stream=torch.cuda.current_stream())
    rows.zero_()
    new.fill_(77)
    maps.fill_(77)
    g.replay()
    torch.cuda.synchronize()
    _same(rows, want['area'], 'graph replay')
    _same(new, want['new'], 'graph replay counts')
    _same(maps.cpu().numpy(), want_maps, 'graph replay maps')
    g.replay()  # onto its own result: nothing new
    torch.cuda.synchronize()
    _same(rows, want['area'], 'second replay')
    assert not new.any().item()


def test_argument_checks_queue_nothing():
    rd.set_device(0)
    world, ws = wad().build_world(1), wad().build_world_set([1, 0])
    host_only, host_set = wad().build_world(1, device=False), wad().build_world_set([1, 0], device=False)
    n, cell = 16, 0.25
    states = _dev(rays_ref.players(wad().build_level(1), 6, count=n))
    lv = torch.zeros(n, dtype=torch.int32, device='cuda')
    fan = _fan(16, 1.0)
    words, set_words = world.area_words(cell), ws.area_words(cell)
    rows = torch.full((n, 2, set_words), 0x11111111, dtype=torch.int32, device='cuda')
    new = torch.full((n, 2), -1, dtype=torch.int32, device='cuda')  # no count is 2^32 - 1
    out = torch.full((n, 53, 77), 77, dtype=torch.uint8, device='cuda')
    small = torch.zeros((n, 1, 3), dtype=torch.float32, device='cuda')
    assert world.game_objects > 1 and ws.n_objects > 1 and set_words > words
    L = rd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    f = ctypes.c_float
    BAD = -1
    view = rd.MapView(77, 53, 0.12, 0.0, 0.0, 0)

    def one(h=world, st=states, k=n, dirs=fan, r=16, rng=10.0, off=None, no=0, c=cell, steps=80, area=rows, stride=set_words, cnt=new):
        return L.rdoom_world_reveal_area(h._h if h is not None else None, p(st), k, p(dirs), r, f(rng), p(off), no, f(c), steps, p(area), stride,
                                         p(cnt), None)

    def many(h=ws, st=states, lv_=lv, k=n, dirs=fan, r=16, rng=10.0, off=None, no=0, c=cell, steps=80, area=rows, stride=set_words, cnt=new):
        return L.rdoom_worldset_reveal_area(h._h if h is not None else None, p(st), p(lv_), k, p(dirs), r, f(rng), p(off), no, f(c), steps,
                                            p(area), stride, p(cnt), None)

    def draw_one(h=world, st=states, k=n, v=view, area=rows, stride=set_words, c=cell, o=out):
        return L.rdoom_world_draw_area_maps(h._h if h is not None else None, p(st), k, ctypes.byref(v) if v is not None else None, p(area), stride,
                                            f(c), p(o), None)

    def draw_many(h=ws, st=states, lv_=lv, k=n, v=view, area=rows, stride=set_words, c=cell, o=out):
        return L.rdoom_worldset_draw_area_maps(h._h if h is not None else None, p(st), p(lv_), k, ctypes.byref(v) if v is not None else None,
                                               p(area), stride, f(c), p(o), None)

    inf, nan = float('inf'), float('nan')
    for call, enough in ((one, words), (many, set_words)):
        for kw in [dict(h=None), dict(st=None), dict(area=None), dict(dirs=None), dict(r=0), dict(rng=0.0), dict(rng=-3.0), dict(rng=inf),
                   dict(rng=nan), dict(c=0.0), dict(c=-1.0), dict(c=inf), dict(c=nan), dict(steps=0), dict(steps=4097),
                   dict(stride=enough - 1), dict(stride=0), dict(c=1e-4, stride=1 << 30), dict(off=small, no=1)]:
            assert call(**kw) == BAD, (call.__name__, list(kw))
            assert L.rdoom_last_error()
    for call, enough in ((draw_one, words), (draw_many, set_words)):
        for kw in [dict(h=None), dict(st=None), dict(area=None), dict(o=None), dict(v=None), dict(c=0.0), dict(c=nan), dict(stride=enough - 1),
                   dict(c=1e-4, stride=1 << 30), dict(v=rd.MapView(0, 53, 0.12, 0.0, 0.0, 0)), dict(v=rd.MapView(77, 53, 0.0, 0.0, 0.0, 0)),
                   dict(v=rd.MapView(77, 53, 0.12, 0.0, 0.0, rd.MAP_SHOW_FLAT))]:
            assert call(**kw) == BAD, (call.__name__, list(kw))
            assert L.rdoom_last_error()
    assert many(lv_=None) == BAD and draw_many(lv_=None) == BAD
    assert one(h=host_only) == BAD and many(h=host_set) == BAD and draw_one(h=host_only) == BAD and draw_many(h=host_set) == BAD
    if rd.device_count() > 1:  # a handle that lives on another device
        rd.set_device(1)
        assert one() == BAD and many() == BAD and draw_one() == BAD and draw_many() == BAD
        rd.set_device(0)
    torch.cuda.synchronize()
    assert (rows == 0x11111111).all().item() and (new == -1).all().item() and (out == 77).all().item()  # nothing was queued
    assert one(k=0) == 0 and many(k=0) == 0 and one(k=0, st=None, area=None, dirs=None) == 0 and draw_one(k=0, st=None, area=None, o=None) == 0
    torch.cuda.synchronize()
    assert (rows == 0x11111111).all().item() and (new == -1).all().item() and (out == 77).all().item()
    assert one(steps=4096) == 0 and many(cnt=None) == 0 and draw_one() == 0
    torch.cuda.synchronize()
    assert not (new == -1).any().item() and not (out == 77).any().item()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        world.reveal_area(states.cpu(), fan, 10.0, cell)
    with pytest.raises(ValueError):
        world.reveal_area(states, torch.zeros((16, 3), device='cuda'), 10.0, cell)
    with pytest.raises(ValueError):
        world.reveal_area(states, fan, 10.0, cell, area=rows[:, :, :words - 1].contiguous())
    with pytest.raises(ValueError):
        world.reveal_area(states, fan, 10.0, cell, area=rows.float())
    with pytest.raises(ValueError):
        world.reveal_area(states, fan, 10.0, cell, area=rows[:, 0].contiguous())
    with pytest.raises(ValueError):
        world.reveal_area(states, fan, 10.0, cell, new_out=new[:5])
    with pytest.raises(ValueError):
        ws.reveal_area(states, lv[:5], fan, 10.0, cell)
    with pytest.raises(ValueError):
        world.draw_area_maps(states, 77, 53, 0.12, rows[:5], cell)
    with pytest.raises(ValueError):
        world.draw_area_maps(states, 77, 53, 0.12, rows, cell, out=out[:, :5])
    with pytest.raises(rd.RdoomError):
        world.reveal_area(states, fan, -1.0, cell, n_steps=4)
    with pytest.raises(rd.RdoomError):
        world.reveal_area(states, fan, 10.0, cell, n_steps=5000)


VIEWS = [dict(width=w, height=h, rotate=r, top_down=t) for (w, h) in ((40, 30), (160, 120)) for r in (False, True) for t in (False, True)]


@pytest.mark.parametrize('level', list(LEVELS))
def test_maps_match_the_restatement(level):
    rd.set_device(0)
    d = inputs(level)
    world = wad().build_world(d['index'])
    states = _dev(d['states'])
    for k in (0, 1):  # cell 0.25: two pixels of 0.12 to a cell; cell 0.0625: two cells to a pixel
        rays, fov, rng, cell = area_ref.CASES[k]
        area_np = d['want'][k, True]['area']
        area = _rows(area_np)
        ones = torch.full_like(area, -1)
        g = area_ref.grid(d['lines'], cell)
        for kw in VIEWS:
            want = area_ref.draw(d['lines'], d['states'], area_np, cell, scale=0.12, **kw)
            assert ((want & 1) != 0).reshape(PLAYERS, -1).any(1).sum() > PLAYERS // 2 and (want == 0).any() and want.max() <= 3
            assert (want >= 2).reshape(PLAYERS, -1).any(1).sum() > PLAYERS // 4  # walls show in many maps
            got = world.draw_area_maps(states, kw['width'], kw['height'], 0.12, area, cell, rotate=kw['rotate'], top_down=kw['top_down'])
            assert got.dtype == torch.uint8 and tuple(got.shape) == (PLAYERS, kw['height'], kw['width'])
            _same(got.cpu().numpy(), want, (level, k, kw))
            # all-ones rows: 3 inside the grid, 0 outside -- the grid's outline as the restatement draws it
            full = world.draw_area_maps(states, kw['width'], kw['height'], 0.12, ones, cell, rotate=kw['rotate'], top_down=kw['top_down']).cpu().numpy()
            want_full = area_ref.draw(d['lines'], d['states'], np.full_like(area_np, 0xFFFFFFFF), cell, scale=0.12, **kw)
            _same(full, want_full, (level, k, kw, 'ones'))
            assert set(np.unique(full).tolist()) <= {0, 3} and (full == 3).any()
        # 160 x 120 pixels of 0.12 are 19.2 x 14.4 units: wider than E1M2, so its maps show the outside of the grid
        if level == 'E1M2':
            assert (want_full == 0).any() and g.gw * cell < 19.2


def test_top_down_is_the_bottom_up_map_flipped_and_north_up_ignores_the_yaw():
    rd.set_device(0)
    d = inputs('E1M1')
    world = wad().build_world(d['index'])
    cell = area_ref.CASES[0][3]
    area = _rows(d['want'][0, False]['area'])
    states = _dev(d['states'])
    for rotate in (False, True):
        up = world.draw_area_maps(states, 40, 30, 0.12, area, cell, rotate=rotate)
        down = world.draw_area_maps(states, 40, 30, 0.12, area, cell, rotate=rotate, top_down=True)
        assert torch.equal(up.flip(1), down) and not torch.equal(up, down)
    turned = d['states'].copy()
    turned['yaw'] += F(1.0)
    assert torch.equal(world.draw_area_maps(_dev(turned), 40, 30, 0.12, area, cell), world.draw_area_maps(states, 40, 30, 0.12, area, cell))
    assert not torch.equal(world.draw_area_maps(_dev(turned), 40, 30, 0.12, area, cell, rotate=True),
                           world.draw_area_maps(states, 40, 30, 0.12, area, cell, rotate=True))


def test_area_maps_register_with_the_line_maps():
    """the same view through draw_maps and draw_area_maps: pixels where the line map shows a one-sided line and the area map shows
    something exist on E1M1 -- the walls a player saw lie where the automap draws them -- and where a one-sided line is drawn and
    the cell under the pixel was marked at all, it is far more often a wall than in the map at large"""
    rd.set_device(0)
    d = inputs('E1M1')
    world = wad().build_world(d['index'])
    rays, fov, rng, cell = area_ref.CASES[2]  # all round, cell 0.0625: two cells to a pixel of 0.12
    area = _rows(d['want'][2, False]['area'])
    states = _dev(d['states'])
    for rotate in (False, True):
        lines_map = world.draw_maps(states, 160, 120, 0.12, half_width=0.75, marker=0.0, rotate=rotate)
        area_map = world.draw_area_maps(states, 160, 120, 0.12, area, cell, rotate=rotate)
        on_line = lines_map == rd.MAP_ONE_SIDED
        marked = area_map != 0
        assert (on_line & marked).sum().item() > 1000
        wall_on_line = ((area_map >= 2) & on_line).sum().item() / max((on_line & marked).sum().item(), 1)
        wall_anywhere = (area_map >= 2).sum().item() / marked.sum().item()
        assert wall_on_line > 4 * wall_anywhere, (wall_on_line, wall_anywhere)
