"""Sectors on the GPU (sectors.hip locate_players_kernel / draw_sector_maps_kernel and their world-set forms) against the test-side
restatement (tests/sector_restatement.c, every point from the root on its own): every element of every output, zero tolerance.
E1M1, E1M8 and the big level; players at floor centroids, outside the map and on NaN; per-player offsets; rows that accumulate; a
wide stride; partial tiles, three scales, both orientations and row orders, each plane alone, the visited filter; registration with
the line table; a floor that moves for one player only, through offsets written by hand and through a lift ridden down by step_game; a world set with slots out of range; streams, caller's tensors and graph
capture; a patched IWAD's secret sector."""
import functools

import numpy as np
import pytest

import rust_doom_amd as rd
import sector_ref
import world_ref
from test_game_host import patched_variant
from test_gpu_game import _floor_y, _front
from util import META_PATH, ensure_big_wad, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
LEVELS = {'E1M1': (ensure_wad, 0, 201), 'E1M8': (ensure_wad, 7, 209), 'big': (ensure_big_wad, 0, 210)}  # (wad, index, seed)
# both sizes (160 x 120: whole tiles but the last row of them; 77 x 53: partial tiles both ways); 0.05: a tile inside one leaf;
# 0.30: many leaves and void per tile; 2.5: the whole level in a few tiles
VIEWS = [
    dict(width=160, height=120, scale=0.05),
    dict(width=160, height=120, scale=0.30, rotate=True, top_down=True),
    dict(width=77, height=53, scale=0.05, rotate=True),
    dict(width=77, height=53, scale=0.30, top_down=True),
    dict(width=160, height=120, scale=2.5, rotate=True),
]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _rows(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _same(got, want, what):
    if not isinstance(got, np.ndarray):
        got = got.cpu().numpy()
    got = got.view(want.dtype) if got.dtype.itemsize == want.dtype.itemsize else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint8) != want.view(np.uint8)  # bytes: -inf, +inf and every float bit for bit
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3])


@functools.lru_cache(maxsize=None)
def inputs(level, players):
    """what the tests of one level share, computed once and left unchanged"""
    ensure, index, seed = LEVELS[level]
    wad = rd.Wad(ensure(), META_PATH)
    host = wad.build_world(index, device=False)
    rng = np.random.default_rng(seed)
    st, on_map = sector_ref.players(wad, index, players, rng)
    off = sector_ref.random_offsets(rng, players, host.game_objects)
    return wad, index, sector_ref.Tables(host), st, off, on_map


def _walk(tables, st, steps, rng):
    """rows of visited bits after a short random walk of every player (the restatement's), and the states where it ends"""
    visited = None
    st = st.copy()
    for _ in range(steps):
        visited = sector_ref.locate(tables, st, visited=visited)['visited']
        st['pos'][:, [0, 2]] += rng.uniform(-1.5, 1.5, (len(st), 2)).astype(F)
    return visited, st


@pytest.mark.parametrize('level', list(LEVELS))
def test_players_are_located_as_the_restatement_locates_them(level):
    rd.set_device(0)
    wad, index, tables, st, off, _ = inputs(level, 256)
    world = wad.build_world(index)
    words = world.visited_words()
    assert words == sector_ref.words_of(len(tables.sectors))
    rng = np.random.default_rng(7)
    for o_np in (None, off):
        o_t = torch.from_numpy(o_np).cuda() if o_np is not None else None
        want = sector_ref.locate(tables, st, o_np)
        inside = want['sector'] != sector_ref.NONE
        assert 0.8 < inside.mean() < 1 and len(set(want['sector'].tolist())) > 2
        heights = torch.full((256, 2), 7.0, device='cuda')
        visited = torch.zeros((256, words), dtype=torch.int32, device='cuda')
        new = torch.full((256,), 9, dtype=torch.int32, device='cuda')
        got = world.locate_players(_dev(st), offsets=o_t, heights_out=heights, visited=visited, new_out=new)
        _same(got, want['sector'], 'sector')
        _same(heights, want['heights'], 'heights')
        _same(visited, want['visited'], 'visited')
        _same(new, want['new'], 'new')
        _same(world.locate_players(_dev(st)), want['sector'], 'sector alone')  # every optional output NULL
        # moved states onto rows holding the first call's bits and random ones, in a wide stride whose padding survives
        moved = st.copy()
        moved['pos'][:, [0, 2]] += rng.uniform(-2, 2, (256, 2)).astype(F)
        rows = np.full((256, words + 3), 0, np.uint32)
        rows[:, :words] = want['visited'] | (rng.integers(0, 2 ** 32, (256, words), dtype=np.uint64).astype(np.uint32) &
                                              rng.integers(0, 2 ** 32, (256, words), dtype=np.uint64).astype(np.uint32))
        n_sec = len(tables.sectors)
        if n_sec % 32:
            rows[:, words - 1] &= np.uint32((1 << (n_sec % 32)) - 1)
        rows[:, words:] = 0xDEADBEEF
        want2 = sector_ref.locate(tables, moved, o_np, visited=rows)
        assert want2['new'].any() and not want2['new'].all()
        rows_t = _rows(rows)
        got2 = world.locate_players(_dev(moved), offsets=o_t, visited=rows_t, new_out=new)
        _same(got2, want2['sector'], 'moved sector')
        _same(rows_t, want2['visited'], 'moved rows')
        _same(new, want2['new'], 'moved new')
        assert (rows_t.cpu().numpy().view(np.uint32)[:, words:] == 0xDEADBEEF).all()


@pytest.mark.parametrize('view', range(len(VIEWS)))
@pytest.mark.parametrize('level', list(LEVELS))
def test_sector_maps_match_the_restatement(level, view):
    rd.set_device(0)
    wad, index, tables, st, off, on_map = inputs(level, 64)
    world = wad.build_world(index)
    kw = VIEWS[view]
    flags = {k: v for k, v in kw.items() if k in ('rotate', 'top_down')}
    size = (kw['width'], kw['height'], kw['scale'])
    states = _dev(st)
    off_t = torch.from_numpy(off).cuda()
    want = sector_ref.draw(tables, st, off, **kw)
    live = want[0][:on_map]  # the players on the map
    if kw['scale'] == 0.30:  # every map holds at least two sectors and some void
        for m in live:
            assert (m == sector_ref.NONE16).any() and len(np.unique(m[m != sector_ref.NONE16])) >= 2
    if kw['scale'] == 0.05:  # some whole tile is a single sector
        assert any(len(np.unique(m[:32, :32])) == 1 and m[0, 0] != sector_ref.NONE16 for m in live)
    assert (want[0][on_map:] == sector_ref.NONE16).all() and np.isposinf(want[1][on_map:]).all() and np.isneginf(want[2][on_map:]).all()
    got = world.draw_sector_maps(states, *size, offsets=off_t, sector_out=True, floor=True, ceiling=True, **flags)
    for g, w, what in zip(got, want, ('sector', 'floor', 'ceiling')):
        _same(g, w, (level, kw, what))
    if view in (1, 3):  # each plane alone, at rest
        rest = sector_ref.draw(tables, st, None, **kw)
        _same(world.draw_sector_maps(states, *size, **flags), rest[0], 'sector alone')
        _same(world.draw_sector_maps(states, *size, floor=True, **flags), rest[1], 'floor alone')
        _same(world.draw_sector_maps(states, *size, ceiling=True, **flags), rest[2], 'ceiling alone')
    # through the rows of a short walk: some pixels become none, not all
    visited, _ = _walk(tables, st, 4, np.random.default_rng(3))
    seen = sector_ref.draw(tables, st, off, visited=visited, **kw)
    hidden = (seen[0] == sector_ref.NONE16) & (want[0] != sector_ref.NONE16)
    assert hidden.any() and (seen[0] != sector_ref.NONE16).any()
    got = world.draw_sector_maps(states, *size, offsets=off_t, sector_out=True, floor=True, ceiling=True, visited=_rows(visited), **flags)
    for g, w, what in zip(got, seen, ('sector', 'floor', 'ceiling')):
        _same(g, w, (level, kw, what, 'visited'))


def test_sector_maps_register_with_the_line_table():
    """E1M1 at 0.12, unrotated: either side of the mid-point of every one-sided linedef, one pixel along the normal, is a sector on
    one side and none on the other -- in the pixels the device drew for a player standing on the mid-point"""
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines = world.map_lines()
    one = lines[(lines['front']['present'] + lines['back']['present']) == 1]
    mid = (one['a'] + one['b']) / F(2)
    pos = np.zeros((len(one), 3), F)
    pos[:, 0], pos[:, 2] = mid[:, 0], mid[:, 1]
    st = rd.player_states(pos, np.zeros(len(one), F))
    w = h = 33  # the player's point is the centre of pixel (16, 16)
    got = world.draw_sector_maps(_dev(st), w, h, 0.12).cpu().numpy().view(np.uint16)
    _same(got, sector_ref.draw(sector_ref.Tables(world), st, width=w, height=h, scale=0.12)[0], 'registration maps')
    d = (one['b'] - one['a']).astype(np.float64)
    normal = np.stack([d[:, 1], -d[:, 0]], 1) / np.hypot(d[:, 0], d[:, 1])[:, None]
    # q = (pos.x - v, pos.z - u): a world step (sx, sz) is the pixel step (column -sz / scale, row -sx / scale); 1.5 pixels
    # along the normal is at least one whole pixel away on the dominant axis
    col = np.rint(-normal[:, 1] * 1.5).astype(int)
    row = np.rint(-normal[:, 0] * 1.5).astype(int)
    k = np.arange(len(one))
    ahead, behind = got[k, 16 + row, 16 + col], got[k, 16 - row, 16 - col]
    assert ((ahead == sector_ref.NONE16) != (behind == sector_ref.NONE16)).all(), np.nonzero((ahead == 0xFFFF) == (behind == 0xFFFF))[0][:8]


def test_a_floor_moves_for_the_player_whose_offsets_move_it():
    rd.set_device(0)
    wad, index, tables, st, _, on_map = inputs('E1M1', 64)
    world = wad.build_world(index)
    at = sector_ref.locate(tables, st)['sector']
    moving = [p for p in range(on_map) if at[p] != sector_ref.NONE and tables.sectors['floor_id'][at[p]] != 0]
    assert moving, 'no player stands on a floor that moves'
    p = moving[0]
    obj = int(tables.sectors['floor_id'][at[p]])
    off = np.zeros((64, world.game_objects, 3), F)
    off[p, obj, 1] = F(-0.64)
    off_t = torch.from_numpy(off).cuda()
    heights = torch.zeros((64, 2), device='cuda')
    world.locate_players(_dev(st), offsets=off_t, heights_out=heights)
    rest = sector_ref.locate(tables, st)['heights']
    want = rest.copy()
    want[p, 0] = rest[p, 0] + F(-0.64)
    _same(heights, want, 'heights')
    kw = dict(width=77, height=53, scale=0.05)
    lowered = world.draw_sector_maps(_dev(st), 77, 53, 0.05, offsets=off_t, floor=True).cpu().numpy()
    flat = sector_ref.draw(tables, st, **kw)
    _same(lowered, sector_ref.draw(tables, st, off, **kw)[1], 'floor')
    changed = lowered != flat[1]
    assert changed[p].any() and not np.delete(changed, p, 0).any()
    assert (tables.sectors['floor_id'][flat[0][p][changed[p]]] == obj).all()


def test_a_lift_ridden_down_lowers_its_riders_floor_only(tmp_path):
    """the recipe of test_gpu_game's lift: on the patched E1M1 three players stand at the lift's height just in front of its
    walk-over line (special 88), facing away; player 1 walks backwards across the line onto the lift and step_game lowers it in
    that player's game.  With the offsets tensor the step left, once the lift is all the way down: player 1 stands in the lift's
    sector, its heights_out floor and the lift's pixels of its floor plane fell by offs[1, object, 1], nothing else of its
    planes changed, and the other players' heights and planes are those at rest.  Everything equals the restatement."""
    rd.set_device(0)
    wad_path, meta_path = patched_variant(str(tmp_path))
    wad = rd.Wad(wad_path, meta_path)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    tables = sector_ref.Tables(world)
    t = world.triggers()
    trig, effs = t['triggers'], t['effects']
    lift_i = int(np.nonzero((trig['special_type'] == 88) & (trig['effect_end'] > trig['effect_start']))[0][0])
    eff = effs[trig['effect_start'][lift_i]]
    obj, lowest = int(eff['object_id']), F(eff['first_height_offset'])
    assert lowest < -0.5
    behind, yaw = _front(trig[[lift_i]], np.array([[-0.35]], F))
    y = _floor_y(ref, behind)
    normal = np.array([-trig['displace'][lift_i, 1], trig['displace'][lift_i, 0]], F)
    at = behind + normal * F(0.45)
    n, rider = 3, 1
    st = rd.player_states(np.repeat([[at[0, 0], y[0] + 0.25, at[0, 1]]], n, 0), np.repeat(yaw, n))
    game, offs = world.game_state(n)
    inp = np.zeros((40, n), rd.PLAYER_INPUT)
    inp['movement'][:, rider, 1] = 1.0
    st = world.step_game(st, inp, game, offs)  # backwards onto the lift, across the line
    still = np.zeros((1, n), rd.PLAYER_INPUT)
    for _ in range(260):
        if offs[rider, obj, 1].item() == lowest:
            break
        st = world.step_game(st, still, game, offs)
    off_np = offs.cpu().numpy()
    assert off_np[rider, obj, 1] == lowest and (np.delete(off_np, rider, 0) == 0).all()

    rest, want = sector_ref.locate(tables, st), sector_ref.locate(tables, st, off_np)
    lift_sector = int(want['sector'][rider])
    assert lift_sector != sector_ref.NONE and tables.sectors['floor_id'][lift_sector] == obj  # the rider stands on the lift
    assert tables.sectors['floor_id'][want['sector'][0]] != obj                                # the others do not
    heights = torch.zeros((n, 2), device='cuda')
    _same(world.locate_players(_dev(st), offsets=offs, heights_out=heights), want['sector'], 'sector')
    _same(heights, want['heights'], 'heights')
    got = heights.cpu().numpy()
    assert got[rider, 0] == rest['heights'][rider, 0] + lowest and got[rider, 1] == rest['heights'][rider, 1]
    assert np.array_equal(np.delete(got, rider, 0), np.delete(rest['heights'], rider, 0))

    kw = dict(width=77, height=53, scale=0.05, rotate=True)
    planes = [g.cpu().numpy() for g in world.draw_sector_maps(_dev(st), 77, 53, 0.05, offsets=offs, rotate=True, sector_out=True,
                                                              floor=True, ceiling=True)]
    flat = sector_ref.draw(tables, st, **kw)
    for g, w, what in zip(planes, sector_ref.draw(tables, st, off_np, **kw), ('sector', 'floor', 'ceiling')):
        _same(g, w, ('lift', what))
    for g, w in zip(planes, flat):  # the others' planes are the planes at rest
        _same(np.delete(g, rider, 0), np.delete(w, rider, 0), 'the others')
    _same(planes[0][rider], flat[0][rider], "the rider's sectors")
    _same(planes[2][rider], flat[2][rider], "the rider's ceilings")
    on_lift = (flat[0][rider] != sector_ref.NONE16) & (tables.sectors['floor_id'][np.minimum(flat[0][rider], len(tables.sectors) - 1)] == obj)
    assert on_lift[53 // 2, 77 // 2] and 0 < on_lift.sum() < on_lift.size
    assert np.array_equal(planes[1][rider][on_lift], flat[1][rider][on_lift] + lowest)
    assert np.array_equal(planes[1][rider][~on_lift].view(np.uint32), flat[1][rider][~on_lift].view(np.uint32))


def test_a_world_set_with_slots_out_of_range():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 7]
    ws = wad.build_world_set(slots)
    tables = [sector_ref.Tables(ws, s) for s in range(3)]
    rng = np.random.default_rng(11)
    parts, lv = [], []
    for s, index in enumerate(slots):
        parts.append(sector_ref.players(wad, index, 40, rng, outside=1, nan=1)[0])
        lv += [s] * 40
    order = rng.permutation(120)
    st, lv = np.concatenate(parts)[order], np.array(lv, np.uint32)[order]
    lv[::17] = 3 + (np.arange(len(lv[::17])) % 2) * 0x7FFFFFF0
    levels_t = _rows(lv)
    off = sector_ref.random_offsets(rng, 120, ws.n_objects)
    off_t = torch.from_numpy(off).cuda()
    words = ws.visited_words()
    rows = rng.integers(0, 2, (120, words)).astype(np.uint32)
    want = sector_ref.locate(tables, st, off, levels=lv, visited=rows)
    assert (want['sector'][lv >= 3] == sector_ref.NONE).all() and not want['new'][lv >= 3].any() and want['new'].any()
    rows_t, new = _rows(rows), torch.full((120,), 9, dtype=torch.int32, device='cuda')
    heights = torch.zeros((120, 2), device='cuda')
    got = ws.locate_players(_dev(st), levels_t, offsets=off_t, heights_out=heights, visited=rows_t, new_out=new)
    for g, k in ((got, 'sector'), (heights, 'heights'), (rows_t, 'visited'), (new, 'new')):
        _same(g, want[k], k)
    for kw in (VIEWS[1], VIEWS[2]):
        flags = {k: v for k, v in kw.items() if k in ('rotate', 'top_down')}
        for vis in (None, want['visited']):
            planes = sector_ref.draw(tables, st, off, levels=lv, visited=vis, **kw)
            got = ws.draw_sector_maps(_dev(st), levels_t, kw['width'], kw['height'], kw['scale'], offsets=off_t, sector_out=True, floor=True,
                                      ceiling=True, visited=_rows(vis) if vis is not None else None, **flags)
            for g, w in zip(got, planes):
                _same(g, w, (kw, vis is not None))
            assert (planes[0][lv >= 3] == sector_ref.NONE16).all() and (planes[0][lv < 3] != sector_ref.NONE16).any()
    world = wad.build_world(2)  # a slot's players alone equal the single world's
    mine = lv == 1
    alone = world.draw_sector_maps(_dev(st[mine]), 77, 53, 0.30)
    both = ws.draw_sector_maps(_dev(st), levels_t, 77, 53, 0.30)
    assert torch.equal(alone, both[torch.from_numpy(mine).cuda()])


def test_a_side_stream_callers_tensors_and_a_captured_graph():
    rd.set_device(0)
    wad, index, tables, st, off, _ = inputs('E1M1', 64)
    world = wad.build_world(index)
    states, off_t = _dev(st), torch.from_numpy(off).cuda()
    kw = dict(width=77, height=53, scale=0.30, rotate=True, top_down=True)
    want = sector_ref.draw(tables, st, off, **kw)
    where = sector_ref.locate(tables, st, off)
    sec = torch.full((64, 53, 77), 7, dtype=torch.int16, device='cuda')
    floor, ceil = torch.zeros((64, 53, 77), device='cuda'), torch.zeros((64, 53, 77), device='cuda')
    out = torch.full((64,), 5, dtype=torch.int32, device='cuda')
    heights = torch.zeros((64, 2), device='cuda')
    rows = torch.zeros((64, world.visited_words()), dtype=torch.int32, device='cuda')
    new = torch.zeros(64, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = world.draw_sector_maps(states, 77, 53, 0.30, offsets=off_t, rotate=True, top_down=True, sector_out=sec, floor=floor, ceiling=ceil,
                                 stream=side)
    assert res[0] is sec and res[1] is floor and res[2] is ceil
    assert world.locate_players(states, offsets=off_t, heights_out=heights, visited=rows, new_out=new, out=out, stream=side) is out
    side.synchronize()
    for g, w in zip((sec, floor, ceil), want):
        _same(g, w, 'side stream')
    for g, k in ((out, 'sector'), (heights, 'heights'), (rows, 'visited'), (new, 'new')):
        _same(g, where[k], k)
    g = torch.cuda.CUDAGraph()
    rows.zero_()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):  # a call that waited or allocated could not be captured
        cur = torch.cuda.current_stream()
        world.locate_players(states, offsets=off_t, heights_out=heights, visited=rows, new_out=new, out=out, stream=cur)
        world.draw_sector_maps(states, 77, 53, 0.30, offsets=off_t, rotate=True, top_down=True, sector_out=sec, floor=floor, ceiling=ceil,
                               visited=rows, stream=cur)
    for t in (sec, floor, ceil, out, heights, new):
        t.fill_(3)
    rows.zero_()
    g.replay()
    torch.cuda.synchronize()
    for t, k in ((out, 'sector'), (heights, 'heights'), (rows, 'visited'), (new, 'new')):
        _same(t, where[k], ('graph', k))
    through = sector_ref.draw(tables, st, off, visited=where['visited'], **kw)
    for t, w in zip((sec, floor, ceil), through):
        _same(t, w, 'graph replay')
    with pytest.raises(rd.RdoomError):  # checked before anything is queued
        world.draw_sector_maps(states, 77, 53, float('nan'))


def test_entering_the_secret_sector_is_new_exactly_once(tmp_path):
    rd.set_device(0)
    base = rd.Wad(ensure_wad(), META_PATH)
    cent = base.build_level(0).floor_centroids().astype(F)
    plain = sector_ref.Tables(base.build_world(0, device=False))
    at = sector_ref.sector_at(plain, cent[:, [0, 2]])
    target = int(np.nonzero(at != sector_ref.NONE)[0][len(cent) // 2])
    secret = int(at[target])
    other = int(at[at != secret][0])
    wad = rd.Wad(sector_ref.patched_wad(tmp_path, secret=secret, damaging=other), META_PATH)
    world = wad.build_world(0)
    types = torch.from_numpy(world.map_sectors().sectors['sector_type'].astype(np.int64)).cuda()
    assert types[secret].item() == 9 and types[other].item() == 5 and (types == 9).sum().item() == 1
    start = cent[np.nonzero(at == other)[0][0]]
    rows = torch.zeros((1, world.visited_words()), dtype=torch.int32, device='cuda')
    new = torch.zeros(1, dtype=torch.int32, device='cuda')
    found = []
    path = [start, start, cent[target], cent[target], start, cent[target]]  # in, stay, out, and in again
    for pos in path:
        st = rd.player_states(pos[None], np.zeros(1, F))
        sector = world.locate_players(_dev(st), visited=rows, new_out=new)
        found.append(int(((types[sector.long().clamp(min=0)] == 9) & (new == 1) & (sector >= 0)).sum().item()))
    assert found == [0, 0, 1, 0, 0, 0]
    assert sorted(np.nonzero(rd.unpack_seen(rows[0], len(types)))[0].tolist()) == sorted({secret, other})
