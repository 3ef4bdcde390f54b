"""Top-down maps on the GPU (automap.hip draw_maps_kernel / worldset_draw_maps_kernel) against the test-side restatement
(tests/automap_restatement.c, a brute force over every line for every pixel): every byte, zero tolerance.  All levels, 1024 players
each, the views of automap_ref.VIEWS; the chunked path; a door the game step opened; world sets; streams, preallocated outputs and
graph capture; the secret and never-on-the-map flags; every argument check of the header."""
import ctypes
import os

import numpy as np
import pytest

import automap_ref
import mapcheck
import rays_ref
import rust_doom_amd as rd
import world_ref
from test_game_host import patched_variant
from test_gpu_game import _door
from test_rays_host import LEVEL_IDS, levels
from util import META_PATH, ensure_big_wad, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32
LIST_CAPACITY = 512  # automap.hip LIST_CAP: the lines a workgroup's LDS list holds before it must fold and empty it
TILE = 32            # automap.hip TILE: a workgroup draws 32 x 32 pixels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _same(got, want, what):
    got = got.cpu().numpy() if not isinstance(got, np.ndarray) else got
    bad = got != want
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3], got[bad][:8], want[bad][:8])


def _is_e1m2(path, index):
    return path == ensure_wad() and index == 1


@pytest.mark.parametrize('path,index', levels(), **LEVEL_IDS)
def test_maps_match_the_restatement(path, index):
    """every view of automap_ref.VIEWS on the synthetic levels; on the rich and the big level (7208 lines: the brute force is the
    cost) the large view at scale 0.30 and two small ones.  The restatement's own output is checked first, so that the comparison
    cannot pass on empty images."""
    rd.set_device(0)
    wad = rd.Wad(path, META_PATH)
    world = wad.build_world(index)
    lines = world.map_lines()
    st = rays_ref.players(wad.build_level(index), 7000 + index, count=1024)
    states = _dev(st)
    views = automap_ref.VIEWS if path == ensure_wad() else [automap_ref.VIEWS[k] for k in (2, 5, 6)]
    seen, seen_flat = set(), set()
    for kw in views:
        want = automap_ref.draw(lines, st, **kw)
        got = world.draw_maps(states, kw['width'], kw['height'], kw['scale'], **{k: v for k, v in kw.items() if k not in ('width', 'height', 'scale')})
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1024, kw['height'], kw['width'])
        _same(got, want, kw)
        codes = set(np.unique(want).tolist())
        seen |= codes
        if kw.get('show_flat'):
            seen_flat |= codes
        else:
            assert rd.MAP_FLAT not in codes
        if kw.get('marker', 3.0) == 0.0:
            assert rd.MAP_PLAYER not in codes
        if kw['scale'] == 0.30 and not _is_e1m2(path, index):
            line_pixels = ((want >= rd.MAP_FLAT) & (want <= rd.MAP_ONE_SIDED)).reshape(1024, -1).any(1)
            assert line_pixels.mean() >= 0.99, line_pixels.mean()
    if not _is_e1m2(path, index):
        assert {rd.MAP_CEILING_STEP, rd.MAP_FLOOR_STEP, rd.MAP_CLOSED, rd.MAP_ONE_SIDED, rd.MAP_PLAYER} <= seen, seen
        if seen_flat:
            assert rd.MAP_FLAT in seen_flat


def _dist64(p, a, b):
    """float64 distance of point p from each segment a[k] -> b[k]"""
    a, b, p = a.astype(np.float64), b.astype(np.float64), np.asarray(p, np.float64)
    d = b - a
    len2 = (d * d).sum(1)
    t = np.clip(((p - a) * d).sum(1) / np.where(len2 > 0, len2, 1.0), 0.0, 1.0)
    return np.hypot(*(p - (a + t[:, None] * d)).T)


def _hide_one_sided(src, directory):
    """a copy of the IWAD at `src` whose first level has flag 0x80 (never on the map) on every one-sided linedef"""
    data, lumps = mapcheck.read_directory(src)
    marker = mapcheck.level_markers(lumps)[0]
    _, pos, size = next(l for l in lumps[marker + 1:marker + 11] if l[0] == b'LINEDEFS')
    raw = np.frombuffer(data, np.uint8).copy()
    recs = raw[pos:pos + size].view('<u2').reshape(-1, 7)
    recs[recs[:, 6] == 0xFFFF, 2] |= rd.LINE_HIDDEN
    path = os.path.join(directory, 'hidden.wad')
    with open(path, 'wb') as f:
        f.write(raw.tobytes())
    return path


def _most_lines_a_tile_must_keep(lines, drawn, states, kw):
    """over the tiles of the north-up maps of `states`: the most drawn lines that pass within half_width - 1 pixels of a tile's
    centre.  The pixel centre nearest to that centre is 0.71 pixels from it, so each such line covers it: ANY correct cull keeps
    them all"""
    most = 0
    a, b = lines['a'][drawn], lines['b'][drawn]
    for s in states:
        for ty in range((kw['height'] + TILE - 1) // TILE):
            for tx in range((kw['width'] + TILE - 1) // TILE):
                u = (tx * TILE + TILE / 2 - kw['width'] / 2) * kw['scale']
                v = (ty * TILE + TILE / 2 - kw['height'] / 2) * kw['scale']
                centre = (s['pos'][0] - v, s['pos'][2] - u)  # north-up: q = (pos.x - v, pos.z - u)
                most = max(most, int((_dist64(centre, a, b) <= (kw['half_width'] - 1.0) * kw['scale']).sum()))
    return most


def test_a_list_longer_than_lds_is_folded_in_chunks(tmp_path):
    """the big level at scale 0.30 with very thick lines: some tile must keep more than LIST_CAPACITY lines, and the maps still
    equal the brute force.  Twice: the level as it is, where lines this thick leave only one-sided pixels (the largest class), the
    marker and the empty border; and a copy with its one-sided linedefs flagged never-on-the-map, where the two-sided classes
    meet in every pixel and the maximum over a list cut in chunks decides it"""
    rd.set_device(0)
    kw = dict(width=160, height=120, scale=0.30, half_width=40.0, marker=3.0)
    plain = ensure_big_wad()
    for path, extra, codes in ((plain, dict(), {rd.MAP_NONE, rd.MAP_ONE_SIDED, rd.MAP_PLAYER}),
                               (_hide_one_sided(plain, str(tmp_path)), dict(show_flat=True),
                                {rd.MAP_NONE, rd.MAP_FLAT, rd.MAP_CEILING_STEP, rd.MAP_FLOOR_STEP, rd.MAP_CLOSED, rd.MAP_PLAYER})):
        wad = rd.Wad(path, META_PATH)
        world = wad.build_world(0)
        lines = world.map_lines()
        st = rays_ref.players(wad.build_level(0), 31, count=128)
        drawn = automap_ref.classes(lines, show_hidden=False) != 0
        most = _most_lines_a_tile_must_keep(lines, drawn, st[:16], kw)
        assert most > LIST_CAPACITY, most
        for rotate in (False, True):
            want = automap_ref.draw(lines, st, rotate=rotate, **kw, **extra)
            assert set(np.unique(want).tolist()) == codes, (np.unique(want), codes)
            _same(world.draw_maps(_dev(st), 160, 120, 0.30, half_width=40.0, rotate=rotate, **extra), want, (path, rotate))


def test_a_door_opens_in_the_pushers_map_only(tmp_path):
    """on the patched E1M1: eight players stand before a manual door, player 1 pushes it.  With the offsets the step left, the
    pusher's map loses CLOSED pixels and changes only within reach of that door's lines; every other player's map is the map at
    rest; all of them are the restatement's under the same offsets"""
    rd.set_device(0)
    wad_path, meta_path = patched_variant(str(tmp_path))
    wad = rd.Wad(wad_path, meta_path)
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    t = world.triggers()
    i, eff, st = _door(world, t, ref)
    door = int(eff['object_id'])
    lines = world.map_lines()
    two_sided = (lines['front']['present'] == 1) & (lines['back']['present'] == 1)
    on_door = two_sided & ((lines['front']['ceiling_id'] == door) | (lines['back']['ceiling_id'] == door))  # the door's faces and sides
    assert on_door.sum() >= 2
    assert (automap_ref.classes(lines)[on_door] == rd.MAP_CLOSED).all()  # shut at rest
    n, ticks = 8, 90
    st = np.repeat(st, n)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    act = np.zeros((ticks, n), np.uint8)
    act[0, 1] = rd.ACTION_PUSH
    game, offs = world.game_state(n)
    st = world.step_game(st, inp, game, offs, actions=act)
    off_np = offs.cpu().numpy()
    assert off_np[1, door, 1] > 0.5 and (off_np[[0] + list(range(2, n))] == 0).all()
    kw = dict(width=160, height=120, scale=0.05, half_width=1.5)
    rest = world.draw_maps(_dev(st), 160, 120, 0.05, half_width=1.5).cpu().numpy()
    moved = world.draw_maps(_dev(st), 160, 120, 0.05, offsets=offs, half_width=1.5).cpu().numpy()
    _same(rest, automap_ref.draw(lines, st, **kw), 'at rest')
    _same(moved, automap_ref.draw(lines, st, off_np, **kw), 'with the offsets')
    others = [0] + list(range(2, n))
    assert np.array_equal(moved[others], rest[others])
    assert (rest[1] == rd.MAP_CLOSED).sum() > 0 and (moved[1] == rd.MAP_CLOSED).sum() < (rest[1] == rd.MAP_CLOSED).sum()
    changed = moved[1] != rest[1]
    assert changed.any() and (rest[1][changed] == rd.MAP_CLOSED).all()
    pts = automap_ref.points(st[1], **kw)[changed]
    reach = 1.5 * 0.05 + 1e-4
    near = np.array([_dist64(q, lines['a'][on_door], lines['b'][on_door]).min() for q in pts])
    assert (near <= reach).all(), near.max()
    assert (automap_ref.classes(lines, off_np[1])[on_door] != rd.MAP_CLOSED).all()


def test_world_set_maps_with_a_slot_out_of_range():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 4]
    ws = wad.build_world_set(slots)
    tables = [ws.map_lines(s) for s in range(3)]
    rng = np.random.RandomState(5)
    parts, lv = [], []
    for s, index in enumerate(slots):
        parts.append(rays_ref.players(wad.build_level(index), 40 + s, count=100))
        lv += [s] * 100
    st = np.concatenate(parts)
    lv = np.array(lv, np.uint32)
    order = rng.permutation(len(st))
    st, lv = st[order], lv[order]
    lv[::37] = 3 + (np.arange(len(lv[::37])) % 2) * 0x7FFFFFF0  # slots 3 and far beyond: out of the set
    levels_t = torch.from_numpy(lv.astype(np.int64).astype(np.uint32).view(np.int32)).cuda()
    offs = rng.choice(np.array([0.0, 0.0, 0.5, 1.28, -0.64], F), (len(st), ws.n_objects, 3)).astype(F)
    offs_t = torch.from_numpy(offs).cuda()
    for kw in (automap_ref.VIEWS[0], automap_ref.VIEWS[3], automap_ref.VIEWS[6]):
        extra = {k: v for k, v in kw.items() if k not in ('width', 'height', 'scale')}
        for o_np, o_t in ((None, None), (offs, offs_t)):
            want = automap_ref.draw(tables, st, o_np, levels=lv, **kw)
            got = ws.draw_maps(_dev(st), levels_t, kw['width'], kw['height'], kw['scale'], offsets=o_t, **extra)
            _same(got, want, kw)
            assert (want[lv >= 3] == 0).all() and (want[lv < 3] != 0).reshape((lv < 3).sum(), -1).any(1).all()
    # a slot's players alone equal the single world's
    world = wad.build_world(2)
    mine = lv == 1
    kw = automap_ref.VIEWS[3]
    extra = {k: v for k, v in kw.items() if k not in ('width', 'height', 'scale')}
    alone = world.draw_maps(_dev(st[mine]), kw['width'], kw['height'], kw['scale'], **extra)
    both = ws.draw_maps(_dev(st), levels_t, kw['width'], kw['height'], kw['scale'], **extra)
    assert torch.equal(alone, both[torch.from_numpy(mine).cuda()])


def test_a_side_stream_a_preallocated_output_and_a_captured_graph():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0)
    lines = world.map_lines()
    st = rays_ref.players(wad.build_level(0), 77, count=256)
    states = _dev(st)
    kw = dict(width=77, height=53, scale=0.12, rotate=True, top_down=True)
    want = automap_ref.draw(lines, st, **kw)
    out = torch.full((256, 53, 77), 99, dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = world.draw_maps(states, 77, 53, 0.12, rotate=True, top_down=True, out=out, stream=side)
    assert res is out
    side.synchronize()
    _same(out, want, 'side stream')
    _, offs = world.game_state(256)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a call that waited or allocated could not be captured
        world.draw_maps(states, 77, 53, 0.12, offsets=offs, rotate=True, top_down=True, out=out, stream=torch.cuda.current_stream())
    out.fill_(99)
    g.replay()
    torch.cuda.synchronize()
    _same(out, want, 'graph replay')
    colors = torch.from_numpy(rd.MAP_COLORS).cuda()
    rgb = colors[out.long()]
    assert tuple(rgb.shape) == (256, 53, 77, 3) and (rgb[out == rd.MAP_PLAYER] == 255).all().item()
    assert len(set(map(tuple, rd.MAP_COLORS[[0, 1, 2, 3, 4, 5, 8]].tolist()))) == 7


def test_secret_and_hidden_linedefs(tmp_path):
    """a copy of the IWAD with flag 0x20 (secret: drawn as one-sided) on E1M1's two-sided linedefs of even index and 0x80 (never on
    the map) on every fifth linedef: the table carries the bits, hidden lines appear only with show_hidden, and the maps are the
    restatement's"""
    rd.set_device(0)
    data, lumps = mapcheck.read_directory(ensure_wad())
    marker = mapcheck.level_markers(lumps)[0]
    name, pos, size = next(l for l in lumps[marker + 1:marker + 11] if l[0] == b'LINEDEFS')
    raw = np.frombuffer(data, np.uint8).copy()
    recs = raw[pos:pos + size].view('<u2').reshape(-1, 7)
    two_sided = recs[:, 6] != 0xFFFF
    secret = two_sided & (np.arange(len(recs)) % 2 == 0)
    hidden = np.arange(len(recs)) % 5 == 0
    recs[secret, 2] |= rd.LINE_SECRET
    recs[hidden, 2] |= rd.LINE_HIDDEN
    path = os.path.join(str(tmp_path), 'flags.wad')
    with open(path, 'wb') as f:
        f.write(raw.tobytes())
    wad = rd.Wad(path, META_PATH)
    world = wad.build_world(0)
    lines = world.map_lines()
    assert np.array_equal((lines['flags'] & rd.LINE_SECRET) != 0, secret) and np.array_equal((lines['flags'] & rd.LINE_HIDDEN) != 0, hidden)
    plain = rd.Wad(ensure_wad(), META_PATH).build_world(0, device=False).map_lines()
    was, now = automap_ref.classes(plain), automap_ref.classes(lines)
    assert (now[secret] == rd.MAP_ONE_SIDED).all() and (was[secret] != rd.MAP_ONE_SIDED).all()
    assert (automap_ref.classes(lines, show_hidden=False)[hidden] == 0).all()
    st = rays_ref.players(wad.build_level(0), 8, count=256)
    states = _dev(st)
    maps = {}
    for show in (False, True):
        kw = dict(width=160, height=120, scale=0.12, show_hidden=show, show_flat=True)
        maps[show] = automap_ref.draw(lines, st, **kw)
        _same(world.draw_maps(states, 160, 120, 0.12, show_hidden=show, show_flat=True), maps[show], kw)
    assert (maps[True] >= maps[False]).all() and (maps[True] > maps[False]).any()
    base = automap_ref.draw(plain, st, width=160, height=120, scale=0.12, show_flat=True)
    assert ((maps[True] == rd.MAP_ONE_SIDED) & (base != rd.MAP_ONE_SIDED) & (base != 0)).any()


def test_argument_checks_queue_nothing():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(0), wad.build_world_set([0, 2])
    host_only, host_set = wad.build_world(0, device=False), wad.build_world_set([0, 2], device=False)
    st = rays_ref.players(wad.build_level(0), 6, count=64)
    states = _dev(st)
    lv = torch.zeros(64, dtype=torch.int32, device='cuda')
    out = torch.full((64, 53, 77), 77, dtype=torch.uint8, device='cuda')
    small = torch.zeros((64, 1, 3), dtype=torch.float32, device='cuda')
    assert world.game_objects > 1 and ws.n_objects > 1
    L = rd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    BAD = -1  # RDOOM_BAD_ARG

    def view(width=77, height=53, scale=0.12, half_width=0.75, marker=3.0, flags=0):
        return rd.MapView(width, height, scale, half_width, marker, flags)

    def one(h=world, st_=states, n=64, off=None, no=0, v=view(), o=out):
        return L.rdoom_world_draw_maps(h._h if h is not None else None, p(st_), n, p(off), no, ctypes.byref(v) if v is not None else None,
                                       p(o), None)

    def many(h=ws, st_=states, lv_=lv, n=64, off=None, no=0, v=view(), o=out):
        return L.rdoom_worldset_draw_maps(h._h if h is not None else None, p(st_), p(lv_), n, p(off), no,
                                          ctypes.byref(v) if v is not None else None, p(o), None)

    inf, nan = float('inf'), float('nan')
    bad_views = [view(width=0), view(height=0), view(width=16385), view(height=16385), view(scale=0.0), view(scale=-1.0), view(scale=inf),
                 view(scale=nan), view(half_width=0.0), view(half_width=-0.5), view(half_width=inf), view(half_width=nan),
                 view(marker=-1.0), view(marker=inf), view(marker=nan), view(flags=16), view(flags=0x80000000)]
    for call in (one, many):
        for kw in [dict(h=None), dict(st_=None), dict(o=None), dict(v=None), dict(off=small, no=1)] + [dict(v=v) for v in bad_views]:
            assert call(**kw) == BAD, (call.__name__, {k: (x if k != 'v' or x is None else [getattr(x, f[0]) for f in x._fields_]) for k, x in kw.items()})
            assert rd.lib().rdoom_last_error()
    assert many(lv_=None) == BAD
    assert one(h=host_only) == BAD and many(h=host_set) == BAD
    # n x tiles beyond one launch: 2^26 maps of 16384 x 16384 pixels (nothing is touched: the check comes first)
    assert one(n=1 << 26, v=view(width=16384, height=16384)) == BAD
    torch.cuda.synchronize()
    assert (out == 77).all().item()  # nothing was queued
    assert one(n=0) == 0 and many(n=0) == 0 and one(n=0, st_=None, o=None) == 0
    torch.cuda.synchronize()
    assert (out == 77).all().item()
    assert one() == 0
    torch.cuda.synchronize()
    assert not (out == 77).any().item()
    out.fill_(77)
    assert many() == 0
    torch.cuda.synchronize()
    assert not (out == 77).any().item()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        world.draw_maps(states.cpu(), 77, 53, 0.12)
    with pytest.raises(ValueError):
        world.draw_maps(states, 0, 53, 0.12)
    with pytest.raises(ValueError):
        world.draw_maps(states, 77, 53, 0.12, out=torch.empty((64, 53, 76), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        world.draw_maps(states, 77, 53, 0.12, out=torch.empty((64, 53, 77), dtype=torch.int8, device='cuda'))
    with pytest.raises(ValueError):
        world.draw_maps(states, 77, 53, 0.12, offsets=small[:5])
    with pytest.raises(ValueError):
        ws.draw_maps(states, lv[:5], 77, 53, 0.12)
    with pytest.raises(rd.RdoomError):
        world.draw_maps(states, 77, 53, -2.0)
