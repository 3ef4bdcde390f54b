"""GPU: WHERE the world and world-set kernels write (world.hip, automap.hip, reveal.hip, area.hip, sectors.hip, spawn.hip, goal.hip,
path.hip).  Every device array of every call is a carving of a guarded arena (tests/guarded.py) at the least alignment the header
allows: states, inputs, offsets, fans, seeds and 32-bit outputs at 4 and 12 mod 16, byte maps and masks at 1, 2 and 3, 16-bit planes
at 2 and 6, the game state at an odd multiple of 16.  After the call every byte outside the outputs -- guard bands, gaps, inputs, the
players and rows behind the last one asked for -- must be what it was, and the outputs must equal the family's *_ref.py bit for bit,
with the arena poisoned 0xFF and again 0x00.  One level (E1M3: 358 lines, 60 sectors, 15 objects) and a world set of E1M1 and E1M3
with the players' slots mixed; 1, 63 and 65 players, and 63 of 65, where a wave serves 64 players; 3 where a workgroup serves one."""
import ctypes
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import area_ref
import automap_ref
import game_ref
import goal_ref
import path_ref
import rays_ref
import reveal_ref
import rust_doom_amd as rd
import sector_ref
import spawn_ref
import world_ref
import worldset_ref
from guarded import GUARD, host_of, run_guarded
from util import META_PATH, ensure_wad

pytestmark = pytest.mark.gpu
F = np.float32
LEVEL, SET = 2, [0, 2]
CELL = 0.25
TICKS = 3
KINDS = ['world', 'set']
WAVE_COUNTS = [(1, 1), (63, 63), (65, 65), (63, 65)]  # (players asked for, players the arrays hold)
MAPS = [(37, 21), (64, 16)]                          # an odd width: rows change alignment; a multiple of everything
SLACK = 16 * (GUARD + 64)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Context:
    """one level, or a set of two with the players' slots mixed: the device handle and what the references read of it"""

    def __init__(self, kind):
        rd.set_device(0)
        self.kind, self.is_set = kind, kind == 'set'
        self.wad = rd.Wad(ensure_wad(), META_PATH)
        self.indices = SET if self.is_set else [LEVEL]
        self.built = [self.wad.build_level(i) for i in self.indices]
        self.h = self.wad.build_world_set(SET) if self.is_set else self.wad.build_world(LEVEL)
        slots = range(len(self.indices))
        self.lines = [self.h.map_lines(s) for s in slots] if self.is_set else self.h.map_lines()
        self.tables = [sector_ref.Tables(self.h, s) for s in slots] if self.is_set else sector_ref.Tables(self.h)
        self.spawn_levels = [spawn_ref.Level(self.h, s) for s in slots] if self.is_set else spawn_ref.Level(self.h)
        self.grids = [self.h.area_grid(s, CELL) for s in slots] if self.is_set else self.h.area_grid(CELL)
        self.n_objects = self.h.n_objects if self.is_set else self.h.game_objects
        self._refs = {}

    def ref_world(self, slot=0):
        if slot not in self._refs:
            self._refs[slot] = world_ref.RefWorld(self.wad, self.indices[slot])
        return self._refs[slot]

    def slots(self, n, seed):
        """the players' slots: None for a world; for a set both levels, mixed"""
        if not self.is_set:
            return None
        lv = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint32)
        lv[:2] = (1, 0)[:n]
        return lv

    def players(self, n, seed):
        """(states, slots): every player at rest above a floor centroid of its own level"""
        lv = self.slots(n, seed)
        per = [rays_ref.players(b, seed + 10 * k, count=n) for k, b in enumerate(self.built)]
        st = per[0].copy()
        if lv is not None:
            st[lv == 1] = per[1][lv == 1]
        return st, lv

    def offsets(self, n, seed):
        return sector_ref.random_offsets(np.random.default_rng(seed), n, self.n_objects)

    def call(self, name, states, d_lv, *args, **kw):
        """World.name(states, ...) or WorldSet.name(states, levels, ...)"""
        f = getattr(self.h, name)
        return f(states, *args, **kw) if not self.is_set else f(states, d_lv, *args, **kw)


@functools.lru_cache(maxsize=None)
def context(kind):
    return Context(kind)


def place_players(arena, st, lv, residue, held=None):
    """the states (and the slots) as carvings; with `held` > len(st) the arrays hold that many records, the rest poison"""
    n = len(st)
    held = n if held is None else held
    d_st = arena.carve((held * 40,), torch.uint8, 16, residue, 'states')
    d_st[:n * 40].copy_(torch.from_numpy(st.view(np.uint8).copy()))
    d_lv = None
    if lv is not None:
        d_lv = arena.carve((held,), torch.int32, 16, 4, 'levels')
        d_lv[:n].copy_(torch.from_numpy(lv.view(np.int32).copy()))
    assert d_st.data_ptr() % 16 == residue
    return d_st, d_lv


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- world.hip: the step, the game step, the reset, the sweep, the rays ----------------------------------------------------------

@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', WAVE_COUNTS)
def test_step(n, held, residue):
    from test_gpu_world import _players, _script
    c = context('world')
    st = _players(c.built[0], n, seed=n)
    inp = _script(n, TICKS, seed=n)
    want = c.ref_world().step(st, inp)
    assert (words(want) != words(st)).any()

    def setup(arena):
        d_st, _ = place_players(arena, st, None, residue, held)
        d_in = arena.place(inp, 16, residue, 'inputs')
        return (lambda: c.h.step(d_st[:n * 40], d_in, n_ticks=TICKS)), [('states', d_st[:n * 40], words(want))]
    run_guarded(held * 40 + n * TICKS * 20 + SLACK, setup, 'step n=%d of %d at %d' % (n, held, residue))


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', WAVE_COUNTS)
def test_sweep(n, held, residue):
    from test_gpu_world import _queries
    c = context('world')
    sph, vel = _queries(c.h.arrays(), c.built[0], n, seed=300 + n)
    off = np.zeros((n, c.h.n_objects, 3), F)
    off[::2, :, 1] = np.random.default_rng(n).uniform(-1.0, 1.0, (len(off[::2]), c.h.n_objects)).astype(F)
    want = c.ref_world().sweep(sph, vel, off)

    def setup(arena):
        d_s = arena.place(sph, 16, residue, 'spheres', torch.float32)
        d_v = arena.place(vel, 16, residue, 'vels', torch.float32)
        d_o = arena.place(off, 16, residue, 'offsets', torch.float32)
        out = arena.carve((held, 4), torch.float32, 16, residue, 'out')
        assert d_s.data_ptr() % 16 == out.data_ptr() % 16 == residue

        def call():
            rd._check(rd.lib().rdoom_world_sweep(c.h._h, ptr(d_s), ptr(d_v), n, ptr(d_o), c.h.n_objects, None, ptr(out)))
        return call, [('out', out[:n], want)]
    run_guarded(held * 16 + n * (28 + c.h.n_objects * 12) + SLACK, setup, 'sweep n=%d of %d at %d' % (n, held, residue))


def game_players(c, n, seed):
    """a world: players before trigger lines, pushing; a set: at their levels' starts.  (states, slots, inputs, actions)"""
    from test_gpu_game import _script, _seed
    if c.is_set:
        lv = c.slots(n, seed)
        st = c.h.start_states(lv)
    else:
        lv = None
        st, _ = _seed(c.ref_world(), c.h.triggers()['triggers'], 3 * n + 8, seed)
        assert len(st) >= n
        st = st[:n].copy()
    inp, act = _script(n, TICKS, seed + 1, push=0.5)
    return st, lv, inp, act


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n', [1, 63, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_step_game(kind, n, residue):
    c = context(kind)
    st, lv, inp, act = game_players(c, n, 40 + n)
    gb = c.h.game_bytes()
    if c.is_set:
        ref = worldset_ref.RefWorldSet(ensure_wad(), META_PATH, SET, lv)
        want = ref.step(st, inp, act)
        want_off, want_lv = ref.offsets(), ref.levels.astype(np.int32)
    else:
        t = c.h.triggers()
        rg = game_ref.RefGame(c.ref_world(), t['triggers'], t['effects'], n, c.h.game_objects)
        want = rg.step(st, inp, act)
        want_off = rg.offsets
    assert (words(want) != words(st)).any()

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue)
        d_in = arena.place(inp, 16, residue, 'inputs')
        d_act = arena.place(act, 16, 1, 'actions')
        game = arena.carve((n * gb // 4,), torch.int32, 32, 16, 'game')
        offs = arena.carve((n, c.n_objects, 3), torch.float32, 16, residue, 'offsets')
        assert game.data_ptr() % 32 == 16  # 16-byte aligned, at an odd multiple of 16
        c.h.reset_game(game, offs, *([d_lv] if c.is_set else []))
        outputs = [('states', d_st, words(want)), ('offsets', offs, want_off), ('game', game, None)]
        if c.is_set:
            outputs.append(('levels', d_lv, want_lv))
        return (lambda: c.h.step_game(d_st, d_in, game, offs, *([d_lv] if c.is_set else []), actions=d_act, n_ticks=TICKS)), outputs
    run_guarded(n * (40 + 4 + TICKS * 21 + gb + c.n_objects * 12) + SLACK, setup, '%s step_game n=%d at %d' % (kind, n, residue))


@pytest.mark.parametrize('n', [1, 63, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_reset_game_with_a_mask(kind, n):
    """the masked players' games are fresh and their offsets zero; the others keep every byte.  The game's bytes have no reference:
    they are compared with the same reset of an ordinary tensor of the same contents; the offsets are the witness with one"""
    c = context(kind)
    gb = c.h.game_bytes()
    lv = c.slots(n, 60 + n)
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    mask[-1] = n == 1
    before = np.random.default_rng(n).uniform(0.1, 1.0, (n, c.n_objects, 3)).astype(F)
    want_off = np.where(mask[:, None, None] != 0, F(0.0), before)
    games = []

    def setup(arena):
        d_lv = arena.place(lv.view(np.int32), 16, 4, 'levels', torch.int32) if c.is_set else None
        d_mask = arena.place(mask, 16, 1, 'mask')
        game = arena.carve((n * gb // 4,), torch.int32, 32, 16, 'game')
        offs = arena.place(before, 16, 4, 'offsets', torch.float32)
        plain_game = torch.full((n * gb // 4,), 0, dtype=torch.int32, device='cuda').view(torch.uint8).fill_(arena.poison).view(torch.int32)
        plain_offs = torch.from_numpy(before).cuda()
        extra = [d_lv.clone()] if c.is_set else []
        c.h.reset_game(plain_game, plain_offs, *extra, mask=torch.from_numpy(mask).cuda())
        assert np.array_equal(plain_offs.cpu().numpy(), want_off)

        def call():
            c.h.reset_game(game, offs, *([d_lv] if c.is_set else []), mask=d_mask)
            games.append((host_of(game), host_of(plain_game)))
        return call, [('offsets', offs, want_off), ('game', game, None)]
    run_guarded(n * (5 + gb + c.n_objects * 12) + SLACK, setup, '%s reset_game n=%d' % (kind, n))
    for got, plain in games:
        assert np.array_equal(got, plain)
    if n > 1:  # the last player, unmasked, kept the poison; the first, masked, did not
        per = gb // 4
        assert (games[0][0][-per:] == 0xFFFFFFFF).all() and (games[1][0][-per:] == 0).all() and (games[0][0][:per] != 0xFFFFFFFF).any()


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n_rays', [5, 64])
@pytest.mark.parametrize('kind', KINDS)
def test_cast_rays(kind, n_rays, residue):
    c = context(kind)
    n = 3
    st, lv = c.players(n, 70 + n_rays)
    dirs = rd.ray_fan(n_rays, 1.5, pitch=0.1)
    off = c.offsets(n, 5)
    frac, hit = np.zeros((n, n_rays), F), np.zeros((n, n_rays), np.uint32)
    for p in range(n):
        slot = 0 if lv is None else int(lv[p])
        o = off[p:p + 1, :c.ref_world(slot).n_objects]
        r = rays_ref.cast(c.ref_world(slot), st[p:p + 1], dirs, 30.0, o)
        frac[p], hit[p] = r['frac'][0], r['hit'][0]
    assert np.isfinite(frac).any()

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue)
        d_dirs = arena.place(dirs, 16, 4, 'dirs', torch.float32)
        d_off = arena.place(off, 16, 4, 'offsets', torch.float32)
        d_frac = arena.carve((n, n_rays), torch.float32, 16, residue, 'frac')
        d_hit = arena.carve((n, n_rays), torch.int32, 16, residue, 'hit')
        assert d_frac.data_ptr() % 16 == d_hit.data_ptr() % 16 == residue
        return (lambda: c.call('cast_rays', d_st, d_lv, d_dirs, 30.0, offsets=d_off, frac_out=d_frac, hit_out=d_hit)), \
            [('frac', d_frac, frac), ('hit', d_hit, hit)]
    run_guarded(n * (44 + c.n_objects * 12 + n_rays * 8) + n_rays * 12 + SLACK, setup, '%s cast_rays %d rays at %d' % (kind, n_rays, residue))


# ---- automap.hip, reveal.hip: the line maps and the seen lines ---------------------------------------------------------------------

def seen_rows(c, st, lv, fan, max_range):
    return reveal_ref.reveal(c.lines, st, fan, max_range, levels=lv)


@pytest.mark.parametrize('with_seen', [False, True], ids=['all_lines', 'seen'])
@pytest.mark.parametrize('size', MAPS, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', KINDS)
def test_draw_maps(kind, size, with_seen):
    c = context(kind)
    n, (w, h) = 3, size
    st, lv = c.players(n, 80)
    kw = dict(width=w, height=h, scale=0.3, half_width=1.0)
    seen = seen_rows(c, st, lv, rd.map_fan(64, 2.0), 8.0)['seen'] if with_seen else None
    want = reveal_ref.draw_seen(c.lines, st, seen, levels=lv, **kw) if with_seen else automap_ref.draw(c.lines, st, levels=lv, **kw)
    assert len(np.unique(want)) >= 3
    for residue in (1, 2, 3):
        def setup(arena):
            d_st, d_lv = place_players(arena, st, lv, 4)
            d_seen = arena.place(seen.view(np.int32), 16, 4, 'seen', torch.int32) if with_seen else None
            out = arena.carve((n, h, w), torch.uint8, 16, residue, 'maps')
            assert out.data_ptr() % 4 == residue
            return (lambda: c.call('draw_maps', d_st, d_lv, w, h, 0.3, half_width=1.0, out=out, seen=d_seen)), [('maps', out, want)]
        run_guarded(n * (44 + w * h) + (seen.nbytes if with_seen else 0) + SLACK, setup, '%s draw_maps %dx%d at %d' % (kind, w, h, residue))


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n_rays', [5, 64])
@pytest.mark.parametrize('kind', KINDS)
def test_reveal_lines(kind, n_rays, residue):
    """the fan is (right, forward) pairs of floats: at 4 and 12 mod 16 no pair is 8-byte aligned.  The rows hold one player more than
    the call is given: the row behind the last player's keeps the poison"""
    c = context(kind)
    n = 3
    st, lv = c.players(n, 90 + n_rays)
    fan = rd.map_fan(n_rays, 2.0)
    off = c.offsets(n, 6)
    want = reveal_ref.reveal(c.lines, st, fan, 8.0, off, levels=lv)
    assert (want['new'] > 0).all()
    n_words = want['seen'].shape[1]
    assert n_words == c.h.seen_words()

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue)
        d_fan = arena.place(fan, 16, residue, 'fan', torch.float32)
        d_off = arena.place(off, 16, 4, 'offsets', torch.float32)
        rows = arena.carve((n + 1, n_words), torch.int32, 16, 4, 'seen')
        rows[:n].zero_()
        new = arena.carve((n,), torch.int32, 16, residue, 'new_out')
        assert d_fan.data_ptr() % 8 == 4 and rows.data_ptr() % 16 == 4
        return (lambda: c.call('reveal_lines', d_st, d_lv, d_fan, 8.0, offsets=d_off, seen=rows[:n], new_out=new)), \
            [('seen', rows[:n], want['seen']), ('new', new, want['new'])]
    run_guarded(n * (48 + c.n_objects * 12) + (n + 1) * n_words * 4 + n_rays * 8 + SLACK, setup,
                '%s reveal_lines %d rays at %d' % (kind, n_rays, residue))


# ---- area.hip: the explored area and its maps --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def explored(kind):
    """three players' explored area by the restatement: (states, slots, the reveal's dict), computed once and left unchanged"""
    c = context(kind)
    st, lv = c.players(3, 100)
    return st, lv, area_ref.reveal(c.lines, st, rd.map_fan(64, 2.0), 8.0, CELL, levels=lv)


@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n_rays', [5, 64])
@pytest.mark.parametrize('kind', KINDS)
def test_reveal_area(kind, n_rays, residue):
    c = context(kind)
    n = 3
    st, lv = c.players(n, 100)
    fan = rd.map_fan(n_rays, 2.0)
    want = area_ref.reveal(c.lines, st, fan, 8.0, CELL, levels=lv)
    assert (want['new'][:, 0] > 0).all() and want['new'][:, 1].any()
    n_words = want['area'].shape[2]
    assert n_words == c.h.area_words(CELL)

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue)
        d_fan = arena.place(fan, 16, residue, 'fan', torch.float32)
        rows = arena.carve((n + 1, 2, n_words), torch.int32, 16, 4, 'area')
        rows[:n].zero_()
        new = arena.carve((n, 2), torch.int32, 16, residue, 'new_out')
        assert d_fan.data_ptr() % 8 == 4
        return (lambda: c.call('reveal_area', d_st, d_lv, d_fan, 8.0, CELL, area=rows[:n], new_out=new)), \
            [('area', rows[:n], want['area']), ('new', new, want['new'])]
    run_guarded(n * 56 + (n + 1) * n_words * 8 + n_rays * 8 + SLACK, setup, '%s reveal_area %d rays at %d' % (kind, n_rays, residue))


@pytest.mark.parametrize('size', MAPS, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', KINDS)
def test_draw_area_maps(kind, size):
    c = context(kind)
    n, (w, h) = 3, size
    st, lv, seen = explored(kind)
    want = area_ref.draw(c.lines, st, seen['area'], CELL, w, h, 0.3, levels=lv)
    assert {rd.AREA_UNKNOWN, rd.AREA_FREE} <= set(np.unique(want).tolist())
    for residue in (1, 2, 3):
        def setup(arena):
            d_st, d_lv = place_players(arena, st, lv, 4)
            d_area = arena.place(seen['area'].view(np.int32), 16, 4, 'area', torch.int32)
            out = arena.carve((n, h, w), torch.uint8, 16, residue, 'maps')
            assert out.data_ptr() % 4 == residue
            return (lambda: c.call('draw_area_maps', d_st, d_lv, w, h, 0.3, d_area, CELL, out=out)), [('maps', out, want)]
        run_guarded(n * (44 + w * h) + seen['area'].nbytes + SLACK, setup, '%s draw_area_maps %dx%d at %d' % (kind, w, h, residue))


# ---- sectors.hip: the sector under a player, the sector maps -----------------------------------------------------------------------

@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', WAVE_COUNTS)
@pytest.mark.parametrize('kind', KINDS)
def test_locate_players(kind, n, held, residue):
    """heights_out is (floor, ceiling) pairs of floats: at 4 and 12 mod 16 no pair is 8-byte aligned"""
    c = context(kind)
    st, lv = c.players(n, 110 + n)
    off = c.offsets(n, 7)
    want = sector_ref.locate(c.tables, st, off, levels=lv)
    n_words = want['visited'].shape[1]
    assert n_words == c.h.visited_words() and (want['sector'] != sector_ref.NONE).any()

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue, held)
        d_off = arena.carve((held, c.n_objects, 3), torch.float32, 16, 4, 'offsets')
        d_off[:n].copy_(torch.from_numpy(off))
        out = arena.carve((held,), torch.int32, 16, residue, 'sector')
        heights = arena.carve((held, 2), torch.float32, 16, residue, 'heights_out')
        visited = arena.carve((held, n_words), torch.int32, 16, 4, 'visited')
        visited[:n].zero_()
        new = arena.carve((held,), torch.int32, 16, residue, 'new_out')
        assert heights.data_ptr() % 8 == 4

        def call():
            c.call('locate_players', d_st[:n * 40], None if d_lv is None else d_lv[:n], offsets=d_off[:n], heights_out=heights[:n], visited=visited[:n],
                   new_out=new[:n], out=out[:n])
        return call, [('sector', out[:n], want['sector']), ('heights', heights[:n], want['heights']), ('visited', visited[:n], want['visited']),
                      ('new', new[:n], want['new'])]
    run_guarded(held * (44 + c.n_objects * 12 + 16 + n_words * 4) + SLACK, setup, '%s locate_players n=%d of %d at %d' % (kind, n, held, residue))


@pytest.mark.parametrize('with_visited', [False, True], ids=['every_sector', 'visited'])
@pytest.mark.parametrize('size', MAPS, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', KINDS)
def test_draw_sector_maps(kind, size, with_visited):
    c = context(kind)
    n, (w, h) = 3, size
    st, lv = c.players(n, 120)
    off = c.offsets(n, 8)
    visited = sector_ref.locate(c.tables, st, off, levels=lv)['visited'] if with_visited else None
    want = sector_ref.draw(c.tables, st, off, levels=lv, visited=visited, width=w, height=h, scale=0.3)
    assert (want[0] != sector_ref.NONE16).any() and np.isfinite(want[1]).any()
    for residue in (2, 6):
        def setup(arena):
            d_st, d_lv = place_players(arena, st, lv, 4)
            d_off = arena.place(off, 16, 4, 'offsets', torch.float32)
            d_vis = arena.place(visited.view(np.int32), 16, 4, 'visited', torch.int32) if with_visited else None
            sector = arena.carve((n, h, w), torch.int16, 16, residue, 'sector')
            floor = arena.carve((n, h, w), torch.float32, 16, 4, 'floor')
            ceiling = arena.carve((n, h, w), torch.float32, 16, 4, 'ceiling')
            assert sector.data_ptr() % 4 == 2 and floor.data_ptr() % 16 == ceiling.data_ptr() % 16 == 4

            def call():
                c.call('draw_sector_maps', d_st, d_lv, w, h, 0.3, offsets=d_off, sector_out=sector, floor=floor, ceiling=ceiling, visited=d_vis)
            return call, [('sector', sector, want[0]), ('floor', floor, want[1]), ('ceiling', ceiling, want[2])]
        run_guarded(n * (44 + c.n_objects * 12 + w * h * 10 + 64) + SLACK, setup, '%s draw_sector_maps %dx%d at %d' % (kind, w, h, residue))


# ---- spawn.hip ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n', [1, 63, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_spawn_players(kind, n, residue):
    """the last player's mask byte is clear: its record, a byte pattern, keeps every byte, and its tries_out entry too"""
    c = context(kind)
    lv = c.slots(n, 130 + n)
    blank = spawn_ref.blank_states(n)
    mask = np.ones(n, np.uint8)
    mask[-1] = 0
    want, tries = spawn_ref.spawn(c.spawn_levels, blank, 1234, level_of=lv, mask=mask)
    assert n == 1 or ((tries[:-1] > 0).any() and (words(want)[:-10] != words(blank)[:-10]).any())
    kept = (n - 1) * 40

    def setup(arena):
        d_st, d_lv = place_players(arena, blank, lv, residue)
        d_mask = arena.place(mask, 16, 1, 'mask')
        d_tries = arena.carve((n,), torch.int32, 16, residue, 'tries_out')
        return (lambda: c.call('spawn_players', d_st, d_lv, 1234, mask=d_mask, tries_out=d_tries)), \
            [('states', d_st[:kept], words(want)[:kept // 4]), ('tries', d_tries[:n - 1], tries[:n - 1])]
    run_guarded(n * 49 + SLACK, setup, '%s spawn_players n=%d at %d' % (kind, n, residue))


# ---- goal.hip, path.hip: the players' cells, the level's planes, the frontier --------------------------------------------------------

@pytest.mark.parametrize('residue', [4, 12])
@pytest.mark.parametrize('n,held', WAVE_COUNTS)
@pytest.mark.parametrize('kind', KINDS)
def test_area_cells(kind, n, held, residue):
    c = context(kind)
    st, lv = c.players(n, 140 + n)
    if n > 2:
        st['pos'][2, 0] = np.nan  # a player in no cell
    want = goal_ref.cells(c.grids, CELL, st, levels=lv)
    assert (want >= 0).any()

    def setup(arena):
        d_st, d_lv = place_players(arena, st, lv, residue, held)
        out = arena.carve((held, 2), torch.int32, 16, residue, 'cells')
        return (lambda: c.call('area_cells', d_st[:n * 40], None if d_lv is None else d_lv[:n], CELL, out=out[:n])), [('cells', out[:n], want)]
    run_guarded(held * 52 + SLACK, setup, '%s area_cells n=%d of %d at %d' % (kind, n, held, residue))


@pytest.mark.parametrize('residue', [2, 6])
@pytest.mark.parametrize('kind', KINDS)
def test_draw_area_planes(kind, residue):
    c = context(kind)
    n = 3
    lv = c.slots(n, 150)
    off = c.offsets(n, 9)
    h, w = c.h.area_plane_shape(CELL)
    w += 3 - w % 4 if w % 4 != 3 else 4  # a caller's planes, wider than the grid and odd: the padding is void, rows change alignment
    want = goal_ref.planes(c.tables, c.grids, CELL, n, levels=lv, offsets=off, shape=(h, w))
    assert w % 2 == 1 and (want[0] != sector_ref.NONE16).any()

    def setup(arena):
        d_lv = arena.place(lv.view(np.int32), 16, 4, 'levels', torch.int32) if c.is_set else None
        d_off = arena.place(off, 16, 4, 'offsets', torch.float32)
        sector = arena.carve((n, h, w), torch.int16, 16, residue, 'sector')
        floor = arena.carve((n, h, w), torch.float32, 16, 4, 'floor')
        ceiling = arena.carve((n, h, w), torch.float32, 16, 12, 'ceiling')
        assert sector.data_ptr() % 4 == 2

        def call():
            args = ([d_lv] if c.is_set else []) + [CELL]
            c.h.draw_area_planes(*args, n=n, offsets=d_off, sector_out=sector, floor=floor, ceiling=ceiling)
        return call, [('sector', sector, want[0]), ('floor', floor, want[1]), ('ceiling', ceiling, want[2])]
    run_guarded(n * (4 + c.n_objects * 12 + w * h * 10 + 64) + SLACK, setup, '%s draw_area_planes at %d' % (kind, residue))


@pytest.mark.parametrize('kind', KINDS)
def test_area_frontiers(kind):
    """path.hip writes the mask four bytes at once where mask + iz * W + ix0 is dword aligned and byte by byte elsewhere: at an odd
    width both happen in one grid whatever the pointer, at a multiple of 64 the pointer alone decides"""
    c = context(kind)
    n = 3
    st, lv, seen = explored(kind)
    gh, gw = c.h.area_plane_shape(CELL)
    branches = set()
    for w in (gw + (1 - gw % 4) % 4, -(-gw // 64) * 64):  # the smallest width of the form 4 k + 1, and the next multiple of 64
        h = gh
        assert w >= gw and (w % 4 == 1 or w % 64 == 0)
        _, floor, ceiling = goal_ref.planes(c.tables, c.grids, CELL, n, levels=lv, area=seen['area'], shape=(h, w))
        dist, _ = goal_ref.flood_grids(floor, ceiling, goal_ref.cells(c.grids, CELL, st, levels=lv))
        cells, dists, counts, masks = path_ref.area_frontiers(seen['area'], c.grids, dist, levels=lv)
        assert (counts > 0).sum() >= 2 and masks.any()  # (a row without a frontier is a case too: its cell is (-1, -1))
        for residue in (1, 2, 3, 0):
            def setup(arena):
                d_lv = arena.place(lv.view(np.int32), 16, 4, 'levels', torch.int32) if c.is_set else None
                d_area = arena.place(seen['area'].view(np.int32), 16, 4, 'area', torch.int32)
                d_dist = arena.place(dist.view(np.int32), 16, 4, 'dist', torch.int32)
                cell_out = arena.carve((n, 2), torch.int32, 16, 4, 'cell_out')
                dist_out = arena.carve((n,), torch.int32, 16, 12, 'dist_out')
                count_out = arena.carve((n,), torch.int32, 16, 4, 'count_out')
                mask = arena.carve((n, h, w), torch.uint8, 16, residue, 'mask_out')
                assert mask.data_ptr() % 16 == residue
                # the kernel's own condition, for every run of 32 cells it stores
                branches.update((mask.data_ptr() + (p * h + iz) * w + ix0) % 4 == 0 for p in range(n) for iz in range(h) for ix0 in range(0, w, 32))

                def call():
                    args = ([d_lv] if c.is_set else []) + [d_area, d_dist, CELL]
                    c.h.area_frontiers(*args, cell_out=cell_out, dist_out=dist_out, count_out=count_out, mask_out=mask)
                return call, [('cells', cell_out, cells), ('dists', dist_out, dists), ('counts', count_out, counts), ('mask', mask, masks)]
            run_guarded(n * (w * h * 5 + 32) + seen['area'].nbytes + SLACK, setup, '%s area_frontiers width %d at %d' % (kind, w, residue))
            if w % 64 == 0:
                assert branches == ({True} if residue == 0 else {False})
            else:
                assert branches == {True, False}
            branches.clear()


# ---- the alignments the header asks for beyond the element's: refused by status, nothing queued -------------------------------------

@pytest.mark.parametrize('residue', [4, 8, 12])
@pytest.mark.parametrize('kind', KINDS)
def test_a_game_state_off_a_16_byte_boundary_is_refused(kind, residue):
    from guarded import Arena
    c = context(kind)
    n = 3
    st, lv, inp, act = game_players(c, n, 170)
    gb = c.h.game_bytes()
    arena = Arena(n * (40 + 4 + TICKS * 21 + gb + c.n_objects * 12) + SLACK, 0xFF)
    d_st, d_lv = place_players(arena, st, lv, 4)
    d_in = arena.place(inp, 16, 4, 'inputs')
    game = arena.carve((n * gb // 4,), torch.int32, 16, residue, 'game')
    offs = arena.carve((n, c.n_objects, 3), torch.float32, 16, 4, 'offsets')
    assert game.data_ptr() % 16 == residue
    arena.snapshot()
    extra = [d_lv] if c.is_set else []
    for call in (lambda: c.h.reset_game(game, offs, *extra), lambda: c.h.step_game(d_st, d_in, game, offs, *extra, n_ticks=TICKS)):
        with pytest.raises(rd.RdoomError) as e:
            call()
        assert e.value.status == -1 and '16-byte aligned' in str(e.value)
    arena.check(written=[], what='%s game state at %d' % (kind, residue))
