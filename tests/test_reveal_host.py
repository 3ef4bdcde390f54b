"""The seen lines on the host, with no GPU: the four entry points and their argument checks on host-only handles, rd.map_fan,
seen_words, and the restatement (tests/reveal_restatement.c) pinned without the library -- every line it marks has, in float64, a
point within range of the player that no blocking line hides; nothing is marked at a range of a millimetre; a door that one
player opened widens that player's set and nobody else's."""
import ctypes

import numpy as np
import pytest

import automap_ref
import reveal_ref
import rust_doom_amd as rd
from util import META_PATH, ensure_big_wad, ensure_wad

F = np.float32
BAD = -1  # RDOOM_BAD_ARG
LEVELS = [(ensure_wad, i) for i in range(9)] + [(ensure_big_wad, 0)]
IDS = ['E1M%d' % (i + 1) for i in range(9)] + ['big']


def test_the_entry_points_check_their_arguments_on_host_only_handles():
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ws = wad.build_world(0, device=False), wad.build_world_set([0, 7], device=False)
    words = world.seen_words()
    assert ws.seen_words() > words  # E1M8's table is the larger: the set's stride is checked against it
    assert world.game_objects > 1
    L = rd.lib()
    # the pointers are never followed: every call fails its checks, the last of them the device check of a host-only handle
    fake = ctypes.c_void_p(0x1000)
    view = rd.MapView(77, 53, 0.12, 0.75, 3.0, 0)

    def reveal(h=world, st=fake, n=4, dirs=fake, rays=8, rng=10.0, off=None, no=0, seen=fake, stride=words, new=None, lv=fake):
        hp = h._h if h is not None else None
        if h is ws or (h is None and lv is not fake):
            return L.rdoom_worldset_reveal_lines(hp, st, lv, n, dirs, rays, ctypes.c_float(rng), off, no, seen, stride, new, None)
        return L.rdoom_world_reveal_lines(hp, st, n, dirs, rays, ctypes.c_float(rng), off, no, seen, stride, new, None)

    def draw(h=world, st=fake, n=4, off=None, no=0, v=view, seen=fake, stride=words, out=fake, lv=fake):
        hp = h._h if h is not None else None
        vp = ctypes.byref(v) if v is not None else None
        if h is ws:
            return L.rdoom_worldset_draw_maps_seen(hp, st, lv, n, off, no, vp, seen, stride, out, None)
        return L.rdoom_world_draw_maps_seen(hp, st, n, off, no, vp, seen, stride, out, None)

    def fails(call, word, **kw):
        assert call(**kw) == BAD, kw
        assert word in L.rdoom_last_error().decode(), (kw, L.rdoom_last_error())

    inf, nan = float('inf'), float('nan')
    for h, w in ((world, words), (ws, ws.seen_words())):
        for kw in (dict(st=None), dict(seen=None), dict(dirs=None)):
            fails(reveal, 'null', h=h, stride=w, **kw)
        fails(reveal, 'n_rays', h=h, stride=w, rays=0)
        for r in (0.0, -1.0, inf, nan):
            fails(reveal, 'max_range', h=h, stride=w, rng=r)
        fails(reveal, 'stride', h=h, stride=w - 1)
        fails(reveal, 'stride', h=h, stride=0)
        fails(reveal, 'n_objects', h=h, stride=w, off=fake, no=1)
        fails(reveal, 'HOST_ONLY', h=h, stride=w)  # all else in order: the handle has no device copy
        fails(reveal, 'HOST_ONLY', h=h, stride=w + 3, new=fake, off=fake, no=64)
        fails(reveal, 'HOST_ONLY', h=h, stride=w, n=0, st=None, seen=None, dirs=None)
        fails(draw, 'stride', h=h, stride=w - 1)
        fails(draw, 'null', h=h, stride=w, v=None)
        fails(draw, 'null', h=h, stride=w, out=None)
        fails(draw, 'n_objects', h=h, stride=w, off=fake, no=1)
        fails(draw, 'HOST_ONLY', h=h, stride=w)
        fails(draw, 'HOST_ONLY', h=h, seen=None, stride=0)  # without a set the stride is not looked at
    fails(reveal, 'stride', h=ws, stride=words)  # enough for E1M1, not for the set's largest level
    fails(reveal, 'null', h=ws, stride=ws.seen_words(), lv=None)
    fails(draw, 'null', h=ws, stride=ws.seen_words(), lv=None)
    assert L.rdoom_world_reveal_lines(None, fake, 4, fake, 8, ctypes.c_float(10.0), None, 0, fake, words, None, None) == BAD
    assert L.rdoom_worldset_reveal_lines(None, fake, fake, 4, fake, 8, ctypes.c_float(10.0), None, 0, fake, words, None, None) == BAD
    assert L.rdoom_world_draw_maps_seen(None, fake, 4, None, 0, ctypes.byref(view), fake, words, fake, None) == BAD
    assert L.rdoom_worldset_draw_maps_seen(None, fake, fake, 4, None, 0, ctypes.byref(view), fake, words, fake, None) == BAD
    assert rd.LINE_MAPPED == 0x100


def test_map_fan():
    fan = rd.map_fan(65, 1.6)
    assert fan.shape == (65, 2) and fan.dtype == np.float32
    assert np.array_equal(fan[32], F([0, 1]))  # the centre ray is straight ahead
    assert np.array_equal(fan[::-1, 1], fan[:, 1]) and np.array_equal(fan[::-1, 0], -fan[:, 0])  # symmetric about it
    assert fan[0, 0] < 0 < fan[-1, 0]  # ray 0 is the leftmost
    angle = np.arctan2(fan[:, 0].astype(np.float64), fan[:, 1].astype(np.float64))
    assert np.allclose(np.diff(angle), 1.6 / 64, atol=1e-6) and np.isclose(angle[-1], 0.8)
    for n, fov in ((65, 1.6), (64, 1.6), (200, 2 * np.pi), (720, 2 * np.pi)):
        f = rd.map_fan(n, fov).astype(np.float64)
        norm = np.hypot(f[:, 0], f[:, 1])
        assert (np.abs(norm - 1.0) <= 2.0 ** -23).all(), np.abs(norm - 1.0).max()  # unit length to 1 ulp
        assert np.array_equal(f[::-1, 1], f[:, 1]) and np.array_equal(f[::-1, 0], -f[:, 0])
    assert np.array_equal(rd.map_fan(1, 2.0), F([[0, 1]]))
    with pytest.raises(ValueError):
        rd.map_fan(0, 1.0)


def test_seen_words_and_unpack_seen():
    wad = rd.Wad(ensure_wad(), META_PATH)
    slots = [0, 2, 7]
    ws = wad.build_world_set(slots, device=False)
    each = []
    for s, index in enumerate(slots):
        world = wad.build_world(index, device=False)
        n = len(world.map_lines())
        assert world.seen_words() == (n + 31) // 32 and world.seen_words() * 32 >= n > (world.seen_words() - 1) * 32
        each.append(world.seen_words())
    assert ws.seen_words() == max(each) and len(set(each)) > 1
    row = np.array([0x80000001, 0x2], np.uint32)
    got = rd.unpack_seen(row, 40)
    assert got.dtype == bool and got.shape == (40,) and np.array_equal(np.nonzero(got)[0], [0, 31, 33])
    assert np.array_equal(rd.unpack_seen(row.view(np.int32), 33), got[:33])
    with pytest.raises(ValueError):
        rd.unpack_seen(row, 65)


def _cross(ax, az, bx, bz):
    return ax * bz - az * bx


def _hidden64(o, q, a, b, slack):
    """float64: which of the segments a[k] -> b[k] the segment o -> q crosses, more than `slack` world units away from o, from q
    and from the ends of a -> b"""
    d, v, w = b - a, q - o, a - o
    den = _cross(v[0], v[1], d[:, 0], d[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        t = _cross(w[:, 0], w[:, 1], d[:, 0], d[:, 1]) / den
        u = _cross(w[:, 0], w[:, 1], v[0], v[1]) / den
    along, length = np.hypot(*v), np.hypot(d[:, 0], d[:, 1])
    return (den != 0) & (t * along > slack) & (t * along < along - slack) & (u * length > slack) & (u * length < length - slack)


@pytest.mark.parametrize('ensure,index', LEVELS, ids=IDS)
def test_what_the_restatement_marks_is_visible_in_float64(ensure, index):
    """a player at the level's start, 720 rays over 2 pi.  Every marked line has a witness -- the first ray that marked it and
    its t -- and, recomputed in float64 from the yaw and the fan, the witness point o + t * vel lies on the line, within max_range
    of the player, and the segment from the player to it crosses no blocking line; 1e-4 world units of slack against grazing
    (float32 positions of some tens of units carry 4e-6).  The blocking set is worked out here in numpy from the table."""
    wad = rd.Wad(ensure(), META_PATH)
    lines = wad.build_world(index, device=False).map_lines()
    pos, yaw = wad.build_level(index).start()
    st = rd.player_states(pos[None], np.array([yaw], F))
    fan = rd.map_fan(720, 2 * np.pi)
    block = reveal_ref.blocking(lines)
    a, b = lines['a'].astype(np.float64), lines['b'].astype(np.float64)
    o = np.array([pos[0], pos[2]], np.float64)
    slack = 1e-4
    for max_range in (6.0, 40.0):
        out = reveal_ref.reveal(lines, st, fan, max_range, detail=True)
        seen = rd.unpack_seen(out['seen'][0], len(lines))
        assert 0 < seen.sum() and out['new'][0] == seen.sum()
        assert seen.sum() < len(lines) or len(lines) == 9  # (E1M2 is one room of nine lines)
        assert np.array_equal(seen, out['witness_ray'][0] != reveal_ref.NO_WITNESS)
        s, c = np.sin(np.float64(yaw)), np.cos(np.float64(yaw))
        for l in np.nonzero(seen)[0]:
            right, forward = fan[out['witness_ray'][0, l]].astype(np.float64)
            vel = np.array([c * right - s * forward, -s * right - c * forward]) * max_range
            t = np.float64(out['witness_t'][0, l])
            q = o + t * vel
            assert 0 <= t <= 1 and np.hypot(*(q - o)) <= max_range + slack, (l, t)
            d = b[l] - a[l]
            on = np.clip(((q - a[l]) * d).sum() / (d * d).sum(), 0, 1)
            assert np.hypot(*(q - (a[l] + on * d))) <= slack, (l, q)
            hidden = _hidden64(o, q, a, b, slack) & block
            hidden[l] = False
            assert not hidden.any(), (l, np.nonzero(hidden)[0])
        # the rays' ends: a blocking hit where the ray stopped short of the range, and every stop is of a kind that blocks
        stopped = out['limit'][0] < 1.0
        assert np.array_equal(stopped, out['stop'][0] != reveal_ref.STOP_RANGE)
        if max_range == 40.0:
            assert stopped.mean() > 0.9
    # at a range of a millimetre nothing is marked -- but for a line the player stands on: E1M3's start lies on a floor step
    # (z = -13.44 of line 292), which is then rightly seen, and it is the only such start
    d = b - a
    on = np.clip(((o - a) * d).sum(1) / np.maximum((d * d).sum(1), 1e-300), 0, 1)
    underfoot = np.hypot(*(o - (a + on[:, None] * d)).T) <= 1e-3 + slack
    assert underfoot.sum() == (1 if IDS[LEVELS.index((ensure, index))] == 'E1M3' else 0)
    near = reveal_ref.reveal(lines, st, fan, 1e-3)
    assert not (rd.unpack_seen(near['seen'][0], len(lines)) & ~underfoot).any() and near['new'][0] <= underfoot.sum()


def test_rows_accumulate_and_count_what_is_new():
    wad = rd.Wad(ensure_wad(), META_PATH)
    lines = wad.build_world(0, device=False).map_lines()
    pos, yaw = wad.build_level(0).start()
    st = rd.player_states(np.repeat(pos[None], 2, 0), np.array([yaw, yaw + 2.0], F))
    fan = rd.map_fan(64, 1.6)
    first = reveal_ref.reveal(lines, st, fan, 20.0, stride=reveal_ref.words_of(len(lines)) + 2)
    assert (first['seen'][0] != first['seen'][1]).any() and (first['seen'][:, -2:] == 0).all()
    again = reveal_ref.reveal(lines, st[::-1].copy(), fan, 20.0, seen=first['seen'])
    assert np.array_equal(again['seen'][0], first['seen'][0] | first['seen'][1])
    assert np.array_equal(again['new'], reveal_ref.popcount(again['seen'] & ~first['seen'])) and (again['new'] > 0).all()
    third = reveal_ref.reveal(lines, st[::-1].copy(), fan, 20.0, seen=again['seen'])
    assert np.array_equal(third['seen'], again['seen']) and not third['new'].any()


def test_a_shut_door_blocks_until_its_player_opens_it():
    """E1M1's doors are shut at rest (MAP_CLOSED: the door sector's ceiling on its floor).  Two players stand half a unit before
    the middle of a door's face: in player 0's game the door is shut, in player 1's its ceiling is raised by `offsets`.  The open
    set strictly contains the shut one, and the door's own face is in both: a blocking line is seen."""
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(0, device=False)
    lines = world.map_lines()
    closed = np.nonzero(automap_ref.classes(lines) == rd.MAP_CLOSED)[0]
    assert len(closed) > 0
    fan = rd.map_fan(720, 2 * np.pi)
    for l in closed[:12]:
        door = int(max(lines['front']['ceiling_id'][l], lines['back']['ceiling_id'][l]))
        if door == 0:
            continue
        a, b = lines['a'][l], lines['b'][l]
        d = b - a
        normal = np.array([d[1], -d[0]], F) / F(np.hypot(*d))
        for side in (1.0, -1.0):
            at = (a + b) / 2 + normal * F(0.5 * side)
            st = rd.player_states(np.array([[at[0], 0.0, at[1]]] * 2, F), np.zeros(2, F))
            off = np.zeros((2, world.game_objects, 3), F)
            off[1, door, 1] = 1.0
            assert reveal_ref.blocking(lines, off[0])[l] and not reveal_ref.blocking(lines, off[1])[l]
            out = reveal_ref.reveal(lines, st, fan, 40.0, off)
            shut, opened = (rd.unpack_seen(r, len(lines)) for r in out['seen'])
            assert shut[l] and opened[l], (l, side)
            assert not (shut & ~opened).any() and (opened & ~shut).any(), (l, side)  # strictly more, and nothing less
            rest = reveal_ref.reveal(lines, st[:1], fan, 40.0)  # NULL offsets: every object at rest, the door shut
            assert np.array_equal(rest['seen'][0], out['seen'][0])
