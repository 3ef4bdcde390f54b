"""GPU: half lanes of the fragment kernel (rust-doom_amd/csrc/hip/fragment.hip).  An 8-pixel run an edge crosses used to list
both of its 4-pixel quads for the general per-pixel body.  Now, where one of the two quads shows ONE record, the lane rides the
per-lane packed body with that record over all 8 positions, stores that quad alone and lists only the other one; if the run-wide
guards of the body fail on the extrapolated half, or the uniform quad shows sky or a decoration, it lists both as before.

Every case compares three frames byte for byte -- the HIP frame, the oracle's, and the HIP frame under the hook no_half_runs=1
(the listing of before) -- and reads the kernel's own census (hook frag_count=1 -> rdoom_batch_path_stats: half_runs,
half_fallbacks, listed_quads) so that a dead path cannot pass:
  * with the hook on no lane is a half lane, and it lists exactly half_runs more quads than without (a finished half lane saves
    exactly one quad);
  * under no_qtab=1 every lane reads visibility words, so the half lanes are exactly the runs of the oracle's winner image that
    are mixed and have a uniform quad: half_runs + half_fallbacks equals that count; the runs whose chosen quad (quad 0 when
    both are uniform) is background all finish, those whose chosen quad is sky or decor all fall back.
The census of the oracle's winners also says that the frames hold what the case is about (every split 1|7 .. 7|1 and 4|4 on both
sides, three records in a run, background / sky / decor / masked / non-power-of-two neighbours).
Both instantiations with two quads per lane run: 16-bit visibility words by default, 32-bit ones under the hook vis32=1."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rust_doom_amd as rd
from oracle import raster
from test_gpu_raster_parity import sweep_poses
from test_kat_analytic import kat_level
from util import reference_projection, render_checked

pytestmark = pytest.mark.gpu

NO_PRIM = 0xFFFFFFFF
BACKGROUND, FLAT, WALL, DECOR, SKY = -1, 0, 1, 2, 3


def field(lv, key):
    return lv[key] if isinstance(lv, dict) else getattr(lv, key)


def view_roll(eye, yaw, pitch, roll):
    """inverse(T(eye) Ry(yaw) Rx(pitch) Rz(roll)), column-major: util.view_matrix with a roll, so that horizontal edges slant"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], np.float64)
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], np.float64)
    r = ry @ rx @ rz
    m = np.eye(4)
    m[:3, :3] = r.T
    m[:3, 3] = -(r.T @ np.asarray(eye, np.float64))
    return m.T.astype(np.float32).reshape(16)


def make_poses(views, w, h):
    poses = np.zeros(len(views), rd.POSE)
    for i, (eye, yaw, pitch, roll) in enumerate(views):
        poses[i]['modelview'] = view_roll(eye, yaw, pitch, roll)
        poses[i]['projection'] = reference_projection(w, h)
    return poses


def prim_tables(lv):
    """per primitive id of the oracle: kind, tile size is an integer that is no power of two, wall texture with transparent texels"""
    draws = np.asarray(field(lv, 'draws'), np.uint32).reshape(-1, 4)  # kind, object, first index, index count
    sv, si = field(lv, 'static_vertices'), np.asarray(field(lv, 'static_indices'), np.uint32)
    wall_atlas = np.asarray(field(lv, 'wall_atlas'))
    kinds, np2, masked = [], [], []
    for kind, _, first, count in draws:
        for t in range(int(count) // 3):
            kinds.append(int(kind))
            n2 = m = False
            if kind in (FLAT, WALL):
                v = sv[si[first + 3 * t + 2]]
                tw, th = float(v['a_tile_size'][0]), float(v['a_tile_size'][1])
                n2 = any(s == int(s) and (int(s) & (int(s) - 1)) != 0 for s in (tw, th))
                if kind == WALL:
                    ax, ay = int(v['a_atlas_uv'][0]), int(v['a_atlas_uv'][1])
                    m = bool((wall_atlas[ay:ay + int(th), ax:ax + int(tw)] & 0x8000).any())
            np2.append(n2), masked.append(m)
    return np.array(kinds, np.int64), np.array(np2, bool), np.array(masked, bool)


def census(prims, tables):
    """what fragment_kernel's classification makes of the oracle's winners when every lane reads visibility words"""
    kinds, np2, masked = tables
    out = dict(candidates=0, background=0, sky_decor=0, three=0, masked=0, np2=0, splits=set())
    for prim in prims:
        h, w = prim.shape
        r = prim.reshape(h, w // 8, 8).astype(np.int64)
        u0 = (r[..., 0:4] == r[..., 0:1]).all(-1)
        u1 = (r[..., 4:8] == r[..., 4:5]).all(-1)
        cand = ~(u0 & u1 & (r[..., 0] == r[..., 4])) & (u0 | u1)
        sel = np.where(u0, r[..., 0], r[..., 4])[cand]  # the chosen quad's winner: quad 0 when both are uniform
        runs = r[cand]
        kind = np.where(sel == NO_PRIM, BACKGROUND, kinds[np.minimum(sel, len(kinds) - 1)])
        static = (kind == FLAT) | (kind == WALL)
        safe = np.minimum(sel, len(kinds) - 1)
        out['candidates'] += int(cand.sum())
        out['background'] += int((kind == BACKGROUND).sum())
        out['sky_decor'] += int(((kind == SKY) | (kind == DECOR)).sum())
        out['masked'] += int((static & masked[safe]).sum())
        out['np2'] += int((static & np2[safe]).sum())
        distinct = (np.diff(np.sort(runs, axis=-1), axis=-1) != 0).sum(-1) + 1
        out['three'] += int((distinct >= 3).sum())
        two = runs[distinct == 2]
        lead = (two == two[:, 0:1]).cumprod(-1).sum(-1)          # leading pixels of the first record,
        tail = (two[:, ::-1] == two[:, 7:8]).cumprod(-1).sum(-1)  # trailing ones of the last: a lead | tail split when they add up
        out['splits'] |= set(int(x) for x in lead[lead + tail == 8])
    return out


def oracle_frames(lv, poses, lights, w, h):
    ro = raster.RasterOracle(lv)

    def one(i):
        return ro.render(poses[i]['modelview'], poses[i]['projection'], float(poses[i]['time']), lights, w, h, want_prim=True)

    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, range(len(poses))))
    return np.stack([r[0] for r in res]), [r[1] for r in res]


def render(dev, poses, lights, w, h, hooks):
    """frames and the fragment kernel's census of one render (after a dirtying render) under hooks + frag_count"""
    try:
        rd.debug_set('frag_count', 1)
        for name, value in hooks.items():
            rd.debug_set(name, value)
        batch = rd.Batch(dev, w, h, len(poses))
        fb, _, _ = render_checked(batch, poses, lights, want_prim=False)
        st = batch.path_stats()
    finally:
        rd.debug_set('reset')
    return fb, st


def three_way(lv, poses, lights, w, h, base=None, two_quads=True):
    """HIP == oracle == HIP under no_half_runs, the two listings differ by exactly the finished half lanes, and under no_qtab the
    kernel's half lanes are the census's candidates.  Returns (census, stats of the default render, stats under no_qtab)."""
    base = dict(base or {})
    want, prims = oracle_frames(lv, poses, lights, w, h)
    dev = rd.DeviceLevel(lv)
    fb, st = render(dev, poses, lights, w, h, base)
    fb_old, st_old = render(dev, poses, lights, w, h, dict(base, no_half_runs=1))
    fb_all, st_all = render(dev, poses, lights, w, h, dict(base, no_qtab=1))
    print('half lanes %s: default %s, no_half_runs %s, no_qtab %s' % ((w, h, base), pick(st), pick(st_old), pick(st_all)))
    assert np.array_equal(fb, want), int((fb != want).sum())
    assert np.array_equal(fb_old, fb) and np.array_equal(fb_all, fb)
    assert st_old['half_runs'] == 0 and st_old['half_fallbacks'] == 0
    assert st_old['listed_quads'] - st['listed_quads'] == st['half_runs']
    if not two_quads:
        return None, st, st_all
    c = census(prims, prim_tables(lv))
    print('census %s' % {k: (sorted(v) if isinstance(v, set) else v) for k, v in c.items()})
    assert st_all['half_runs'] + st_all['half_fallbacks'] == c['candidates']
    assert st_all['half_fallbacks'] >= c['sky_decor'] and st_all['half_runs'] >= c['background']
    assert st_all['half_runs'] <= c['candidates'] - c['sky_decor']
    assert st['half_runs'] <= st_all['half_runs']  # (runs in described quadrants are never mixed: fewer lanes read words, none more)
    return c, st, st_all


def pick(st):
    return {k: st[k] for k in ('half_runs', 'half_fallbacks', 'listed_quads')}


def kat_views():
    """the KAT room from inside: a wall seen at a slant (its top and bottom edges cross the runs at every split) and the floor
    fan's diagonals, with a roll so that vertical edges slant too"""
    return [((0.3, 0.05, 0.4), 0.9, -0.25, 0.35), ((-0.4, 0.1, -0.3), -1.1, -0.4, -0.6)]


@pytest.mark.parametrize('size,hooks', [((1280, 720), {}), ((1280, 724), {}), ((320, 200), {}), ((320, 200), {'vis32': 1}),
                                        ((1280, 724), {'vis32': 1})])
def test_kat_room_every_split(oracle_levels, size, hooks):
    """E1M2 of the synthetic IWAD, 32 x 16 blocks (1280 wide; 724 rows: the last block row is cut) and 64 x 8 blocks (320 x 200),
    16- and 32-bit visibility words: every split on both sides, triangles next to background"""
    lv, (w, h) = oracle_levels(1), size
    sp = np.array([float(x) for x in lv.start_pos])
    views = [((sp[0] + 0.2, sp[1] + 0.1, sp[2] - 0.1), float(lv.start_yaw) + 0.8, -0.3, 0.4),
             ((sp[0] - 0.1, sp[1] + 0.3, sp[2] + 0.2), float(lv.start_yaw) - 1.0, -0.45, -0.7)]
    c, st, st_all = three_way(lv, make_poses(views, w, h), lv.lights.fill_buffer_at(0.0), w, h, hooks)
    assert c['splits'] >= set(range(1, 8)), sorted(c['splits'])
    assert st['half_runs'] > 0 and st_all['half_runs'] > 0


def test_one_quad_per_lane_is_untouched(oracle_levels):
    """324 x 200: rows do not divide into 8-pixel runs, one quad per lane -- no half lanes, the same listing under both hooks"""
    lv, w, h = oracle_levels(1), 324, 200
    sp = np.array([float(x) for x in lv.start_pos])
    views = [((sp[0] + 0.2, sp[1] + 0.1, sp[2] - 0.1), float(lv.start_yaw) + 0.8, -0.3, 0.4)]
    _, st, st_all = three_way(lv, make_poses(views, w, h), lv.lights.fill_buffer_at(0.0), w, h, two_quads=False)
    assert st['half_runs'] == 0 and st['half_fallbacks'] == 0 and st_all['half_runs'] == 0 and st_all['half_fallbacks'] == 0
    assert st_all['listed_quads'] > 0


def test_e1m1_sky_decor_masked_three_records(oracle_levels):
    """E1M1 sweep poses: walls next to sky and to decorations (the half lane lists both quads), masked textures on the uniform
    side, runs with three records, background"""
    lv, w, h = oracle_levels(0), 1280, 720
    poses = sweep_poses(lv, 4, w, h, seed=11, time=0.4)
    c, st, st_all = three_way(lv, poses, lv.lights.fill_buffer_at(0.4), w, h)
    assert c['sky_decor'] > 0 and c['three'] > 0 and c['masked'] > 0
    assert st_all['half_fallbacks'] > 0 and st['half_runs'] > 0


def scene(tile_wall, tile_floor, floor_extent):
    lvl, lights = kat_level()
    lvl['static_vertices'][0:4]['a_tile_size'] = tile_wall
    lvl['static_vertices'][4:8]['a_tile_size'] = tile_floor
    for k, (x, z) in enumerate([(-1, 1), (1, 1), (1, -1), (-1, -1)]):
        x, z = x * floor_extent, (1.0 if z > 0 else -floor_extent)
        lvl['static_vertices'][4 + k]['a_pos'] = (x, lvl['static_vertices'][4 + k]['a_pos'][1], z)
        lvl['static_vertices'][4 + k]['a_tile_uv'] = (-x * 100.0, -z * 100.0)
    return lvl, lights


@pytest.mark.parametrize('size', [(320, 200), (1280, 720)])
def test_integer_tile_sizes(size):
    """tile sizes 48 x 100 and 40 x 56: the modulus certificate runs on the extrapolated positions of every half lane"""
    (w, h), (lvl, lights) = size, scene((48, 100), (40, 56), 4.0)
    c, st, st_all = three_way(lvl, make_poses(kat_views(), w, h), lights, w, h)
    assert c['np2'] > 0 and c['np2'] + c['background'] == c['candidates']
    assert st_all['half_runs'] > c['background']  # (some half lane with a non-power-of-two record finished)


def test_floor_towards_the_horizon_falls_back():
    """a floor that reaches past the far plane, camera rolled: along the slanted far-plane line the floor side's 1/w, extrapolated
    over the other quad, turns negative -- out of the verified range of the reciprocal -- and the lane lists both quads"""
    w, h = 320, 200
    lvl, lights = scene((64, 128), (64, 64), 300.0)
    views = [((0.0, 0.0, 0.0), 0.0, 0.05, 0.5), ((0.0, 0.2, 0.0), 2.0, -0.05, -0.8)]
    c, st, st_all = three_way(lvl, make_poses(views, w, h), lights, w, h)
    assert c['sky_decor'] == 0  # (every fallback below is a guard of the packed body)
    assert st_all['half_fallbacks'] > 0 and st['half_fallbacks'] > 0
